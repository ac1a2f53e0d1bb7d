"""Time the actor-critic collection (cs_rollout_actor_critic) and the advantages (cs_gae) against what they replace.
Lander3D, float32 storage, next_step auto-reset, K = 64, actor and critic of the same width, hidden in {0, 32, 64}.

Per (N, hidden), in one process, interleaved over `--rounds` rounds, the best round kept and the spread of the rounds
(max / min - 1) beside it, in us per step:
  states      rollout_mlp_states(actor, K, hidden): the closed-loop forward without noise, values or env state
  collect     rollout_actor_critic(actor, critic, log_std, K, hidden, means=True)
  loop        the loop it replaces: K x (torch actor, critic, sampler, log-prob + step), the tapes stacked
  gae         gae(reward, values, terminated, truncated)
  scan        the K-step torch scan gae replaces
Ratios, no bars.  The shader clock under load (CopterVecEnv.clock_probe) is printed per row.
--variant NAME=PATH repeats states and collect in a child process on another build of the library (COPTERSTEP_LIB):
`make -C gym_copter_amd/csrc exp NAME=ac_full DEFS=-DCS_EXP_AC_FULL`, pass
ac_full=gym_copter_amd/csrc/build/libcopterstep_ac_full.so -- the collection in its full-featured form for every
configuration, where the library in the tree runs the lean form (advance()'s optional features compiled out) in this one.

    python tools/rollout_ac_bench.py [--rounds 5] [--steps 64] [--envs 65536 1048576] [--hidden 0 32 64]
                                     [--variant NAME=path/to/libcopterstep_NAME.so ...] [--out profiles/rollout_ac_bench]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn):
    import torch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3          # us


def _hover():
    import numpy as np
    return float(np.sqrt(9.80665 * 1.380 / (4 * 5.e-3 * (15000 * np.pi / 30) ** 2)))


def measure(n, hidden, K, rounds, only=None):
    import torch
    import gym_copter_amd
    from gym_copter_amd import mlp
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", autoreset_mode="next_step",
                                      seed=1)
    try:
        env.reset()
        dev = env.device
        gen = torch.Generator().manual_seed(3)
        actor = mlp.init(10, 4, hidden, generator=gen, out_bias=_hover(), out_scale=0.01).to(dev)
        critic = mlp.init(10, 1, hidden, generator=gen).to(dev)
        log_std = torch.full((4,), math.log(0.05), dtype=torch.float32, device=dev)
        pa, pc = mlp.unpack(actor, 10, 4, hidden), mlp.unpack(critic, 10, 1, hidden)

        def net(p, o):
            if hidden == 0:
                return o @ p["W"].T + p["b"]
            return torch.tanh(o @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]

        got = {}

        def states():
            env.rollout_mlp_states(actor, K, hidden)

        def collect():
            got["roll"] = env.rollout_actor_critic(actor, critic, log_std, K, hidden, means=True)

        obs0 = env.reset()[0].clone()

        def loop():
            o = obs0
            tape = []
            sigma = torch.exp(log_std)
            for _ in range(K):
                mu, v = net(pa, o), net(pc, o)[:, 0]
                a = mu + sigma * torch.randn_like(mu)
                z = (a - mu) / sigma
                logp = -0.5 * (z * z).sum(-1) - log_std.sum() - 2.0 * math.log(2.0 * math.pi)
                o2, r, term, trunc, _ = env.step(a)
                tape.append((o, a, mu, logp, v, r.clone(), term.clone(), trunc.clone()))
                o = o2.clone()
            got["tape"] = [torch.stack(t) for t in zip(*tape)]

        def gae():
            roll = got["roll"]
            got["gae"] = env.gae(roll.reward, roll.values, roll.terminated, roll.truncated)

        def scan():
            roll = got["roll"]
            nd = 1.0 - (roll.terminated | roll.truncated).float()
            adv = torch.empty_like(roll.reward)
            nxt = torch.zeros(n, device=dev)
            for k in range(K - 1, -1, -1):
                delta = roll.reward[k] + 0.99 * roll.values[k + 1] * nd[k] - roll.values[k]
                nxt = delta + 0.99 * 0.95 * nd[k] * nxt
                adv[k] = nxt
            got["scan"] = (adv, adv + roll.values[:K])

        fns = {"states": states, "collect": collect, "loop": loop, "gae": gae, "scan": scan}
        if only is not None:
            fns = {k: v for k, v in fns.items() if k in only}
        for fn in fns.values():
            fn()
        if only is None:
            assert torch.allclose(got["gae"][0], got["scan"][0], rtol=1e-4, atol=1e-3)
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                times[name].append(_time(fn))
        clock = env.clock_probe()
    finally:
        env.close()
    out = {"envs": n, "hidden": hidden, "K": K, "rounds": rounds, "clock_mhz": round(clock / 1e6)}
    for name, ts in times.items():
        out[name + "_us_per_step"] = round(min(ts) / K, 3)
        out[name + "_spread"] = round(max(ts) / min(ts) - 1, 4)
    out["collect_over_states"] = round(min(times["collect"]) / min(times["states"]), 3)
    if only is None:
        out["loop_over_collect"] = round(min(times["loop"]) / min(times["collect"]), 1)
        out["scan_over_gae"] = round(min(times["scan"]) / min(times["gae"]), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--hidden", type=int, nargs="*", default=[0, 32, 64])
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library")
    ap.add_argument("--child", action="store_true", help="(internal) states and collect only, rows as JSON lines")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ac_bench"))
    args = ap.parse_args()
    if args.child:
        for n in args.envs:
            for H in args.hidden:
                print("ROW " + json.dumps(measure(n, H, args.steps, args.rounds, only=("states", "collect"))), flush=True)
        return
    rows = []
    lines = ["# tools/rollout_ac_bench.py: Lander3D, float32 storage, next_step auto-reset, K = %d; us per step, best of %d "
             "interleaved rounds in one process, the rounds' spread (max / min - 1) beside each figure"
             % (args.steps, args.rounds)]
    for n in args.envs:
        for H in args.hidden:
            r = measure(n, H, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  H %2d: states %8.3f (+-%4.1f %%) | collect %8.3f (+-%4.1f %%) = %.3f x states | loop "
                         "%9.3f (+-%4.1f %%) = %.1f x collect | gae %7.3f (+-%4.1f %%) | scan %8.3f (+-%4.1f %%) = %.1f x "
                         "gae | clock %d MHz"
                         % (r["envs"], r["hidden"], r["states_us_per_step"], 100 * r["states_spread"],
                            r["collect_us_per_step"], 100 * r["collect_spread"], r["collect_over_states"],
                            r["loop_us_per_step"], 100 * r["loop_spread"], r["loop_over_collect"], r["gae_us_per_step"],
                            100 * r["gae_spread"], r["scan_us_per_step"], 100 * r["scan_spread"], r["scan_over_gae"],
                            r["clock_mhz"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)
    record = {"default": rows}
    for spec in args.variant:
        name, path = spec.split("=", 1)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--steps",
               str(args.steps), "--envs"] + [str(n) for n in args.envs] + ["--hidden"] + [str(h) for h in args.hidden]
        p = subprocess.run(cmd, env=dict(os.environ, COPTERSTEP_LIB=os.path.abspath(path)), capture_output=True,
                           text=True, timeout=600)
        if p.returncode != 0:
            raise SystemExit("variant %s failed (%d):\n%s" % (name, p.returncode, p.stderr[-4000:]))
        record[name] = [json.loads(ln[4:]) for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        for r in record[name]:
            lines.append("%-8s %8d envs  H %2d: states %8.3f (+-%4.1f %%) | collect %8.3f (+-%4.1f %%) = %.3f x states | "
                         "clock %d MHz" % (name, r["envs"], r["hidden"], r["states_us_per_step"], 100 * r["states_spread"],
                                           r["collect_us_per_step"], 100 * r["collect_spread"], r["collect_over_states"],
                                           r["clock_mhz"]))
            print(lines[-1], flush=True)
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
