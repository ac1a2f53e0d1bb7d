"""Time the population rollout (cs_rollout_mlp_population) against the closed-loop forward it copies
(cs_rollout_mlp_states on the same N with one shared theta), and one evolution-strategies iteration on the new entry
points against the route a caller had before them.  Lander3D, float32 storage, K = 64, hidden in {0, 32, 64}.

(a) per (N, hidden), in one process, interleaved over `--rounds` rounds, the best round kept and the spread of the rounds
    (max / min - 1) beside it:
      states      rollout_mlp_states(theta, K, hidden): every tape written (x, reward, flags, status, obs, actions)
      pop         rollout_mlp_population(table [N/64, P], K, hidden, 64): a different theta per wavefront, no tape (the
                  member-mean kernel behind it included)
    both from the same explicit starts 5-20 m up under near-hover policies (nobody lands inside the horizon, so no
    wavefront leaves the loop early and the two do the same arithmetic).
    --variant NAME=PATH repeats (a) in a child process on another build of the library (COPTERSTEP_LIB): edit
    copterstep_rollout_es.hip, `make -C gym_copter_amd/csrc exp NAME=x`, pass x=gym_copter_amd/csrc/build/libcopterstep_x.so.
    The recorded rows "waves2" and "lds" are such builds: amdgpu_waves_per_eu(2, 2), and the member's row staged in the
    LDS at 2 wavefronts per SIMD.
(b) at `--es-envs` envs (M = N/64 members): es_perturb + rollout_mlp_population + es_gradient against a loop of M
    rollout_mlp_states calls on a 64-env batch with torch reductions of their tapes (returns with the first-flag mask and
    the discount, the member mean), the table and the gradient in torch.  The ratio only.
The shader clock under load (CopterVecEnv.clock_probe) is printed before and after each block.

    python tools/rollout_es_bench.py [--rounds 5] [--steps 64] [--envs 65536 1048576] [--es-envs 65536]
                                     [--variant NAME=path/to/libcopterstep_NAME.so ...]
                                     [--out profiles/rollout_es_bench]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E = 64


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


def _policies(M, hidden, rng, dev):
    """M near-hover policies [M,P] float32 that differ in every weight (the output stays within a few per cent of the
    hover motor value, so that nobody tilts out, leaves the bounds or lands inside the horizon)."""
    import numpy as np
    import torch
    from gym_copter_amd import mlp
    P = mlp.num_params(10, 4, hidden)
    t = rng.uniform(-1, 1, (M, P)) * (2e-5 if hidden == 0 else 0.3)
    t[:, -4:] = _hover() * rng.uniform(0.98, 1.02, (M, 4))
    if hidden:
        t[:, hidden * 11:hidden * 11 + 4 * hidden] *= 2e-5 / 0.3
    return torch.from_numpy(t.astype(np.float32)).to(dev)


def _starts(n, rng, dev):
    import numpy as np
    import torch
    x0 = np.zeros((12, n))
    x0[0], x0[2] = rng.uniform(-2, 2, (2, n))
    x0[4] = -rng.uniform(5, 20, n)
    x0[5] = rng.uniform(-1, 1, n)
    return {"x": torch.from_numpy(x0).to(dev), "status": torch.full((n,), 3, dtype=torch.uint8, device=dev)}


def measure_kernels(n, hidden, K, rounds):
    import numpy as np
    import gym_copter_amd
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", autoreset_mode="disabled",
                                      seed=1, max_steps=100000)
    try:
        env.reset()
        rng = np.random.default_rng(0)
        table = _policies(n // E, hidden, rng, env.device)
        one = table[:1].contiguous()
        state = _starts(n, rng, env.device)
        clock0 = env.clock_probe()
        got = {}

        def states():
            got["ro"] = env.rollout_mlp_states(one[0], K, hidden, state=state)

        def pop():
            got["pop"] = env.rollout_mlp_population(table, K, hidden, E, 0.99, state=state)

        fns = {"states": states, "pop": pop}
        for fn in fns.values():
            fn()
        # nobody may have left the loop early
        assert int(got["pop"].lengths.min()) == K
        ro = got["ro"]
        assert not bool((ro.terminated | ro.truncated).any())
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                times[name].append(_time(fn))
        clock1 = env.clock_probe()
    finally:
        env.close()
    out = {"envs": n, "hidden": hidden, "K": K, "rounds": rounds, "clock_mhz": [round(clock0 / 1e6), round(clock1 / 1e6)]}
    for name, ts in times.items():
        out[name + "_us"] = round(min(ts), 1)
        out[name + "_spread"] = round(max(ts) / min(ts) - 1, 4)
    out["pop_over_states"] = round(min(times["pop"]) / min(times["states"]), 4)
    out["pop_us_per_step_per_1M"] = round(min(times["pop"]) / K / (n / 2 ** 20), 3)
    return out


def measure_iteration(n, hidden, K, rounds):
    import numpy as np
    import torch
    import gym_copter_amd
    kw = dict(task="lander3d", state_dtype="float32", autoreset_mode="disabled", seed=1, max_steps=100000)
    env = gym_copter_amd.CopterVecEnv(num_envs=n, **kw)
    small = gym_copter_amd.CopterVecEnv(num_envs=E, **kw)
    try:
        env.reset()
        small.reset()
        dev = env.device
        rng = np.random.default_rng(1)
        M = n // E
        theta = _policies(1, hidden, rng, dev)[0]
        P = int(theta.shape[0])
        s64 = _starts(E, rng, dev)
        big = {"x": s64["x"].repeat(1, M).contiguous(), "status": s64["status"].repeat(M).contiguous()}
        sigma, gamma = 0.002, 0.99
        disc = gamma ** torch.arange(K, dtype=torch.float64, device=dev)[:, None]
        got = {}

        def shaped(f):
            ranks = torch.empty(M, dtype=torch.float64, device=dev)
            ranks[torch.argsort(f)] = torch.arange(M, dtype=torch.float64, device=dev)
            return ranks / (M - 1) - 0.5

        def iteration():
            table = env.es_perturb(theta, sigma, M, 3)
            f = env.rollout_mlp_population(table, K, hidden, E, gamma, state=big).member_returns
            got["g"] = env.es_gradient(shaped(f), 3, P) / (M * sigma)

        def loop():
            eps = torch.randn((M // 2, P), dtype=torch.float32, device=dev)
            table = torch.stack([theta + sigma * eps, theta - sigma * eps], dim=1).view(M, P)
            f = torch.empty(M, dtype=torch.float64, device=dev)
            for m in range(M):
                ro = small.rollout_mlp_states(table[m], K, hidden, state=s64)
                done = (ro.terminated | ro.truncated).cumsum(0)
                alive = (done - (ro.terminated | ro.truncated).to(done.dtype)) == 0     # up to and including the first flag
                f[m] = (ro.reward * alive * disc).sum(0).mean()
            w = shaped(f)
            got["g0"] = ((w[0::2] - w[1::2]) @ eps.double()) / (M * sigma)

        fns = {"iteration": iteration, "loop": loop}
        for fn in fns.values():
            fn()
        times = {k: [] for k in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                times[name].append(_time(fn))
        clock = env.clock_probe()
    finally:
        env.close()
        small.close()
    out = {"envs": n, "members": M, "hidden": hidden, "K": K, "rounds": rounds, "clock_mhz": round(clock / 1e6)}
    for name, ts in times.items():
        out[name + "_us"] = round(min(ts), 1)
        out[name + "_spread"] = round(max(ts) / min(ts) - 1, 4)
    out["loop_over_iteration"] = round(min(times["loop"]) / min(times["iteration"]), 1)
    return out


def _line(r, label):
    return ("%-8s %8d envs  H %2d  K %d: states %10.1f us (+-%4.1f %%) | pop %10.1f us (+-%4.1f %%, %6.2f us/step per 2^20 "
            "envs) | pop/states %.3f | clock %s MHz"
            % (label, r["envs"], r["hidden"], r["K"], r["states_us"], 100 * r["states_spread"], r["pop_us"],
               100 * r["pop_spread"], r["pop_us_per_step_per_1M"], r["pop_over_states"],
               "/".join(str(c) for c in r["clock_mhz"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--hidden", type=int, nargs="*", default=[0, 32, 64])
    ap.add_argument("--es-envs", type=int, default=65536)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of another build of the library")
    ap.add_argument("--child", action="store_true", help="(internal) part (a) only, rows as JSON lines on stdout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_es_bench"))
    args = ap.parse_args()
    if args.child:
        for n in args.envs:
            for H in args.hidden:
                print("ROW " + json.dumps(measure_kernels(n, H, args.steps, args.rounds)), flush=True)
        return
    record = {"kernels": {"default": []}, "iteration": []}
    lines = ["# tools/rollout_es_bench.py: Lander3D, float32 storage, E = 64; best of %d interleaved rounds in one process, "
             "the rounds' spread (max / min - 1) beside each figure" % args.rounds]

    def save():
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(record, f, indent=1)

    for n in args.envs:
        for H in args.hidden:
            r = measure_kernels(n, H, args.steps, args.rounds)
            record["kernels"]["default"].append(r)
            lines.append(_line(r, "default"))
            print(lines[-1], flush=True)
            save()
    for H in args.hidden:
        r = measure_iteration(args.es_envs, H, args.steps, max(2, args.rounds // 2))
        record["iteration"].append(r)
        lines.append("ES iteration %d envs = %d members x %d  H %2d  K %d: perturb + population + gradient %9.1f us (+-%4.1f %%) | "
                     "loop of %d rollout_mlp_states calls + torch reductions %11.1f us (+-%4.1f %%) = %.1fx | clock %d MHz"
                     % (r["envs"], r["members"], E, H, r["K"], r["iteration_us"], 100 * r["iteration_spread"], r["members"],
                        r["loop_us"], 100 * r["loop_spread"], r["loop_over_iteration"], r["clock_mhz"]))
        print(lines[-1], flush=True)
        save()
    for spec in args.variant:
        name, path = spec.split("=", 1)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds), "--steps",
               str(args.steps), "--envs"] + [str(n) for n in args.envs] + ["--hidden"] + [str(h) for h in args.hidden]
        p = subprocess.run(cmd, env=dict(os.environ, COPTERSTEP_LIB=os.path.abspath(path)), capture_output=True,
                           text=True, timeout=900)
        if p.returncode != 0:
            raise SystemExit("variant %s failed (%d):\n%s" % (name, p.returncode, p.stderr[-4000:]))
        rows = [json.loads(ln[4:]) for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        record["kernels"][name] = rows
        for r in rows:
            lines.append(_line(r, name))
            print(lines[-1], flush=True)
        save()


if __name__ == "__main__":
    main()
