"""Time PPO's minibatch loss and gradient on the device (cs_ppo_grad, CopterVecEnv.ppo_grad) against what it replaces:
the body of gym_copter_amd/ppo.py's minibatch loop up to and including loss.backward() -- the optimizer's step excluded on
both sides -- on the same tapes and the same index.  Lander3D shapes, actor and critic of the same width.

Per (B, hidden), in one process, interleaved over `--rounds` rounds, the best round kept and the spread of the rounds
(max / min - 1) beside it, in us per minibatch:
  device      env.ppo_grad(..., index=idx) into preallocated outputs
  torch       the gather of five tapes, two float32 MLP forwards, the loss, loss.backward()
The tapes hold 4 B rows (an iteration of four minibatches) and the index is the first B of a permutation of them.
Then a whole iteration of gym_copter_amd.ppo at the driver's settings (8 192 envs, K = 64, H = Hv = 16, 4 epochs x 4
minibatches: collection, advantages and 16 updates with Adam's steps) for update="torch" and update="device", wall
clock with the device idle at both ends, best of `--rounds`.  Ratios, no bars.

    python tools/ppo_update_bench.py [--rounds 5] [--samples 131072 1048576 4194304] [--hidden 0 16 64]
                                     [--out profiles/ppo_update_bench]
"""
import argparse
import json
import math
import os
import sys
import time

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


def measure(env, B, hidden, rounds):
    import torch
    from gym_copter_amd import mlp
    from gym_copter_amd.ppo import _forward, gaussian_logp
    dev, R, od, A = env.device, 4 * B, 10, 4
    gen = torch.Generator(device=dev).manual_seed(3)
    cpu = torch.Generator().manual_seed(3)
    old = mlp.init(od, A, hidden, generator=cpu, out_bias=_hover(), out_scale=0.3).to(dev)
    critic0 = mlp.init(od, 1, hidden, generator=cpu).to(dev)
    ls_old = torch.full((A,), math.log(0.05), dtype=torch.float32, device=dev)
    with torch.no_grad():
        obs = torch.randn((R, od), device=dev, generator=gen)
        mu = _forward(torch, old, obs, hidden, od, A)
        act = mu + 0.05 * torch.randn((R, A), device=dev, generator=gen)
        logp_old = gaussian_logp(torch, act, mu, ls_old)
        del mu
        adv = 0.3 + torch.randn(R, device=dev, generator=gen)
        ret = torch.randn(R, device=dev, generator=gen)
        live_b = torch.rand(R, device=dev, generator=gen) < 0.9
        live = live_b.to(torch.float32)
        idx = torch.randperm(R, device=dev, generator=gen)[:B].contiguous()
        shift = 0.02 * float(old.abs().mean())
        actor0 = old + shift * torch.randn(old.shape, device=dev, generator=gen)
    actor = actor0.clone().requires_grad_(True)
    critic = critic0.clone().requires_grad_(True)
    log_std = (ls_old + 0.01).requires_grad_(True)
    one = torch.ones((), dtype=torch.float32, device=dev)
    clip, vf_coef, ent_coef = 0.2, 0.5, 0.0
    P, Pv = actor.shape[0], critic.shape[0]
    out = torch.empty(P + Pv + A, dtype=torch.float64, device=dev)
    stats = torch.empty(8, dtype=torch.float64, device=dev)

    def device():
        env.ppo_grad(actor, critic, log_std, hidden, hidden, obs, act, logp_old, adv, ret, live=live_b, index=idx,
                     clip=clip, vf_coef=vf_coef, ent_coef=ent_coef, out=out, stats_out=stats)

    def torch_path():                                # gym_copter_amd/ppo.py's loop body, without the optimizer
        w = live[idx]
        wsum = torch.maximum(w.sum(), one)
        a_mb = adv[idx]
        a_mean = (a_mb * w).sum() / wsum
        a_std = (((a_mb - a_mean) ** 2 * w).sum() / wsum).sqrt()
        a_mb = (a_mb - a_mean) / (a_std + 1e-8)
        o_mb = obs[idx]
        logp = gaussian_logp(torch, act[idx], _forward(torch, actor, o_mb, hidden, od, A), log_std)
        ratio = torch.exp(logp - logp_old[idx])
        surr = torch.minimum(ratio * a_mb, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_mb)
        pol_loss = -(surr * w).sum() / wsum
        value = _forward(torch, critic, o_mb, hidden, od, 1)[:, 0]
        val_loss = 0.5 * (((value - ret[idx]) ** 2) * w).sum() / wsum
        entropy = log_std.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
        loss = pol_loss + vf_coef * val_loss - ent_coef * entropy
        actor.grad = critic.grad = log_std.grad = None
        loss.backward()

    fns = {"device": device, "torch": torch_path}
    for fn in fns.values():
        fn()
    got = torch.cat([actor.grad, critic.grad, log_std.grad]).double()
    err = float(((got - out).abs() / out.abs().clamp_min(1.0)).max())
    assert err < 1e-3, err                            # (the two sides compute the same gradient)
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(_time(fn))
    row = {"samples": B, "rows": R, "hidden": hidden, "rounds": rounds, "float32_scaled_distance": err}
    for name, ts in times.items():
        row[name + "_us"] = round(min(ts), 1)
        row[name + "_spread"] = round(max(ts) / min(ts) - 1, 4)
    row["torch_over_device"] = round(min(times["torch"]) / min(times["device"]), 2)
    return row


def iteration(rounds):
    """One iteration of gym_copter_amd.ppo at the driver's settings, ms, per update path: iterations = 3 less
    iterations = 1 over two, so that the optimizer's construction and the first call's allocations drop out."""
    import torch
    import gym_copter_amd
    from gym_copter_amd import mlp
    n, K, H = 8192, 64, 16
    out = {}
    for update in ("torch", "device"):
        env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32",
                                          autoreset_mode="next_step", seed=2, max_steps=1000)
        try:
            env.reset()
            gen = torch.Generator().manual_seed(11)
            actor = mlp.init(10, 4, H, generator=gen, out_bias=_hover(), out_scale=0.01)
            critic = mlp.init(10, 1, H, generator=gen, out_scale=0.01)
            log_std = torch.full((4,), math.log(0.1), dtype=torch.float32)

            def run(its):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gym_copter_amd.ppo(env, actor, critic, log_std, H, H, K, its, update=update)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            run(1)
            ts = [(run(3) - run(1)) / 2 for _ in range(rounds)]
            out[update + "_ms"] = round(min(ts), 3)
            out[update + "_spread"] = round(max(ts) / min(ts) - 1, 4)
            clock = env.clock_probe()
        finally:
            env.close()
    out["torch_over_device"] = round(out["torch_ms"] / out["device_ms"], 2)
    out["clock_mhz"] = round(clock / 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, nargs="*", default=[131072, 1048576, 4194304])
    ap.add_argument("--hidden", type=int, nargs="*", default=[0, 16, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_update_bench"))
    args = ap.parse_args()
    import gym_copter_amd
    rows = []
    lines = ["# tools/ppo_update_bench.py: Lander3D shapes, H = Hv; us per minibatch of B samples out of 4 B rows, best of %d "
             "interleaved rounds in one process, the rounds' spread (max / min - 1) beside each figure" % args.rounds]

    def save(record):
        with open(args.out + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(record, f, indent=1)
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=64, state_dtype="float32", seed=1)
    try:
        for B in args.samples:
            for H in args.hidden:
                r = measure(env, B, H, args.rounds)
                rows.append(r)
                lines.append("B %8d  H %2d: device %10.1f (+-%4.1f %%) | torch %10.1f (+-%4.1f %%) = %6.2f x device"
                             % (r["samples"], r["hidden"], r["device_us"], 100 * r["device_spread"], r["torch_us"],
                                100 * r["torch_spread"], r["torch_over_device"]))
                print(lines[-1], flush=True)
                save({"minibatch": rows})
    finally:
        env.close()
    it = iteration(args.rounds)
    lines.append("one ppo iteration, 8192 envs x K = 64, H = Hv = 16, 4 epochs x 4 minibatches, ms: update='torch' %.3f "
                 "(+-%4.1f %%) | update='device' %.3f (+-%4.1f %%) = torch / %.2f | clock %d MHz"
                 % (it["torch_ms"], 100 * it["torch_spread"], it["device_ms"], 100 * it["device_spread"],
                    it["torch_over_device"], it["clock_mhz"]))
    print(lines[-1], flush=True)
    save({"minibatch": rows, "iteration": it})


if __name__ == "__main__":
    main()
