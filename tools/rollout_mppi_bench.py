"""Time one MPPI iteration on the MPPI kernels (cs_rollout_mppi_costs, cs_rollout_mppi_update) against the same
iteration done with what a caller had before them: rollout_states on an env of N x P tiled starts fed a torch-generated
noise tape, and torch reductions over its state tape.  Lander3D, float32 storage, K = 64, N in {256, 4 096} envs,
P in {256, 1 024} samples, substeps 1 and 10.

For each configuration, in one process, interleaved over `--rounds` rounds with the best round kept per figure:
  costs     CopterVecEnv.rollout_mppi_costs(actions, sigma, P, x_ref, Q, R, reward_weight=1)       -> us per iteration
  update    CopterVecEnv.rollout_mppi_update(actions, costs, sigma, lam)                           -> us per iteration
  baseline  noise = sigma randn [K, N P, A]; rollout_states(tiled actions + noise) on the N P env; the quadratic cost and
            the reward summed over the tape; softmin weights over P; the weighted mean of the noise -> us per iteration,
            with its rollout_states part alone beside it
  costs_smooth, update_smooth   the same two calls with knots=mppi_knots(K, hold) (the kernels of
            cs_rollout_mppi_costs_ex / cs_rollout_mppi_update_ex), in the same rounds -> us per iteration
Timed with torch.cuda events around device-synchronised windows.  The sample-step rate is N P K / costs.  The smooth
kernels against the white ones go to `--smooth-out`; --pairs-only leaves the torch baseline (and its N x P env) out.

    python tools/rollout_mppi_bench.py [--rounds 3] [--steps 64] [--hold 16] [--pairs-only]
                                       [--out profiles/rollout_mppi_bench] [--smooth-out profiles/rollout_mppi_smooth_bench]
"""
import argparse
import json
import os
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


def measure(n, P, substeps, K, rounds, hold=16, pairs_only=False):
    import numpy as np
    import torch
    import gym_copter_amd
    kw = dict(task="lander3d", state_dtype="float32", substeps=substeps, autoreset_mode="disabled", seed=1,
              max_steps=100000)
    env = gym_copter_amd.CopterVecEnv(num_envs=n, **kw)
    tiled = None if pairs_only else gym_copter_amd.CopterVecEnv(num_envs=n * P, **kw)
    try:
        env.reset()
        if tiled is not None:
            tiled.reset()
        dev = env.device
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.uniform(0.45, 0.6, (K, n, 4)).astype(np.float32)).to(dev)
        x0 = np.zeros((12, n))
        x0[4] = -rng.uniform(5, 20, n)
        state = {"x": torch.from_numpy(x0).to(dev), "status": torch.full((n,), 3, dtype=torch.uint8, device=dev)}
        big = None if pairs_only else {"x": state["x"].repeat(1, P).contiguous(),
                                       "status": state["status"].repeat(P).contiguous()}
        knots = gym_copter_amd.mppi_knots(K, hold)
        x_ref = torch.zeros((n, 12), dtype=torch.float64, device=dev)
        Q, R = np.eye(12), 0.1 * np.eye(4)
        Qd = torch.eye(12, dtype=torch.float64, device=dev)
        sigma, lam = 0.05, 1.0
        got = {}

        def costs():
            got["costs"] = env.rollout_mppi_costs(a, sigma, P, x_ref, Q, R, reward_weight=1.0, state=state).costs

        def update():
            env.rollout_mppi_update(a, got["costs"], sigma, lam)

        def costs_smooth():
            got["costs_s"] = env.rollout_mppi_costs(a, sigma, P, x_ref, Q, R, reward_weight=1.0, state=state,
                                                    knots=knots).costs

        def update_smooth():
            env.rollout_mppi_update(a, got["costs_s"], sigma, lam, knots=knots)

        def rollout():
            got["noise"] = sigma * torch.randn((K, n * P, 4), dtype=torch.float32, device=dev)
            got["acts"] = a.repeat(1, P, 1) + got["noise"]             # (sample-major, as costs [P,N])
            got["ro"] = tiled.rollout_states(got["acts"], big)

        def baseline():
            rollout()
            ro, xr = got["ro"], x_ref.repeat(P, 1)
            S = -ro.reward.sum(0)
            for k in range(K):                                    # (step by step: the whole tape at once needs 4 copies of it)
                dx, ak = ro.x[k] - xr, got["acts"][k].double()
                S += 0.5 * ((dx @ Qd) * dx).sum(-1) + 0.05 * (ak * ak).sum(-1)
            w = torch.softmax(-S.view(P, n) / lam, dim=0)
            step = (w[None, :, :, None] * got["noise"].view(K, P, n, 4).double()).sum(1)
            got["new"] = (a.double() + step).float().clamp_(0, 1)

        fns = {"costs": costs, "costs_smooth": costs_smooth, "update": update, "update_smooth": update_smooth}
        if not pairs_only:
            fns.update({"rollout": rollout, "baseline": baseline})
        for fn in fns.values():                                   # warm-up of every shape
            fn()
        best = {}
        for _ in range(rounds):
            for name, fn in fns.items():
                t = _time(fn)
                best[name] = min(best.get(name, t), t)
    finally:
        env.close()
        if tiled is not None:
            tiled.close()
    out = {"envs": n, "samples": P, "substeps": substeps, "K": K, "hold": hold}
    for name in fns:
        out[name + "_us"] = round(best[name], 1)
    out["iteration_us"] = round(best["costs"] + best["update"], 1)
    out["costs_us_per_step_per_1M"] = round(best["costs"] / K / (n * P / 2 ** 20), 3)
    out["sample_steps_per_s"] = round(n * P * K / best["costs"] * 1e6, -6)
    out["costs_smooth_over_white"] = round(best["costs_smooth"] / best["costs"], 3)
    out["update_smooth_over_white"] = round(best["update_smooth"] / best["update"], 3)
    if not pairs_only:
        out["rollout_us_per_step_per_1M"] = round(best["rollout"] / K / (n * P / 2 ** 20), 3)
        out["baseline_over_iteration"] = round(best["baseline"] / (best["costs"] + best["update"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--samples", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_mppi_bench"))
    ap.add_argument("--hold", type=int, default=16, help="steps between two knots of the smooth rows")
    ap.add_argument("--pairs-only", action="store_true", help="the white and smooth kernels only, no torch baseline")
    ap.add_argument("--smooth-out", default=os.path.join(ROOT, "profiles", "rollout_mppi_smooth_bench"))
    args = ap.parse_args()
    rows, lines, pairs = [], [], []
    for n in args.envs:
        for P in args.samples:
            for substeps in (1, 10):
                r = measure(n, P, substeps, args.steps, args.rounds, args.hold, args.pairs_only)
                rows.append(r)
                pairs.append("%5d envs x %4d samples  substeps %2d  K %d  hold %d: costs white %9.1f us, smooth %9.1f us "
                             "(%.3fx) | update white %8.1f us, smooth %8.1f us (%.3fx)"
                             % (n, P, substeps, args.steps, args.hold, r["costs_us"], r["costs_smooth_us"],
                                r["costs_smooth_over_white"], r["update_us"], r["update_smooth_us"],
                                r["update_smooth_over_white"]))
                print(pairs[-1], flush=True)
                with open(args.smooth_out + ".txt", "w") as f:
                    f.write("# tools/rollout_mppi_bench.py: Lander3D, float32 storage, the knot-noise kernels against the "
                            "white ones, each pair in one process, best of %d interleaved rounds\n" % args.rounds
                            + "\n".join(pairs) + "\n")
                if args.pairs_only:
                    continue
                lines.append("%5d envs x %4d samples  substeps %2d  K %d: costs %9.1f us (%6.2f us/step per 2^20 sample-envs, "
                             "%.3g sample-steps/s) + update %8.1f us = %9.1f us | baseline %10.1f us (its rollout_states "
                             "and noise %10.1f us, %6.2f us/step per 2^20) = %.2fx"
                             % (n, P, substeps, args.steps, r["costs_us"], r["costs_us_per_step_per_1M"],
                                r["sample_steps_per_s"], r["update_us"], r["iteration_us"], r["baseline_us"],
                                r["rollout_us"], r["rollout_us_per_step_per_1M"], r["baseline_over_iteration"]))
                print(lines[-1], flush=True)
                with open(args.out + ".txt", "w") as f:
                    f.write("# tools/rollout_mppi_bench.py: Lander3D, float32 storage, best of %d interleaved rounds\n"
                            % args.rounds + "\n".join(lines) + "\n")
                with open(args.out + ".json", "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
