"""Time the control-limited iLQR kernels (cs_ilqr_box_backward, cs_ilqr_box_forward) beside the unconstrained ones they
extend (cs_rollout_lqr, cs_rollout_feedback_states), in the same process: Lander3D, float32 storage, K = 64, substeps 1
and 10, at 65 536 and 1 048 576 envs.  The box is hover x (1 +- 0.3) around nominal motors drawn from hover x (0.72,
1.33), with cost gradients scaled so that the box binds in part of the (step, env) pairs (the share is reported).

For each configuration, interleaved over `--rounds` rounds after one warm-up call of each, the best round kept per
figure and the spread (worst round / best round - 1) beside it:
  lqr       CopterVecEnv.rollout_lqr(actions, tape, Q, R, q, r)                        -> us per step
  box       CopterVecEnv.rollout_lqr_box(actions, tape, Q, R, lo, hi, q, r)            -> us per step
  box_inf   the same with lo = -inf, hi = +inf (one iteration per step, nothing clamped)
  fwd       CopterVecEnv.rollout_feedback_states(actions, tape, gains, alpha)          -> us per step
  box_fwd   CopterVecEnv.rollout_feedback_box_states(actions, tape, gains, alpha, lo, hi)
Timed with torch.cuda events around device-synchronised windows.

    python tools/ilqr_box_bench.py [--rounds 3] [--steps 64] [--out profiles/ilqr_box_bench]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOVER = 0.016560178212092172     # the motor value at which the default vehicle hovers


def _time(fn):
    import torch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3          # us


def measure(n, substeps, K, rounds):
    import numpy as np
    import torch
    import gym_copter_amd
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", substeps=substeps,
                                      autoreset_mode="disabled", seed=1, max_steps=100000)
    try:
        env.reset()
        dev = env.device
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, 4)).astype(np.float32)).to(dev)
        q = 0.03 * torch.randn((K, n, 12), dtype=torch.float64, device=dev)
        r = 0.03 * torch.randn((K, n, 4), dtype=torch.float64, device=dev)
        Q, R = np.eye(12), np.eye(4)
        lo, hi = np.float32(0.7 * HOVER), np.float32(1.3 * HOVER)
        inf = float("inf")
        tape = env.rollout_states(a)
        gains = env.rollout_lqr_box(a, tape, Q, R, lo, hi, q=q, r=r)
        not_ok = float((~gains.ok).double().mean())
        share = float((gains.clamped != 0).double().mean())
        iters = float(gains.iters.double().mean())
        gains = type(gains)(*(t.clone() for t in gains))
        alpha = torch.full((n,), 0.5, dtype=torch.float64, device=dev)
        fns = {"lqr": lambda: env.rollout_lqr(a, tape, Q, R, q=q, r=r),
               "box": lambda: env.rollout_lqr_box(a, tape, Q, R, lo, hi, q=q, r=r),
               "box_inf": lambda: env.rollout_lqr_box(a, tape, Q, R, -inf, inf, q=q, r=r),
               "fwd": lambda: env.rollout_feedback_states(a, tape, gains, alpha),
               "box_fwd": lambda: env.rollout_feedback_box_states(a, tape, gains, alpha, lo, hi)}
        for fn in fns.values():
            fn()
        times = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                times[name].append(_time(fn))
    finally:
        env.close()
    out = {"envs": n, "substeps": substeps, "K": K, "pairs_clamped": round(share, 4), "mean_iters": round(iters, 3),
           "envs_not_ok": not_ok}
    for name, ts in times.items():
        out[name + "_us_per_step"] = round(min(ts) / K, 3)
        out[name + "_spread"] = round(max(ts) / min(ts) - 1.0, 4)
    out["box_over_lqr"] = round(min(times["box"]) / min(times["lqr"]), 4)
    out["box_inf_over_lqr"] = round(min(times["box_inf"]) / min(times["lqr"]), 4)
    out["box_fwd_over_fwd"] = round(min(times["box_fwd"]) / min(times["fwd"]), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ilqr_box_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  substeps %2d  K %d  (%.1f %% of pairs clamped, %.2f iterations per step, ok = 0 in %.4f %% "
                         "of the envs): backward "
                         "%10.3f us/step (spread %.1f %%) | box %10.3f (%.1f %%) = %.3fx | box, infinite bounds %10.3f "
                         "(%.1f %%) = %.3fx | forward %8.3f (%.1f %%) | box forward %8.3f (%.1f %%) = %.3fx"
                         % (n, substeps, args.steps, 100 * r["pairs_clamped"], r["mean_iters"], 100 * r["envs_not_ok"],
                            r["lqr_us_per_step"],
                            100 * r["lqr_spread"], r["box_us_per_step"], 100 * r["box_spread"], r["box_over_lqr"],
                            r["box_inf_us_per_step"], 100 * r["box_inf_spread"], r["box_inf_over_lqr"],
                            r["fwd_us_per_step"], 100 * r["fwd_spread"], r["box_fwd_us_per_step"],
                            100 * r["box_fwd_spread"], r["box_fwd_over_fwd"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("# tools/ilqr_box_bench.py: Lander3D, float32 storage, best of %d interleaved rounds (spread: worst "
                        "round over best - 1)\n" % args.rounds + "\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
