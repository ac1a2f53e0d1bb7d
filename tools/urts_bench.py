"""Time the unscented Rauch-Tung-Striebel smoother kernel (cs_urts_smooth) beside the extended smoother and the filter
whose tapes it reads.  Lander3D, float64 storage, K = 64, M = 6 measured slots, substeps 1 and 10, at 65 536 and
1 048 576 envs, the same inputs for all three.

For each configuration, in one process, interleaved over `--rounds` rounds, the best round kept per figure and the spread
(worst / best) beside it:
  urts    CopterVecEnv.rollout_urts(actions, ukf's result, Q, x0, P0, tape=False) (float64: the smoothed means, variances
          and starting point; no covariance tape)                                                     -> us per step
  rts     CopterVecEnv.rollout_rts(actions, ekf's result, Q, x0, P0, tape=False), the extended smoother on the extended
          filter's tapes of the same measurements                                                     -> us per step
  ukf     CopterVecEnv.rollout_ukf(actions, z, H, r, Q, x0, P0, tape=True), the filter whose tapes urts reads
                                                                                                       -> us per step
Timed with torch.cuda events around device-synchronised windows.

    python tools/urts_bench.py [--rounds 3] [--steps 64] [--envs 65536 1048576] [--out profiles/urts_bench]
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


def measure(n, substeps, K, rounds):
    import numpy as np
    import torch
    import gym_copter_amd
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float64", substeps=substeps,
                                      autoreset_mode="disabled", seed=1, max_steps=100000)
    try:
        env.reset()
        dev = env.device
        rng = np.random.default_rng(0)
        M = 6
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, 4)).astype(np.float32)).to(dev)
        x0 = torch.zeros((12, n), dtype=torch.float64, device=dev)
        x0[4] = -10.0
        st0 = torch.full((n,), 3, dtype=torch.uint8, device=dev)                  # AIRBORNE
        H = np.zeros((M, 12))
        H[np.arange(M), [0, 2, 4, 6, 8, 10]] = 1.0
        r = np.array([0.01, 0.01, 0.01, 1e-4, 1e-4, 1e-4])
        Q = 1e-6 * np.eye(12)
        P0 = (0.1 * torch.eye(12, dtype=torch.float64, device=dev)).expand(n, 12, 12).contiguous()
        z = gym_copter_amd.measure(env.rollout_states(a, {"x": x0, "status": st0}).x, H, r, 0)
        # (the env's buffers are the smoothers' inputs: each filter keeps its own, and the timed filter call rewrites the
        # same values)
        fe = env.rollout_ekf(a, z, H, r, Q, x0, P0, status0=st0, tape=True)
        fu = env.rollout_ukf(a, z, H, r, Q, x0, P0, status0=st0, tape=True)
        assert bool(fe.ok.all()) and bool(fu.ok.all())
        fns = {"urts": lambda: env.rollout_urts(a, fu, Q, x0, P0, status0=st0, tape=False),
               "rts": lambda: env.rollout_rts(a, fe, Q, x0, P0, status0=st0, tape=False),
               "ukf": lambda: env.rollout_ukf(a, z, H, r, Q, x0, P0, status0=st0, tape=True)}
        for name in fns:                                     # warm-up
            res = fns[name]()
            assert bool(res.ok.all()), name
        best, worst = {}, {}
        for _ in range(rounds):
            for name, fn in fns.items():
                t = _time(fn)
                best[name] = min(best.get(name, t), t)
                worst[name] = max(worst.get(name, t), t)
        # the two smoothers estimate the same starting point from the same measurements (free flight: no branch is
        # straddled, so they differ by the filters' second-order terms only)
        su, se = fns["urts"](), fns["rts"]()
        gap = float((su.x0 - se.x0).abs().max())
    finally:
        env.close()
    out = {"envs": n, "substeps": substeps, "K": K, "M": M}
    for name in fns:
        out[name + "_us_per_step"] = round(best[name] / K, 3)
        out[name + "_spread"] = round(worst[name] / best[name], 3)
    out["urts_over_rts"] = round(best["urts"] / best["rts"], 2)
    out["urts_over_ukf"] = round(best["urts"] / best["ukf"], 2)
    out["urts_minus_rts_x0"] = gap
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "urts_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  substeps %2d  K %d: urts %10.3f us/step (spread %.3f) | rts on the ekf's tapes %10.3f "
                         "us/step (%.3f) | ukf with its tape %10.3f us/step (%.3f) | urts = %.2fx rts, %.2fx ukf"
                         % (n, substeps, args.steps, r["urts_us_per_step"], r["urts_spread"], r["rts_us_per_step"],
                            r["rts_spread"], r["ukf_us_per_step"], r["ukf_spread"], r["urts_over_rts"], r["urts_over_ukf"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("# tools/urts_bench.py: Lander3D, float64 storage, no covariance tape, best of %d interleaved rounds "
                        "(spread = worst / best)\n" % args.rounds + "\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
