"""Time the extended Kalman filter kernel (cs_rollout_ekf) against the chain a caller had before it.  Lander3D, float64
storage, K = 64, M = 6 measured slots, substeps 1 and 10, at 65 536 and 1 048 576 envs.

For each configuration, in one process, interleaved over `--rounds` rounds, the best round kept per figure and the spread
(worst / best) beside it:
  ekf     CopterVecEnv.rollout_ekf(actions, z, H, r, Q, x0, P0) (float64, no P tape)        -> us per step
  states  CopterVecEnv.rollout_states(actions, state) (the open-loop forward, for scale)     -> us per step
  chain   K x (step_jacobian at the explicit point + a one-step rollout_states from it + in torch: P- = A P A^T + Q by two
          bmm, then the M sequential scalar updates as batched matrix-vector products)      -> us per step
Timed with torch.cuda events around device-synchronised windows.

    python tools/rollout_ekf_bench.py [--rounds 3] [--steps 64] [--out profiles/rollout_ekf_bench]
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
        state = {"x": x0, "status": st0}
        truth = env.rollout_states(a, state).x
        z = gym_copter_amd.measure(truth, H, r, 0)
        Hd, rd, Qd = (torch.from_numpy(m).to(dev) for m in (H, r, Q))
        res = env.rollout_ekf(a, z, H, r, Q, x0, P0, status0=st0)
        assert bool(res.ok.all())

        def chain():
            x, P, st = x0, P0, st0
            for k in range(K):
                point = {"x": x, "status": st}
                A = env.step_jacobian(a[k], state=point).dx
                one = env.rollout_states(a[k:k + 1], point)
                xm, st = one.x[0], one.status[0]
                P = torch.bmm(torch.bmm(A, P), A.transpose(1, 2)) + Qd
                for i in range(M):
                    h = Hd[i]
                    p = P @ h
                    s = p @ h + rd[i]
                    nu = z[k, :, i] - xm @ h
                    g = p / s.unsqueeze(1)
                    xm = xm + g * nu.unsqueeze(1)
                    P = P - g.unsqueeze(2) * p.unsqueeze(1)
                x = xm.T.contiguous()

        fns = {"ekf": lambda: env.rollout_ekf(a, z, H, r, Q, x0, P0, status0=st0),
               "states": lambda: env.rollout_states(a, state), "chain": chain}
        for name in ("ekf", "states"):                        # warm-up (the chain's first round is its warm-up)
            fns[name]()
        best, worst = {}, {}
        for rnd in range(rounds + 1):
            for name, fn in fns.items():
                t = _time(fn)
                if rnd > 0 or name != "chain":
                    best[name] = min(best.get(name, t), t)
                    worst[name] = max(worst.get(name, t), t)
    finally:
        env.close()
    out = {"envs": n, "substeps": substeps, "K": K, "M": M}
    for name in fns:
        out[name + "_us_per_step"] = round(best[name] / K, 3)
        out[name + "_spread"] = round(worst[name] / best[name], 3)
    out["chain_over_ekf"] = round(best["chain"] / best["ekf"], 2)
    out["ekf_over_states"] = round(best["ekf"] / best["states"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_ekf_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  substeps %2d  K %d  M %d: ekf %10.3f us/step (spread %.3f) | open-loop forward %9.3f "
                         "us/step (%.3f) | chain %10.3f us/step (%.3f) = %.2fx the kernel"
                         % (n, substeps, args.steps, r["M"], r["ekf_us_per_step"], r["ekf_spread"],
                            r["states_us_per_step"], r["states_spread"], r["chain_us_per_step"], r["chain_spread"],
                            r["chain_over_ekf"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("# tools/rollout_ekf_bench.py: Lander3D, float64 storage, best of %d interleaved rounds "
                        "(spread = worst / best)\n" % args.rounds + "\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
