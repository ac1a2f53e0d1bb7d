"""Time the Rauch-Tung-Striebel smoother kernel (cs_rollout_rts) against the chain a caller had before it.  Lander3D,
float64 storage, K = 64, M = 6 measured slots, substeps 1 and 10, at 65 536 and 1 048 576 envs.

For each configuration, in one process, interleaved over `--rounds` rounds, the best round kept per figure and the spread
(worst / best) beside it:
  rts     CopterVecEnv.rollout_rts(actions, filt, Q, x0, P0, tape=False) (float64: the smoothed means, variances and
          starting point; the covariance tape is not written, as the chain keeps none)                -> us per step
  ekf     CopterVecEnv.rollout_ekf(actions, z, H, r, Q, x0, P0, tape=True), the filter whose tapes it reads, for scale
                                                                                                       -> us per step
  chain   K x (step_jacobian at the filter's point + in torch: W = A P_f and P- = W A^T + Q by two bmm,
          torch.linalg.cholesky and cholesky_solve for G, then the mean's and the covariance's updates) -> us per step
Timed with torch.cuda events around device-synchronised windows.
After the rounds the chain's smoothed starting point is compared with the kernel's (to 1e-8), in a pass of the chain that
waits for the device after every step.

    python tools/rollout_rts_bench.py [--rounds 3] [--steps 64] [--envs 65536 1048576] [--out profiles/rollout_rts_bench]
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
        truth = env.rollout_states(a, {"x": x0, "status": st0}).x
        z = gym_copter_amd.measure(truth, H, r, 0)
        del truth
        Qd = torch.from_numpy(Q).to(dev)
        filt = env.rollout_ekf(a, z, H, r, Q, x0, P0, status0=st0, tape=True)     # (the env's buffers: the smoother's input)
        assert bool(filt.ok.all())
        res = env.rollout_rts(a, filt, Q, x0, P0, status0=st0, tape=False)
        assert bool(res.ok.all())

        def chain(sync=False):
            xs, Ps = filt.x[K - 1], filt.P_tape[K - 1]
            for j in range(K - 2, -2, -1):
                if j >= 0:
                    xf, Pf, point = filt.x[j], filt.P_tape[j], {"x": filt.x[j].T.contiguous(), "status": filt.status[j]}
                else:
                    xf, Pf, point = x0.T, P0, {"x": x0, "status": st0}
                A = env.step_jacobian(a[j + 1], state=point).dx
                W = torch.bmm(A, Pf)
                Pm = torch.bmm(W, A.transpose(1, 2)) + Qd
                G = torch.cholesky_solve(W, torch.linalg.cholesky(Pm))
                xs = xf + torch.bmm((xs - filt.x_pred[j + 1]).unsqueeze(1), G).squeeze(1)     # (G^T dx)^T = dx^T G
                Ps = Pf + torch.bmm(G.transpose(1, 2).contiguous(), torch.bmm(Ps - Pm, G))
                if sync:
                    torch.cuda.synchronize()
            return xs, Ps

        fns = {"rts": lambda: env.rollout_rts(a, filt, Q, x0, P0, status0=st0, tape=False),
               "ekf": lambda: env.rollout_ekf(a, z, H, r, Q, x0, P0, status0=st0, tape=True), "chain": chain}
        for name in ("rts", "ekf"):                           # warm-up (the chain's first round is its warm-up)
            fns[name]()
        best, worst = {}, {}
        for rnd in range(rounds + 1):
            for name, fn in fns.items():
                t = _time(fn)
                if rnd > 0 or name != "chain":
                    best[name] = min(best.get(name, t), t)
                    worst[name] = max(worst.get(name, t), t)
        # the chain computes what the kernel computes (checked in a run that waits for the device after every step; the
        # free-running sequence above is what is timed)
        cx, cP = chain(sync=True)
        res = env.rollout_rts(a, filt, Q, x0, P0, status0=st0, tape=False)
        ex = float((cx - res.x0.T).abs().max())
        eP = float((cP - res.P0).abs().max())
        assert ex < 1e-8 and eP < 1e-8, (ex, eP)
    finally:
        env.close()
    out = {"envs": n, "substeps": substeps, "K": K, "M": M}
    for name in fns:
        out[name + "_us_per_step"] = round(best[name] / K, 3)
        out[name + "_spread"] = round(worst[name] / best[name], 3)
    out["chain_over_rts"] = round(best["chain"] / best["rts"], 2)
    out["rts_over_ekf"] = round(best["rts"] / best["ekf"], 2)
    out["chain_minus_rts_x0"] = ex
    out["chain_minus_rts_P0"] = eP
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_rts_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  substeps %2d  K %d: rts %10.3f us/step (spread %.3f) | ekf with its tape %10.3f us/step "
                         "(%.3f) | chain %10.3f us/step (%.3f) = %.2fx the kernel"
                         % (n, substeps, args.steps, r["rts_us_per_step"], r["rts_spread"], r["ekf_us_per_step"],
                            r["ekf_spread"], r["chain_us_per_step"], r["chain_spread"], r["chain_over_rts"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("# tools/rollout_rts_bench.py: Lander3D, float64 storage, best of %d interleaved rounds "
                        "(spread = worst / best)\n" % args.rounds + "\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
