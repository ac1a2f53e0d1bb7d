"""Time the iLQR kernels (cs_rollout_lqr, cs_rollout_feedback_states) against what a caller had before them: the
one-step Jacobian chain with the Riccati recursion in torch.  Lander3D, float32 storage, K = 64, substeps 1 and 10, at
65 536 and 1 048 576 envs.

For each configuration, in one process, interleaved over `--rounds` rounds with the best round kept per figure:
  backward  CopterVecEnv.rollout_lqr(actions, tape, Q, R, q, r) (float64 gains)      -> us per step
  forward   CopterVecEnv.rollout_feedback_states(actions, tape, gains, alpha)        -> us per step
  states    CopterVecEnv.rollout_states(actions) (the open-loop forward, for scale)  -> us per step
  chain     K x (step_jacobian + step) + per step the torch recursion on the blocks: bmm products for Qxx, Qux, Quu,
            torch.linalg.cholesky_ex + cholesky_solve for the gains, bmm for S.  ONE Jacobian buffer is reused for every
            step (storing K of them needs K x N x 1.5 KB), so this is a lower bound of what the chain costs.
Timed with torch.cuda events around device-synchronised windows.

    python tools/rollout_lqr_bench.py [--rounds 3] [--steps 64] [--out profiles/rollout_lqr_bench]
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
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", substeps=substeps,
                                      autoreset_mode="disabled", seed=1, max_steps=100000)
    try:
        env.reset()
        dev = env.device
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, 4)).astype(np.float32)).to(dev)
        q = torch.randn((K, n, 12), dtype=torch.float64, device=dev)
        r = torch.randn((K, n, 4), dtype=torch.float64, device=dev)
        Q, R = np.eye(12), np.eye(4)
        Qd, Rd = torch.eye(12, dtype=torch.float64, device=dev), torch.eye(4, dtype=torch.float64, device=dev)
        tape = env.rollout_states(a)
        gains = env.rollout_lqr(a, tape, Q, R, q=q, r=r)
        assert bool(gains.ok.all())
        alpha = torch.full((n,), 0.5, dtype=torch.float64, device=dev)

        def chain():
            S = torch.zeros((n, 12, 12), dtype=torch.float64, device=dev)
            s = torch.zeros((n, 12, 1), dtype=torch.float64, device=dev)
            for k in range(K):
                env.step_jacobian(a[k])
                env.step(a[k])
            jac = env.step_jacobian(a[0])
            Am, Bm = jac.dx, jac.du
            AT, BT = Am.transpose(1, 2), Bm.transpose(1, 2)
            for k in range(K - 1, -1, -1):
                V, v = S + Qd, s + q[k].unsqueeze(-1)
                VA = torch.bmm(V, Am)
                Qxx, Qux = torch.bmm(AT, VA), torch.bmm(BT, VA)
                Quu = Rd + torch.bmm(BT, torch.bmm(V, Bm))
                Qx, Qu = torch.bmm(AT, v), r[k].unsqueeze(-1) + torch.bmm(BT, v)
                L, _ = torch.linalg.cholesky_ex(Quu)
                Kd = -torch.cholesky_solve(torch.cat([Qux, Qu], dim=2), L)
                Kk, dk = Kd[:, :, :12], Kd[:, :, 12:]
                KT = Kk.transpose(1, 2)
                S = Qxx + torch.bmm(KT, torch.bmm(Quu, Kk) + Qux) + torch.bmm(Qux.transpose(1, 2), Kk)
                s = Qx + torch.bmm(KT, torch.bmm(Quu, dk) + Qu) + torch.bmm(Qux.transpose(1, 2), dk)

        fns = {"bwd": lambda: env.rollout_lqr(a, tape, Q, R, q=q, r=r),
               "fwd": lambda: env.rollout_feedback_states(a, tape, gains, alpha),
               "states": lambda: env.rollout_states(a), "chain": chain}
        for name in ("bwd", "fwd", "states"):                 # warm-up (the chain's first round is its warm-up)
            fns[name]()
        best = {}
        for rnd in range(rounds + 1):
            for name, fn in fns.items():
                t = _time(fn)
                if rnd > 0 or name != "chain":
                    best[name] = min(best.get(name, t), t)
    finally:
        env.close()
    out = {"envs": n, "substeps": substeps, "K": K}
    for name in fns:
        out[name + "_us_per_step"] = round(best[name] / K, 3)
    out["chain_over_bwd"] = round(best["chain"] / best["bwd"], 2)
    out["chain_over_bwd_plus_fwd"] = round(best["chain"] / (best["bwd"] + best["fwd"]), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_lqr_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  substeps %2d  K %d: backward %10.3f us/step | feedback forward %9.3f us/step "
                         "(open-loop forward %9.3f) | chain %10.3f us/step = %.2fx the backward, %.2fx backward + forward"
                         % (n, substeps, args.steps, r["bwd_us_per_step"], r["fwd_us_per_step"], r["states_us_per_step"],
                            r["chain_us_per_step"], r["chain_over_bwd"], r["chain_over_bwd_plus_fwd"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("# tools/rollout_lqr_bench.py: Lander3D, float32 storage, best of %d interleaved rounds\n"
                        % args.rounds + "\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
