"""Time the output-feedback kernel (cs_rollout_lqg) against the filter alone and against the chain a caller had before it.
Lander3D, float64 storage, K = 64, M = 6 measured slots, substeps 1 and 10, at 65 536 and 1 048 576 envs.

For each configuration, in one process, interleaved over `--rounds` rounds, the best round kept per figure and the spread
(worst / best) beside it:
  lqg     CopterVecEnv.rollout_lqg(actions, gains, xbar, noise, H, r, Q, xhat0, P0, state=) (float64, no P tape)
                                                                                             -> us per step
  ekf     CopterVecEnv.rollout_ekf on the same tapes: the call's own actions_out and z     -> us per step
  chain   K x (the law in torch at the estimate, a one-step rollout_states of the truth under it, the measurement in
          torch, a one-step rollout_ekf under the same action): the per-step chain the call replaces
                                                                                             -> us per step
Timed with torch.cuda events around device-synchronised windows.

    python tools/rollout_lqg_bench.py [--rounds 3] [--steps 64] [--out profiles/rollout_lqg_bench]
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
        M, A = 6, 4
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, A)).astype(np.float32)).to(dev)
        x0 = torch.zeros((12, n), dtype=torch.float64, device=dev)
        x0[4] = -10.0
        st0 = torch.full((n,), 3, dtype=torch.uint8, device=dev)                  # AIRBORNE
        H = np.zeros((M, 12))
        H[np.arange(M), [0, 2, 4, 6, 8, 10]] = 1.0
        r = np.array([0.01, 0.01, 0.01, 1e-4, 1e-4, 1e-4])
        Q = 1e-6 * np.eye(12)
        P0 = (0.1 * torch.eye(12, dtype=torch.float64, device=dev)).expand(n, 12, 12).contiguous()
        state = {"x": x0, "status": st0}
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        xhat0 = x0 + 0.1 * torch.randn((12, n), generator=gen, dtype=torch.float64, device=dev)
        gains = 1e-3 * torch.randn((K, n, A, 12), generator=gen, dtype=torch.float64, device=dev)
        nominal = env.rollout_states(a, state)
        xbar = torch.cat([x0.T[None], nominal.x[:-1]]).contiguous()
        noise = gym_copter_amd.measurement_noise(K, n, r, 0, device=dev)
        Hd = torch.from_numpy(H).to(dev)
        res = env.rollout_lqg(a, gains, xbar, noise, H, r, Q, xhat0, P0, status0=st0, state=state)
        assert bool(res.filter.ok.all())
        acts, z = res.actions.clone(), res.z.clone()

        def chain():
            xh, P, fst = xhat0, P0, st0
            xt, stt = x0, st0
            for k in range(K):
                u = a[k].double() + torch.einsum("naj,nj->na", gains[k], xh.T - xbar[k])
                act = u.float()[None]
                one = env.rollout_states(act, {"x": xt, "status": stt})
                xt, stt = one.x[0].T.contiguous(), one.status[0].clone()
                zk = (xt.T @ Hd.T + noise[k])[None]
                f = env.rollout_ekf(act, zk, H, r, Q, xh, P, status0=fst)
                xh, P, fst = f.x[0].T.contiguous(), f.P.clone(), f.status[0].clone()

        fns = {"lqg": lambda: env.rollout_lqg(a, gains, xbar, noise, H, r, Q, xhat0, P0, status0=st0, state=state),
               "ekf": lambda: env.rollout_ekf(acts, z, H, r, Q, xhat0, P0, status0=st0), "chain": chain}
        for name in ("lqg", "ekf"):                           # warm-up (the chain's first round is its warm-up)
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
    out["chain_over_lqg"] = round(best["chain"] / best["lqg"], 2)
    out["lqg_over_ekf"] = round(best["lqg"] / best["ekf"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_lqg_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            lines.append("%8d envs  substeps %2d  K %d  M %d: lqg %10.3f us/step (spread %.3f) = %.3fx the filter alone | "
                         "ekf %10.3f us/step (%.3f) | chain %10.3f us/step (%.3f) = %.2fx the kernel"
                         % (n, substeps, args.steps, r["M"], r["lqg_us_per_step"], r["lqg_spread"], r["lqg_over_ekf"],
                            r["ekf_us_per_step"], r["ekf_spread"], r["chain_us_per_step"], r["chain_spread"],
                            r["chain_over_lqg"]))
            print(lines[-1], flush=True)
            with open(args.out + ".txt", "w") as f:
                f.write("# tools/rollout_lqg_bench.py: Lander3D, float64 storage, best of %d interleaved rounds "
                        "(spread = worst / best)\n" % args.rounds + "\n".join(lines) + "\n")
            with open(args.out + ".json", "w") as f:
                json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
