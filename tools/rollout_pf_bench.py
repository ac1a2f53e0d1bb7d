"""Time the bootstrap particle filter kernel (cs_rollout_pf) against the chain a caller had before it, and one
demonstration.  Lander3D, float64 storage, K steps, M = 6 measurements, in one process, best of interleaved rounds with
their spread (worst / best):

  pf      CopterVecEnv.rollout_pf(actions, z, H, r, Q, x0, P0, particles=P) (no tapes)                -> us per step
  chain   per step: a K = 1 rollout_states on an env of N P lanes from the explicit particles, torch.randn noise
          coloured by Lq, the weights (a matrix product, logsumexp), ess, cumsum / searchsorted / gather -- the route
          DESIGN.md section 14 measured for MPPI
  ekf     CopterVecEnv.rollout_ekf on the same data, for scale
  states  the open-loop forward rollout_states on the N envs, for scale

    python tools/rollout_pf_bench.py [--rounds 3] [--steps 64] [--out profiles/rollout_pf_bench]
    python tools/rollout_pf_bench.py --demo        # a descent to touchdown with altitude-only measurements (not timed)

Writes <out>.txt and <out>.json (the demonstration: <out>_demo.txt)."""
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


def _env(n, substeps):
    import gym_copter_amd
    return gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float64", substeps=substeps,
                                       autoreset_mode="disabled", seed=1, max_steps=100000)


def measure(n, P, substeps, K, rounds):
    import numpy as np
    import torch
    import gym_copter_amd
    env, tiled = _env(n, substeps), _env(n * P, substeps)
    try:
        env.reset()
        tiled.reset()
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
        Qv = np.full(12, 1e-4)
        P0 = (0.01 * torch.eye(12, dtype=torch.float64, device=dev)).expand(n, 12, 12).contiguous()
        state = {"x": x0, "status": st0}
        truth = env.rollout_states(a, state).x
        z = gym_copter_amd.measure(truth, H, r, 0)
        Hd, rd = (torch.from_numpy(m).to(dev) for m in (H, r))
        sq = torch.from_numpy(np.sqrt(Qv)).to(dev)
        res = env.rollout_pf(a, z, H, r, Qv, x0, P0, particles=P, status0=st0)
        assert bool(res.ok.all())
        share = float(res.resampled.double().mean())

        def chain():
            X = x0.T[:, None, :] + torch.randn((n, P, 12), dtype=torch.float64, device=dev) * 0.1
            S = st0[:, None].expand(n, P).contiguous()
            lw = torch.full((n, P), -float(np.log(P)), dtype=torch.float64, device=dev)
            slots = torch.arange(P, dtype=torch.float64, device=dev)
            for k in range(K):
                one = tiled.rollout_states(a[k:k + 1].repeat_interleave(P, dim=1),
                                           {"x": X.reshape(n * P, 12).T.contiguous(), "status": S.reshape(n * P)})
                X = one.x[0].reshape(n, P, 12) + torch.randn((n, P, 12), dtype=torch.float64, device=dev) * sq
                S = one.status[0].reshape(n, P)
                nu = z[k][:, None, :] - X @ Hd.T
                lw = lw - 0.5 * (nu * nu / rd).sum(dim=2)
                lw = lw - torch.logsumexp(lw, dim=1, keepdim=True)
                w = torch.exp(lw)
                ess = 1.0 / (w * w).sum(dim=1)
                cum = torch.cumsum(w, dim=1)
                u = (slots + torch.rand((n, 1), dtype=torch.float64, device=dev)) / P
                anc = torch.searchsorted(cum, u.expand(n, P).contiguous()).clamp_(max=P - 1)
                anc = torch.where((ess < 0.5 * P)[:, None], anc, torch.arange(P, device=dev)[None])
                X = torch.gather(X, 1, anc[:, :, None].expand(n, P, 12))
                S = torch.gather(S, 1, anc)
                lw = torch.where((ess < 0.5 * P)[:, None], torch.full_like(lw, -float(np.log(P))), lw)
                (w[:, :, None] * X).sum(dim=1)                                       # the estimate

        fns = {"pf": lambda: env.rollout_pf(a, z, H, r, Qv, x0, P0, particles=P, status0=st0),
               "ekf": lambda: env.rollout_ekf(a, z, H, r, np.diag(Qv), x0, P0, status0=st0),
               "states": lambda: env.rollout_states(a, state), "chain": chain}
        for name in ("pf", "ekf", "states"):                  # warm-up (the chain's first round is its warm-up)
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
        tiled.close()
    out = {"envs": n, "particles": P, "substeps": substeps, "K": K, "M": M, "resampled_share": round(share, 3)}
    for name in fns:
        out[name + "_us_per_step"] = round(best[name] / K, 3)
        out[name + "_spread"] = round(worst[name] / best[name], 3)
    out["chain_over_pf"] = round(best["chain"] / best["pf"], 2)
    out["pf_over_ekf"] = round(best["pf"] / best["ekf"], 2)
    out["pf_us_per_step_per_2^20_particle_envs"] = round(best["pf"] / K * (1 << 20) / (n * P), 3)
    return out


def demo(out_path, n=256, P=1024, K=96):
    """A Lander3D descent to touchdown, altitude the only measurement: the belief straddles the ground in the last
    centimetres.  The particle filter's and the EKF's RMSE and calibration (RMSE / sqrt(mean var)) of z and dz over the
    steps from 10 before the first touchdown of the truth to the end, and the share of (step, env) pairs in which the
    particles are on both sides of the touchdown (some AIRBORNE, some not)."""
    import numpy as np
    import torch
    env = _env(n, 1)
    try:
        env.reset()
        dev = env.device
        rng = np.random.default_rng(3)
        hover = 0.0166
        a = torch.from_numpy((hover * rng.uniform(0.97, 1.03, (K, n, 4))).astype(np.float32)).to(dev)
        p0 = np.full(12, 1e-4)
        p0[4], p0[5] = 0.1 ** 2, 0.3 ** 2
        xh = np.zeros((12, n))
        xh[4], xh[5] = -0.6, 0.9                                       # 60 cm up, descending at 0.9 m/s: crash above 1
        x0 = xh + np.sqrt(p0)[:, None] * rng.standard_normal((12, n))
        st0 = np.full(n, 3, np.uint8)
        ro = env.rollout_states(a, {"x": x0, "status": st0})
        truth, tstat = ro.x.clone(), ro.status.clone()
        H = np.zeros((1, 12))
        H[0, 4] = 1.0
        r = np.array([0.05 ** 2])
        z = torch.from_numpy(rng.standard_normal((K, n, 1))).to(dev) * 0.05 + truth[:, :, 4:5]
        P0 = torch.from_numpy(np.repeat(np.diag(p0)[None], n, axis=0)).to(dev)
        Qv = np.full(12, 1e-6)
        xhd = torch.from_numpy(xh).to(dev)
        res = env.rollout_pf(a, z, H, r, Qv, xhd, P0, particles=P, tape=True)
        ekf = env.rollout_ekf(a, z, H, r, np.diag(Qv), xhd, P0)
        touched = (tstat != 3).any(dim=1).nonzero()
        k0 = max(int(touched[0]) - 10, 0) if touched.numel() else 0
        air = (res.pstatus_tape == 3)
        straddle = (air.any(dim=2) & (~air).any(dim=2))[k0:]
        lines = ["# tools/rollout_pf_bench.py --demo: Lander3D, %d envs, %d particles, K %d, altitude-only z (sigma 0.05 m); "
                 "steps %d .. %d" % (n, P, K, k0 + 1, K),
                 "truth at the end: %d landed, %d crashed, %d leveling, %d airborne"
                 % tuple(int((tstat[-1] == s).sum()) for s in (1, 0, 2, 3)),
                 "share of (step, env) pairs whose particles straddle the touchdown: %.3f; of envs that ever do: %.3f"
                 % (float(straddle.double().mean()), float(straddle.any(dim=0).double().mean()))]
        for name, x, var in (("pf ", res.x, res.var), ("ekf", ekf.x, ekf.var)):
            err = (x - truth)[k0:]
            rmse = torch.sqrt((err ** 2).mean(dim=(0, 1)))
            cal = rmse / torch.sqrt(var[k0:].mean(dim=(0, 1)))
            lines.append("%s: rmse z %.4f m, dz %.4f m/s; rmse / sqrt(mean var) z %.2f, dz %.2f; status of the estimate "
                         "equals the truth's in %.3f of the pairs"
                         % (name, float(rmse[4]), float(rmse[5]), float(cal[4]), float(cal[5]),
                            float((res.status[k0:] == tstat[k0:]).double().mean()) if name == "pf " else
                            float((ekf.status[k0:] == tstat[k0:]).double().mean())))
        print("\n".join(lines))
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[256, 4096])
    ap.add_argument("--particles", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_pf_bench"))
    args = ap.parse_args()
    if args.demo:
        demo(args.out + "_demo.txt")
        return
    rows, lines = [], []
    for n in args.envs:
        for P in args.particles:
            for substeps in (1, 10):
                r = measure(n, P, substeps, args.steps, args.rounds)
                rows.append(r)
                lines.append("%6d envs x %4d particles  substeps %2d  K %d  M %d: pf %10.3f us/step (spread %.3f) = %8.3f per "
                             "2^20 particle-envs | chain %11.3f us/step (%.3f) = %.2fx the kernel | ekf %9.3f (%.3f) | "
                             "open-loop forward %8.3f (%.3f) | resampled %.2f of the steps"
                             % (n, P, substeps, args.steps, r["M"], r["pf_us_per_step"], r["pf_spread"],
                                r["pf_us_per_step_per_2^20_particle_envs"], r["chain_us_per_step"], r["chain_spread"],
                                r["chain_over_pf"], r["ekf_us_per_step"], r["ekf_spread"], r["states_us_per_step"],
                                r["states_spread"], r["resampled_share"]))
                print(lines[-1], flush=True)
                with open(args.out + ".txt", "w") as f:
                    f.write("# tools/rollout_pf_bench.py: Lander3D, float64 storage, best of %d interleaved rounds "
                            "(spread = worst / best)\n" % args.rounds + "\n".join(lines) + "\n")
                with open(args.out + ".json", "w") as f:
                    json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
