"""Time the backward-simulation particle smoother kernel (cs_pf_smooth) beside the particle filter whose tapes it reads.
Lander3D, float64 storage, N envs, K steps, M = 6 measurements, in one process, best of interleaved rounds with their
spread (worst / best):

  pf      CopterVecEnv.rollout_pf(actions, z, H, r, Q, x0, P0, particles=P, tape=True)                -> us per env-step
  smooth  CopterVecEnv.rollout_pf_smooth(actions, filt, Q, paths=S) on those tapes (no diagnostic tapes)  -> us per env-step

and, from the shapes, what the backward weights need per env-step: S P (12 sub + 12 mul + 12 add) float64 operations
and S P 12 float64 reads of the LDS.  One workgroup runs one env on one CU, so a CU's rate is that count over the call's
time per step (every env's workgroup runs at once while N <= 256).  The bounds of one CU at 2.4 GHz: 64 float64 vector
operations per clock (half the float32 vector rate) = 153.6 Gop/s, and 256 B of LDS reads per clock = 614 GB/s.

    python tools/pf_smooth_bench.py [--rounds 5] [--envs 32] [--steps 32] [--out profiles/pf_smooth_bench]

Writes <out>.txt and <out>.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CU_F64_OPS = 64 * 2.4e9        # float64 vector operations per second and CU (an fma counts once: nothing here is fused)
CU_LDS_BYTES = 256 * 2.4e9     # LDS bytes read per second and CU


def _time(fn):
    import torch
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3          # us


def measure(n, P, paths, K, rounds, repeat):
    import numpy as np
    import torch
    import gym_copter_amd
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float64", autoreset_mode="disabled",
                                      seed=1, max_steps=100000)
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
        Qv = np.full(12, 1e-4)
        P0 = (0.01 * torch.eye(12, dtype=torch.float64, device=dev)).expand(n, 12, 12).contiguous()
        truth = env.rollout_states(a, {"x": x0, "status": st0}).x
        z = gym_copter_amd.measure(truth, H, r, 0)
        pf = lambda: env.rollout_pf(a, z, H, r, Qv, x0, P0, particles=P, status0=st0, tape=True)      # noqa: E731
        filt = pf()
        assert bool(filt.ok.all())
        fns = {"pf": lambda: [pf() for _ in range(repeat)]}
        for S in paths:
            fns["smooth_S%d" % S] = lambda S=S: [env.rollout_pf_smooth(a, filt, Qv, paths=S) for _ in range(repeat)]
        for fn in fns.values():                               # warm-up of every shape
            fn()
        best, worst = {}, {}
        for _ in range(rounds):
            for name, fn in fns.items():
                t = _time(fn) / repeat
                best[name] = min(best.get(name, t), t)
                worst[name] = max(worst.get(name, t), t)
    finally:
        env.close()
    rows = []
    for S in paths:
        t = best["smooth_S%d" % S]
        per_step = t * 1e-6 / K                               # seconds per backward step of every env's workgroup
        ops, lds = S * P * 36, S * P * 12 * 8
        rows.append({"envs": n, "K": K, "particles": P, "paths": S,
                     "pf_us_per_env_step": round(best["pf"] / (n * K), 4), "pf_spread": round(worst["pf"] / best["pf"], 3),
                     "smooth_us_per_env_step": round(t / (n * K), 4),
                     "smooth_spread": round(worst["smooth_S%d" % S] / t, 3),
                     "smooth_over_pf": round(t / best["pf"], 3),
                     "f64_ops_per_env_step": ops, "lds_bytes_per_env_step": lds,
                     "share_of_cu_f64_rate": round(ops / per_step / CU_F64_OPS, 3),
                     "share_of_cu_lds_rate": round(lds / per_step / CU_LDS_BYTES, 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=4, help="calls per timed window")
    ap.add_argument("--envs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--particles", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--paths", type=int, nargs="*", default=[64, 256, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pf_smooth_bench"))
    args = ap.parse_args()
    rows, lines = [], []
    for P in args.particles:
        for r in measure(args.envs, P, args.paths, args.steps, args.rounds, args.repeat):
            rows.append(r)
            lines.append("%4d envs  K %d  %4d particles  %4d paths: smooth %9.3f us/env-step (spread %.3f) | pf with tapes "
                         "%8.3f (%.3f) | smooth = %6.2fx pf | per CU: %.3f of the float64 vector rate, %.3f of the LDS read "
                         "rate" % (r["envs"], r["K"], r["particles"], r["paths"], r["smooth_us_per_env_step"],
                                   r["smooth_spread"], r["pf_us_per_env_step"], r["pf_spread"], r["smooth_over_pf"],
                                   r["share_of_cu_f64_rate"], r["share_of_cu_lds_rate"]))
            print(lines[-1], flush=True)
        with open(args.out + ".txt", "w") as f:
            f.write("# tools/pf_smooth_bench.py: Lander3D, float64 storage, best of %d interleaved rounds of %d calls "
                    "(spread = worst / best); us per env-step = the call's time / (N K)\n" % (args.rounds, args.repeat)
                    + "\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
