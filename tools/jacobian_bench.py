"""Time CopterVecEnv.step_jacobian (cs_step_jacobian): us per call for Lander3D, float32 storage, at 65 536 and
1 048 576 envs, float64 and float32 outputs, substeps 1 and 10.  Each figure is one device-synchronised window of
`--calls` back-to-back calls after `--warmup` untimed ones (torch.cuda events around the window).

Bytes per call come from the shapes: written = N x (12 x 12 + 12 x 4 + 12 + 4) x (8 | 4) + N (branch bits); read =
N x (64 B of state groups + 16 B of actions).  The roofline fraction is against 8 TB/s.  For substeps 10 the float64
issue bound is printed beside it: F64_PER_SUBSTEP_BLOCK float64 VALU instructions per wavefront per substep and
direction block (an estimate from the gfx950 ISA of the Lander3D kernel's substep loop: the non-gyro half of its 574
float64 instructions), 8 blocks, at 4 cycles per wave64 float64 instruction on 1 024 SIMDs at 2.4 GHz.

    python tools/jacobian_bench.py [--calls 50] [--warmup 10] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12
F64_PER_SUBSTEP_BLOCK = 287
BLOCKS = 8                      # (12 + 4) directions, 2 per block
SIMDS, CLOCK_HZ, CYCLES_PER_F64 = 1024, 2.4e9, 4


def measure(n, substeps, dtype, calls, warmup):
    import numpy as np
    import torch
    import gym_copter_amd
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", substeps=substeps,
                                      autoreset_mode="disabled", seed=1)
    try:
        env.reset()
        a = torch.from_numpy(np.random.default_rng(0).uniform(0.01, 0.03, (n, 4)).astype(np.float32)).to(env.device)
        for _ in range(warmup):
            env.step_jacobian(a, dtype=dtype)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            env.step_jacobian(a, dtype=dtype)
        t1.record()
        torch.cuda.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / calls
    finally:
        env.close()
    word = 8 if dtype == torch.float64 else 4
    written = n * ((144 + 48 + 12 + 4) * word + 1)
    read = n * (64 + 16)
    r = {"envs": n, "substeps": substeps, "out_dtype": str(dtype).split(".")[-1], "us_per_call": round(us, 2),
         "bytes_written": written, "bytes_read": read,
         "hbm_fraction": round((written + read) / (us * 1e-6) / HBM_BPS, 3)}
    waves = (n + 63) // 64
    r["f64_issue_bound_us"] = round(waves * F64_PER_SUBSTEP_BLOCK * BLOCKS * substeps * CYCLES_PER_F64
                                    / SIMDS / CLOCK_HZ * 1e6, 2)
    r["hbm_bound_us"] = round((written + read) / HBM_BPS * 1e6, 2)
    r["binds"] = "hbm" if r["hbm_bound_us"] >= r["f64_issue_bound_us"] else "f64 issue"
    return r


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for n in (65536, 1048576):
        for substeps in (1, 10):
            for dtype in (torch.float64, torch.float32):
                r = measure(n, substeps, dtype, args.calls, args.warmup)
                rows.append(r)
                print("%8d envs  substeps %2d  %-7s  %9.2f us/call  %.3f of 8 TB/s  (HBM bound %.2f us, "
                      "f64 issue bound %.2f us: %s binds)" % (n, substeps, r["out_dtype"], r["us_per_call"],
                                                              r["hbm_fraction"], r["hbm_bound_us"],
                                                              r["f64_issue_bound_us"], r["binds"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
