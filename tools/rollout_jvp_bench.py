"""Time the forward-mode rollout tangents (cs_jvp_rollout) beside the reverse sweep they complement (cs_rollout_vjp_ex)
on the same tape, in the same process: Lander3D, float32 storage, K = 64, substeps 1 and 10, at 65 536 and 1 048 576
envs; and the wall time of gym_copter_amd.identify on the identification problem of
tests/test_gpu_rollout_param_grad.py::test_system_identification_of_mass_and_inertias beside that test's 300-iteration
Adam loop through the backward.

For each configuration, interleaved over `--rounds` rounds after one warm-up call of each, the best round kept per figure
and the spread (worst round / best round - 1) beside it:
  vjp_ex    CopterVecEnv.rollout_vjp_params(actions, tape, gx, gr)              one reverse sweep with g_vehicle, g_force
  jvp_D     CopterVecEnv.rollout_jvp(actions, tape, t_actions [D,K,N,A])        the plain build, D = 2, 4, 6
  jvpp_D    CopterVecEnv.rollout_jvp(actions, tape, t_vehicle, t_force)         the PARAM build, D = 2, 4, 6
and per direction block (2 directions) the time over one reverse sweep.  A jvp call writes D x K x N x 13 float64, a
reverse sweep K x N x 4 + 27 N: the bytes written per call are reported beside the times.  Timed with torch.cuda events
around device-synchronised windows.

    python tools/rollout_jvp_bench.py [--rounds 3] [--steps 64] [--out profiles/rollout_jvp_bench]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIRS = (2, 4, 6)
ROWS = ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm", "G", "rho", "C_L")


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
        tape = env.rollout_states(a)
        gx = torch.randn((K, n, 12), dtype=torch.float64, device=dev)
        gr = torch.randn((K, n), dtype=torch.float64, device=dev)
        fns = {"vjp_ex": lambda: env.rollout_vjp_params(a, tape, gx=gx, gr=gr)}
        for D in DIRS:
            t_a = torch.randn((D, K, n, 4), dtype=torch.float64, device=dev)
            t_v = torch.randn((D, 12, n), dtype=torch.float64, device=dev)
            t_f = torch.randn((D, 3, n), dtype=torch.float64, device=dev)
            fns["jvp_%d" % D] = lambda t_a=t_a: env.rollout_jvp(a, tape, t_actions=t_a)
            fns["jvpp_%d" % D] = lambda t_v=t_v, t_f=t_f: env.rollout_jvp(a, tape, t_vehicle=t_v, t_force=t_f)
        for fn in fns.values():
            fn()
        times = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                times[name].append(_time(fn))
    finally:
        env.close()
    out = {"envs": n, "substeps": substeps, "K": K}
    best = {name: min(ts) for name, ts in times.items()}
    for name, ts in times.items():
        out[name + "_us_per_step"] = round(min(ts) / K, 3)
        out[name + "_spread"] = round(max(ts) / min(ts) - 1.0, 4)
    for D in DIRS:
        out["jvp_%d_block_over_vjp_ex" % D] = round(best["jvp_%d" % D] / (D // 2) / best["vjp_ex"], 4)
        out["jvpp_%d_block_over_vjp_ex" % D] = round(best["jvpp_%d" % D] / (D // 2) / best["vjp_ex"], 4)
        out["jvp_%d_written_GBps" % D] = round(D * K * n * 13 * 8 / best["jvp_%d" % D] / 1e3, 1)
        out["jvpp_%d_written_GBps" % D] = round(D * K * n * 13 * 8 / best["jvpp_%d" % D] / 1e3, 1)
    return out


def identify_times(n=4096, K=50):
    """Wall time (host clock around a device synchronise) of identify() with the fewest iterations that bring the median
    relative error of M, Ix, Iy under 1 %, beside the existing test's 300-iteration Adam loop on the same problem."""
    import numpy as np
    import torch
    import gym_copter_amd
    rng = np.random.default_rng(2024)
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float64", autoreset_mode="disabled",
                                      seed=3, max_steps=100000)
    try:
        dev = env.device
        nominal = np.array([np.full(n, v) for v in (5e-3, 2e-6, 1.38, 0.35, 2.0, 2.0, 3.0, 38e-4, 15000.0, 9.80665,
                                                    env.config.rho, env.config.C_L)])
        idx = [ROWS.index(k) for k in ("M", "Ix", "Iy")]
        hidden = nominal.copy()
        hidden[idx] *= rng.uniform(0.8, 1.2, (3, n))
        x0 = np.zeros((12, n))
        x0[4] = -30.0
        state = {"x": torch.from_numpy(x0).to(dev), "status": torch.full((n,), 3, dtype=torch.uint8, device=dev)}
        acts = torch.from_numpy((0.016560178212092172 * (1.0 + 0.15 * rng.standard_normal((K, n, 4))))
                                .astype(np.float32)).to(dev)
        obs = env.rollout_states(acts, state=state, vehicle=torch.from_numpy(hidden).to(dev)).x.clone()
        base = torch.from_numpy(nominal).to(dev)

        def err(vehicle):
            return np.median(np.abs(vehicle.cpu().numpy()[idx] / hidden[idx] - 1.0), axis=1)

        out = {"envs": n, "K": K}
        gym_copter_amd.identify(env, acts, obs, vehicle0=base, state=state, iterations=1)      # warm-up
        for iters in range(1, 9):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = gym_copter_amd.identify(env, acts, obs, vehicle0=base, state=state, iterations=iters)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            e = err(res.vehicle)
            out["identify_%d_iterations" % iters] = {"seconds": round(dt, 4), "median_rel_err": [float(v) for v in e]}
            if np.all(e < 0.01) and "identify_iterations_to_1pct" not in out:
                out["identify_iterations_to_1pct"], out["identify_seconds_to_1pct"] = iters, round(dt, 4)
            if np.all(e < 1e-9):
                break
        logp = torch.zeros((3, n), dtype=torch.float64, device=dev, requires_grad=True)
        opt = torch.optim.Adam([logp], lr=0.02)
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 300, eta_min=2e-4)
        scale = obs.abs().amax(dim=0, keepdim=True).clamp_min(1e-3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(300):
            opt.zero_grad()
            veh = base.clone()
            veh[idx] = base[idx] * torch.exp(logp)
            o = gym_copter_amd.differentiable_rollout(env, acts, state=state, vehicle=veh)
            (((o.x - obs) / scale) ** 2).sum().backward()
            opt.step()
            sched.step()
        torch.cuda.synchronize()
        out["adam_300_seconds"] = round(time.perf_counter() - t0, 4)
        veh = base.clone()
        veh[idx] = base[idx] * torch.exp(logp.detach())
        out["adam_300_median_rel_err"] = [float(v) for v in err(veh)]
    finally:
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="*", default=[65536, 1048576])
    ap.add_argument("--identify-envs", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_jvp_bench"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("rollout_jvp_bench.py needs a HIP device: nothing is measured without one")
    rows, lines = [], []
    result = {"kernels": rows}

    def write():
        with open(args.out + ".txt", "w") as f:
            f.write("# tools/rollout_jvp_bench.py: Lander3D, float32 storage, float64 outputs, best of %d interleaved "
                    "rounds (spread: worst round over best - 1); block = 2 directions\n" % args.rounds
                    + "\n".join(lines) + "\n")
        with open(args.out + ".json", "w") as f:
            json.dump(result, f, indent=1)

    for n in args.envs:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.rounds)
            rows.append(r)
            line = "%8d envs  substeps %2d  K %d: vjp_ex %10.3f us/step (spread %.1f %%)" % (
                n, substeps, args.steps, r["vjp_ex_us_per_step"], 100 * r["vjp_ex_spread"])
            for D in DIRS:
                line += " | D=%d plain %10.3f (%.1f %%) = %.3fx per block, %.0f GB/s written; PARAM %10.3f (%.1f %%) = " \
                        "%.3fx per block" % (D, r["jvp_%d_us_per_step" % D], 100 * r["jvp_%d_spread" % D],
                                             r["jvp_%d_block_over_vjp_ex" % D], r["jvp_%d_written_GBps" % D],
                                             r["jvpp_%d_us_per_step" % D], 100 * r["jvpp_%d_spread" % D],
                                             r["jvpp_%d_block_over_vjp_ex" % D])
            lines.append(line)
            print(line, flush=True)
            write()
    ident = identify_times(args.identify_envs)
    result["identify"] = ident
    lines.append("identify, %d envs, K %d, M Ix Iy at +-20 %%: %s iterations and %s s to a median error under 1 %%; "
                 "the 300-iteration Adam loop %.3f s (median errors %s)"
                 % (ident["envs"], ident["K"], ident.get("identify_iterations_to_1pct"),
                    ident.get("identify_seconds_to_1pct"), ident["adam_300_seconds"],
                    ", ".join("%.2e" % v for v in ident["adam_300_median_rel_err"])))
    for k in sorted(k for k in ident if k.endswith("_iterations")):
        lines.append("  %s: %.4f s, median relative errors %s"
                     % (k, ident[k]["seconds"], ", ".join("%.2e" % v for v in ident[k]["median_rel_err"])))
    print("\n".join(lines[-1 - sum(k.endswith("_iterations") for k in ident):]), flush=True)
    write()


if __name__ == "__main__":
    main()
