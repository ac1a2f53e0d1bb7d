"""Time the parameter-gradient backward (cs_rollout_vjp_ex: CopterVecEnv.rollout_vjp_params, g_vehicle + g_force)
against the plain backward (cs_rollout_vjp: CopterVecEnv.rollout_vjp) on the same tape.  Lander3D, float32 storage,
K = 64, substeps 1 and 10, at 65 536 and 1 048 576 envs, float64 gradients.

The two are timed in alternation (plain, params, plain, params, ...: `--rounds` rounds), each round one
device-synchronised window of `--reps` back-to-back calls after `--warmup` untimed ones (torch.cuda events); the figure
is the best round of each.  The params call includes its unfold kernel.  Extra bytes per rollout: the [11,N] float64
coefficient adjoints written and read once and the [12,N] + [3,N] outputs.

    python tools/rollout_param_grad_bench.py [--reps 5] [--warmup 2] [--rounds 3] [--steps 64] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps          # us per call


def measure(n, substeps, K, reps, warmup, rounds):
    import numpy as np
    import torch
    import gym_copter_amd
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", substeps=substeps,
                                      autoreset_mode="disabled", seed=1, max_steps=100000)
    try:
        env.reset()
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, 4)).astype(np.float32)).to(env.device)
        gx = torch.randn((K, n, 12), dtype=torch.float64, device=env.device)
        gr = torch.randn((K, n), dtype=torch.float64, device=env.device)
        tape = env.rollout_states(a)
        plain, params = [], []
        for _ in range(rounds):
            plain.append(_window(lambda: env.rollout_vjp(a, tape, gx=gx, gr=gr), reps, warmup))
            params.append(_window(lambda: env.rollout_vjp_params(a, tape, gx=gx, gr=gr), reps, warmup))
        p, q = min(plain), min(params)
        return {"envs": n, "substeps": substeps, "K": K, "plain_us": p, "params_us": q, "ratio": q / p,
                "plain_ns_per_env_step": p * 1e3 / (n * K), "params_ns_per_env_step": q * 1e3 / (n * K),
                "plain_rounds_us": plain, "params_rounds_us": params}
    finally:
        env.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    rows = []
    print("%10s %4s %12s %12s %7s %14s" % ("envs", "sub", "plain us", "params us", "ratio", "params ns/e-s"))
    for n in [int(s) for s in args.sizes.split(",")]:
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.reps, args.warmup, args.rounds)
            rows.append(r)
            print("%10d %4d %12.1f %12.1f %7.3f %14.4f" % (n, substeps, r["plain_us"], r["params_us"], r["ratio"],
                                                          r["params_ns_per_env_step"]), flush=True)
    worst = max(r["ratio"] for r in rows)
    print("worst params / plain: %.3f (target <= 1.25: %s)" % (worst, "met" if worst <= 1.25 else "MISSED"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rows": rows, "worst_ratio": worst}, f, indent=1)


if __name__ == "__main__":
    main()
