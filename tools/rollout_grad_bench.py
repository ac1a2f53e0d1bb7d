"""Time differentiable K-step rollouts (cs_rollout_states / cs_rollout_vjp) against the one-step Jacobian chain that
gives the same gradient.  Lander3D, float32 storage, K = 64, substeps 1 and 10, at 65 536 and 1 048 576 envs.

For each configuration, in one process:
  forward   CopterVecEnv.rollout_states(actions [K,N,4])                        -> us per step, ns per env-step
  backward  CopterVecEnv.rollout_vjp(actions, tape, gx, gr) (float64 gradients) -> us per step, ns per env-step
  chain     K x (step_jacobian + step) + the reverse bmm chain (2 torch.bmm per step: du^T lam and dx^T lam) -- the
            same gradient from one-step Jacobians.  ONE Jacobian buffer is reused for every step (storing K of them
            needs K x N x 1.5 KB, 103 GB at 1 M envs x 64), so this is a lower bound of what the chain costs.
Each figure is one device-synchronised window of `--reps` back-to-back calls (the chain: one pass) after `--warmup`
untimed ones, timed with torch.cuda events.

Bytes per env-step from the shapes: forward writes x (96 B) + reward (8) + terminated, truncated, status (3) = 107 B
(+ 16 B of actions read); backward reads x_{k-1} (96) + status (1) + action (16) + gx (96) + gr (8) and writes
g_actions (16) = 233 B.  HBM bound at 8 TB/s.  Instruction-issue bound, bench.py's arithmetic: wavefronts per SIMD x
VALU instructions per wavefront-step x 4 cycles / 2.4 GHz on 1 024 SIMDs, with the VALU count MEASURED by rocprofv3 PMC
(SQ_INSTS_VALU / SQ_WAVES / K per kernel and configuration, profiles/rollout_grad_pmc.json, made by
tools/rollout_grad_pmc.py from a `--no-chain` run of this tool under `rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU`).  Without
that file the issue bound is not printed.

    python tools/rollout_grad_bench.py [--reps 5] [--warmup 2] [--steps 64] [--no-chain] [--pmc counts.json] [--json out.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BPS = 8.0e12
FWD_BYTES, BWD_BYTES = 107 + 16, 233
SIMDS, CLOCK_HZ, CYCLES_PER_VALU = 1024, 2.4e9, 4
PMC_PATH = os.path.join(ROOT, "profiles", "rollout_grad_pmc.json")


def config_key(n, substeps):
    return "lander3d_%d_substeps%d" % (n, substeps)


def load_pmc(path=PMC_PATH):
    """{config_key: {"fwd": VALU instructions per wavefront-step, "bwd": ...}} or {} (tools/rollout_grad_pmc.py)"""
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return json.load(f).get("valu_per_wavefront_step", {})


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


def measure(n, substeps, K, reps, warmup, chain_pass=True, pmc=None):
    import numpy as np
    import torch
    import gym_copter_amd
    mk = lambda: gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", substeps=substeps,
                                             autoreset_mode="disabled", seed=1, max_steps=100000)
    env = mk()
    try:
        env.reset()
        rng = np.random.default_rng(0)
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, 4)).astype(np.float32)).to(env.device)
        gx = torch.randn((K, n, 12), dtype=torch.float64, device=env.device)
        gr = torch.randn((K, n), dtype=torch.float64, device=env.device)
        tape = env.rollout_states(a)
        fwd = _window(lambda: env.rollout_states(a), reps, warmup)
        bwd = _window(lambda: env.rollout_vjp(a, tape, gx=gx, gr=gr), reps, warmup)

        lam = torch.zeros((n, 12, 1), dtype=torch.float64, device=env.device)

        def chain():
            for k in range(K):
                env.step_jacobian(a[k])
                env.step(a[k])
            jac = env.step_jacobian(a[0])
            dxT, duT = jac.dx.transpose(1, 2), jac.du.transpose(1, 2)
            lm = lam
            for k in range(K - 1, -1, -1):
                torch.bmm(duT, lm)
                lm = torch.bmm(dxT, lm)
        chain_us = _window(chain, 1, 1) if chain_pass else None
    finally:
        env.close()
    waves = (n + 63) // 64
    us_per_valu = waves * CYCLES_PER_VALU / SIMDS / CLOCK_HZ * 1e6     # one VALU instruction of every wavefront
    counts = (pmc or {}).get(config_key(n, substeps), {})
    r = {"envs": n, "substeps": substeps, "K": K,
         "fwd_us_per_step": round(fwd / K, 3), "bwd_us_per_step": round(bwd / K, 3),
         "fwd_ns_per_env_step": round(fwd / K / n * 1e3, 4), "bwd_ns_per_env_step": round(bwd / K / n * 1e3, 4),
         "fwd_hbm_bound_us": round(n * FWD_BYTES / HBM_BPS * 1e6, 3),
         "bwd_hbm_bound_us": round(n * BWD_BYTES / HBM_BPS * 1e6, 3)}
    for p in ("fwd", "bwd"):
        hb = r[p + "_hbm_bound_us"]
        ib = round(counts[p] * us_per_valu, 3) if p in counts else None
        r[p + "_valu_per_wavefront_step"] = counts.get(p)
        r[p + "_issue_bound_us"] = ib
        r[p + "_binds"] = "hbm" if ib is None or hb >= ib else "valu issue"
        r[p + "_fraction_of_bound"] = round(max(hb, ib or 0.0) / r[p + "_us_per_step"], 3)
        r[p + "_fraction_of_hbm"] = round(hb / r[p + "_us_per_step"], 3)
    if chain_us is not None:
        r["chain_us_per_step"] = round(chain_us / K, 3)
        r["chain_over_bwd"] = round(r["chain_us_per_step"] / r["bwd_us_per_step"], 1)
        r["chain_over_fwd_plus_bwd"] = round(r["chain_us_per_step"] / (r["bwd_us_per_step"] + r["fwd_us_per_step"]), 1)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-chain", action="store_true", help="skip the step_jacobian chain (the PMC run)")
    ap.add_argument("--pmc", default=PMC_PATH, help="VALU counts (tools/rollout_grad_pmc.py's output)")
    args = ap.parse_args()
    pmc = load_pmc(args.pmc)
    rows = []
    for n in (65536, 1048576):
        for substeps in (1, 10):
            r = measure(n, substeps, args.steps, args.reps, args.warmup, not args.no_chain, pmc)
            rows.append(r)
            print("%8d envs  substeps %2d  K %d" % (n, substeps, args.steps))
            for p, name in (("fwd", "forward "), ("bwd", "backward")):
                ib = r[p + "_issue_bound_us"]
                issue = ("issue bound %.3f us (%.0f VALU / wavefront-step, PMC)" % (ib, r[p + "_valu_per_wavefront_step"])
                         if ib is not None else "issue bound n/a: no PMC counts")
                print("    %s %9.3f us/step  %7.4f ns/env-step  (HBM bound %.3f us, %s: %s binds;"
                      " %.3f of the binding bound, %.3f of 8 TB/s)"
                      % (name, r[p + "_us_per_step"], r[p + "_ns_per_env_step"], r[p + "_hbm_bound_us"], issue,
                         r[p + "_binds"], r[p + "_fraction_of_bound"], r[p + "_fraction_of_hbm"]))
            if "chain_us_per_step" in r:
                print("    chain    %9.3f us/step  (K x (step_jacobian + step) + bmm chain): %.1fx the backward, %.1fx"
                      " forward + backward" % (r["chain_us_per_step"], r["chain_over_bwd"],
                                               r["chain_over_fwd_plus_bwd"]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
