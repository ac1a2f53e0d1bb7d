"""Time the closed-loop rollouts (CopterVecEnv.rollout_mlp_states / rollout_mlp_vjp) against the
open-loop calls on the same shapes (rollout_states / rollout_vjp), and the end-to-end policy gradient (forward +
backward + the torch g_theta reduction) against the loop it replaces: K chained differentiable_rollout calls with K = 1,
each from the previous step's state, a torch MLP between them, stitched by autograd.  Lander3D, float32 storage, K = 64,
one substep, H in {0, 32, 64}, at 65 536 and 1 048 576 envs, float64 gradients.

Each figure is the best of `--rounds` device-synchronised windows of `--reps` back-to-back calls after `--warmup` untimed
ones (torch.cuda events), the calls of one shape timed in alternation.  The chained loop is timed at 65 536 envs only
(one window of one call: it takes seconds) and is skipped with --no-loop.

    python tools/rollout_mlp_bench.py [--reps 3] [--warmup 2] [--rounds 2] [--steps 64] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

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


def _chained_loop(env, p, K, hidden, x0, st):
    """The Python loop the fused calls replace: K differentiable_rollout calls of one step, a torch MLP between them."""
    import torch
    import gym_copter_amd
    from gym_copter_amd import mlp
    pr = p.detach().clone().requires_grad_(True)
    parts = mlp.unpack(pr, env.obs_dim, env.action_dim, hidden)
    x = x0
    loss = 0.0
    st_t = torch.from_numpy(st).to(env.device)
    for k in range(K):
        o = x[:env.obs_dim].T.float()
        if hidden == 0:
            a = o @ parts["W"].T + parts["b"]
        else:
            a = torch.tanh(o @ parts["W1"].T + parts["b1"]) @ parts["W2"].T + parts["b2"]
        r = gym_copter_amd.differentiable_rollout(env, a[None].contiguous(), state={"x": x, "status": st_t})
        x = r.x[0].T
        st_t = r.status[0]
        loss = loss + r.reward[0].sum()
    loss.backward()
    return pr.grad


def measure(n, hidden, K, reps, warmup, rounds, loop):
    import numpy as np
    import torch
    import gym_copter_amd
    from gym_copter_amd import mlp
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", autoreset_mode="disabled",
                                      seed=1, max_steps=100000)
    try:
        env.reset()
        rng = np.random.default_rng(0)
        p = mlp.init(10, 4, hidden, generator=torch.Generator().manual_seed(0), out_bias=0.0163, out_scale=0.01)
        p = p.to(env.device)
        a = torch.from_numpy(rng.uniform(0.012, 0.022, (K, n, 4)).astype(np.float32)).to(env.device)
        gx = torch.randn((K, n, 12), dtype=torch.float64, device=env.device)
        gr = torch.randn((K, n), dtype=torch.float64, device=env.device)
        tape = env.rollout_states(a)
        mtape = env.rollout_mlp_states(p, K, hidden)
        res = {"envs": n, "hidden": hidden, "K": K}
        cols = {"states": lambda: env.rollout_states(a),
                "mlp_states": lambda: env.rollout_mlp_states(p, K, hidden),
                "vjp": lambda: env.rollout_vjp(a, tape, gx=gx, gr=gr),
                "mlp_vjp": lambda: env.rollout_mlp_vjp(p, mtape, gx=gx, gr=gr, hidden=hidden, param_grad=False),
                "g_theta": lambda: mlp.param_grad(p, hidden, mtape.obs, mtape.actions.double()),
                "end_to_end": lambda: env.rollout_mlp_vjp(p, env.rollout_mlp_states(p, K, hidden), gr=gr,
                                                          hidden=hidden)}
        best = {k: [] for k in cols}
        for _ in range(rounds):
            for k, fn in cols.items():
                best[k].append(_window(fn, reps, warmup))
        for k in cols:
            res[k + "_us"] = min(best[k])
            res[k + "_us_per_step"] = min(best[k]) / K
        res["fwd_ratio"] = res["mlp_states_us"] / res["states_us"]
        res["bwd_ratio"] = res["mlp_vjp_us"] / res["vjp_us"]
        if loop:
            st = np.full(n, 0, np.uint8)
            s = env.get_state(only=("x", "status"))
            x0 = torch.from_numpy(s["x"]).to(env.device)
            st = s["status"]
            _chained_loop(env, p, 4, hidden, x0, st)              # warm-up (allocations, kernels)
            torch.cuda.synchronize()
            t = time.perf_counter()
            _chained_loop(env, p, K, hidden, x0, st)
            torch.cuda.synchronize()
            res["chained_loop_us"] = (time.perf_counter() - t) * 1e6
            res["end_to_end_speedup"] = res["chained_loop_us"] / res["end_to_end_us"]
        return res
    finally:
        env.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--hidden", type=int, nargs="+", default=[0, 32, 64])
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--json")
    args = ap.parse_args(argv)
    rows = []
    for n in args.envs:
        for h in args.hidden:
            r = measure(n, h, args.steps, args.reps, args.warmup, args.rounds, loop=(not args.no_loop and n <= 65536))
            rows.append(r)
            print("envs %8d H %2d: fwd %8.2f us/step (open loop %8.2f, x%.2f)  bwd %8.2f us/step (open loop %8.2f, "
                  "x%.2f)  g_theta %8.1f us  end-to-end %9.1f us%s"
                  % (n, h, r["mlp_states_us_per_step"], r["states_us_per_step"], r["fwd_ratio"],
                     r["mlp_vjp_us_per_step"], r["vjp_us_per_step"], r["bwd_ratio"], r["g_theta_us"],
                     r["end_to_end_us"], ("  chained loop %.0f us (x%.1f)" % (r["chained_loop_us"],
                                                                             r["end_to_end_speedup"]))
                     if "chained_loop_us" in r else ""), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"task": "lander3d", "state_dtype": "float32", "substeps": 1, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
