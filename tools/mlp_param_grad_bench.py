"""Time the policy-parameter gradient on the device (CopterVecEnv.mlp_param_grad, cs_mlp_param_grad; DESIGN.md section
12) against gym_copter_amd.mlp.param_grad, the torch reduction it stands beside, and the cost of the cotangent on the
action tape (rollout_mlp_vjp's g_actions_in).  Lander3D, float32 storage, K = 64, one substep, H in {0, 32, 64}, at
65 536 and 1 048 576 envs, float64 gradients: the six rows of section 12's table.  On the same tapes and in the same
process, the two calls of a pair timed in alternation:

  g_theta      mlp.param_grad against mlp_param_grad, us per call, and torch / device
  end to end   forward + backward + reduction, reduce="torch" against reduce="device"
  issue share  the device reduction's float64 issue floor / its time, bench.py's arithmetic: wavefronts per SIMD x
               vector instructions per wavefront x 4 cycles / 2.4 GHz.  The instruction count is STATIC, from the ISA
               listing (make asm-rollout: build/copterstep_mlp_grad-*.s, the vector instructions of the row loop's
               longest path x rows per wavefront + those of a tile's staging x tiles per wavefront), not a counter
  cotangent    the backward alone with and without g_actions_in

Each figure is the best of `--rounds` device-synchronised windows of `--reps` back-to-back calls after `--warmup`
untimed ones (torch.cuda events); `spread` is (worst - best) / best over the rounds of the device reduction and of the
torch reduction, the larger of the two.

    python tools/mlp_param_grad_bench.py [--reps 3] [--warmup 2] [--rounds 3] [--out profiles/mlp_param_grad_bench]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLOCK_HZ, SIMDS, ISSUE_CYCLES = 2.4e9, 256 * 4, 4     # bench.py: PEAK_ENGINE_CLOCK_HZ, 256 CUs x 4 SIMDs, 4 cycles
MAX_GROUPS, WAVES_PER_GROUP = 1024, 4                  # copterstep_mlp_grad.hip: kGradMaxGroups, kGradWaves
# Static vector-instruction counts of mlp_param_grad_kernel<10, 4, HP> from the ISA listing: (per row iteration of a
# wavefront -- the longest path through tanh --, per tile staged); H = 0 has no row loop: per tile only.
ISA_VALU = {0: (0, 104), 32: (185, 80), 64: (185, 80)}


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


def issue_floor_us(rows, hidden):
    """The float64 issue floor of the device reduction at `rows` = K N rows (bench.py's issue_bound arithmetic)."""
    per_row, per_tile = ISA_VALU[hidden]
    tiles = (rows + 63) // 64
    per_group = (tiles + MAX_GROUPS - 1) // MAX_GROUPS
    groups = (tiles + per_group - 1) // per_group
    tiles_per_wave = (per_group + WAVES_PER_GROUP - 1) // WAVES_PER_GROUP
    hp = 0 if hidden == 0 else max(8, 1 << (hidden - 1).bit_length())
    iters_per_tile = hp                               # 64 / (64 / HP) rows per slot
    valu = tiles_per_wave * (per_tile + iters_per_tile * per_row)
    waves_per_simd = (groups * WAVES_PER_GROUP + SIMDS - 1) // SIMDS
    return waves_per_simd * valu * ISSUE_CYCLES / CLOCK_HZ * 1e6, valu, waves_per_simd


def measure(n, hidden, K, reps, warmup, rounds):
    import torch
    import gym_copter_amd
    from gym_copter_amd import mlp
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float32", autoreset_mode="disabled",
                                      seed=1, max_steps=100000)
    try:
        env.reset()
        p = mlp.init(10, 4, hidden, generator=torch.Generator().manual_seed(0), out_bias=0.0163, out_scale=0.01)
        p = p.to(env.device)
        gx = torch.randn((K, n, 12), dtype=torch.float64, device=env.device)
        gr = torch.randn((K, n), dtype=torch.float64, device=env.device)
        gact = torch.randn((K, n, 4), dtype=torch.float64, device=env.device)
        tape = env.rollout_mlp_states(p, K, hidden)
        _, ga, _ = env.rollout_mlp_vjp(p, tape, gx=gx, gr=gr, hidden=hidden, param_grad=False)
        ga = ga.clone()
        cols = {"torch": lambda: mlp.param_grad(p, hidden, tape.obs, ga),
                "device": lambda: env.mlp_param_grad(p, hidden, tape.obs, ga),
                "e2e_torch": lambda: env.rollout_mlp_vjp(p, env.rollout_mlp_states(p, K, hidden), gr=gr, hidden=hidden),
                "e2e_device": lambda: env.rollout_mlp_vjp(p, env.rollout_mlp_states(p, K, hidden), gr=gr, hidden=hidden,
                                                          reduce="device"),
                "vjp": lambda: env.rollout_mlp_vjp(p, tape, gx=gx, gr=gr, hidden=hidden, param_grad=False),
                "vjp_cot": lambda: env.rollout_mlp_vjp(p, tape, gx=gx, gr=gr, hidden=hidden, param_grad=False,
                                                       g_actions_in=gact)}
        times = {k: [] for k in cols}
        for _ in range(rounds):
            for k, fn in cols.items():
                times[k].append(_window(fn, reps, warmup))
        res = {"envs": n, "hidden": hidden, "K": K}
        for k in cols:
            res[k + "_us"] = min(times[k])
            res[k + "_us_rounds"] = times[k]
        res["spread"] = max((max(times[k]) - min(times[k])) / min(times[k]) for k in ("torch", "device"))
        res["ratio_torch_over_device"] = res["torch_us"] / res["device_us"]
        res["device_slower_than_spread"] = res["device_us"] > res["torch_us"] * (1.0 + res["spread"])
        res["e2e_ratio"] = res["e2e_torch_us"] / res["e2e_device_us"]
        res["cotangent_cost"] = res["vjp_cot_us"] / res["vjp_us"] - 1.0
        floor, valu, wps = issue_floor_us(K * n, hidden)
        res["issue"] = {"bound": "valu_f64_issue", "source": "ISA listing (static count, longest path)",
                        "valu_per_wavefront": valu, "wavefronts_per_simd": wps, "floor_us": floor,
                        "frac": floor / res["device_us"]}
        return res
    finally:
        env.close()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--envs", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--hidden", type=int, nargs="+", default=[0, 32, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mlp_param_grad_bench"))
    args = ap.parse_args(argv)
    rows, lines = [], []
    for n in args.envs:
        for h in args.hidden:
            r = measure(n, h, args.steps, args.reps, args.warmup, args.rounds)
            rows.append(r)
            lines.append("envs %8d H %2d: g_theta torch %9.1f us  device %8.1f us  x%6.2f (spread %4.1f %%%s)  end-to-end "
                         "torch %9.1f us  device %9.1f us  x%.2f  issue floor %7.1f us = %4.1f %% of the time (ISA count "
                         "%d per wavefront, %d per SIMD)  backward %9.1f us, with a cotangent %9.1f us (%+.1f %%)"
                         % (n, h, r["torch_us"], r["device_us"], r["ratio_torch_over_device"], 100 * r["spread"],
                            ", DEVICE SLOWER" if r["device_slower_than_spread"] else "", r["e2e_torch_us"],
                            r["e2e_device_us"], r["e2e_ratio"], r["issue"]["floor_us"], 100 * r["issue"]["frac"],
                            r["issue"]["valu_per_wavefront"], r["issue"]["wavefronts_per_simd"], r["vjp_us"],
                            r["vjp_cot_us"], 100 * r["cotangent_cost"]))
            print(lines[-1], flush=True)
    with open(args.out + ".txt", "w") as f:
        f.write("# tools/mlp_param_grad_bench.py: Lander3D, float32 storage, K = %d, --reps %d --warmup %d --rounds %d\n"
                % (args.steps, args.reps, args.warmup, args.rounds))
        f.write("\n".join(lines) + "\n")
    with open(args.out + ".json", "w") as f:
        json.dump({"task": "lander3d", "state_dtype": "float32", "substeps": 1, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
