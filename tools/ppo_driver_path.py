"""The PPO driver's path on the problem of tests/test_gpu_rollout_ac.py: the mean reward per live
step of every iteration's collection, and the initial and the final policy on a fresh env (T.evaluate), for the test's
settings and -- with --sweep -- for the few other settings that were tried (at most six runs in all).

    python tools/ppo_driver_path.py [--sweep] > profiles/ppo_driver_path.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (label, keyword arguments of gym_copter_amd.ppo, sigma0); the first is the test's
RUNS = (("test", dict(lr=3e-4), 0.1),
        ("lr 1e-3", dict(lr=1e-3), 0.1),
        ("sigma0 0.01", dict(lr=3e-4), 0.01),
        ("sigma0 0.01, lr 1e-3", dict(lr=1e-3), 0.01),
        ("sigma0 0.003, lr 1e-3", dict(lr=1e-3), 0.003),
        ("sigma0 0.01, lr 1e-3, epochs 8", dict(lr=1e-3, epochs=8), 0.01))


def main():
    import numpy as np
    import torch
    import gym_copter_amd
    import test_gpu_rollout_ac as T
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    args = ap.parse_args()
    d = T.DRIVER
    actor0, critic0, log_std0 = T.driver_problem()
    print("# tools/ppo_driver_path.py: Lander3D, float32 storage, next_step auto-reset, %d envs, K %d, H %d, Hv %d, %d "
          "iterations; mean reward per live step" % (d["n"], d["K"], d["H"], d["Hv"], d["iterations"]))
    for label, kw, sigma0 in RUNS if args.sweep else RUNS[:1]:
        ls0 = torch.full_like(log_std0, float(np.log(sigma0)))
        before = T.evaluate(actor0, critic0, ls0)
        env = T._env(d["task"], d["n"], "float32", "next_step", seed=2, max_steps=1000)
        try:
            env.reset()
            res = gym_copter_amd.ppo(env, actor0, critic0, ls0, d["H"], d["Hv"], d["K"], d["iterations"], **kw)
        finally:
            env.close()
        after = T.evaluate(res.actor, res.critic, res.log_std)
        print("%s (sigma0 %g, %s): fresh env, initial policy %.4f -> final policy %.4f (%+.4f); final sigma %s"
              % (label, sigma0, ", ".join("%s %g" % kv for kv in kw.items()), before, after, after - before,
                 np.exp(T.to_np(res.log_std)).round(4).tolist()))
        print("  per iteration: " + " ".join("%.4f" % v for v in T.to_np(res.history)), flush=True)


if __name__ == "__main__":
    main()
