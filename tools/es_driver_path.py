"""The evolution-strategies driver's path on the problem of tests/test_gpu_rollout_es.py: theta's
own mean return, landed and crashed share on the 64 common starts after 0, 5, 10, .. 30, 60 and 90 iterations --
gym_copter_amd.es is deterministic, so a run of t iterations is the first t iterations of a longer one -- and the mean
member return of the last population.

    python tools/es_driver_path.py > profiles/es_driver_path.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import gym_copter_amd
    import test_gpu_rollout_es as T
    d = T.DRIVER
    M = 2 * d["pairs"]
    env = T._env(d["task"], M * d["E"], "float32", seed=2)
    try:
        env.reset()
        x0, theta0 = T.driver_problem()
        print("# tools/es_driver_path.py: Lander3D, H %d, %d pairs x %d envs, K %d, sigma %g, lr %g"
              % (d["H"], d["pairs"], d["E"], d["K"], d["sigma"], d["lr"]))
        print("iterations %3d: theta's return %8.3f  landed %5.1f %%  crashed %5.1f %%"
              % ((0,) + tuple(v * s for v, s in zip(T.evaluate(env, theta0, x0), (1, 100, 100)))), flush=True)
        for it in (5, 10, 15, 20, 25, 30, 60, 90):
            res = gym_copter_amd.es(env, theta0, d["H"], d["K"], d["pairs"], d["sigma"], d["lr"], it,
                                    envs_per_member=d["E"], start_x=x0)
            r, landed, crashed = T.evaluate(env, res.params, x0)
            print("iterations %3d: theta's return %8.3f  landed %5.1f %%  crashed %5.1f %%  | last population's mean %8.3f"
                  % (it, r, 100 * landed, 100 * crashed, float(res.history[-1])), flush=True)
    finally:
        env.close()


if __name__ == "__main__":
    main()
