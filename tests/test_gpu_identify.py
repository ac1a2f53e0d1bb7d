"""gym_copter_amd.identify on the device: the identification problem of
tests/test_gpu_rollout_param_grad.py::test_system_identification_of_mass_and_inertias at n = 256, K = 50, float64
storage, hidden M, Ix, Iy at +-20 % -- solved by Levenberg-Marquardt on the forward-mode Jacobian of rollout_jvp in 6
iterations where Adam through the backward needs 300 for 1 %.  tests/test_jvp_cpu.py solves the same inputs on the
float64 oracle with a central-difference Jacobian (tests/jvp_ref.py): 1.9e-11 after 4 iterations and 1.1e-15 after 5
there, so the bars below leave five orders of magnitude and one spare iteration."""
import numpy as np
import pytest

import jvp_ref
from gpu_util import have_gpu, to_np

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]


def _setup(shared=False, with_force=False):
    import gym_copter_amd
    import torch
    pb = jvp_ref.identify_problem(shared=shared)
    n = pb["x0"].shape[1]
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float64", autoreset_mode="disabled",
                                      max_steps=100000, seed=3)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.device)     # noqa: E731
    state = {"x": dev(pb["x0"]), "status": dev(pb["status"])}
    acts = dev(pb["actions"])
    hidden_state = dict(state, force=dev(pb["force"])) if with_force else state
    x_obs = env.rollout_states(acts, state=hidden_state, vehicle=dev(pb["hidden"])).x.clone()
    return pb, env, acts, state, x_obs, dev(pb["nominal"])


@pytest.mark.parametrize("shared", [False, True], ids=["per_env", "shared"])
def test_identify_recovers_mass_and_inertias(shared):
    import gym_copter_amd
    pb, env, acts, state, x_obs, nominal = _setup(shared=shared)
    try:
        idx = pb["idx"]
        err0 = np.abs(pb["nominal"][idx] / pb["hidden"][idx] - 1.0)
        assert np.median(err0) > 0.05
        res = gym_copter_amd.identify(env, acts, x_obs, fit=jvp_ref.FIT, vehicle0=nominal, state=state, iterations=6,
                                      shared=shared)
        rel = np.max(np.abs(to_np(res.vehicle)[idx] / pb["hidden"][idx] - 1.0))
        print("identify (%s): max relative error %.3g" % ("shared" if shared else "per env", rel))
        assert rel <= 1e-6, rel
        accepted = to_np(res.history["accepted"])
        assert accepted.shape == (6, 1 if shared else env.num_envs) and np.all(accepted.any(axis=0))
        others = [j for j in range(12) if j not in idx]
        assert np.array_equal(to_np(res.vehicle)[others], pb["nominal"][others]) and res.force is None
        cost = to_np(res.history["cost"])
        assert np.all(cost[-1] <= cost[0]) and np.array_equal(to_np(res.cost), cost[-1])
    finally:
        env.close()


def test_identify_recovers_the_pending_force_as_well():
    import gym_copter_amd
    pb, env, acts, state, x_obs, nominal = _setup(with_force=True)
    try:
        idx = pb["idx"]
        res = gym_copter_amd.identify(env, acts, x_obs, fit=jvp_ref.FIT, vehicle0=nominal, fit_force=True, state=state,
                                      iterations=6)
        rel = np.max(np.abs(to_np(res.vehicle)[idx] / pb["hidden"][idx] - 1.0))
        ferr = np.max(np.abs(to_np(res.force) - pb["force"]))
        print("identify with the force: max relative error %.3g, max force error %.3g N" % (rel, ferr))
        assert rel <= 1e-6, rel
        assert ferr <= 1e-4, ferr
        assert np.all(to_np(res.history["accepted"]).any(axis=0))
    finally:
        env.close()


def test_identify_argument_errors():
    import gym_copter_amd
    pb, env, acts, state, x_obs, nominal = _setup()
    try:
        for kw, match in ((dict(fit=("M", "mass")), "fit must name"), (dict(fit=("M", "M")), "fit must name"),
                          (dict(fit_force=True, state=None), "fit_force"), (dict(iterations=0), "iterations"),
                          (dict(damping=0.0), "damping"), (dict(shared=True, fit_force=True), "shared"),
                          (dict(vehicle0=nominal[:, :-1]), "vehicle0")):
            with pytest.raises(ValueError, match=match):
                gym_copter_amd.identify(env, acts, x_obs, **dict(dict(state=state), **kw))
        with pytest.raises(ValueError, match="x_obs"):
            gym_copter_amd.identify(env, acts, x_obs[:, :-1], state=state)
    finally:
        env.close()
