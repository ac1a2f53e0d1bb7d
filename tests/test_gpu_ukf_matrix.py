"""Every instantiation of the unscented filter's kernel (tests/filter_cases.py, imported unchanged: six tasks x three
storage modes x the rotor-gyro term off or on, 36 kernels), each launched once and held to the step-by-step induction of
tests/test_gpu_rollout_ukf.py (_check_steps) at its bar: 100 x the float64 reference's distance from its longdouble twin,
floored at 1e-12 scaled.  72 lanes (one whole wavefront and 8 lanes; nine lanes per group of starts), K = 10, M = 6 dense
measurements.  In the float32 modes the propagated points are held to rollout_states within 2^-23 max(1, |value|)
(rollout_states rounds its stored words once, the filter's points are not rounded); in float64 bit for bit.  The weight
setting alternates over the cases, so that each of the three meets every task and mode."""
import zlib

import numpy as np
import pytest

import model_variants
import test_gpu_rollout_ukf as U
import ukf_ref
from filter_cases import CASES, case_id
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K, M = 72, 10, 6
OVERALL = {}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ukf_in_every_instantiation(case):
    task, mode, gyro = case
    name = "matrix " + case_id(case)
    seed = zlib.crc32(repr(("ukf", task, mode, gyro)).encode())
    setting = ukf_ref.SETTINGS[CASES.index(case) % len(ukf_ref.SETTINGS)]
    kw = model_variants.env_kwargs("gyro_only") if gyro else {}
    env, penv = U._pair(task, N, mode, **kw)
    try:
        assert bool(env.config.rotor_gyro) == gyro and bool(penv.config.rotor_gyro) == gyro
        env.reset()
        penv.reset()
        p = U._problem(env, U.inputs(task, N, K, seed=seed, M=M))
        res = U._clone(U._run(env, p, setting, tape=True, points=True))
        ps = U._check_steps(name, env, penv, p, res, setting, exact=mode == "float64")
        for key, v in U.WORST[name].items():
            OVERALL[key] = max(OVERALL.get(key, 0.0), v)
        print("the worst over the cases so far: " + " ".join("%s %.5f" % kv for kv in OVERALL.items()))
        # the points of every case land on more than one branch, and meet the ground, a crash and free flight
        assert (to_np(res.spread) > 0).any(), name
        for s in (AIRBORNE, CRASHED, LANDED):
            assert (ps == s).any(), (name, s)
        assert np.isfinite(to_np(res.x)).all() and bool(res.ok.all()), name
    finally:
        env.close()
        penv.close()
