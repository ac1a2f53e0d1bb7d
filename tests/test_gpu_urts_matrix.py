"""Every instantiation of the unscented smoother's kernel (tests/filter_cases.py, imported unchanged: six tasks x three
storage modes x the rotor-gyro term off or on, 36 kernels), each launched once on the tapes of that case's unscented
filter and held to the row-by-row induction of tests/test_gpu_urts.py (_check_rows) at its bar.  72 lanes (one whole
wavefront and 8 lanes; nine lanes per group of starts), K = 10, M = 6 dense measurements.  The weight setting alternates
over the cases, so that each of the three meets every task and mode.  Then once on the wide-attitude points of
tests/attitude_points.py."""
import zlib

import numpy as np
import pytest

import attitude_points as ap
import ekf_ref
import model_variants
import test_gpu_rollout_ekf as E
import test_gpu_rollout_ukf as U
import test_gpu_urts as T
import ukf_ref
from filter_cases import CASES, case_id
from gpu_util import have_gpu, to_np

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K, M = 72, 10, 6
OVERALL = {}


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_urts_in_every_instantiation(case):
    task, mode, gyro = case
    name = "matrix " + case_id(case)
    seed = zlib.crc32(repr(("urts", task, mode, gyro)).encode())
    setting = ukf_ref.SETTINGS[CASES.index(case) % len(ukf_ref.SETTINGS)]
    kw = model_variants.env_kwargs("gyro_only") if gyro else {}
    env = E._env(task, N, mode, seed=3, **kw)
    try:
        assert bool(env.config.rotor_gyro) == gyro
        env.reset()
        p = U._problem(env, U.inputs(task, N, K, seed=seed, M=M))
        filt = T._filter(env, p, setting)
        res = U._clone(T._urts(env, p, filt, setting))
        T._check_rows(name, p, filt, res, setting)
        for key, v in T.WORST[name].items():
            OVERALL[key] = max(OVERALL.get(key, 0.0), v)
        print("the worst over the cases so far: " + " ".join("%s %.3g" % kv for kv in OVERALL.items()))
        assert (to_np(filt.spread) > 0).any(), name
        assert np.isfinite(to_np(res.x)).all() and np.isfinite(to_np(res.P_tape)).all() and bool(res.ok.all()), name
    finally:
        env.close()


def test_urts_at_wide_attitudes():
    """the wide groups with finite yaws up to 300 rad and motors around hover, K = 4, a small P0 (the inputs the extended
    filter and smoother are given in tests/test_gpu_wide_attitudes.py): every backward step at the bar"""
    from gym_copter_amd import measure
    p = ap.points()
    sel = np.flatnonzero(np.isin(p.group, [g for g in ap.WIDE_GROUPS if g != "fold"]) & (np.arange(ap.N) % 8 != 0))
    n, steps = sel.size, 4
    rng = np.random.default_rng(19)
    setting = ukf_ref.SETTINGS[1]
    env = E._env("lander3d", n, seed=3)
    try:
        env.reset()
        x0, st0 = np.ascontiguousarray(p.x[:, sel]), p.status[sel].copy()
        acts = (p.actions[sel][None] * rng.uniform(0.9, 1.1, (steps, n, 4))).astype(np.float32)
        H, r = E._model(rng, 6, True)
        acts_d = E._dev(acts, env)
        truth = env.rollout_states(acts_d, state={"x": x0, "status": st0}).x.clone()
        prob = dict(acts=acts_d, z=measure(truth, H, r, 5), H=H, r=r, Q=ekf_ref.test_Q(), x0=E._dev(x0, env),
                    P0=E._dev(1e-4 * E._spd(rng, n), env), st0=E._dev(st0, env))
        assert (np.abs(x0[[6, 8]]) > 2.0).any() and (np.abs(x0[10]) > 100).any()
        filt = T._filter(env, prob, setting)
        res = U._clone(T._urts(env, prob, filt, setting))
        T._check_rows("wide attitudes", prob, filt, res, setting)
    finally:
        env.close()
