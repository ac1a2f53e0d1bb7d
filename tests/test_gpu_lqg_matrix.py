"""Every instantiation of the output-feedback kernel (cs_rollout_lqg; tests/filter_cases.py: six tasks x three storage
modes x the rotor-gyro term off or on, 36 kernels), each launched once on 72 lanes (one whole wavefront and 8 lanes; nine
lanes per group of lqg_ref.points), K = 10, M = 6 dense measurements, and held to the four exact statements of
tests/test_gpu_rollout_lqg.py (check_composition: the truth is rollout_states', the measurement lqg_ref's, the filter
rollout_ekf's, the law lqg_ref's at the estimate, all bit for bit) and to its conditions that the feedback is active.

In the float32 storage modes the truth's rows are the stored words, as rollout_states rounds them (asserted in float32_rn), and the filter's mean
is not rounded, as in rollout_ekf: both comparisons stay bit for bit.  With the rotor-gyro term on, the 3-D tasks' truth
differs from the plain model's in every lane that flies; the 2-D and 1-D fan-outs make the term an exact zero
(tests/test_gpu_filter_matrix.py)."""
import zlib

import numpy as np
import pytest

import model_variants
import test_gpu_rollout_lqg as L
from filter_cases import CASES, case_id
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K, M = 72, 10, 6


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lqg_in_every_instantiation(case):
    task, mode, gyro = case
    name = "matrix " + case_id(case)
    rng = np.random.default_rng(zlib.crc32(repr(("lqg", task, mode, gyro)).encode()))
    kw = model_variants.env_kwargs("gyro_only") if gyro else {}
    env = L._env(task, N, mode, seed=3, **kw)
    ref = L._env(task, N, mode, seed=3) if gyro else None
    try:
        assert bool(env.config.rotor_gyro) == gyro
        env.reset()
        p = L._problem(env, task, rng, steps=K, M=M)
        res = L._clone(L._run(env, p, tape=True))
        assert tuple(res.actions.shape) == (K, N, L.lqg_ref.TASK_A[task]) and tuple(res.z.shape) == (K, N, M)
        at_truth, _ = L.check_composition(name, env, p, res)
        L.assert_feedback_active(name, env, p, res, at_truth)
        frac = L._fractions(res.filter.branch)
        assert all(v > 0 for v in frac.values()), (name, frac)
        if mode == "float32_rn":          # (the "float32" mode keeps five guard bits more than a float32 word)
            x = to_np(res.rollout.x)
            assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), name
        if gyro:
            ref.reset()
            plain = to_np(ref.rollout_states(res.actions, state=p.state).x)
            mine = to_np(res.rollout.x)
            flying = to_np(res.rollout.status[0]) == AIRBORNE
            if L.lqg_ref.TASK_A[task] == 4:
                assert np.any(plain != mine, axis=(0, 2))[flying].all(), name
            else:
                assert np.array_equal(plain, mine), name
    finally:
        env.close()
        if ref is not None:
            ref.close()
