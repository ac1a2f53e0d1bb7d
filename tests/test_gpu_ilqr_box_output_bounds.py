"""The memory contract of CopterVecEnv.rollout_lqr_box and rollout_feedback_box_states with tests/guarded_outputs.py, as
tests/test_gpu_output_bounds.py holds the other entry points to it: a call writes nothing outside the arrays it is given,
it writes every element of every tensor it returns -- the clamp and iteration bytes included -- and it modifies no input.
N = 300 (four whole wavefronts and one of 44 lanes: both store paths) and N = 1, K = 3 and K = 1, float64 and float32
outputs.  The fill byte is 0x11: a clamp byte never has a control at both bounds, an iteration count stays below 17."""
import numpy as np
import pytest

import test_gpu_ilqr_box as T
from gpu_util import have_gpu
from guarded_outputs import guarded

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]
L = T.L
FILL = 0x11


def _checked(g, call, **inputs):
    import torch
    g.release()
    g.freeze(**inputs)
    res = call()
    torch.cuda.synchronize()
    g.assert_bands_intact()
    g.assert_fully_written(res)
    g.assert_inputs_unchanged()
    return res


@pytest.mark.parametrize("n,K", [(300, 3), (300, 1), (1, 3), (1, 1)])
@pytest.mark.parametrize("task", ["lander3d", "hover1d"])
def test_box_outputs_are_written_exactly(n, K, task):
    import torch
    A = L.TASK_A[task]
    rng = np.random.default_rng(12000 + 10 * n + K)
    lo, hi = np.float32(T.AH * 0.9), np.float32(T.AH * 1.1)
    env = L._env(task, n, "float32", seed=3)
    try:
        env.reset()
        state, acts, Q, Qf, R, q, r = L._small_problem(env, n, K, A, rng)
        state = {"x": L._dev(state["x"], env), "status": state["status"]}
        q, r = T.GRAD_SCALE * q, T.GRAD_SCALE * r
        ro = T._clone(env.rollout_states(acts, state))
        ins = dict(actions=acts, q=q, r=r, x=ro.x, status=ro.status, start_x=state["x"])
        with guarded(n, fill=FILL) as g:
            for dtype in (None, torch.float32):
                gains = _checked(g, lambda: env.rollout_lqr_box(acts, ro, Q, R, lo, hi, q=q, r=r, Q_final=Qf, mu=0.1,
                                                                state=state, dtype=dtype), **ins)
                assert gains.clamped.shape == (K, n) and gains.iters.shape == (K, n)
                g.refill(gains)                              # (the two byte arrays are shared by both dtypes' calls)
            gains = T._clone(env.rollout_lqr_box(acts, ro, Q, R, lo, hi, q=q, r=r, Q_final=Qf, mu=0.1, state=state))
            out = _checked(g, lambda: env.rollout_feedback_box_states(acts, ro, gains, 1.0, lo, hi, state=state),
                           K_gain=gains.K, d=gains.d, **ins)
            assert out[2].shape == (K, n) and len(g.allocations) >= 15
    finally:
        env.close()
