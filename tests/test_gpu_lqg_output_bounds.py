"""The memory contract of CopterVecEnv.rollout_lqg with tests/guarded_outputs.py, as tests/test_gpu_output_bounds.py
holds the other entry points to it: the call writes nothing outside the arrays it is given (every output sits between two
bands of the byte 0xA5), it writes every element of every tensor it returns, and it modifies no input tensor.  N = 300
(four whole wavefronts and one of 44 lanes: both store paths) and N = 1; with and without the covariance tape, float64
and float32 outputs, an explicit start and the stored one.  Every comparison is exact."""
import numpy as np
import pytest

import test_gpu_rollout_lqg as L
from gpu_util import have_gpu
from guarded_outputs import guarded

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]


def _guarded_call(g, env, p, **kw):
    import torch
    g.release()
    ins = dict(actions=p.abar, gains=p.gains, xbar=p.xbar, noise=p.e, xhat0=p.xhat0, P0=p.P0, status0=p.fst0)
    if p.state is not None:
        ins.update({"state_" + k: v for k, v in p.state.items()})
    g.freeze(**ins)
    res = L._run(env, p, **kw)
    torch.cuda.synchronize()
    g.assert_bands_intact()
    g.assert_fully_written(res)
    g.assert_inputs_unchanged()
    return res


@pytest.mark.parametrize("n,steps", [(300, 3), (300, 1), (1, 3), (1, 1)])
@pytest.mark.parametrize("task", ["lander3d", "lander1d"])
def test_lqg_outputs_are_written_exactly(n, steps, task):
    import torch
    rng = np.random.default_rng(11000 + 10 * n + steps)
    env = L._env(task, n, seed=3)
    try:
        env.reset()
        p = L._problem(env, task, rng, steps=steps)
        stored = L._problem(env, task, rng, steps=steps, stored=True)
        with guarded(n) as g:
            first = _guarded_call(g, env, p)
            assert first.filter.P_tape is None and len(g.allocations) >= 16      # (5 + 1 + 1 + 9 tensors)
            res = _guarded_call(g, env, p, tape=True)
            assert tuple(res.filter.P_tape.shape) == (steps, n, 12, 12)
            res = _guarded_call(g, env, p, tape=True, dtype=torch.float32)
            assert res.filter.P_tape.dtype == torch.float32 and res.filter.x.dtype == torch.float64
            g.refill(first)                                  # (the same K, M, dtype and tape: the first call's buffers)
            res = _guarded_call(g, env, stored)
            assert res.actions.data_ptr() == first.actions.data_ptr()
            assert tuple(res.actions.shape) == (steps, n, L.lqg_ref.TASK_A[task])
    finally:
        env.close()
