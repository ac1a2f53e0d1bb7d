"""The memory contract of CopterVecEnv.rollout_urts with tests/guarded_outputs.py, as tests/test_gpu_output_bounds.py
holds the class body's entry points to it: a call writes nothing outside the arrays it is given -- its workspace among
them, whose bands are checked like any other allocation's --, it writes every element of every tensor it returns, and it
modifies no input.  N = 300 (four whole wavefronts and one of 44 lanes: both store paths) and N = 1, K = 3 and K = 1,
with and without the covariance tape and the caller's end row, float64 and float32 outputs."""
import pytest

import test_gpu_rollout_ekf as E
import test_gpu_rollout_ukf as U
import test_gpu_urts as T
import ukf_ref
from gpu_util import have_gpu
from guarded_outputs import guarded

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]


@pytest.mark.parametrize("n,K", [(300, 3), (300, 1), (1, 3), (1, 1)])
def test_smoother_outputs_are_written_exactly(n, K):
    import torch
    from gym_copter_amd import _lib
    setting = ukf_ref.SETTINGS[1]
    env = E._env("lander3d", n, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs("lander3d", n, K, seed=13000 + 10 * n + K))
        filt = T._filter(env, p, setting)
        end = (filt.x[-1].T.contiguous() + 0.01, filt.P_tape[-1] * 0.5)
        ins = dict(actions=p["acts"], x_f=filt.x, x_pred=filt.x_pred, status_f=filt.status, P_f=filt.P_tape, x0=p["x0"],
                   P0=p["P0"], status0=p["st0"], end_x=end[0], end_P=end[1])
        with guarded(n) as g:
            for kw in (dict(), dict(tape=False), dict(end=end), dict(end=end, tape=False), dict(dtype=torch.float32),
                       dict(dtype=torch.float32, tape=False, end=end)):
                g.release()
                g.freeze(**ins)
                res = T._urts(env, p, filt, setting, **kw)
                torch.cuda.synchronize()
                g.assert_bands_intact()
                g.assert_fully_written(res)
                g.assert_inputs_unchanged()
                assert (res.P_tape is None) == (kw.get("tape") is False) and res.x.shape == (K, n, 12)
            # the workspace is one of the guarded allocations: a column of 102 float64 per lane of every tile
            shapes = [a.shape for a in g.allocations]
            # (the four cached sets of outputs -- two dtypes, with and without the tape -- and the workspace)
            assert ((n + 63) // 64, _lib.URTS_WORKSPACE_ROWS, 64) in shapes and len(g.allocations) >= 6 + 5 + 6 + 5 + 1
    finally:
        env.close()
