"""The memory contract of CopterVecEnv.rollout_ukf with tests/guarded_outputs.py, as tests/test_gpu_output_bounds.py
holds the other entry points to it: the call writes nothing outside the arrays it is given (every output sits between two
bands of the byte 0xA5), it writes every element of every tensor it returns -- the point tapes of a LANDED step included
-- and it modifies no input tensor.  N = 300 (four whole wavefronts and one of 44 lanes: both store paths) and N = 1; with
and without the covariance tape and the point tapes, float64 and float32 outputs.  Every comparison is exact."""
import numpy as np
import pytest

import test_gpu_rollout_ukf as U
from gpu_util import have_gpu
from guarded_outputs import guarded
from oracle.refcpu import LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]


def _guarded_call(g, env, p, **kw):
    import torch
    g.release()
    g.freeze(actions=p["acts"], z=p["z"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
    res = U._run(env, p, **kw)
    torch.cuda.synchronize()
    g.assert_bands_intact()
    g.assert_fully_written(res)
    g.assert_inputs_unchanged()
    return res


@pytest.mark.parametrize("n,steps", [(300, 3), (300, 1), (1, 3), (1, 1)])
@pytest.mark.parametrize("task", ["lander3d", "lander1d"])
def test_ukf_outputs_are_written_exactly(n, steps, task):
    import torch
    env = U.E._env(task, n, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs(task, n, steps, seed=12000 + 10 * n + steps))
        if n == 1:                                                # (the lone env flies: also run it LANDED below)
            grounded = dict(p, st0=torch.full((1,), int(LANDED), dtype=torch.uint8, device=env.device))
        else:
            assert (np.asarray(p["grp"]) == "landed").any()
            grounded = None
        with guarded(n) as g:
            first = _guarded_call(g, env, p)
            assert first.P_tape is None and first.points is None and len(g.allocations) >= 9
            res = _guarded_call(g, env, p, tape=True)
            assert tuple(res.P_tape.shape) == (steps, n, 12, 12) and res.points is None
            res = _guarded_call(g, env, p, points=True)
            assert tuple(res.points.shape) == (steps, n, 25, 12) and res.P_tape is None
            assert tuple(res.points_pred.shape) == (steps, n, 25, 12) and tuple(res.point_status.shape) == (steps, n, 25)
            res = _guarded_call(g, env, p, tape=True, points=True, dtype=torch.float32)
            assert res.P_tape.dtype == torch.float32 and res.x.dtype == torch.float64 and res.points.dtype == torch.float64
            if grounded is not None:
                g.refill(res)                                     # (the same K, dtype, tape and points: those buffers)
                again = _guarded_call(g, env, grounded, tape=True, points=True, dtype=torch.float32)
                assert again.points.data_ptr() == res.points.data_ptr()
                assert bool((again.point_status == int(LANDED)).all())
    finally:
        env.close()
