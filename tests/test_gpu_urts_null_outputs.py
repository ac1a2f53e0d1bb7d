"""Optional outputs of cs_urts_smooth, NULL.  CopterVecEnv.rollout_urts always wires every output, so the kernel's
`!= nullptr` branches run only for C callers; the smoother has no row in tests/null_outputs.py's table (a closed list),
so this file sets its blocks' pointers to NULL directly: the library object's function attribute is replaced for a block
by a callable that nulls the named members of the byref'd io blocks, forwards the call and puts them back.

Each optional output -- io's x_dev and the block's P_tape_dev, var_dev, x0_dev, P0_s_dev, ok_dev -- NULL in turn, all but
one NULL, and all NULL: the call succeeds, a nulled tensor keeps the guard's fill in every byte, every other tensor has
the full call's bits, the guard bands stay intact and the inputs unchanged.  The stores through the stage (x, P_tape, P0)
share wave_sync() sequences, which is why the subsets matter.  Required pointers NULL are refused with a message that
names them."""
import contextlib
import ctypes as C

import pytest

import test_gpu_rollout_ekf as E
import test_gpu_rollout_ukf as U
import test_gpu_urts as T
import ukf_ref
from gpu_util import have_gpu
from guarded_outputs import _int_view, _walk, guarded

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

OPTIONAL = ("RolloutIO.x_dev", "RolloutUrtsIO.P_tape_dev", "RolloutUrtsIO.var_dev", "RolloutUrtsIO.x0_dev",
            "RolloutUrtsIO.P0_s_dev", "RolloutUrtsIO.ok_dev")
REQUIRED = ("RolloutIO.actions_dev", "RolloutIO.start_x_dev", "RolloutIO.start_status_dev", "RolloutUrtsIO.x_f_dev",
            "RolloutUrtsIO.x_pred_dev", "RolloutUrtsIO.status_f_dev", "RolloutUrtsIO.P_f_dev", "RolloutUrtsIO.Q_dev",
            "RolloutUrtsIO.P0_dev", "RolloutUrtsIO.workspace_dev")


@contextlib.contextmanager
def _nulling(lib, fields, calls):
    """cs_urts_smooth with the members `fields` ("Struct.member") of its blocks NULL; calls collects (seen, rc, message)"""
    real = lib.cs_urts_smooth

    def forward(*args):
        blocks = {type(a._obj).__name__: a._obj for a in args if isinstance(getattr(a, "_obj", None), C.Structure)}
        seen = {f: getattr(blocks[f.split(".")[0]], f.split(".")[1]) or 0 for f in OPTIONAL + REQUIRED}
        saved = [(blocks[f.split(".")[0]], f.split(".")[1]) for f in fields]
        saved = [(b, m, getattr(b, m)) for b, m in saved]
        try:
            for b, m, _ in saved:
                setattr(b, m, None)
            rc = real(*args)
        finally:
            for b, m, v in saved:
                setattr(b, m, v)
        calls.append((seen, rc, lib.cs_last_error().decode("utf-8", "replace") if rc != 0 else ""))
        return rc

    lib.cs_urts_smooth = forward
    try:
        yield
    finally:
        lib.cs_urts_smooth = real


def _holds_fill(g, t):
    pattern = int.from_bytes(bytes([g.fill]) * t.element_size(), "little", signed=True)
    return bool((_int_view(t) == pattern).all())


@pytest.mark.parametrize("n,with_end", [(65, False), (65, True), (300, False)])
def test_each_optional_output_null_leaves_the_others_bits(n, with_end):
    import torch
    K = 3
    setting = ukf_ref.SETTINGS[1]
    env = E._env("lander3d", n, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs("lander3d", n, K, seed=14000 + n))
        filt = T._filter(env, p, setting)
        end = (filt.x[-1].T.contiguous() + 0.01, filt.P_tape[-1] * 0.5) if with_end else None
        call = lambda: T._urts(env, p, filt, setting, end=end)          # noqa: E731
        with guarded(n) as g:
            g.freeze(actions=p["acts"], x_f=filt.x, x_pred=filt.x_pred, status_f=filt.status, P_f=filt.P_tape, x0=p["x0"],
                     P0=p["P0"])
            calls = []
            with _nulling(env._lib, (), calls):
                res = call()
            torch.cuda.synchronize()
            seen, rc, _ = calls[-1]
            assert rc == 0 and all(seen[f] for f in OPTIONAL + REQUIRED)
            g.assert_bands_intact()
            g.assert_fully_written(res)
            full = [(path, t, t.clone()) for path, t in _walk(res)]
            assert {seen[f] for f in OPTIONAL} == {t.data_ptr() for _, t, _ in full}
            plans = [(f,) for f in OPTIONAL] + [tuple(o for o in OPTIONAL if o != f) for f in OPTIONAL] + [OPTIONAL]
            for nulled in plans:
                what = "%s nulled" % " ".join(nulled)
                g.refill(res)
                with _nulling(env._lib, nulled, calls):
                    again = call()
                torch.cuda.synchronize()
                assert calls[-1][1] == 0, (what, calls[-1][2])
                gone = {seen[f] for f in nulled}
                for (path, t), (_, _, clone) in zip(_walk(again), full):
                    if t.data_ptr() in gone:
                        assert _holds_fill(g, t), "%s: %s was written" % (what, path)
                    else:
                        assert torch.equal(t, clone), "%s: %s has other bits than the full call's" % (what, path)
                g.assert_bands_intact()
            g.assert_inputs_unchanged()
    finally:
        env.close()


def test_required_pointers_null_are_refused_by_name():
    from gym_copter_amd import CopterStepError
    n, K = 65, 3
    env = E._env("lander3d", n, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs("lander3d", n, K, seed=14100))
        filt = T._filter(env, p)
        good = U._clone(T._urts(env, p, filt))
        for f in REQUIRED:
            calls = []
            with _nulling(env._lib, (f,), calls):
                with pytest.raises(CopterStepError):
                    T._urts(env, p, filt)
            seen, rc, msg = calls[-1]
            member = f.split(".")[1]
            assert rc == -1 and msg.startswith("cs_urts_smooth: ") and member in msg, (f, msg)
        # a half-given end row
        end = (filt.x[-1].T.contiguous(), filt.P_tape[-1].clone())
        for f in ("RolloutUrtsIO.end_x_dev", "RolloutUrtsIO.end_P_dev"):
            calls = []
            with _nulling(env._lib, (f,), calls):
                with pytest.raises(CopterStepError, match="both or neither"):
                    T._urts(env, p, filt, end=end)
        # ... and the refusals left nothing behind: the next call gives the clean bits
        assert T._same(T._urts(env, p, filt), good)
    finally:
        env.close()
