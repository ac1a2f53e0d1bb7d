"""The memory contract of CopterVecEnv.rollout_pf_smooth with tests/guarded_outputs.py, as tests/test_gpu_output_bounds.py
holds the class body's entry points to it -- a call writes nothing outside the arrays it is given, it writes every element
of every tensor it returns (but row K-1 of the two diagnostic tapes when the caller gives the last row: the header says
so, and the test holds it to that too), and it modifies no input -- and the optional outputs of cs_pf_smooth, NULL.

CopterVecEnv.rollout_pf_smooth wires every output it allocates, so the kernel's `!= nullptr` branches run only for C
callers; the smoother has no row in tests/null_outputs.py's table (a closed list), so this file sets its blocks' pointers
to NULL the way tests/test_gpu_urts_null_outputs.py does: the library object's function attribute is replaced for a block
by a callable that nulls the named members of the byref'd io blocks, forwards the call and puts them back.  Each optional
output NULL in turn, all but one NULL, and all NULL: the call succeeds, a nulled tensor keeps the guard's fill in every
byte, every other tensor has the full call's bits.  (x and var share two workgroup reductions that run when either is
wanted, which is why the subsets matter.)"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import pf_ref
import test_gpu_rollout_pf as F
from gpu_util import have_gpu
from guarded_outputs import _int_view, _walk, guarded

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K = pf_ref.TEST_N, pf_ref.TEST_K
OPTIONAL = ("RolloutIO.x_dev", "PfSmoothIO.var_dev", "PfSmoothIO.idx_dev", "PfSmoothIO.idx0_dev", "PfSmoothIO.ok_dev",
            "PfSmoothIO.logb_tape_dev", "PfSmoothIO.bwq_tape_dev")
REQUIRED = ("RolloutIO.actions_dev", "PfSmoothIO.part_tape_dev", "PfSmoothIO.pstatus_tape_dev", "PfSmoothIO.lw_tape_dev",
            "PfSmoothIO.wq_tape_dev", "PfSmoothIO.Linv_dev")


def _holds_fill(g, t):
    pattern = int.from_bytes(bytes([g.fill]) * t.element_size(), "little", signed=True)
    return bool((_int_view(t) == pattern).all())


def _setup(env, rng, P):
    p = F._problem(env, "lander3d", rng)
    filt = F._clone(F._run(env, p, P))
    k0 = 4           # the rows k0 .. K-1, started from the filter's row k0 - 1
    sub = type(filt)(*[None] * 12, *(t[k0:] for t in (filt.part_tape, filt.pstatus_tape, filt.lw_tape, filt.wq_tape)), None)
    start = tuple(t[k0 - 1].clone() for t in (filt.part_tape, filt.pstatus_tape, filt.lw_tape))
    return p, filt, sub, start, k0


@pytest.mark.parametrize("P,S,dtype", [(64, 5, None), (256, 64, "float32"), (1024, 80, None)])
def test_outputs_are_written_fully_and_nothing_else(P, S, dtype):
    import torch
    rng = np.random.default_rng(2600 + P)
    env = F._env("lander3d", N)
    try:
        env.reset()
        p, filt, sub, start, k0 = _setup(env, rng, P)
        dt = None if dtype is None else getattr(torch, dtype)
        end = torch.randint(0, P, (N, S), dtype=torch.int32, device=env.device,
                            generator=torch.Generator(device=env.device).manual_seed(P))
        tapes = dict(part_tape=filt.part_tape, pstatus_tape=filt.pstatus_tape, lw_tape=filt.lw_tape, wq_tape=filt.wq_tape)

        def run(g, call, except_=lambda res: (), **inputs):
            g.release()
            g.freeze(**inputs)
            res = call()
            torch.cuda.synchronize()
            g.assert_bands_intact()
            g.assert_fully_written(res, except_=except_(res))
            g.assert_inputs_unchanged()
            return res
        kw = dict(paths=S, nonce=3, dtype=dt)
        with guarded(N) as g:
            a = run(g, lambda: env.rollout_pf_smooth(p["acts"], filt, p["Q"], **kw), actions=p["acts"], **tapes)
            assert a.logb_tape is None and a.idx0 is None and tuple(a.idx.shape) == (K, N, S)
            b = run(g, lambda: env.rollout_pf_smooth(p["acts"], filt, p["Q"], tapes=True, **kw), actions=p["acts"], **tapes)
            assert tuple(b.logb_tape.shape) == tuple(b.bwq_tape.shape) == (K, N, S, P)
            # a chunk: a start set and the caller's last row, from tensors of the caller's own
            c = run(g, lambda: env.rollout_pf_smooth(p["acts"][k0:], sub, p["Q"], first_step=k0 + 1, start=start, end=end,
                                                     **kw),
                    actions=p["acts"], part=start[0], pstatus=start[1], lw=start[2], end=end, **tapes)
            assert tuple(c.idx0.shape) == (N, S) and torch.equal(c.idx[-1], end)
            # ... and with the diagnostic tapes: their row K-1 is not written when the last row is the caller's
            d = run(g, lambda: env.rollout_pf_smooth(p["acts"][k0:], sub, p["Q"], first_step=k0 + 1, start=start, end=end,
                                                     tapes=True, **kw),
                    except_=lambda res: (res.logb_tape, res.bwq_tape),
                    actions=p["acts"], part=start[0], pstatus=start[1], lw=start[2], end=end, **tapes)
            assert _holds_fill(g, d.logb_tape[-1]) and _holds_fill(g, d.bwq_tape[-1])
            g.assert_fully_written((d.logb_tape[:-1], d.bwq_tape[:-1]))
            assert torch.equal(d.idx, c.idx) and torch.equal(d.idx0, c.idx0)
    finally:
        env.close()


@contextlib.contextmanager
def _nulling(lib, fields, calls):
    """cs_pf_smooth with the members `fields` ("Struct.member") of its blocks NULL; calls collects (seen, rc, message)"""
    real = lib.cs_pf_smooth

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

    lib.cs_pf_smooth = forward
    try:
        yield
    finally:
        lib.cs_pf_smooth = real


@pytest.mark.parametrize("P,S", [(64, 5), (512, 70)])
def test_each_optional_output_null_leaves_the_others_bits(P, S):
    import torch
    rng = np.random.default_rng(2700 + P)
    env = F._env("lander3d", N)
    try:
        env.reset()
        p, filt, sub, start, k0 = _setup(env, rng, P)
        call = lambda: env.rollout_pf_smooth(p["acts"][k0:], sub, p["Q"], paths=S, nonce=3, first_step=k0 + 1,      # noqa: E731
                                             start=start, tapes=True)
        with guarded(N) as g:
            g.freeze(actions=p["acts"], part_tape=filt.part_tape, pstatus_tape=filt.pstatus_tape, lw_tape=filt.lw_tape,
                     wq_tape=filt.wq_tape, part=start[0], pstatus=start[1], lw=start[2])
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
    import torch
    from gym_copter_amd import CopterStepError
    rng = np.random.default_rng(2800)
    P, S = 64, 5
    env = F._env("lander3d", N)
    try:
        env.reset()
        p, filt, sub, start, k0 = _setup(env, rng, P)
        call = lambda **kw: env.rollout_pf_smooth(p["acts"], filt, p["Q"], paths=S, **kw)      # noqa: E731
        good = F._clone(call())
        for f in REQUIRED:
            calls = []
            with _nulling(env._lib, (f,), calls):
                with pytest.raises(CopterStepError):
                    call()
            seen, rc, msg = calls[-1]
            assert rc == -1 and msg.startswith("cs_pf_smooth: ") and f.split(".")[1] in msg, (f, msg)
        # a partial start triple, and idx0 left without its start
        for f in ("PfSmoothIO.part_in_dev", "PfSmoothIO.pstatus_in_dev", "PfSmoothIO.lw_in_dev"):
            calls = []
            with _nulling(env._lib, (f,), calls):
                with pytest.raises(CopterStepError, match="all three or none"):
                    env.rollout_pf_smooth(p["acts"][k0:], sub, p["Q"], paths=S, first_step=k0 + 1, start=start)
        calls = []
        with _nulling(env._lib, ("PfSmoothIO.part_in_dev", "PfSmoothIO.pstatus_in_dev", "PfSmoothIO.lw_in_dev"), calls):
            with pytest.raises(CopterStepError, match="idx0_dev needs"):
                env.rollout_pf_smooth(p["acts"][k0:], sub, p["Q"], paths=S, first_step=k0 + 1, start=start)
        # with the caller's last row the wq tape is not read: NULL is accepted there
        end = torch.zeros((N, S), dtype=torch.int32, device=env.device)
        with _nulling(env._lib, ("PfSmoothIO.wq_tape_dev",), calls):
            call(end=end)
        assert calls[-1][1] == 0
        # ... and the refusals left nothing behind: the next call gives the clean bits
        for a, b in zip(call(), good):
            assert (a is None and b is None) or torch.equal(a, b)
    finally:
        env.close()
