"""CPU-side checks of cs_rollout_lqr / cs_rollout_feedback_states: the NumPy restatement the GPU tests hold the kernel
to (tests/lqr_ref.py) against the dense solution of the stacked quadratic programme; both entry points declared,
exported and bound, the ctypes structs mirroring the header; bad argument blocks refused without touching a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_copter_amd import _lib
from lqr_ref import chol_solve, cholesky, dense_qp, feedback_action, lqr_backward

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()


def _problem(rng, K, A):
    """random time-varying (A_k, B_k, q_k, r_k) and PD (Q, Q_final, R), scaled for a well-conditioned KKT system"""
    Ab = np.eye(12) + 0.3 * rng.standard_normal((K, 12, 12)) / np.sqrt(12)
    Bb = rng.standard_normal((K, 12, A))
    m = rng.standard_normal((12, 12))
    Q = m @ m.T / 12 + np.eye(12)
    m = rng.standard_normal((12, 12))
    Qf = m @ m.T / 12 + 2 * np.eye(12)
    m = rng.standard_normal((A, A))
    R = m @ m.T / A + np.eye(A)
    return Ab, Bb, Q, Qf, R, rng.standard_normal((K, 12)), rng.standard_normal((K, A))


@pytest.mark.parametrize("A", [1, 2, 4])
@pytest.mark.parametrize("K", [1, 3, 6])
def test_recursion_solves_the_stacked_quadratic_programme(K, A):
    """mu = 0: d_1 and K_1 are the first-step block of the QP's minimiser (as a function of dx_0), and dV1 + dV2 its
    optimal decrease.  The QP is exactly quadratic, so the tolerance is that of the dense solve: 1e-9 x cond(KKT)."""
    rng = np.random.default_rng(1000 + 10 * K + A)
    for final in (False, True):
        Ab, Bb, Q, Qf, R, q, r = _problem(rng, K, A)
        Qf = Qf if final else None
        out = lqr_backward(Ab[:, None], Bb[:, None], Q, R, q[:, None], r[:, None], Q_final=Qf)
        d1, K1, dec, cond = dense_qp(Ab, Bb, Q, R, q, r, Q_final=Qf)
        tol = 1e-9 * cond
        assert tol < 1e-2, cond
        assert out["ok"].all()
        assert np.max(np.abs(out["d"][0, 0] - d1)) <= tol * max(1.0, np.abs(d1).max())
        assert np.max(np.abs(out["K"][0, 0] - K1)) <= tol * max(1.0, np.abs(K1).max())
        assert abs(out["dV"][0].sum() - dec) <= tol * max(1.0, abs(dec))
        assert dec < 0
        # the value model at the start: V(dx_0) - V(0) = s0^T dx_0 + 1/2 dx_0^T S0 dx_0 is symmetric PSD
        assert np.array_equal(out["S0"][0], out["S0"][0].T) and np.linalg.eigvalsh(out["S0"][0]).min() > -1e-9


def test_recursion_in_longdouble_agrees_and_levenberg_shrinks_the_step():
    rng = np.random.default_rng(5)
    Ab, Bb, Q, Qf, R, q, r = _problem(rng, 5, 4)
    a = lqr_backward(Ab[:, None], Bb[:, None], Q, R, q[:, None], r[:, None])
    b = lqr_backward(Ab[:, None], Bb[:, None], Q, R, q[:, None], r[:, None], dtype=np.longdouble)
    for k in ("K", "d", "dV", "S0", "s0"):
        assert b[k].dtype == np.longdouble
        assert np.max(np.abs(a[k] - b[k].astype(np.float64))) < 1e-11
    c = lqr_backward(Ab[:, None], Bb[:, None], Q, R, q[:, None], r[:, None], mu=10.0)
    assert np.linalg.norm(c["d"]) < np.linalg.norm(a["d"])


def test_cholesky_restatement():
    rng = np.random.default_rng(6)
    m = rng.standard_normal((50, 4, 4))
    m = m @ np.swapaxes(m, 1, 2) + 0.5 * np.eye(4)
    b = rng.standard_normal((50, 4))
    l, ok = cholesky(m)
    assert ok.all()
    np.testing.assert_allclose(l, np.linalg.cholesky(m), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(chol_solve(l, b), np.linalg.solve(m, b[..., None])[..., 0], rtol=1e-9)
    bad = np.array([[[1.0, 2.0], [2.0, 1.0]], [[0.0, 0.0], [0.0, 1.0]], [[np.nan, 0.0], [0.0, 1.0]],
                    [[2.0, 1.0], [1.0, 2.0]]])
    assert cholesky(bad)[1].tolist() == [False, False, False, True]


def test_feedback_action_formula():
    """float64 throughout, one rounding: equal to the exactly rounded sum where that sum is exact in float64"""
    abar = np.array([[0.5, 0.25]], np.float32)
    K = np.zeros((1, 2, 12))
    K[0, 0, 3], K[0, 1, 11] = 0.5, -2.0
    x, xbar = np.zeros((1, 12)), np.zeros((1, 12))
    x[0, 3], x[0, 11], xbar[0, 11] = 0.25, 1.0, 0.5
    a = feedback_action(abar, np.array([0.5]), np.array([[0.25, -0.125]]), K, x, xbar)
    assert a.dtype == np.float32 and a.tolist() == [[0.5 + 0.125 + 0.125, 0.25 - 0.0625 - 1.0]]
    a = feedback_action(abar, np.array([0.0]), np.array([[7.0, 7.0]]), K)
    assert np.array_equal(a, abar)


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    for name, struct, mirror in (("cs_rollout_lqr", "cs_rollout_lqr_io", _lib.RolloutLqrIO),
                                 ("cs_rollout_feedback_states", "cs_rollout_feedback_io", _lib.RolloutFeedbackIO)):
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const %s\* \w+,\s*void\* stream\);"
                         % (name, struct), HEADER)
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes[2] is C.POINTER(mirror)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert fields == [f for f, _ in mirror._fields_]
    assert C.sizeof(_lib.RolloutLqrIO) == 16 + 11 * 8 and C.sizeof(_lib.RolloutFeedbackIO) == 8 + 5 * 8


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev, io.x_dev, io.status_dev = 0x1000, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _lio(**kw):
    lio = _lib.RolloutLqrIO()
    lio.struct_size = C.sizeof(lio)
    lio.Q_dev, lio.R_dev = 0x6000, 0x7000
    for k, v in kw.items():
        setattr(lio, k, v)
    return lio


def _fio(**kw):
    fio = _lib.RolloutFeedbackIO()
    fio.struct_size = C.sizeof(fio)
    fio.xbar_dev, fio.K_dev, fio.d_dev, fio.alpha_dev, fio.actions_out_dev = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(fio, k, v)
    return fio


def test_lqr_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_lqr
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in lib.cs_last_error()
    assert fn(None, C.byref(_io(x_dev=None)), C.byref(_lio()), None) == _lib.ERR_ARG
    assert b"tape" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null lio" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_lio(struct_size=C.sizeof(_lib.RolloutLqrIO) - 8)), None) == _lib.ERR_ABI
    assert b"struct_size" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_lio(out_dtype=5)), None) == _lib.ERR_ARG
    assert b"out_dtype" in lib.cs_last_error()
    for key in ("Q_dev", "R_dev"):
        assert fn(None, C.byref(_io()), C.byref(_lio(**{key: None})), None) == _lib.ERR_ARG
        assert b"required" in lib.cs_last_error()
    for mu in (-1.0, float("inf"), float("nan")):
        assert fn(None, C.byref(_io()), C.byref(_lio(mu=mu)), None) == _lib.ERR_ARG
        assert b"mu must be" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_lio(mu=0.5)), None) == _lib.ERR_ARG    # ... as far as the context
    assert lib.cs_last_error() == b"null context"


def test_feedback_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_feedback_states
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in lib.cs_last_error()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_fio()), None) == _lib.ERR_ARG
    assert b"actions_dev" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null fio" in lib.cs_last_error()
    bad = _fio(struct_size=C.sizeof(_lib.RolloutFeedbackIO) + 8)
    assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in lib.cs_last_error()
    for key in ("K_dev", "d_dev", "alpha_dev", "actions_out_dev"):
        assert fn(None, C.byref(_io()), C.byref(_fio(**{key: None})), None) == _lib.ERR_ARG
        assert b"required" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_fio(xbar_dev=None)), None) == _lib.ERR_ARG
    assert b"xbar_dev" in lib.cs_last_error()
    assert fn(None, C.byref(_io(num_steps=1)), C.byref(_fio(xbar_dev=None)), None) == _lib.ERR_ARG
    assert lib.cs_last_error() == b"null context"
    assert fn(None, C.byref(_io()), C.byref(_fio()), None) == _lib.ERR_ARG and lib.cs_last_error() == b"null context"
