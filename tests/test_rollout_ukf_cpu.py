"""CPU-side checks of cs_rollout_ukf: the entry point declared, exported and bound, the ctypes struct mirroring the header
field by field; bad argument blocks refused without touching a device; the sigma points and moments of the kernel's own
header compiled for the host (tests/host/ukf_points_host) against the NumPy restatement the GPU tests hold the kernel to
(tests/ukf_ref.py), bit for bit; self-checks of that restatement (these pass without the feature and are labelled so);
and the inputs of the GPU tests -- the touchdown starts and the application -- on the restatement over the float64
oracle's step, so that no device sees an input that does not meet its test's conditions."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ekf_ref
import ukf_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "ukf_points_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors (these fail without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    import gym_copter_amd
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    lib = _lib.load()
    assert re.search(r"int cs_rollout_ukf\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_rollout_ukf_io\* \w+,"
                     r"\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_rollout_ukf") and "cs_rollout_ukf" in _lib.SYMBOLS
    assert lib.cs_rollout_ukf.argtypes[2] is C.POINTER(_lib.RolloutUkfIO)
    from gym_copter_amd.ukf import rollout_ukf, ukf, UkfResult
    assert gym_copter_amd.CopterVecEnv.rollout_ukf is rollout_ukf and gym_copter_amd.ukf is ukf
    assert gym_copter_amd.UkfResult is UkfResult and hasattr(ShardedCopterVecEnv, "rollout_ukf")
    # bound, not defined, in the class body (as every family's wrappers are)
    src = open(os.path.join(ROOT, "gym_copter_amd", "vecenv.py")).read()
    assert re.search(r"^    rollout_ukf = _ukf\.rollout_ukf$", src, re.M) and "def rollout_ukf" not in src


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_rollout_ukf_io \{(.*?)\} cs_rollout_ukf_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.RolloutUkfIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.RolloutUkfIO._fields_):
        size = 8 if "*" in ctype or "double" in ctype else 4
        assert C.sizeof(mirror) == size, name
        assert (mirror is C.c_double) == ("double" in ctype and "*" not in ctype), name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.RolloutUkfIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.RolloutUkfIO) == offset == 16 + 4 * 8 + 16 * 8


def test_the_abi_version_is_unchanged():
    assert _lib.load().cs_version() == 5 == _lib.ABI_VERSION
    assert re.search(r"#define CS_ABI_VERSION 5\b", HEADER)


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev, io.start_x_dev, io.start_status_dev, io.x_dev, io.status_dev = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _uio(**kw):
    uio = _lib.RolloutUkfIO()
    uio.struct_size = C.sizeof(uio)
    uio.num_meas = 6
    uio.gamma, uio.wm0, uio.wc0, uio.wi = (float(v) for v in ukf_ref.weights())
    uio.H_dev, uio.r_dev, uio.Q_dev, uio.P0_dev, uio.z_dev = 0x6000, 0x7000, 0x8000, 0x9000, 0xa000
    for k, v in kw.items():
        setattr(uio, k, v)
    return uio


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_ukf
    err = lib.cs_last_error
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in err()
    assert fn(None, C.byref(_io(struct_size=8)), C.byref(_uio()), None) == _lib.ERR_ABI
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null uio" in err()
    # a wrong struct_size is reported before anything else in the block
    bad = _uio(struct_size=C.sizeof(_lib.RolloutUkfIO) - 8, num_meas=99, H_dev=None, gamma=-1.0)
    assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in err()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_uio()), None) == _lib.ERR_ARG and b"num_steps" in err()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_uio()), None) == _lib.ERR_ARG and b"actions_dev" in err()
    assert fn(None, C.byref(_io(start_x_dev=None, start_status_dev=None)), C.byref(_uio()), None) == _lib.ERR_ARG
    assert b"start_x_dev" in err()
    assert fn(None, C.byref(_io(start_status_dev=None)), C.byref(_uio()), None) == _lib.ERR_ARG
    assert b"start_status_dev" in err()
    for key in ("start_force_dev", "start_prev_shaping_dev"):
        assert fn(None, C.byref(_io(**{key: 0xb000})), C.byref(_uio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err()
    for key in ("reward_dev", "terminated_dev", "truncated_dev", "gx_dev", "gr_dev", "g_actions_dev", "g_x0_dev"):
        assert fn(None, C.byref(_io(**{key: 0xb000})), C.byref(_uio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err()
    assert fn(None, C.byref(_io()), C.byref(_uio(out_dtype=5)), None) == _lib.ERR_ARG and b"out_dtype" in err()
    for m in (0, -1, 13):
        assert fn(None, C.byref(_io()), C.byref(_uio(num_meas=m)), None) == _lib.ERR_ARG and b"num_meas" in err()
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(None, C.byref(_io()), C.byref(_uio(gamma=g)), None) == _lib.ERR_ARG and b"gamma" in err()
    for key in ("wm0", "wc0", "wi"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert fn(None, C.byref(_io()), C.byref(_uio(**{key: v})), None) == _lib.ERR_ARG and b"weights" in err()
    for key in ("H_dev", "r_dev", "Q_dev", "P0_dev", "z_dev"):
        assert fn(None, C.byref(_io()), C.byref(_uio(**{key: None})), None) == _lib.ERR_ARG and b"required" in err()
    for key in ("H_dev", "r_dev", "Q_dev", "P0_dev", "z_dev", "x_pred_dev", "P_tape_dev", "nis_dev", "points_dev",
                "points_pred_dev"):
        assert fn(None, C.byref(_io()), C.byref(_uio(**{key: 0xc004})), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io(x_dev=0x4004)), C.byref(_uio()), None) == _lib.ERR_ARG and b"aligned" in err()
    # float32 outputs need 4 bytes only; negative and zero weights are weights
    ok32 = _uio(out_dtype=_lib.JAC_F32, P_tape_dev=0xc004, nis_dev=0xc004, wm0=-3.0, wc0=-0.25)
    assert fn(None, C.byref(_io()), C.byref(ok32), None) == _lib.ERR_ARG and err() == b"null context"
    assert fn(None, C.byref(_io(x_dev=None, status_dev=None)), C.byref(_uio(wm0=0.0)), None) == _lib.ERR_ARG
    assert err() == b"null context"                                                   # ... as far as the context


def test_python_weights_are_the_restatements_and_refuse_a_nonpositive_scale():
    from gym_copter_amd.ukf import weights
    for s in ukf_ref.SETTINGS:
        assert weights(*s) == tuple(float(v) for v in ukf_ref.weights(*s))
    assert weights() == weights(1.0, 0.0, 1.0) and min(weights()) > 0
    assert weights(0.5, 2.0, 0.0)[1:3] == (-3.0, -0.25) and weights(1.0, 0.0, 0.0)[1] == 0.0
    for bad in ((1.0, 0.0, -12.0), (0.0, 0.0, 1.0), (1.0, 0.0, -13.0), (float("nan"), 0.0, 1.0)):
        with pytest.raises(ValueError):
            weights(*bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the points header on the host (fails without the feature: the program is its code)
# ---------------------------------------------------------------------------------------------------------------------
def _unpack(v):
    Pm = np.zeros((12, 12))
    for (i, j), val in zip([(i, j) for j in range(12) for i in range(j + 1)], v):
        Pm[i, j] = Pm[j, i] = val
    return Pm


def _host(w, x, P, Q, y):
    args = [repr(float(v)) for v in np.concatenate([np.asarray(w, np.float64), x, np.ravel(P), np.ravel(Q), np.ravel(y)])]
    out = subprocess.run([HOST] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0] in ("ok 0", "ok 1")
    v = np.array([float.fromhex(s) for s in out[1:1 + 78 + 300 + 12 + 78 + 78]])
    return dict(ok=out[0] == "ok 1", U=np.triu(_unpack(v[:78])), points=v[78:378].reshape(25, 12), x_pred=v[378:390],
                P_pred=_unpack(v[390:468]), P_landed=_unpack(v[468:546]))


def _spd(rng, scale=1.0):
    m = rng.standard_normal((12, 12))
    P = scale * (m @ m.T / 12 + 0.2 * np.eye(12))
    return (P + P.T) / 2


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_host_points_and_moments_match_the_restatement_bit_for_bit(setting):
    rng = np.random.default_rng(int(100 * setting[0] + 10 * setting[1] + setting[2]))
    w = ukf_ref.weights(*setting)
    for _ in range(3):
        x, P, Q = rng.standard_normal(12) * 3, _spd(rng, 0.1), ekf_ref.test_Q()
        pts, ok, U = ukf_ref.points(x[None], P[None], w[0])
        y = np.sin(pts[0]) + 0.3 * pts[0] ** 2 + rng.standard_normal((25, 12)) * 0.01     # any map will do
        xm, Pm = ukf_ref.moments(y[None], w, Q)
        got = _host(w, x, P, Q, y)
        assert got["ok"] and ok[0]
        assert np.array_equal(_bits(got["U"]), _bits(np.triu(U[0])))
        assert np.array_equal(_bits(got["points"]), _bits(pts[0]))
        assert np.array_equal(_bits(got["x_pred"]), _bits(xm[0]))
        assert np.array_equal(_bits(got["P_pred"]), _bits(Pm[0]))
        assert np.array_equal(_bits(got["P_landed"]), _bits(ekf_ref.mirror_upper(P + Q)))
        # point 0 is the mean itself, and the pairs are centred on it
        assert np.array_equal(pts[0, 0], x) and np.allclose(pts[0, 1:13] + pts[0, 13:], 2 * x, rtol=0, atol=1e-14)


def test_host_nonpositive_pivot_clears_ok_and_is_carried_through():
    rng = np.random.default_rng(7)
    w = ukf_ref.weights()
    x, Q = rng.standard_normal(12), ekf_ref.test_Q()
    y = rng.standard_normal((25, 12))
    got = _host(w, x, -np.eye(12), Q, y)
    pts, ok, _ = ukf_ref.points(x[None], -np.eye(12)[None], w[0])
    assert not got["ok"] and not ok[0]
    assert np.isnan(got["points"][1:]).any() and np.array_equal(got["points"][0], x)     # sqrt of a negative pivot
    assert np.array_equal(np.isnan(got["points"]), np.isnan(pts[0]))
    xm, Pm = ukf_ref.moments(y[None], w, Q)
    assert np.array_equal(_bits(got["x_pred"]), _bits(xm[0])) and np.array_equal(_bits(got["P_pred"]), _bits(Pm[0]))
    P = _spd(rng)
    P[5, 5] = 0.0                                                  # a zero pivot further down
    got = _host(w, x, P * np.eye(12), Q, y)
    assert not got["ok"]
    assert _host(w, x, _spd(rng), Q, y)["ok"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. self-checks of the reference (these pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_reference_weights_sum_to_one(setting):
    """passes without the feature"""
    for dtype in (np.float64, np.longdouble):
        g, wm0, wc0, wi = ukf_ref.weights(*setting, dtype=dtype)
        assert abs(wm0 + 24 * wi - 1) <= 4 * np.finfo(dtype).eps
        a, b, k = setting
        assert abs(g * g - a * a * (12 + k)) <= 64 * np.finfo(dtype).eps
        assert abs((wc0 - wm0) - (1 - a * a + b)) <= 8 * np.finfo(dtype).eps


@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_reference_is_exact_for_a_linear_map(setting):
    """passes without the feature: y = A x + b gives x- = A xhat + b and P- = A P A^T + Q, within 1e-12 x cond"""
    rng = np.random.default_rng(50)
    w = ukf_ref.weights(*setting)
    for _ in range(5):
        x, P, Q = rng.standard_normal(12), _spd(rng), _spd(rng, 0.05)
        A, b = np.eye(12) + 0.3 * rng.standard_normal((12, 12)) / np.sqrt(12), rng.standard_normal(12)
        pts, ok, U = ukf_ref.points(x[None], P[None], w[0])
        L = np.triu(U[0]).T.copy()
        L[np.arange(12), np.arange(12)] = 1.0 / np.diag(U[0])
        tol = 1e-12 * np.linalg.cond(P)
        assert ok[0] and tol < 1e-6 and ekf_ref.scaled(L @ L.T, P) <= tol
        xm, Pm = ukf_ref.moments(pts @ A.T + b, w, Q)
        assert ekf_ref.scaled(xm[0], A @ x + b) <= tol and ekf_ref.scaled(Pm[0], A @ P @ A.T + Q) <= tol
        x2, P2 = ukf_ref.moments_two_pass(pts @ A.T + b, w, Q)
        assert ekf_ref.scaled(xm[0], x2[0].astype(np.float64)) <= tol
        assert ekf_ref.scaled(Pm[0], P2[0].astype(np.float64)) <= tol


@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_reference_mean_is_second_order_accurate(setting):
    """passes without the feature: for y = x^T M x the predicted mean is xhat^T M xhat + tr(M P)"""
    rng = np.random.default_rng(60)
    w = ukf_ref.weights(*setting)
    for _ in range(5):
        x, P = rng.standard_normal(12), _spd(rng)
        Mq = rng.standard_normal((12, 12))
        pts, ok, _ = ukf_ref.points(x[None], P[None], w[0])
        y = np.zeros((1, 25, 12))
        y[0, :, 0] = np.einsum("ia,ab,ib->i", pts[0], Mq, pts[0])
        xm, _ = ukf_ref.moments(y, w, np.zeros((12, 12)))
        want = x @ Mq @ x + np.trace(Mq @ P)
        assert abs(xm[0, 0] - want) <= 1e-12 * np.linalg.cond(P) * max(1.0, abs(want))


def test_reference_in_longdouble_agrees():
    """passes without the feature"""
    rng = np.random.default_rng(61)
    n = 40
    x, P = rng.standard_normal((n, 12)), np.array([_spd(rng, 0.1) for _ in range(n)])
    for setting in ukf_ref.SETTINGS:
        w, wl = ukf_ref.weights(*setting), ukf_ref.weights(*setting, dtype=np.longdouble)
        a, _, _ = ukf_ref.points(x, P, w[0])
        b, _, _ = ukf_ref.points(x, P, wl[0], dtype=np.longdouble)
        assert b.dtype == np.longdouble and ekf_ref.scaled(a, b.astype(np.float64)) < 1e-13
        y = np.tanh(a)
        m64, m80 = ukf_ref.moments(y, w, ekf_ref.test_Q()), ukf_ref.moments(y, wl, ekf_ref.test_Q(), dtype=np.longdouble)
        for u, v in zip(m64, m80):
            assert ekf_ref.scaled(u, v.astype(np.float64)) < 1e-13


# ---------------------------------------------------------------------------------------------------------------------
# 4. the GPU tests' inputs on the oracle restatement (these pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
def test_touchdown_starts_spread_the_points_over_the_branches(substeps):
    """passes without the feature: the starts of tests/test_gpu_rollout_ukf.py (its inputs(), NumPy only) under the
    restated filter on the float64 oracle: points of one env end a step with different statuses in at least 2 % of the
    (k, env) pairs, each of the four statuses occurs among them, and every factorisation succeeds."""
    import test_gpu_rollout_ukf as G
    from branch_fd import run_rollout
    from oracle.refcpu import AIRBORNE, CRASHED, LANDED, LEVELING
    p = G.inputs("lander3d", G.N, G.K, seed=700 + substeps)
    truth, _ = run_rollout("lander3d", p["x0"], p["st0"], p["acts"].astype(np.float64), substeps=substeps)
    z = truth["x"] @ p["H"].T + p["noise"]
    res = ukf_ref.oracle_filter("lander3d", p["acts"], z, p["H"], p["r"], p["Q"], p["x0"], p["P0"], p["st0"],
                                substeps=substeps)
    share = float((res["spread"] > 0).mean())
    print("substeps %d: spread > 0 in %.3f of the (k, env) pairs" % (substeps, share))
    assert share >= 0.02, share
    assert res["ok"].all() and np.isfinite(res["x"]).all()
    for s in (AIRBORNE, CRASHED, LANDED, LEVELING):
        assert (res["point_status"] == s).any(), s


def test_application_conditions_hold_on_the_oracle_restatement():
    """passes without the feature: the application of the GPU tests (section 19's Hover3D case: 300 envs, 48 steps,
    positions and angles measured, NumPy seed 1) under the restated filter with the default weights on the float64
    oracle: the four conditions the device result must satisfy"""
    from branch_fd import run_rollout
    from jacobian_fd import hover_action
    from oracle.refcpu import AIRBORNE
    a, x0, xhat0, H, r = ekf_ref.app_inputs(hover_action(), seed=1)
    n, K = ekf_ref.APP_N, ekf_ref.APP_K
    st = np.full(n, AIRBORNE, np.uint8)
    tape, _ = run_rollout("hover3d", x0, st, a.astype(np.float64))
    truth = tape["x"]
    assert (tape["status"] == AIRBORNE).all()
    rng = np.random.default_rng(2)
    z = truth @ H.T + np.sqrt(r) * rng.standard_normal((K, n, 6))
    P0 = np.repeat(ekf_ref.APP_P0[None], n, axis=0)
    res = ukf_ref.oracle_filter("hover3d", a, z, H, r, ekf_ref.APP_Q, xhat0, P0, st)
    assert res["ok"].all() and (res["spread"] == 0).all()
    rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
    fig = ekf_ref.app_conditions(res["x"], np.diagonal(res["P"], axis1=1, axis2=2), res["nis"], truth, rmse0)
    print("mean NIS %.3f rmse %s sd %s" % (fig["mean_nis"], np.round(fig["rmse"], 4), np.round(fig["sd"], 4)))
