"""CPU-side checks of cs_rollout_rts: the entry point declared, exported and bound, the ctypes struct mirroring the header
field by field; bad argument blocks refused without touching a device; the dense algebra of the kernel's own header
compiled for the host (tests/host/rts_solve_host) on its three paths -- positive definite, a non-positive pivot, a
non-finite pivot; and self-checks of the NumPy restatement the GPU tests hold the kernel to (tests/rts_ref.py) -- these
pass without the feature and are labelled so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ekf_ref
import rts_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "rts_solve_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors (these fail without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_rollout_rts\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_rollout_rts_io\* \w+,"
                     r"\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_rollout_rts") and "cs_rollout_rts" in _lib.SYMBOLS
    assert lib.cs_rollout_rts.argtypes[2] is C.POINTER(_lib.RolloutRtsIO)


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_rollout_rts_io \{(.*?)\} cs_rollout_rts_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.RolloutRtsIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.RolloutRtsIO._fields_):
        size = 8 if "*" in ctype else 4
        assert C.sizeof(mirror) == size, name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.RolloutRtsIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.RolloutRtsIO) == offset == 8 + 13 * 8


def test_the_abi_version_is_unchanged():
    assert _lib.load().cs_version() == 5 == _lib.ABI_VERSION
    assert re.search(r"#define CS_ABI_VERSION 5\b", HEADER)
    assert hasattr(_lib.load(), "cs_rollout_rts")              # ... with the entry point added


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev, io.start_x_dev, io.start_status_dev, io.x_dev = 0x1000, 0x2000, 0x3000, 0x4000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _rio(**kw):
    rio = _lib.RolloutRtsIO()
    rio.struct_size = C.sizeof(rio)
    rio.x_f_dev, rio.x_pred_dev, rio.status_f_dev, rio.P_f_dev = 0x6000, 0x7000, 0x8001, 0x9000
    rio.Q_dev, rio.P0_dev = 0xa000, 0xb000
    for k, v in kw.items():
        setattr(rio, k, v)
    return rio


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_rts
    err = lib.cs_last_error
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in err()
    assert fn(None, C.byref(_io(struct_size=8)), C.byref(_rio()), None) == _lib.ERR_ABI
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null rio" in err()
    # a wrong struct_size is reported before anything else in the block
    bad = _rio(struct_size=C.sizeof(_lib.RolloutRtsIO) - 8, out_dtype=9, x_f_dev=None)
    assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in err()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_rio()), None) == _lib.ERR_ARG and b"num_steps" in err()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_rio()), None) == _lib.ERR_ARG and b"actions_dev" in err()
    assert fn(None, C.byref(_io(start_x_dev=None, start_status_dev=None)), C.byref(_rio()), None) == _lib.ERR_ARG
    assert b"start_x_dev" in err()
    assert fn(None, C.byref(_io(start_status_dev=None)), C.byref(_rio()), None) == _lib.ERR_ARG
    assert b"start_status_dev" in err()
    for key in ("start_force_dev", "start_prev_shaping_dev", "reward_dev", "terminated_dev", "truncated_dev",
                "status_dev", "gx_dev", "gr_dev", "g_actions_dev", "g_x0_dev"):
        assert fn(None, C.byref(_io(**{key: 0xc000})), C.byref(_rio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err(), key
    assert fn(None, C.byref(_io()), C.byref(_rio(out_dtype=5)), None) == _lib.ERR_ARG and b"out_dtype" in err()
    for key in ("x_f_dev", "x_pred_dev", "status_f_dev", "P_f_dev", "Q_dev", "P0_dev"):
        assert fn(None, C.byref(_io()), C.byref(_rio(**{key: None})), None) == _lib.ERR_ARG and b"required" in err()
    for kw in (dict(end_x_dev=0xd000), dict(end_P_dev=0xd000)):
        assert fn(None, C.byref(_io()), C.byref(_rio(**kw)), None) == _lib.ERR_ARG and b"both or neither" in err()
    for key in ("x_f_dev", "x_pred_dev", "P_f_dev", "Q_dev", "P0_dev", "x0_dev", "P_tape_dev", "var_dev", "P0_s_dev"):
        assert fn(None, C.byref(_io()), C.byref(_rio(**{key: 0xc004})), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io()), C.byref(_rio(end_x_dev=0xd004, end_P_dev=0xd000)), None) == _lib.ERR_ARG
    assert b"aligned" in err()
    assert fn(None, C.byref(_io(x_dev=0x4004)), C.byref(_rio()), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io(actions_dev=0x1002)), C.byref(_rio()), None) == _lib.ERR_ARG and b"aligned" in err()
    # float32 outputs need 4 bytes only; the status tape none
    ok32 = _rio(out_dtype=_lib.JAC_F32, P_tape_dev=0xc004, var_dev=0xc004, P0_s_dev=0xc004)
    assert fn(None, C.byref(_io()), C.byref(ok32), None) == _lib.ERR_ARG and err() == b"null context"
    assert fn(None, C.byref(_io(x_dev=None)), C.byref(_rio(end_x_dev=0xd000, end_P_dev=0xe000)), None) == _lib.ERR_ARG
    assert err() == b"null context"                                                   # ... as far as the context


# ---------------------------------------------------------------------------------------------------------------------
# 2. the algebra header on the host (fails without the feature: the program is its code)
# ---------------------------------------------------------------------------------------------------------------------
IU = [(i, j) for j in range(12) for i in range(j + 1)]


def _host(xf, dx, Pm, W, D, Pf):
    args = [float(v).hex() for v in np.concatenate([xf, dx] + [np.asarray(m, np.float64).ravel() for m in (Pm, W, D, Pf)])]
    out = subprocess.run([HOST] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[0] in ("ok 0", "ok 1")
    v = np.array([float.fromhex(s) for s in out[1:1 + 78 + 144 + 12 + 78]])
    U, P = np.zeros((12, 12)), np.zeros((12, 12))
    for (i, j), u, p in zip(IU, v[:78], v[234:]):
        U[i, j] = u
        P[i, j] = P[j, i] = p
    return dict(ok=out[0] == "ok 1", inv=np.diagonal(U).copy(), U=np.triu(U, 1), G=v[78:222].reshape(12, 12), x=v[222:234],
                P=P)


def _spd(rng, scale=1.0):
    m = rng.standard_normal((12, 12))
    P = scale * (m @ m.T / 12 + 0.2 * np.eye(12))
    return (P + P.T) / 2


def _case(rng):
    A = np.eye(12) + 0.1 * rng.standard_normal((12, 12))
    Pf = _spd(rng, 0.1)
    W = A @ Pf
    Pm = ekf_ref.mirror_upper(W @ A.T + ekf_ref.test_Q())
    D = _spd(rng, 0.05) - Pm
    return rng.standard_normal(12), 0.1 * rng.standard_normal(12), Pm, W, ekf_ref.mirror_upper(D), Pf


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_host_positive_definite_path_is_the_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    for _ in range(3):
        xf, dx, Pm, W, D, Pf = _case(rng)
        got = _host(xf, dx, Pm, W, D, Pf)
        ref = rts_ref.algebra(Pm[None], W[None], D[None], Pf[None], xf[None], dx[None])
        assert got["ok"] and ref["ok"][0]
        for key in ("U", "inv", "G", "x", "P"):
            assert _same(got[key], ref[key][0]), key
        assert np.array_equal(got["P"], got["P"].T)
        # ... and it solves the system: P- G = W to the solve's forward bound
        kappa = np.linalg.cond(Pm)
        assert ekf_ref.scaled(got["G"], np.linalg.solve(Pm, W)) <= 100 * 12 * rts_ref.EPS * kappa
        # only the upper triangles of P- and D are read
        low = np.tril(rng.standard_normal((12, 12)), -1)
        again = _host(xf, dx, Pm + low, W, D + low, Pf)
        assert all(_same(again[key], got[key]) for key in ("U", "inv", "G", "x", "P"))


def test_host_reports_a_nonpositive_pivot_and_carries_on():
    rng = np.random.default_rng(12)
    xf, dx, Pm, W, D, Pf = _case(rng)
    got = _host(xf, dx, -np.eye(12), W, D, Pf)
    ref = rts_ref.algebra(-np.eye(12)[None], W[None], D[None], Pf[None], xf[None], dx[None])
    assert not got["ok"] and not ref["ok"][0]
    assert np.isnan(got["inv"]).all() and np.isnan(got["x"]).all()       # the sqrt of -1, carried through
    for key in ("U", "inv", "G", "x", "P"):
        assert _same(np.isnan(got[key]), np.isnan(ref[key][0])), key
    # a zero pivot (a PSD prior, rank 11): 1 / sqrt(0) = inf
    Z = Pm.copy()
    Z[0, :] = Z[:, 0] = 0.0
    got = _host(xf, dx, Z, W, D, Pf)
    ref = rts_ref.algebra(Z[None], W[None], D[None], Pf[None], xf[None], dx[None])
    assert not got["ok"] and not ref["ok"][0] and np.isposinf(got["inv"][0])
    # a pivot that turns negative in the last column only: the eleven before it are the clean factor's
    clean = _host(xf, dx, Pm, W, D, Pf)
    last = Pm.copy()
    last[11, 11] = -1.0
    got = _host(xf, dx, last, W, D, Pf)
    assert not got["ok"] and _same(got["inv"][:11], clean["inv"][:11]) and np.isnan(got["inv"][11])


def test_host_reports_a_nonfinite_pivot_and_carries_on():
    rng = np.random.default_rng(13)
    xf, dx, Pm, W, D, Pf = _case(rng)
    for bad in (np.inf, np.nan):
        B = Pm.copy()
        B[3, 3] = bad
        got = _host(xf, dx, B, W, D, Pf)
        ref = rts_ref.algebra(B[None], W[None], D[None], Pf[None], xf[None], dx[None])
        assert not got["ok"] and not ref["ok"][0], bad
        for key in ("U", "inv", "G", "x", "P"):
            assert _same(np.isnan(got[key]), np.isnan(ref[key][0])), (bad, key)
        if bad != bad:
            assert np.isnan(got["P"]).any()
    # an infinite pivot alone is not "positive": inf > 0, and still ok is cleared
    B = np.diag(np.full(12, 2.0))
    B[0, 0] = np.inf
    assert not _host(xf, dx, B, W, D, Pf)["ok"]
    assert _host(xf, dx, np.diag(np.full(12, 2.0)), W, D, Pf)["ok"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. self-checks of the reference (these pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def _random_step(rng, n):
    A = np.eye(12) + 0.1 * rng.standard_normal((n, 12, 12))
    Pf = np.array([_spd(rng, 0.1) for _ in range(n)])
    Ps = np.array([_spd(rng, 0.05) for _ in range(n)])
    xf, xp, xs = rng.standard_normal((3, n, 12))
    return A, Pf, xf, xf + 0.1 * xp, xf + 0.1 * xs, Ps


def test_reference_equals_the_textbook_form():
    """passes without the feature: tests/rts_ref.py against C = P_f A^T P-^-1 by numpy.linalg.solve"""
    rng = np.random.default_rng(20)
    n = 20
    A, Pf, xf, xp, xs, Ps = _random_step(rng, n)
    Q = ekf_ref.test_Q()
    out = rts_ref.one_step(A, Pf, xf, xp, xs, Ps, Q)
    assert out["ok"].all()
    for e in range(n):
        x, P, kappa = rts_ref.textbook_step(A[e], Pf[e], xf[e], xp[e], xs[e], Ps[e], Q)
        tol = 1e-12 * kappa
        assert tol < 1e-6
        assert ekf_ref.scaled(out["x"][e], x) <= tol and ekf_ref.scaled(out["P"][e], P) <= tol
    assert np.array_equal(out["P"], np.swapaxes(out["P"], 1, 2))


@pytest.mark.parametrize("K", [1, 2, 4])
def test_reference_is_the_conditional_gaussian_of_the_joint_density(K):
    """passes without the feature: a linear system x_k = A x_{k-1} + w, z_k = H x_k + v; filter (ekf_ref) then smoother
    (rts_ref) give the mean and covariance of every x_k, the starting point included, given ALL the measurements -- the
    conditional of the stacked joint Gaussian, by a dense solve"""
    rng = np.random.default_rng(30 + K)
    M = 3
    A = np.eye(12) + 0.2 * rng.standard_normal((12, 12)) / np.sqrt(12)
    H, r = rng.standard_normal((M, 12)), rng.uniform(0.05, 0.5, M)
    Q, P0, x0 = _spd(rng, 0.05), _spd(rng), rng.standard_normal(12)
    z = rng.standard_normal((K, M))
    # stages 0 .. K are x_{-1} .. x_{K-1}: s = mean + F xi, xi = (x_{-1} - x0, w_0, .., w_{K-1})
    S = K + 1
    F = np.zeros((12 * S, 12 * S))
    for k in range(S):
        for j in range(k + 1):
            F[12 * k:12 * k + 12, 12 * j:12 * j + 12] = np.linalg.matrix_power(A, k - j)
    Cxi = np.kron(np.eye(S), Q)
    Cxi[:12, :12] = P0
    Cs = F @ Cxi @ F.T
    mean = np.concatenate([np.linalg.matrix_power(A, k) @ x0 for k in range(S)])
    Hb = np.kron(np.eye(K), H)
    Czz = Hb @ Cs[12:, 12:] @ Hb.T + np.kron(np.eye(K), np.diag(r))
    Csz = Cs[:, 12:] @ Hb.T
    cm = mean + Csz @ np.linalg.solve(Czz, z.ravel() - Hb @ mean[12:])
    cc = Cs - Csz @ np.linalg.solve(Czz, Csz.T)
    # the filter, then the smoother
    xf, Pf, xp = [x0], [P0], [None]
    for k in range(K):
        out = ekf_ref.one_step(A[None], Pf[-1][None], (A @ xf[-1])[None], Q, H, r, z[k][None])
        xp.append(A @ xf[-1])
        xf.append(out["x"][0])
        Pf.append(out["P"][0])
    xs, Ps = {K: xf[K]}, {K: Pf[K]}
    for j in range(K - 1, -1, -1):                       # stage j from stage j + 1
        out = rts_ref.one_step(A[None], Pf[j][None], xf[j][None], xp[j + 1][None], xs[j + 1][None], Ps[j + 1][None], Q)
        assert out["ok"][0]
        xs[j], Ps[j] = out["x"][0], out["P"][0]
    tol = 1e-12 * max(np.linalg.cond(Czz), np.linalg.cond(Cs))
    assert tol < 1e-6
    for k in range(S):
        assert ekf_ref.scaled(xs[k], cm[12 * k:12 * k + 12]) <= tol, k
        assert ekf_ref.scaled(Ps[k], cc[12 * k:12 * k + 12, 12 * k:12 * k + 12]) <= tol, k


def test_reference_in_longdouble_agrees_and_q_is_far_above_the_bar():
    """passes without the feature: float64 against longdouble on random steps with the tests' Q; dropping Q moves some
    entry of every env's x_s and P_s by far more than 1 000 x its bar"""
    rng = np.random.default_rng(40)
    n = 200
    A, Pf, xf, xp, xs, Ps = _random_step(rng, n)
    Q = ekf_ref.test_Q()
    a = rts_ref.one_step(A, Pf, xf, xp, xs, Ps, Q)
    b = rts_ref.one_step(A, Pf, xf, xp, xs, Ps, Q, dtype=np.longdouble)
    for k in ("P_pred", "x", "P", "G"):
        assert b[k].dtype == np.longdouble
        assert ekf_ref.scaled(a[k], b[k].astype(np.float64)) < 1e-13, k
    assert a["ok"].all() and np.array_equal(a["ok"], b["ok"])
    kappa = rts_ref.cond(a["P_pred"])
    assert kappa.max() <= 1e3
    bar = rts_ref.bars(a, b)
    noq = rts_ref.one_step(A, Pf, xf, xp, xs, Ps, 0.0 * Q)
    for k in ("x", "P"):
        share = rts_ref.scaled_env(noq[k], a[k])
        assert np.all(share >= 1e3 * bar[k]), (k, share.min(), bar[k].max())
    print("kappa <= %.0f, f64 - longdouble <= %.1e, Q's share of x >= %.1e, of P >= %.1e" % (
        kappa.max(), max(ekf_ref.scaled(a[k], b[k].astype(np.float64)) for k in ("x", "P")),
        rts_ref.scaled_env(noq["x"], a["x"]).min(), rts_ref.scaled_env(noq["P"], a["P"]).min()))


def test_application_conditions_hold_on_the_oracle_restatement():
    """passes without the feature: the application of the GPU tests (Hover3D, 300 envs, 48 steps) with the filter and the
    smoother restated in NumPy on the float64 oracle and central-difference Jacobians, NumPy seed 1: the conditions the
    device result must satisfy, with their margins.  The smoother takes the very Jacobians the filter took."""
    from branch_fd import fd_step, run_rollout
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
    x, P, status = xhat0.T.copy(), np.repeat(ekf_ref.APP_P0[None], n, axis=0), st
    xf, Pf, xp, As = [x], [P], [None], [None]             # stage k + 1 is row k; stage 0 the starting point
    for k in range(K):
        fd, A, *_ = fd_step("hover3d", x.T, status, a[k].astype(np.float64))
        out = ekf_ref.one_step(A, P, fd.tape["x"][0], ekf_ref.APP_Q, H, r, z[k])
        x, P, status = out["x"], out["P"], fd.tape["status"][0].astype(np.uint8)
        xf.append(x)
        Pf.append(P)
        xp.append(fd.tape["x"][0])
        As.append(A)
    xs, Ps = {K: xf[K]}, {K: Pf[K]}
    for j in range(K - 1, -1, -1):
        out = rts_ref.one_step(As[j + 1], Pf[j], xf[j], xp[j + 1], xs[j + 1], Ps[j + 1], ekf_ref.APP_Q)
        assert out["ok"].all()
        xs[j], Ps[j] = out["x"], out["P"]
    diag = lambda m: np.diagonal(m, axis1=1, axis2=2)     # noqa: E731
    rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
    fig = rts_ref.app_conditions(np.array([xs[k] for k in range(1, K + 1)]), np.array([diag(Ps[k]) for k in range(1, K + 1)]),
                                 xs[0], diag(Ps[0]), np.array(xf[1:]), np.array([diag(m) for m in Pf[1:]]), truth, x0.T,
                                 rmse0)
    print(fig)
