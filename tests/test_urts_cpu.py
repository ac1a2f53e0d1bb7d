"""CPU-side checks of cs_urts_smooth: the entry point declared, exported and bound, the ctypes struct
mirroring the header field by field; bad argument blocks refused without touching a device; one backward step of the
kernel's own headers compiled for the host (tests/host/urts_cross_host) against the NumPy restatement the GPU tests hold
the kernel to (tests/urts_ref.py), bit for bit, under section 23's three weight settings and with a non-positive pivot in
each of the two factorisations; the Python side (the mixin, smooth()'s dispatch); self-checks of the restatement (these
pass without the feature and are labelled so); and the inputs of the GPU tests on the restatement over the float64
oracle's step, so that no device sees an input that does not meet its test's conditions."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ekf_ref
import rts_ref
import ukf_ref
import urts_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "urts_cross_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors (these fail without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_urts_smooth\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_urts_io\* \w+,"
                     r"\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_urts_smooth") and "cs_urts_smooth" in _lib.SYMBOLS
    assert lib.cs_urts_smooth.argtypes[2] is C.POINTER(_lib.RolloutUrtsIO)
    assert int(re.search(r"#define CS_URTS_WORKSPACE_ROWS (\d+)", HEADER).group(1)) == _lib.URTS_WORKSPACE_ROWS == 102


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_urts_io \{(.*?)\} cs_urts_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.RolloutUrtsIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.RolloutUrtsIO._fields_):
        size = 8 if "*" in ctype or "double" in ctype else 4
        assert C.sizeof(mirror) == size, name
        assert (mirror is C.c_double) == ("double" in ctype and "*" not in ctype), name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.RolloutUrtsIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.RolloutUrtsIO) == offset == 8 + 4 * 8 + 14 * 8


def test_the_abi_version_is_unchanged():
    assert _lib.load().cs_version() == 5 == _lib.ABI_VERSION
    assert re.search(r"#define CS_ABI_VERSION 5\b", HEADER)
    assert hasattr(_lib.load(), "cs_urts_smooth")              # ... with the entry point added


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev, io.start_x_dev, io.start_status_dev, io.x_dev = 0x1000, 0x2000, 0x3000, 0x4000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _sio(**kw):
    sio = _lib.RolloutUrtsIO()
    sio.struct_size = C.sizeof(sio)
    sio.gamma, sio.wm0, sio.wc0, sio.wi = (float(v) for v in ukf_ref.weights())
    sio.x_f_dev, sio.x_pred_dev, sio.status_f_dev, sio.P_f_dev = 0x6000, 0x7000, 0x8001, 0x9000
    sio.Q_dev, sio.P0_dev, sio.workspace_dev = 0xa000, 0xb000, 0xf000
    for k, v in kw.items():
        setattr(sio, k, v)
    return sio


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_urts_smooth
    err = lib.cs_last_error
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in err()
    assert fn(None, C.byref(_io(struct_size=8)), C.byref(_sio()), None) == _lib.ERR_ABI
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null sio" in err()
    # a wrong struct_size is reported before anything else in the block
    bad = _sio(struct_size=C.sizeof(_lib.RolloutUrtsIO) - 8, out_dtype=9, x_f_dev=None, gamma=-1.0, workspace_dev=None)
    assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in err()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_sio()), None) == _lib.ERR_ARG and b"num_steps" in err()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_sio()), None) == _lib.ERR_ARG and b"actions_dev" in err()
    assert fn(None, C.byref(_io(start_x_dev=None, start_status_dev=None)), C.byref(_sio()), None) == _lib.ERR_ARG
    assert b"start_x_dev" in err()
    assert fn(None, C.byref(_io(start_status_dev=None)), C.byref(_sio()), None) == _lib.ERR_ARG
    assert b"start_status_dev" in err()
    for key in ("start_force_dev", "start_prev_shaping_dev", "reward_dev", "terminated_dev", "truncated_dev",
                "status_dev", "gx_dev", "gr_dev", "g_actions_dev", "g_x0_dev"):
        assert fn(None, C.byref(_io(**{key: 0xc000})), C.byref(_sio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err(), key
    assert fn(None, C.byref(_io()), C.byref(_sio(out_dtype=5)), None) == _lib.ERR_ARG and b"out_dtype" in err()
    for g in (0.0, -1.0, float("nan"), float("inf")):
        assert fn(None, C.byref(_io()), C.byref(_sio(gamma=g)), None) == _lib.ERR_ARG and b"gamma" in err()
    for key in ("wm0", "wc0", "wi"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert fn(None, C.byref(_io()), C.byref(_sio(**{key: v})), None) == _lib.ERR_ARG and b"weights" in err()
    for key in ("x_f_dev", "x_pred_dev", "status_f_dev", "P_f_dev", "Q_dev", "P0_dev"):
        assert fn(None, C.byref(_io()), C.byref(_sio(**{key: None})), None) == _lib.ERR_ARG and b"required" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(workspace_dev=None)), None) == _lib.ERR_ARG
    assert b"workspace_dev is required" in err()
    for kw in (dict(end_x_dev=0xd000), dict(end_P_dev=0xd000)):
        assert fn(None, C.byref(_io()), C.byref(_sio(**kw)), None) == _lib.ERR_ARG and b"both or neither" in err()
    for key in ("x_f_dev", "x_pred_dev", "P_f_dev", "Q_dev", "P0_dev", "x0_dev", "P_tape_dev", "var_dev", "P0_s_dev",
                "workspace_dev"):
        assert fn(None, C.byref(_io()), C.byref(_sio(**{key: 0xc004})), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(end_x_dev=0xd004, end_P_dev=0xd000)), None) == _lib.ERR_ARG
    assert b"aligned" in err()
    assert fn(None, C.byref(_io(x_dev=0x4004)), C.byref(_sio()), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io(actions_dev=0x1002)), C.byref(_sio()), None) == _lib.ERR_ARG and b"aligned" in err()
    # float32 outputs need 4 bytes only; negative and zero weights are weights; the status tape needs no alignment
    ok32 = _sio(out_dtype=_lib.JAC_F32, P_tape_dev=0xc004, var_dev=0xc004, P0_s_dev=0xc004, wm0=-3.0, wc0=-0.25)
    assert fn(None, C.byref(_io()), C.byref(ok32), None) == _lib.ERR_ARG and err() == b"null context"
    assert fn(None, C.byref(_io(x_dev=None)), C.byref(_sio(end_x_dev=0xd000, end_P_dev=0xe000, wm0=0.0)), None) == \
        _lib.ERR_ARG
    assert err() == b"null context"                                                   # ... as far as the context


# ---------------------------------------------------------------------------------------------------------------------
# 2. one backward step of the kernel's headers on the host (fails without the feature: the program is its code)
# ---------------------------------------------------------------------------------------------------------------------
IU = [(i, j) for j in range(12) for i in range(j + 1)]


def _unpack(v):
    Pm = np.zeros((12, 12))
    for (i, j), val in zip(IU, v):
        Pm[i, j] = Pm[j, i] = val
    return Pm


def _host(w, landed, xf, xp, xs, Pf, Q, Ps, y):
    vals = np.concatenate([np.asarray(w, np.float64), xf, xp, xs] + [np.ravel(m) for m in (Pf, Q, Ps, y)])
    args = [float(v).hex() for v in vals]
    args.insert(4, "1" if landed else "0")
    out = subprocess.run([HOST] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    m = re.fullmatch(r"ok ([01]) ([01])", out[0])
    assert m, out[0]
    v = np.array([float.fromhex(s) for s in out[1:1 + 144 + 78 + 144 + 12 + 78]])
    return dict(ok_factor=m.group(1) == "1", ok_solve=m.group(2) == "1", W=v[:144].reshape(12, 12),
                P_pred=_unpack(v[144:222]), G=v[222:366].reshape(12, 12), x=v[366:378], P=_unpack(v[378:456]))


def _spd(rng, scale=1.0):
    m = rng.standard_normal((12, 12))
    P = scale * (m @ m.T / 12 + 0.2 * np.eye(12))
    return (P + P.T) / 2


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _case(rng, w, Pf=None):
    Pf = _spd(rng, 0.1) if Pf is None else Pf
    xf = rng.standard_normal(12) * 3
    with np.errstate(invalid="ignore"):
        pts = ukf_ref.points(xf[None], Pf[None], w[0])[0][0]
    pts = np.where(np.isnan(pts), 0.0, pts)
    y = np.sin(pts) + 0.3 * pts ** 2 + rng.standard_normal((25, 12)) * 0.01       # any map will do
    xp = y[0] + 0.01 * rng.standard_normal(12)
    return dict(xf=xf, xp=xp, xs=xp + 0.1 * rng.standard_normal(12), Pf=Pf, Q=ekf_ref.test_Q(), Ps=_spd(rng, 0.05), y=y)


def _both(w, c, landed=False):
    got = _host(w, landed, c["xf"], c["xp"], c["xs"], c["Pf"], c["Q"], c["Ps"], c["y"])
    ref = urts_ref.one_step(c["y"][None], np.array([landed]), c["Pf"][None], c["xf"][None], c["xp"][None], c["xs"][None],
                            c["Ps"][None], w, c["Q"])
    return got, ref


@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_host_step_is_the_restatement_bit_for_bit(setting):
    rng = np.random.default_rng(int(1000 + 100 * setting[0] + 10 * setting[1] + setting[2]))
    w = ukf_ref.weights(*setting)
    for landed in (False, False, True):
        c = _case(rng, w)
        got, ref = _both(w, c, landed)
        assert got["ok_factor"] and got["ok_solve"] and ref["ok"][0]
        for key in ("W", "P_pred", "G", "x", "P"):
            assert _same(got[key], ref[key][0]), (landed, key)
        assert np.array_equal(got["P"], got["P"].T)
        if landed:
            assert _same(got["W"], ekf_ref.mirror_upper(c["Pf"])) and _same(got["P_pred"], ekf_ref.mirror_upper(c["Pf"] + c["Q"]))
        else:
            # W is the textbook cross-covariance of the points, transposed
            pts = ukf_ref.points(c["xf"][None], c["Pf"][None], w[0])[0]
            want = urts_ref.textbook_cross(pts, c["y"][None], w)[0].astype(np.float64)
            assert ekf_ref.scaled(got["W"], want) <= 1e-12 * np.linalg.cond(c["Pf"])
        # only the upper triangles of P_f (for the factor) and P_s' are read ... but whole columns of P_f enter P_s
        low = np.tril(rng.standard_normal((12, 12)), -1)
        again = _host(w, landed, c["xf"], c["xp"], c["xs"], c["Pf"], c["Q"], c["Ps"] + low, c["y"])
        assert all(_same(again[key], got[key]) for key in ("W", "P_pred", "G", "x", "P"))


@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_host_reports_a_nonpositive_pivot_in_each_factorisation_and_carries_on(setting):
    rng = np.random.default_rng(int(2000 + 100 * setting[0] + 10 * setting[1] + setting[2]))
    w = ukf_ref.weights(*setting)
    # the first factorisation: P_f = -I (its roots are NaN: W is NaN, P- is the moments', which need no factor)
    c = _case(rng, w, Pf=-np.eye(12))
    got, ref = _both(w, c)
    assert not got["ok_factor"] and not ref["ok_factor"][0] and not ref["ok"][0]
    assert np.isnan(got["W"]).all()
    assert _same(got["P_pred"], ref["P_pred"][0]) and np.isfinite(got["P_pred"]).all()
    for key in ("W", "G", "x", "P"):
        assert _same(np.isnan(got[key]), np.isnan(ref[key][0])), key
    assert got["ok_solve"] == bool(ref["ok_solve"][0])
    # a LANDED row factors nothing of P_f
    got, ref = _both(w, c, landed=True)
    assert got["ok_factor"] and ref["ok_factor"][0]
    # a zero pivot in the last column only
    Z = _spd(rng, 0.1)
    Z[11, :] = Z[:, 11] = 0.0
    got, ref = _both(w, _case(rng, w, Pf=Z))
    assert not got["ok_factor"] and not ref["ok_factor"][0]
    # the second factorisation: propagated points that make P- indefinite (a large negative Q entry stands in)
    c = _case(rng, w)
    c["Q"] = c["Q"] - 50.0 * np.eye(12)
    got, ref = _both(w, c)
    assert got["ok_factor"] and not got["ok_solve"] and ref["ok_factor"][0] and not ref["ok_solve"][0] and not ref["ok"][0]
    assert _same(got["W"], ref["W"][0]) and _same(got["P_pred"], ref["P_pred"][0])
    for key in ("G", "x", "P"):
        assert _same(np.isnan(got[key]), np.isnan(ref[key][0])), key
    assert np.isnan(got["x"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python side (fails without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_method_is_inherited_from_the_ukf_module_and_forwarded_by_the_sharded_env():
    import importlib
    import gym_copter_amd
    from gym_copter_amd import sharded
    ukf = importlib.import_module("gym_copter_amd.ukf")      # (gym_copter_amd.ukf names the driver function)
    cls = gym_copter_amd.CopterVecEnv
    assert callable(cls.rollout_urts) and cls.rollout_urts is ukf.rollout_urts
    assert "rollout_urts" not in vars(cls) and ukf.UnscentedSmoother in cls.__mro__       # inherited, not bound
    assert "rollout_urts" in sharded._LOCAL_ROLLOUTS and hasattr(sharded.ShardedCopterVecEnv, "rollout_urts")
    assert "MUST be the filter's" in ukf.rollout_urts.__doc__


def test_smooth_dispatches_on_the_type_of_the_filters_result():
    import torch
    from gym_copter_amd import EkfResult, RtsResult, UkfResult, smooth
    K, n = 5, 3
    calls = []

    class Env:
        def _res(self, name, actions, filt, end, kw):
            k = actions.shape[0]
            calls.append((name, k, type(filt), end is not None, kw))
            return RtsResult(torch.zeros(k, n, 12), torch.zeros(k, n, 12, 12), torch.zeros(k, n, 12), torch.zeros(12, n),
                             torch.zeros(n, 12, 12), torch.ones(n, dtype=torch.bool))

        def rollout_rts(self, actions, filt, Q, x0, P0, status0=None, end=None, tape=True):
            return self._res("rts", actions, filt, end, {})

        def rollout_urts(self, actions, filt, Q, x0, P0, status0=None, end=None, tape=True, **kw):
            return self._res("urts", actions, filt, end, kw)

    acts = torch.zeros(K, n, 4)
    tapes = dict(x=torch.zeros(K, n, 12), x_pred=torch.zeros(K, n, 12), status=torch.zeros(K, n, dtype=torch.uint8),
                 P_tape=torch.zeros(K, n, 12, 12))
    ekf = EkfResult(**{f: tapes.get(f) for f in EkfResult._fields})
    ukf = UkfResult(**{f: tapes.get(f) for f in UkfResult._fields})
    args = (np.eye(12), torch.zeros(12, n), torch.zeros(n, 12, 12))
    out = smooth(Env(), acts, ekf, *args, chunk=2)
    assert [c[:4] for c in calls] == [("rts", 1, EkfResult, False), ("rts", 2, EkfResult, True), ("rts", 2, EkfResult, True)]
    assert all(c[4] == {} for c in calls) and out.x.shape == (K, n, 12)
    calls.clear()
    out = smooth(Env(), acts, ukf, *args, chunk=3, alpha=0.5, beta=2.0, kappa=0.0)
    assert [c[:4] for c in calls] == [("urts", 2, UkfResult, False), ("urts", 3, UkfResult, True)]
    assert all(c[4] == dict(alpha=0.5, beta=2.0, kappa=0.0) for c in calls) and out.P_tape.shape == (K, n, 12, 12)
    calls.clear()
    smooth(Env(), acts, ukf, *args)
    assert calls == [("urts", K, UkfResult, False, dict(alpha=1.0, beta=0.0, kappa=1.0))]
    Other = collections.namedtuple("Other", UkfResult._fields)
    for bad, match in ((tuple(ukf), "EkfResult or a UkfResult"), (Other(*ukf), "EkfResult or a UkfResult"),
                       (ukf._replace(P_tape=None), "P_tape"), (ekf._replace(P_tape=None), "P_tape"),
                       (ukf._replace(x=tapes["x"][:2]), "filt.x must be a tensor of K"),
                       (ukf._replace(status=None), "filt.status must be a tensor of K")):
        with pytest.raises(ValueError, match=match):
            smooth(Env(), acts, bad, *args)
    with pytest.raises(ValueError, match="chunk must be"):
        smooth(Env(), acts, ukf, *args, chunk=0)


# ---------------------------------------------------------------------------------------------------------------------
# 4. self-checks of the reference (these pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_reference_cross_covariance_is_the_textbook_sum(setting):
    """passes without the feature: W against C^T, C = sum_i wc_i (chi_i - xhat)(y_i - x-)^T over all 25 points in
    longdouble, for an arbitrary nonlinear map"""
    rng = np.random.default_rng(70)
    n = 20
    w = ukf_ref.weights(*setting)
    x, P = rng.standard_normal((n, 12)), np.array([_spd(rng, 0.1) for _ in range(n)])
    pts, ok, U = ukf_ref.points(x, P, w[0])
    y = np.tanh(pts) + 0.2 * pts ** 2
    W = urts_ref.cross(y, U, w)
    want = urts_ref.textbook_cross(pts, y, w).astype(np.float64)
    tol = 1e-12 * max(np.linalg.cond(m) for m in P)
    assert ok.all() and tol < 1e-9 and ekf_ref.scaled(W, want) <= tol
    Wl = urts_ref.cross(y, ukf_ref.cholesky(P, np.longdouble)[0], ukf_ref.weights(*setting, dtype=np.longdouble),
                        dtype=np.longdouble)
    assert Wl.dtype == np.longdouble and ekf_ref.scaled(W, Wl.astype(np.float64)) < 1e-13


@pytest.mark.parametrize("setting", ukf_ref.SETTINGS)
def test_reference_equals_the_extended_smoother_for_a_linear_map(setting):
    """passes without the feature: for y = A chi + b the step is rts_ref's with that A"""
    rng = np.random.default_rng(71)
    n = 12
    w = ukf_ref.weights(*setting)
    Q = ekf_ref.test_Q()
    A = np.eye(12) + 0.1 * rng.standard_normal((n, 12, 12))
    b = rng.standard_normal((n, 1, 12))
    Pf, Ps = np.array([_spd(rng, 0.1) for _ in range(n)]), np.array([_spd(rng, 0.05) for _ in range(n)])
    xf, xp, xs = rng.standard_normal((3, n, 12))
    xp, xs = xf + 0.1 * xp, xf + 0.1 * xs
    pts = ukf_ref.points(xf, Pf, w[0])[0]
    y = np.einsum("nij,npj->npi", A, pts) + b
    a = urts_ref.one_step(y, np.zeros(n, bool), Pf, xf, xp, xs, Ps, w, Q)
    e = rts_ref.one_step(A, Pf, xf, xp, xs, Ps, Q)
    tol = 1e-11 * max(rts_ref.cond(e["P_pred"]).max(), max(np.linalg.cond(m) for m in Pf))
    assert a["ok"].all() and tol < 1e-7
    for key in ("P_pred", "x", "P"):
        assert ekf_ref.scaled(a[key], e[key]) <= tol, key
    assert ekf_ref.scaled(a["W"], np.einsum("nij,njk->nik", A, Pf)) <= tol
    # a LANDED row is the extended smoother's with A = I
    a = urts_ref.one_step(y, np.ones(n, bool), Pf, xf, xp, xs, Ps, w, Q)
    e = rts_ref.one_step(np.repeat(np.eye(12)[None], n, axis=0), Pf, xf, xp, xs, Ps, Q)
    for key in ("P_pred", "x", "P"):
        assert ekf_ref.scaled(a[key], e[key]) <= 1e-13, key


@pytest.mark.parametrize("K", [1, 2, 4])
def test_reference_is_the_conditional_gaussian_of_the_joint_density(K):
    """passes without the feature: a linear system x_k = A x_{k-1} + w, z_k = H x_k + v; the unscented filter (ukf_ref)
    then this smoother give the mean and covariance of every x_k, the starting point included, given ALL the measurements
    -- the conditional of the stacked joint Gaussian, by a dense solve"""
    rng = np.random.default_rng(130 + K)
    M = 3
    w = ukf_ref.weights(*ukf_ref.SETTINGS[K % 3])
    A = np.eye(12) + 0.2 * rng.standard_normal((12, 12)) / np.sqrt(12)
    H, r = rng.standard_normal((M, 12)), rng.uniform(0.05, 0.5, M)
    Q, P0, x0 = _spd(rng, 0.05), _spd(rng), rng.standard_normal(12)
    z = rng.standard_normal((K, M))
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
    x, P = x0[None], P0[None]
    tapes = dict(x=[], x_pred=[], P_tape=[], status=[], y=[])
    for k in range(K):
        y = ukf_ref.points(x, P, w[0])[0] @ A.T
        out = ukf_ref.one_step(y, np.zeros(1, bool), x, P, w, Q, H, r, z[k][None])
        x, P = out["x"], out["P"]
        for key, v in (("x", x), ("x_pred", out["x_pred"]), ("P_tape", P), ("status", np.zeros(1, np.uint8)), ("y", y)):
            tapes[key].append(v)
    sm = urts_ref.smoother({k: np.array(v) for k, v in tapes.items()}, x0[None], P0[None], np.zeros(1, np.uint8), w, Q,
                           landed_code=255)
    assert sm["ok"].all()
    tol = 1e-11 * max(np.linalg.cond(Czz), np.linalg.cond(Cs))
    assert tol < 1e-6
    xs = [sm["x0"][0]] + [sm["x"][k][0] for k in range(K)]
    Ps = [sm["P0"][0]] + [sm["P"][k][0] for k in range(K)]
    for k in range(S):
        assert ekf_ref.scaled(xs[k], cm[12 * k:12 * k + 12]) <= tol, k
        assert ekf_ref.scaled(Ps[k], cc[12 * k:12 * k + 12, 12 * k:12 * k + 12]) <= tol, k


# ---------------------------------------------------------------------------------------------------------------------
# 5. the GPU tests' inputs on the oracle restatement (these pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_problem(task, p, setting, substeps=1):
    from branch_fd import run_rollout
    truth, _ = run_rollout(task, p["x0"], p["st0"], p["acts"].astype(np.float64), substeps=substeps)
    z = truth["x"] @ p["H"].T + p["noise"]
    return urts_ref.oracle_filter_tapes(task, p["acts"], z, p["H"], p["r"], p["Q"], p["x0"], p["P0"], p["st0"],
                                        setting=setting, substeps=substeps)


@pytest.mark.parametrize("substeps,setting", [(1, ukf_ref.SETTINGS[0]), (10, ukf_ref.SETTINGS[1]), (1, ukf_ref.SETTINGS[2])],
                         ids=lambda v: str(v))
def test_main_case_inputs_meet_the_gpu_tests_conditions(substeps, setting):
    """passes without the feature: the main case of tests/test_gpu_urts.py (its inputs, NumPy only: section 19's starts,
    M = 6, 30 % missing) under the restated filter and smoother on the float64 oracle.  For every env and backward step:
    kappa_2(P-) <= 1e8 (asserted inside the bar), Q's share of x_s and P_s >= 1 000 x the bar, and the float64
    restatement within its own bar of the longdouble one; spread > 0 and LANDED rows in >= 1 % of the (j, env) pairs."""
    import test_gpu_urts as G
    from oracle.refcpu import LANDED
    p = G.main_inputs(substeps)
    f = _oracle_problem("lander3d", p, setting, substeps)
    assert f["ok"].all()
    share, landed = float((f["spread"] > 0).mean()), float((f["status"] == LANDED).mean())
    print("substeps %d %r: spread > 0 in %.3f, LANDED rows %.3f of the (j, env) pairs" % (substeps, setting, share, landed))
    assert share >= 0.01 and landed >= 0.01
    w, wl = ukf_ref.weights(*setting), ukf_ref.weights(*setting, dtype=np.longdouble)
    x0, P0, st0 = p["x0"].T, p["P0"], p["st0"]
    sm = urts_ref.smoother(f, x0, P0, st0, w, p["Q"], LANDED)
    assert sm["ok"].all() and np.isfinite(sm["x"]).all() and np.isfinite(sm["P"]).all()
    K = f["x"].shape[0]
    least, kmax = {}, 0.0
    for idx, j in enumerate(range(K - 2, -2, -1)):
        xf, Pf, st = (f["x"][j], f["P_tape"][j], f["status"][j]) if j >= 0 else (x0, P0, st0)
        nxt = (f["x_pred"][j + 1], sm["x"][j + 1], sm["P"][j + 1])
        r64 = sm["steps"][idx]
        rld = urts_ref.one_step(f["y"][j + 1], st == LANDED, Pf, xf, *nxt, wl, p["Q"], dtype=np.longdouble)
        bar = urts_ref.bars(r64, rld)
        kmax = max(kmax, float(rts_ref.cond(r64["P_pred"]).max()))
        noq = urts_ref.one_step(f["y"][j + 1], st == LANDED, Pf, xf, *nxt, w, 0.0 * p["Q"])
        for key in ("x", "P"):
            with np.errstate(invalid="ignore"):
                s = rts_ref.scaled_env(noq[key], r64[key])
            s = np.where(np.isnan(s), np.inf, s)
            least[key] = min(least.get(key, np.inf), float(np.min(s / bar[key])))
            assert np.all(s >= 1e3 * bar[key]), (key, j, least[key])
    print("kappa_2(P-) <= %.2e; Q's least share / bar " % kmax + " ".join("%s %.1e" % kv for kv in least.items()))


def test_application_conditions_hold_on_the_oracle_restatement():
    """passes without the feature: the application of the GPU tests (section 20's Hover3D case: 300 envs, 48 steps,
    positions and angles measured, NumPy seeds 1 and 2) under the restated unscented filter and smoother with the default
    weights on the float64 oracle: section 20's conditions (smoothed / filtered RMSE <= 0.6 in the measured and <= 0.3 in
    the unmeasured slots, RMSE / sd in [0.8, 1.25], var_s <= var_f) hold here, so they are the device's thresholds too."""
    from branch_fd import run_rollout
    from jacobian_fd import hover_action
    from oracle.refcpu import AIRBORNE, LANDED
    a, x0, xhat0, H, r = ekf_ref.app_inputs(hover_action(), seed=1)
    n, K = ekf_ref.APP_N, ekf_ref.APP_K
    st = np.full(n, AIRBORNE, np.uint8)
    tape, _ = run_rollout("hover3d", x0, st, a.astype(np.float64))
    truth = tape["x"]
    assert (tape["status"] == AIRBORNE).all()
    z = truth @ H.T + np.sqrt(r) * np.random.default_rng(2).standard_normal((K, n, 6))
    P0 = np.repeat(ekf_ref.APP_P0[None], n, axis=0)
    f = urts_ref.oracle_filter_tapes("hover3d", a, z, H, r, ekf_ref.APP_Q, xhat0, P0, st)
    assert f["ok"].all() and (f["spread"] == 0).all()
    sm = urts_ref.smoother(f, xhat0.T, P0, st, ukf_ref.weights(), ekf_ref.APP_Q, LANDED)
    assert sm["ok"].all()
    diag = lambda m: np.diagonal(m, axis1=-2, axis2=-1)     # noqa: E731
    rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
    fig = rts_ref.app_conditions(sm["x"], diag(sm["P"]), sm["x0"], diag(sm["P0"]), f["x"], f["var"], truth, x0.T, rmse0)
    print(fig)
