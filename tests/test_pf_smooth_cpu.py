"""The backward-simulation particle smoother without a GPU (cs_pf_smooth): the ABI layout and the
argument errors of the entry point; the kernel's draw and whitening header (gym_copter_amd/csrc/pfs_draw.h) compiled for
the host (tests/host/pfs_draw_host) against the NumPy restatement (tests/pf_smooth_ref.py), bit for bit; the host side's
inverse factor; and self-checks of that restatement -- a linear-Gaussian system against the Kalman / Rauch-Tung-Striebel
smoother, the status indicator, the dead row, and the application of the GPU tests on the float64 oracle.  Those that
pass without the feature are labelled so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ekf_ref
import pf_ref
import pf_smooth_ref as R
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "pfs_draw_host")
WRAP = (1 << 32) - 1


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors (these fail without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    import gym_copter_amd
    lib = _lib.load()
    assert re.search(r"int cs_pf_smooth\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_pf_smooth_io\* \w+,"
                     r"\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_pf_smooth") and "cs_pf_smooth" in _lib.SYMBOLS
    assert lib.cs_pf_smooth.argtypes[2] is C.POINTER(_lib.PfSmoothIO)
    assert re.search(r"#define CS_PFS_MAX_PATHS %d\b" % _lib.PFS_MAX_PATHS, HEADER)
    assert lib.cs_version() == 5 == _lib.ABI_VERSION and re.search(r"#define CS_ABI_VERSION 5\b", HEADER)
    import importlib
    pf_module = importlib.import_module("gym_copter_amd.pf")     # (gym_copter_amd.pf names the driver function)
    assert gym_copter_amd.CopterVecEnv.rollout_pf_smooth is pf_module.rollout_pf_smooth
    assert gym_copter_amd.pf_smooth is pf_module.pf_smooth
    assert gym_copter_amd.PfSmoothResult._fields == ("x", "var", "idx", "idx0", "ok", "logb_tape", "bwq_tape")
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    assert "shard-local" in ShardedCopterVecEnv.rollout_pf_smooth.__doc__


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_pf_smooth_io \{(.*?)\} cs_pf_smooth_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.PfSmoothIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.PfSmoothIO._fields_):
        size = 8 if "*" in ctype or "double" in ctype else 4
        assert C.sizeof(mirror) == size, name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.PfSmoothIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.PfSmoothIO) == offset == 24 + 15 * 8


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev, io.x_dev = 0x1000, 0x4000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _sio(**kw):
    sio = _lib.PfSmoothIO()
    sio.struct_size = C.sizeof(sio)
    sio.num_particles, sio.num_paths, sio.first_step = 256, 64, 1
    sio.part_tape_dev, sio.pstatus_tape_dev, sio.lw_tape_dev, sio.wq_tape_dev = 0x6000, 0x7001, 0x8000, 0x9000
    sio.Linv_dev = 0xa000
    for k, v in kw.items():
        setattr(sio, k, v)
    return sio


START = dict(part_in_dev=0xb000, pstatus_in_dev=0xc001, lw_in_dev=0xd000)


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_pf_smooth
    err = lib.cs_last_error
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in err()
    assert fn(None, C.byref(_io(struct_size=8)), C.byref(_sio()), None) == _lib.ERR_ABI
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null sio" in err()
    # a wrong struct_size is reported before anything else in the block
    bad = _sio(struct_size=C.sizeof(_lib.PfSmoothIO) + 8, num_particles=3, num_paths=0, Linv_dev=None)
    assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in err()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_sio()), None) == _lib.ERR_ARG and b"num_steps" in err()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_sio()), None) == _lib.ERR_ARG and b"actions_dev" in err()
    for key in ("start_force_dev", "start_prev_shaping_dev", "reward_dev", "terminated_dev", "truncated_dev",
                "status_dev", "gx_dev", "gr_dev", "g_actions_dev", "g_x0_dev"):
        assert fn(None, C.byref(_io(**{key: 0xb000})), C.byref(_sio()), None) == _lib.ERR_ARG, key
        assert b"NULL" in err() or b"start_x_dev is required" in err(), key
    assert fn(None, C.byref(_io(start_x_dev=0xb000, start_status_dev=0xc000)), C.byref(_sio()), None) == _lib.ERR_ARG
    assert b"must be NULL" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(out_dtype=5)), None) == _lib.ERR_ARG and b"out_dtype" in err()
    for P in (0, 32, 96, 1000, 2048, -64):
        assert fn(None, C.byref(_io()), C.byref(_sio(num_particles=P)), None) == _lib.ERR_ARG
        assert b"num_particles" in err()
    for S in (0, -1, 1025):
        assert fn(None, C.byref(_io()), C.byref(_sio(num_paths=S)), None) == _lib.ERR_ARG and b"num_paths" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(first_step=0)), None) == _lib.ERR_ARG and b"first_step" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(first_step=0xFFFFFFFE)), None) == _lib.ERR_ARG and b"first_step" in err()
    for key in ("part_tape_dev", "pstatus_tape_dev", "lw_tape_dev", "Linv_dev"):
        assert fn(None, C.byref(_io()), C.byref(_sio(**{key: None})), None) == _lib.ERR_ARG and b"required" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(wq_tape_dev=None)), None) == _lib.ERR_ARG and b"wq_tape_dev" in err()
    # a partial start triple, and idx0 without a start
    for gone in START:
        part = dict(START, **{gone: None})
        assert fn(None, C.byref(_io()), C.byref(_sio(**part)), None) == _lib.ERR_ARG and b"all three or none" in err()
    assert fn(None, C.byref(_io()), C.byref(_sio(idx0_dev=0xe000)), None) == _lib.ERR_ARG and b"idx0_dev needs" in err()
    for key in ("part_tape_dev", "lw_tape_dev", "Linv_dev", "logb_tape_dev", "var_dev"):
        assert fn(None, C.byref(_io()), C.byref(_sio(**{key: 0xe004})), None) == _lib.ERR_ARG and b"aligned" in err()
    for key in ("wq_tape_dev", "end_idx_dev", "idx_dev", "bwq_tape_dev"):
        assert fn(None, C.byref(_io()), C.byref(_sio(**{key: 0xe002})), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io(x_dev=0x4004)), C.byref(_sio()), None) == _lib.ERR_ARG and b"aligned" in err()
    # what is right reaches the context: a float32 var needs 4 bytes only; end_idx replaces the wq tape; every output NULL
    for good in (_sio(out_dtype=_lib.JAC_F32, var_dev=0xe004), _sio(wq_tape_dev=None, end_idx_dev=0xe004),
                 _sio(idx0_dev=0xe000, **START), _sio()):
        assert fn(None, C.byref(_io()), C.byref(good), None) == _lib.ERR_ARG and err() == b"null context"
    assert fn(None, C.byref(_io(x_dev=None)), C.byref(_sio()), None) == _lib.ERR_ARG and err() == b"null context"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the draws and the whitening: the kernel's header on the host against the restatement, bit for bit (fails without the
#    feature: the program is its code)
# ---------------------------------------------------------------------------------------------------------------------
def _host(*args):
    return subprocess.run([HOST] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split()


def test_reference_uniforms_match_the_host_program():
    pts = [(s, g, nonce, kg, m) for s in (0, 3, (1 << 64) - 1) for g in (0, 5, WRAP) for nonce in (0, WRAP)
           for kg in (0, 1, 12, WRAP) for m in (0, 1, 255, 1023)]
    out = _host("u", *[v for p in pts for v in p])
    assert len(out) == len(pts)
    for line, (s, g, nonce, kg, m) in zip(out, pts):
        u = int(R.draw_u(s, g, nonce, kg, m))
        assert u == int(line, 16) < 1 << 24, (s, g, nonce, kg, m)
        # slot 13 of the filter's keys: neither a state component's words nor the resampling word
        assert u == int(pf_ref.words(s, g, nonce, kg, m, 13)[0]) >> 8


def test_reference_index_matches_the_host_program_in_exact_integers():
    rng = np.random.default_rng(7)
    one = pf_ref.WQ_ONE
    cases = [(np.array([one] * 64), u) for u in (0, 1, (1 << 24) - 1, 1 << 23)]
    cases += [(np.array([0] * 63 + [one]), 0), (np.array([one] + [0] * 63), (1 << 24) - 1)]
    cases += [(np.array([0, 0, 5, 0, 0, 7, 0, 0]), u) for u in (0, 6990506, 6990507, (1 << 24) - 1)]
    cases += [(np.zeros(64, np.int64), 12345)]                           # every weight 0: P - 1
    cases += [(np.full(1024, one), u) for u in (0, (1 << 24) - 1, 16384, 16383)]       # S1 = 2^34: both sides < 2^58
    for P in (64, 256, 1024):
        for _ in range(6):
            w = np.where(rng.uniform(size=P) < 0.3, 0, rng.integers(0, one + 1, P))
            w[rng.integers(P)] = one
            cases.append((w, int(rng.integers(0, 1 << 24))))
    for w, u in cases:
        got = int(_host("index", u, *w.tolist())[0])
        want = int(R.draw_index(w[None], np.array([u]))[0])
        assert got == want, (w[:8], u, got, want)
        # the definition, in Python integers
        C_, S1 = np.cumsum([int(v) for v in w]).tolist(), int(sum(int(v) for v in w))
        first = next((p for p, c in enumerate(C_) if (c << 24) > u * S1), len(w) - 1)
        assert got == first
    # 5 / 12 of 2^24 = 6 990 506.67: u = 6 990 506 still draws index 2, the next one index 5
    assert int(R.draw_index(np.array([[0, 0, 5, 0, 0, 7, 0, 0]]), np.array([6990506]))[0]) == 2
    assert int(R.draw_index(np.array([[0, 0, 5, 0, 0, 7, 0, 0]]), np.array([6990507]))[0]) == 5


def test_reference_whitening_matches_the_host_program_bit_for_bit():
    rng = np.random.default_rng(5)
    L = np.tril(rng.standard_normal((12, 12))) * 30.0
    L[7, :5] = 0.0
    for _ in range(4):
        x = rng.standard_normal(12) * 10.0 ** rng.integers(-3, 3)
        out = _host("whiten", *[float(v).hex() for v in L.ravel()], *[float(v).hex() for v in x])
        got = np.array([float.fromhex(t) for t in out])
        assert np.array_equal(got.view(np.uint64), R.whiten(L, x[None])[0].view(np.uint64))


def test_host_side_inverse_factor_is_the_restatement_and_refuses_a_singular_q():
    import importlib
    noise_inverse = importlib.import_module("gym_copter_amd.pf").noise_inverse
    for Q in (ekf_ref.test_Q(), pf_ref.APP_Q, np.linspace(1e-6, 2.0, 12)):
        Linv = noise_inverse(Q)
        assert np.array_equal(Linv.view(np.uint64), R.noise_inverse(Q).view(np.uint64))
        assert np.array_equal(Linv, np.tril(Linv))
        assert np.abs(Linv @ pf_ref.factor_q(Q) - np.eye(12)).max() < 1e-12
    q = pf_ref.APP_Q.copy()
    q[4] = 0.0
    with pytest.raises(ValueError, match="slot 4 has zero variance"):
        noise_inverse(q)
    with pytest.raises(ValueError, match="positive definite"):
        noise_inverse(np.ones((12, 12)))
    with pytest.raises(ValueError, match="Q must have shape"):
        noise_inverse(np.ones(6))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the restatement itself (these pass with tests/pf_smooth_ref.py alone)
# ---------------------------------------------------------------------------------------------------------------------
def test_status_indicator_excludes_the_nearest_particle():
    """the particle whose propagated point IS the path's next point, but whose status after the step differs, has
    log beta = -inf and weight 0; among the others the nearest weighs most"""
    rng = np.random.default_rng(11)
    P, S = 64, 8
    Linv = R.noise_inverse(np.full(12, 0.01))
    mu = rng.standard_normal((1, P, 12)) * 0.1
    sigma = np.full((1, P), pf_ref.AIRBORNE_, np.uint8)
    Xt = np.repeat(mu[:, :1], S, axis=1) + 0.0                         # the next point of every path: particle 0's mu
    st = np.full((1, S), pf_ref.AIRBORNE_, np.uint8)
    lw = np.full((1, P), pf_ref.neg_ln(P))
    idx, logb, bwq, dead = R.backward_step(3, [0], 0, 5, lw, mu, sigma, Xt, st, Linv)
    assert np.all(logb[0, :, 0] == lw[0, 0]) and np.all(bwq[0, :, 0] == pf_ref.WQ_ONE) and not dead.any()
    sigma[0, 0] = pf_ref.LANDED_                                        # ... now it lands, and the path's point flies
    idx, logb, bwq, dead = R.backward_step(3, [0], 0, 5, lw, mu, sigma, Xt, st, Linv)
    assert np.all(np.isneginf(logb[0, :, 0])) and np.all(bwq[0, :, 0] == 0) and not dead.any()
    assert np.all(idx != 0) and np.all(np.isfinite(logb[0, :, 1:]))
    d = np.sum((R.whiten(Linv, mu[0, 1:]) - R.whiten(Linv, mu[0, 0])) ** 2, axis=1)
    assert np.all(bwq[0, :, 1:].argmax(axis=1) == d.argmin())


def test_a_row_of_minus_infinity_draws_uniformly_and_clears_ok():
    rng = np.random.default_rng(12)
    P, S, K = 64, 256, 2
    Linv = R.noise_inverse(np.full(12, 0.01))
    part = rng.standard_normal((K, 2, P, 12)) * 0.1
    pst = np.full((K, 2, P), pf_ref.AIRBORNE_, np.uint8)
    pst[1, 1] = pf_ref.CRASHED_                                         # env 1: no airborne particle reaches a crashed one
    lw = np.full((K, 2, P), pf_ref.neg_ln(P))
    wq = np.full((K, 2, P), pf_ref.WQ_ONE)
    res = R.run(lambda k, X, s: (X, s), 3, [0, 1], 0, part, pst, lw, wq, Linv, S, keep_tapes=True)
    assert res["ok"].tolist() == [True, False]
    assert np.all(np.isneginf(res["logb"][0, 1])) and np.all(res["bwq"][0, 1] == pf_ref.WQ_ONE)
    assert np.all(np.isfinite(res["logb"][0, 0]))
    # uniform: index = floor(u P / 2^24)
    u = R.draw_u(3, 1, 0, 1, np.arange(S))
    assert np.array_equal(res["idx"][0, 1], (u * P) >> 24)
    assert len(np.unique(res["idx"][0, 1])) > P // 2


def _kalman_rts(A, Q, H, r, x0, P0, z):
    """the exact filtered and smoothed means and covariances of x' = A x + w, z = H x + e"""
    xf, Pf, xp, Pp = [], [], [], []
    x, Pk = x0, P0
    for zk in z:
        x, Pk = A @ x, A @ Pk @ A.T + Q
        xp.append(x)
        Pp.append(Pk)
        s = H @ Pk @ H.T + np.diag(r)
        G = Pk @ H.T @ np.linalg.inv(s)
        x, Pk = x + G @ (zk - H @ x), Pk - G @ s @ G.T
        xf.append(x)
        Pf.append(Pk)
    xs, Ps = [xf[-1]], [Pf[-1]]
    for k in range(len(z) - 2, -1, -1):
        G = Pf[k] @ A.T @ np.linalg.inv(Pp[k + 1])
        xs.insert(0, xf[k] + G @ (xs[0] - xp[k + 1]))
        Ps.insert(0, Pf[k] + G @ (Ps[0] - Pp[k + 1]) @ G.T)
    return np.array(xf), np.array(xs), np.array(Ps)


def test_linear_gaussian_toy_matches_the_rts_smoother_within_monte_carlo_error():
    """passes without the kernel.  x' = A x + w with A = [[0.5, 0.5], [0, 0.5]] on slots 0 and 1 (a position driven by a
    velocity that is not measured) and 0 elsewhere -- the other ten slots are fresh noise every step, the same density
    for every particle, so they cancel in the backward weights --, z = x_0 + e.  P = 256, S = 256, K = 16, one env.

    The S paths are draws of the smoothing distribution, so their mean has the standard error sqrt(var / S) with var
    the smoother's posterior variance (the exact one, from the RTS recursion): the bar is 4 of them.  The sample
    variance of S Gaussian draws has the relative standard error sqrt(2 / S) = 0.088: the bar is a factor within
    1 -+ 4 sqrt(2 / S) = [0.646, 1.354].

    These bars count the S draws only.  The paths are drawn from the filter's P = 256 particles, whose own error is at
    best another sqrt(var / P) = one such standard error, and more where the weights are uneven or the dynamics carry
    an error from step to step.  The toy is therefore chosen so that the filter sits near that floor: a contraction by
    0.5 per step (an error is forgotten within two steps) and a sensor as wide as the state (r = 1: the weights stay
    even).  Measured over the nonces 0 .. 9 the deviations then have an RMS of 1.37 standard errors (sqrt 2 expected)
    and a worst entry of 2.2 .. 4.1 among the 32; with A = [[1, 0.5], [0, 0.9]] and r = 0.04 the RMS is 1.6 .. 3.2 and the
    worst entry 4 .. 8, all of it the filter's (its own mean is as far from the Kalman filter's).  So at these sizes the
    test is a known answer at a fixed seed, not a guarantee over seeds: 6 of those 10 nonces stay inside both bars."""
    rng = np.random.default_rng(2)
    P, S, K, seed, nonce = 256, 256, 16, 5, 1
    A = np.zeros((12, 12))
    A[0, 0], A[0, 1], A[1, 1] = 0.5, 0.5, 0.5
    q = np.full(12, 0.01)
    q[1] = 0.04
    H = np.zeros((1, 12))
    H[0, 0] = 1.0
    r = np.array([1.0])
    P0 = np.diag([0.25, 0.25] + [1e-6] * 10)
    x0 = np.zeros(12)
    x = x0 + np.sqrt(np.diag(P0)) * rng.standard_normal(12)
    z = []
    for _ in range(K):
        x = A @ x + np.sqrt(q) * rng.standard_normal(12)
        z.append(H @ x + np.sqrt(r) * rng.standard_normal(1))
    z = np.array(z)
    xf, xs, Ps = _kalman_rts(A, np.diag(q), H, r, x0, P0, z)

    step = lambda k, X, s: (X @ A.T, s)                                 # noqa: E731
    X = pf_ref.gaussian_start(seed, [0], nonce, x0[:, None], np.linalg.cholesky(P0)[None], P)
    st = np.full((1, P), pf_ref.AIRBORNE_, np.uint8)
    f = R.filter_tapes(step, seed, [0], nonce, X, st, np.full((1, P), pf_ref.neg_ln(P)), z[:, None, :], H, r,
                       pf_ref.factor_q(q))
    res = R.run(step, seed, [0], nonce, f["part_tape"], f["pstatus_tape"], f["lw_tape"], f["wq_tape"],
                R.noise_inverse(q), S)
    assert res["ok"].all()
    var = np.diagonal(Ps, axis1=1, axis2=2)[:, :2]
    se = np.sqrt(var / S)
    dev = np.abs(res["x"][:, 0, :2] - xs[:, :2]) / se
    factor = res["var"][:, 0, :2] / var
    lo, hi = 1 - 4 * np.sqrt(2 / S), 1 + 4 * np.sqrt(2 / S)
    filt_dev = np.abs(f["x"][:, 0, :2] - xs[:, :2]) / se
    print("mean: worst %.2f standard errors (the filtered mean: %.2f); variance factor %.3f .. %.3f (bar %.3f .. %.3f)"
          % (dev.max(), filt_dev.max(), factor.min(), factor.max(), lo, hi))
    assert dev.max() <= 4.0, dev
    assert lo <= factor.min() and factor.max() <= hi, factor


# ---------------------------------------------------------------------------------------------------------------------
# 4. the application of the GPU tests on the float64 oracle (passes without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_application_improves_the_velocities_on_the_oracle():
    """pf_ref's Hover3D problem (32 envs, 32 steps, 1 024 particles) filtered and smoothed with 256 paths in NumPy over the
    oracle step: over the interior rows the smoothed RMSE of the unmeasured velocities dX, dY, dZ is below the filter's,
    in every one of the three slots; the pooled ratio is recorded as pf_smooth_ref.APP_CPU_RATIO (the GPU test allows
    the device 25 % more)."""
    from branch_fd import run_rollout
    from jacobian_fd import hover_action
    from oracle.refcpu import AIRBORNE
    a, x0, xhat0, H, r = pf_ref.app_inputs(hover_action(), seed=1)
    n, P = pf_ref.APP_N, pf_ref.APP_P
    st = np.full(n, AIRBORNE, np.uint8)
    tape, _ = run_rollout("hover3d", x0, st, a.astype(np.float64))
    truth = tape["x"]
    z = pf_ref.app_measurements(truth, H, r)

    def step(k, X, S):
        t, _ = run_rollout("hover3d", X.reshape(-1, 12).T, S.ravel(), np.repeat(a[k].astype(np.float64), P, axis=0)[None])
        return t["x"][0].reshape(n, P, 12), t["status"][0].reshape(n, P)
    g = np.arange(n)
    X = pf_ref.gaussian_start(pf_ref.APP_SEED, g, pf_ref.APP_NONCE, xhat0,
                              np.repeat(np.linalg.cholesky(ekf_ref.APP_P0)[None], n, axis=0), P)
    f = R.filter_tapes(step, pf_ref.APP_SEED, g, pf_ref.APP_NONCE, X, np.repeat(st[:, None], P, axis=1),
                       np.full((n, P), pf_ref.neg_ln(P)), z, H, r, pf_ref.factor_q(pf_ref.APP_Q))
    res = R.run(step, pf_ref.APP_SEED, g, R.APP_SMOOTH_NONCE, f["part_tape"], f["pstatus_tape"], f["lw_tape"],
                f["wq_tape"], R.noise_inverse(pf_ref.APP_Q), R.APP_S)
    assert res["ok"].all()
    for slot in R.APP_VEL_SLOTS:
        s, fl = R.app_ratio(res["x"], f["x"], truth, slots=(slot,))
        print("slot %d: smoothed rmse %.4f, filtered %.4f, ratio %.3f" % (slot, s, fl, s / fl))
        assert s < fl, slot
    s, fl = R.app_ratio(res["x"], f["x"], truth)
    print("pooled: smoothed rmse %.4f, filtered %.4f, ratio %.4f" % (s, fl, s / fl))
    assert s < fl
    assert abs(s / fl - R.APP_CPU_RATIO) < 0.005
