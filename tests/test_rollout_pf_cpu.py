"""CPU-side checks of cs_rollout_pf: the entry point declared, exported and bound, the ctypes struct mirroring the header
field by field; bad argument blocks refused without touching a device; the draws of the kernel's own header compiled for
the host (tests/host/pf_noise_host) against the NumPy restatement (tests/pf_ref.py), bit for bit; and self-checks of
that restatement -- its integer resampling, its log-likelihood against the exact Gaussian one, and the application of
the GPU tests on the float64 oracle.  Those that pass without the feature are labelled so."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import ekf_ref
import pf_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "pf_noise_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors (these fail without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_rollout_pf\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_rollout_pf_io\* \w+,"
                     r"\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_rollout_pf") and "cs_rollout_pf" in _lib.SYMBOLS
    assert lib.cs_rollout_pf.argtypes[2] is C.POINTER(_lib.RolloutPfIO)
    assert re.search(r"#define CS_PF_MAX_PARTICLES %d\b" % _lib.PF_MAX_PARTICLES, HEADER)
    assert re.search(r"#define CS_PF_MIN_PARTICLES %d\b" % _lib.PF_MIN_PARTICLES, HEADER)


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_rollout_pf_io \{(.*?)\} cs_rollout_pf_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.RolloutPfIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.RolloutPfIO._fields_):
        size = 8 if "*" in ctype or "double" in ctype else 4
        assert C.sizeof(mirror) == size, name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.RolloutPfIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.RolloutPfIO) == offset == 24 + 8 + 23 * 8


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


def _pio(**kw):
    pio = _lib.RolloutPfIO()
    pio.struct_size = C.sizeof(pio)
    pio.num_meas, pio.num_particles, pio.first_step, pio.ess_frac = 6, 256, 1, 0.5
    pio.H_dev, pio.r_dev, pio.Lq_dev, pio.z_dev, pio.L0_dev = 0x6000, 0x7000, 0x8000, 0x9000, 0xa000
    for k, v in kw.items():
        setattr(pio, k, v)
    return pio


CARRIED = dict(part_in_dev=0xb000, pstatus_in_dev=0xc001, lw_in_dev=0xd000)


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_pf
    err = lib.cs_last_error
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in err()
    assert fn(None, C.byref(_io(struct_size=8)), C.byref(_pio()), None) == _lib.ERR_ABI
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null pio" in err()
    # a wrong struct_size is reported before anything else in the block
    bad = _pio(struct_size=C.sizeof(_lib.RolloutPfIO) - 8, num_meas=99, num_particles=3, H_dev=None)
    assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in err()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_pio()), None) == _lib.ERR_ARG and b"num_steps" in err()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_pio()), None) == _lib.ERR_ARG and b"actions_dev" in err()
    for key in ("start_force_dev", "start_prev_shaping_dev"):
        assert fn(None, C.byref(_io(**{key: 0xb000})), C.byref(_pio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err()
    for key in ("reward_dev", "terminated_dev", "truncated_dev", "gx_dev", "gr_dev", "g_actions_dev", "g_x0_dev"):
        assert fn(None, C.byref(_io(**{key: 0xb000})), C.byref(_pio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err()
    assert fn(None, C.byref(_io()), C.byref(_pio(out_dtype=5)), None) == _lib.ERR_ARG and b"out_dtype" in err()
    for m in (0, -1, 13):
        assert fn(None, C.byref(_io()), C.byref(_pio(num_meas=m)), None) == _lib.ERR_ARG and b"num_meas" in err()
    for P in (0, 32, 96, 1000, 2048, -64):
        assert fn(None, C.byref(_io()), C.byref(_pio(num_particles=P)), None) == _lib.ERR_ARG
        assert b"num_particles" in err()
    assert fn(None, C.byref(_io()), C.byref(_pio(first_step=0)), None) == _lib.ERR_ARG and b"first_step" in err()
    assert fn(None, C.byref(_io()), C.byref(_pio(first_step=0xFFFFFFFE)), None) == _lib.ERR_ARG and b"first_step" in err()
    for v in (-0.1, 1.5, float("nan")):
        assert fn(None, C.byref(_io()), C.byref(_pio(ess_frac=v)), None) == _lib.ERR_ARG and b"ess_frac" in err()
    for key in ("H_dev", "r_dev", "Lq_dev", "z_dev"):
        assert fn(None, C.byref(_io()), C.byref(_pio(**{key: None})), None) == _lib.ERR_ARG and b"required" in err()
    # exactly one start
    none = _io(start_x_dev=None, start_status_dev=None)
    assert fn(None, C.byref(none), C.byref(_pio(L0_dev=None)), None) == _lib.ERR_ARG and b"exactly one start" in err()
    assert fn(None, C.byref(_io()), C.byref(_pio(**CARRIED)), None) == _lib.ERR_ARG and b"exactly one start" in err()
    part = dict(CARRIED, lw_in_dev=None)
    assert fn(None, C.byref(none), C.byref(_pio(L0_dev=None, **part)), None) == _lib.ERR_ARG
    assert b"exactly one start" in err()
    assert fn(None, C.byref(none), C.byref(_pio(**CARRIED)), None) == _lib.ERR_ARG and b"L0_dev" in err()
    assert fn(None, C.byref(_io(start_status_dev=None)), C.byref(_pio()), None) == _lib.ERR_ARG
    assert b"start_status_dev" in err()
    for key in ("H_dev", "r_dev", "Lq_dev", "z_dev", "L0_dev", "part_out_dev", "lw_out_dev", "part_tape_dev",
                "lw_tape_dev", "var_dev", "P_dev"):
        assert fn(None, C.byref(_io()), C.byref(_pio(**{key: 0xe004})), None) == _lib.ERR_ARG and b"aligned" in err()
    for key in ("best_dev", "wq_tape_dev", "anc_tape_dev"):
        assert fn(None, C.byref(_io()), C.byref(_pio(**{key: 0xe002})), None) == _lib.ERR_ARG and b"aligned" in err()
    assert fn(None, C.byref(_io(x_dev=0x4004)), C.byref(_pio()), None) == _lib.ERR_ARG and b"aligned" in err()
    # float32 outputs need 4 bytes only; both start forms reach the context
    ok32 = _pio(out_dtype=_lib.JAC_F32, var_dev=0xe004, ess_dev=0xe004)
    assert fn(None, C.byref(_io()), C.byref(ok32), None) == _lib.ERR_ARG and err() == b"null context"
    assert fn(None, C.byref(none), C.byref(_pio(L0_dev=None, **CARRIED)), None) == _lib.ERR_ARG
    assert err() == b"null context"
    assert fn(None, C.byref(_io(x_dev=None, status_dev=None)), C.byref(_pio(L0_dev=None)), None) == _lib.ERR_ARG
    assert err() == b"null context"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the draws: the kernel's header on the host against the restatement, bit for bit (fails without the feature: the
#    program is its code)
# ---------------------------------------------------------------------------------------------------------------------
WRAP = (1 << 32) - 1


def _seed_with_key_near_wrap():
    """a seed whose particle-filter key is within 2^24 of 2^32: key + ((k 1024 + p) 16 + j) wraps inside the grid"""
    for seed in range(1, 2000):
        if int(pf_ref.noise_key(seed)) > WRAP - (1 << 24):
            return seed
    raise AssertionError("no seed found")


def test_reference_draws_match_the_host_program_bit_for_bit():
    near = _seed_with_key_near_wrap()
    pts = [(s, g, nonce, k, p) for s in (0, 1, near, (1 << 64) - 1) for g in (0, 5, WRAP) for nonce in (0, WRAP)
           for k, p in ((0, 0), (0, 1023), (1, 0), (1, 1023), (1100, 1023), ((1 << 18) - 1, 7), (WRAP, 1023))]
    assert any(int(pf_ref.noise_key(s)) + ((k * 1024 + p) * 16 + 12) % (1 << 32) > WRAP for s, _, _, k, p in pts)
    args = [str(v) for pt in pts for v in pt]
    assert subprocess.run([HOST, "key", str(near)], check=True, capture_output=True, text=True).stdout.strip() == \
        "%08x" % int(pf_ref.noise_key(near))
    out = subprocess.run([HOST, "point"] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    for line, (s, g, nonce, k, p) in zip(out, pts):
        w = [int(t, 16) for t in line.split()]
        eps = pf_ref.noise(s, g, nonce, k, p, np.arange(12))
        assert eps.dtype == np.float32 and np.array_equal(eps.view(np.uint32), np.array(w[:12], np.uint32)), (s, g, k, p)
        assert int(pf_ref.resample_u(s, g, nonce, k)) == w[12] < 1 << 16


def test_reference_colouring_matches_the_host_program_bit_for_bit():
    rng = np.random.default_rng(5)
    L = np.tril(rng.standard_normal((12, 12)))
    L[3] = 0.0                                                  # a zero row
    L[7, :5] = 0.0
    for seed, g, nonce, k, p in ((1, 0, 0, 0, 1023), (9, WRAP, 3, 17, 255)):
        args = [str(v) for v in (seed, g, nonce, k, p)] + [float(v).hex() for v in L.ravel()]
        out = subprocess.run([HOST, "colour"] + args, check=True, capture_output=True, text=True).stdout.split()
        got = np.array([float.fromhex(t) for t in out])
        want = pf_ref.colour(L, pf_ref.noise(seed, g, nonce, k, p, np.arange(12))[None, None])[0, 0]
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert got[3] == 0.0


def test_reference_draws_have_the_irwin_hall_variance():
    """passes with tests/pf_ref.py alone.  T is a sum of four independent 16-bit uniforms: Var eps = 1 - 2^-32 (section
    14), and the fourth central moment of eps is 3 - 6/20 = 2.7 to the same accuracy, so the sample variance of n draws
    (known mean 0) has the standard error sqrt((2.7 - 1) / n).  n = 12 * 2^16 draws: one standard error is 1.5e-3."""
    n_p = 1 << 16
    eps = pf_ref.noise(11, 0, 0, 1 + np.arange(n_p)[:, None] // 1024, np.arange(n_p)[:, None] % 1024,
                       np.arange(12)[None, :]).astype(np.float64)
    n = eps.size
    var = np.mean(eps ** 2)
    se = np.sqrt(1.7 / n)
    assert abs(var - (1 - 2.0 ** -32)) <= 5 * se, (var, se)
    assert abs(np.mean(eps)) <= 5 / np.sqrt(n)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the integer resampling of the restatement (these pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_resampling_counts_are_within_one_of_their_expectation_and_monotone():
    """passes without the kernel"""
    rng = np.random.default_rng(61)
    for P in (64, 256, 1024):
        for trial in range(6):
            e = np.exp(-rng.exponential(3.0 + 3 * trial, P))
            e /= e.max()
            wq = pf_ref.quantise(e)
            if trial % 2:
                wq[rng.uniform(size=P) < 0.3] = 0
                wq[rng.integers(P)] = pf_ref.WQ_ONE
            for u in (0, 1, 12345, (1 << 16) - 1):
                anc = pf_ref.ancestors(wq, u)
                assert anc.min() >= 0 and anc.max() < P and np.all(np.diff(anc) >= 0)
                counts = np.bincount(anc, minlength=P)
                assert np.all(np.abs(counts - P * wq / wq.sum()) < 1), (P, trial, u)
                assert np.all(counts[wq == 0] == 0)


def test_reference_resampling_special_weights():
    """passes without the kernel: equal weights give the identity for every u, one heavy particle gives all-that-particle,
    and the products stay below 2^64 with every weight at 2^24"""
    for P in (64, 1024):
        full = np.full(P, pf_ref.WQ_ONE)
        for u in list(range(0, 1 << 16, 257)) + [(1 << 16) - 1]:
            assert np.array_equal(pf_ref.ancestors(full, u), np.arange(P)), (P, u)
        assert np.array_equal(pf_ref.ancestors(np.full(P, 7), 65535), np.arange(P))
        for heavy in (0, 17, P - 1):
            one = np.zeros(P, np.int64)
            one[heavy] = pf_ref.WQ_ONE
            for u in (0, 40000, 65535):
                assert np.all(pf_ref.ancestors(one, u) == heavy)
    P, S1 = 1024, 1024 * pf_ref.WQ_ONE
    assert S1 == 1 << 34 and S1 * (P << 16) == 1 << 60 and (((P - 1) << 16) + 65535) * S1 < 1 << 61
    assert P * pf_ref.WQ_ONE ** 2 == 1 << 58
    it = pf_ref.integer_step(np.full((1, P), pf_ref.WQ_ONE), np.array([65535]), 0.5)
    assert it["ess"][0] == P and not it["resampled"][0] and int(it["S2"][0]) == 1 << 58


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement's log-likelihood on a linear system (passes without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_loglik_is_the_exact_gaussian_one_within_monte_carlo_error():
    """passes without the kernel.  A LANDED start is the identity step, so x_k = x_{k-1} + w_k: a linear Gaussian system
    whose exact log-likelihood the Kalman filter (tests/ekf_ref.py) gives.  The particle filter's exp(loglik) is an
    unbiased estimate of the likelihood; over independent nonces the mean of loglik lies below the exact value by half
    the variance of loglik (second order) and scatters around it with the standard error sd / sqrt(nonces).  16 nonces
    at P = 1 024; the bar is 4 standard errors, with the bias term added to the exact value.  Measured on this input:
    |mean + bias term - exact| = 1.8 standard errors (exact -5.3873, mean -5.3287, sd 0.159)."""
    rng = np.random.default_rng(81)
    n, P, K, M = 1, 1024, 6, 2
    H = np.zeros((M, 12))
    H[0, 0], H[1, 4] = 1.0, 1.0
    r = np.array([0.04, 0.09])
    q = np.zeros(12)
    q[[0, 4]] = 0.01, 0.02
    P0 = np.diag(np.where(np.arange(12) % 4 == 0, 0.25, 1e-6))
    x0 = np.zeros((12, n))
    truth = np.cumsum(np.sqrt(q) * rng.standard_normal((K, n, 12)), axis=0) + 0.5 * rng.standard_normal((1, n, 12)) * \
        (np.arange(12) % 4 == 0)
    z = truth @ H.T + np.sqrt(r) * rng.standard_normal((K, n, M))
    # the exact value
    x, Pk, exact = x0.T.copy(), P0[None].copy(), 0.0
    for k in range(K):
        out = ekf_ref.one_step(np.eye(12)[None], Pk, x, np.diag(q), H, r, z[k])
        x, Pk, exact = out["x"], out["P"], exact + out["loglik"][0]
    nonces = 16
    ll = []
    for nonce in range(nonces):
        X = pf_ref.gaussian_start(4, np.arange(n), nonce, x0, np.linalg.cholesky(P0)[None], P)
        S = np.full((n, P), pf_ref.LANDED_, np.uint8)
        res = pf_ref.run(lambda k, X, S: (X, S), 4, np.arange(n), nonce, X, S, np.full((n, P), pf_ref.neg_ln(P)),
                         None, z, H, r, pf_ref.factor_q(q))
        assert res["ok"].all()
        ll.append(res["loglik"][0])
    ll = np.array(ll)
    se = ll.std(ddof=1) / np.sqrt(nonces)
    print("exact %.4f  mean %.4f  sd %.4f  se %.4f  bias term %.4f" % (exact, ll.mean(), ll.std(ddof=1), se,
                                                                      0.5 * ll.var(ddof=1)))
    assert abs(ll.mean() + 0.5 * ll.var(ddof=1) - exact) <= 4 * se, (ll.mean(), exact, se)
    assert se < 0.1


# ---------------------------------------------------------------------------------------------------------------------
# 5. the application of the GPU tests on the float64 oracle (passes without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def app_on_the_oracle():
    """(particle filter's result, EKF's filtered means [K,N,12], truth [K,N,12]) of the application restated in NumPy on
    the float64 oracle: Hover3D, section 19's sensors and P0, 32 envs, 32 steps, 1 024 particles"""
    from branch_fd import fd_step, run_rollout
    from jacobian_fd import hover_action
    from oracle.refcpu import AIRBORNE
    a, x0, xhat0, H, r = pf_ref.app_inputs(hover_action(), seed=1)
    n, K, P = pf_ref.APP_N, pf_ref.APP_K, pf_ref.APP_P
    st = np.full(n, AIRBORNE, np.uint8)
    tape, _ = run_rollout("hover3d", x0, st, a.astype(np.float64))
    truth = tape["x"]
    assert (tape["status"] == AIRBORNE).all()
    z = pf_ref.app_measurements(truth, H, r)
    x, Pk, xs = xhat0.T.copy(), np.repeat(ekf_ref.APP_P0[None], n, axis=0), []
    for k in range(K):
        fd, A, *_ = fd_step("hover3d", x.T, st, a[k].astype(np.float64))
        out = ekf_ref.one_step(A, Pk, fd.tape["x"][0], ekf_ref.APP_Q, H, r, z[k])
        x, Pk = out["x"], out["P"]
        xs.append(x)

    def step(k, X, S):
        t, _ = run_rollout("hover3d", X.reshape(-1, 12).T, S.ravel(), np.repeat(a[k].astype(np.float64), P, axis=0)[None])
        return t["x"][0].reshape(n, P, 12), t["status"][0].reshape(n, P)
    g = np.arange(n)
    X = pf_ref.gaussian_start(pf_ref.APP_SEED, g, pf_ref.APP_NONCE, xhat0,
                              np.repeat(np.linalg.cholesky(ekf_ref.APP_P0)[None], n, axis=0), P)
    res = pf_ref.run(step, pf_ref.APP_SEED, g, pf_ref.APP_NONCE, X, np.repeat(st[:, None], P, axis=1),
                     np.full((n, P), pf_ref.neg_ln(P)), a, z, H, r, pf_ref.factor_q(pf_ref.APP_Q))
    return res, np.array(xs), truth


def test_application_conditions_hold_on_the_oracle_restatement():
    """passes without the feature: the inputs of tests/test_gpu_rollout_pf.py::test_hover_tracking_is_calibrated satisfy
    both conditions on the CPU, at the device's seed and nonce.  Measured: position RMSE 0.055 / 0.053 / 0.062 m (the
    sensor's sigma is 0.1), ratios 0.74 .. 1.22; the EKF on the same data 0.039 / 0.031 / 0.040 m -- the particle
    filter's position RMSE is 1.53 x the EKF's (the margin the GPU test allows, plus 25 %)."""
    res, ekf_x, truth = app_on_the_oracle()
    assert res["ok"].all()
    rmse, ratio = pf_ref.app_conditions(res["x"][-1], res["var"][-1], truth[-1])
    ekf_rmse = np.sqrt(np.mean((ekf_x[-1] - truth[-1]) ** 2, axis=0))
    margin = pf_ref.position_rmse(rmse) / pf_ref.position_rmse(ekf_rmse)
    print("pf rmse %s ratio %s\nekf rmse %s\nposition rmse pf / ekf %.3f" % (np.round(rmse, 4), np.round(ratio, 2),
                                                                            np.round(ekf_rmse, 4), margin))
    assert 0.6 <= ratio.min() and ratio.max() <= 1.6                 # (room for the device's other resampling ties)
    assert abs(margin - pf_ref.APP_CPU_MARGIN) < 0.01
