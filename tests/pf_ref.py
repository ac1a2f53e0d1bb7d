"""A plain NumPy restatement of the bootstrap particle filter of cs_rollout_pf (include/copterstep.h), written from the
contract in the header: the draws (bit for bit: integer arithmetic, one float32 multiply, float64 multiplies and adds in
a fixed order), the weights in float64 or numpy.longdouble, the integer weights and everything that follows from them in
exact integer arithmetic (Python ints / uint64), the estimates, and a chained filter over any step function for the CPU
checks.  The GPU tests hold the kernel to it one step at a time on the kernel's own tapes.  The Philox round function
and the seed mix are the oracle's."""
import math

import numpy as np

from oracle.refvec import philox2x32_10, splitmix64
from mppi_ref import NOISE_SCALE

LOG_2PI = np.log(2 * np.pi)
FLOOR = 1e-12              # scaled (ekf_ref.scaled's scaling), as section 19's
WQ_ONE = 1 << 24


def neg_ln(P, dtype=np.float64):
    """-ln P: the C library's log in float64 (what the host side of cs_rollout_pf passes to the kernel)"""
    return -math.log(P) if dtype is np.float64 else -np.log(dtype(P))


def noise_key(seed):
    """lo32 of the fifth splitmix64 of the seed."""
    z = int(seed) & ((1 << 64) - 1)
    for _ in range(5):
        z = splitmix64(z)
    return np.uint32(z & 0xFFFFFFFF)


def words(seed, g, nonce, k, p, j):
    """the two Philox words of (seed, global env id, nonce, step k, particle p, slot j) as int64; the arguments broadcast"""
    g, nonce, k, p, j = (np.asarray(v, dtype=np.int64) for v in (g, nonce, k, p, j))
    key = (int(noise_key(seed)) + (((k * 1024 + p) * 16 + j) & 0xFFFFFFFF)) & 0xFFFFFFFF
    g, nonce, key = np.broadcast_arrays(g & 0xFFFFFFFF, nonce & 0xFFFFFFFF, key)
    r0, r1 = philox2x32_10(g.astype(np.uint32), nonce.astype(np.uint32), key.astype(np.uint32))
    return r0.astype(np.int64), r1.astype(np.int64)


def noise(seed, g, nonce, k, p, j):
    """eps of state component j = 0 .. 11, float32"""
    r0, r1 = words(seed, g, nonce, k, p, j)
    t = (r0 >> 16) + (r0 & 0xFFFF) + (r1 >> 16) + (r1 & 0xFFFF) - 131070
    return t.astype(np.float32) * NOISE_SCALE


def resample_u(seed, g, nonce, k):
    """u of step k: the top 16 bits of the first word of slot 12 at particle 0"""
    return words(seed, g, nonce, k, 0, 12)[0] >> 16


def eps_block(seed, g, nonce, k, P):
    """eps [len(g), P, 12] float32 of step k for the envs g"""
    g = np.asarray(g, np.int64)
    return noise(seed, g[:, None, None], nonce, k, np.arange(P)[None, :, None], np.arange(12)[None, None, :])


def colour(L, eps):
    """L eps in the kernel's order: row i = sum_{j <= i} L[i][j] (double)eps_j, j ascending, the first term starting the
    sum.  L [12,12] or [N,12,12]; eps [N,P,12] float32 -> [N,P,12] float64."""
    L = np.asarray(L, np.float64)
    if L.ndim == 2:
        L = L[None]
    e = np.asarray(eps, np.float32).astype(np.float64)
    out = np.empty(e.shape, np.float64)
    for i in range(12):
        acc = L[:, None, i, 0] * e[..., 0]
        for j in range(1, i + 1):
            acc = acc + L[:, None, i, j] * e[..., j]
        out[..., i] = acc
    return out


def factor_q(Q):
    """what CopterVecEnv.rollout_pf uploads: Q [12] -> diag sqrt(Q), Q [12,12] -> its Cholesky factor"""
    Q = np.asarray(Q, np.float64)
    return np.diag(np.sqrt(Q)) if Q.ndim == 1 else np.linalg.cholesky(Q)


# ---------------------------------------------------------------------------------------------------------------------
# one step's weights, from the previous lw and the prior particles
# ---------------------------------------------------------------------------------------------------------------------
def weight_step(lw, X, H, r, z, dtype=np.float64):
    """lw [N,P], X [N,P,12], H [M,12], r [M], z [N,M] (NaN = absent).  Returns dict: lw (normalised), e [N,P] =
    exp(lw' - m), loglik [N] (the step's term), dead [N] (no finite lw'), present [N]."""
    lw, X, H, r = (np.asarray(v).astype(dtype) for v in (lw, X, H, r))
    z = np.asarray(z, np.float64)
    n, P = lw.shape
    two_pi = dtype(2) * np.arccos(dtype(-1))
    ll = np.zeros((n, P), dtype)
    lnr = np.zeros(n, dtype)
    present = np.zeros(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(H.shape[0]):
            use = ~np.isnan(z[:, i])
            zi = np.where(use, z[:, i], 0.0).astype(dtype)
            nu = zi[:, None] - X @ H[i]
            ll = np.where(use[:, None], ll - dtype(0.5) * (nu * nu) / r[i], ll)
            lnr = np.where(use, lnr + np.log(two_pi * r[i]), lnr)
            present |= use
        lwp = lw + ll
        lwp = np.where(np.isfinite(lwp.astype(np.float64)), lwp, -np.inf)
        m = lwp.max(axis=1)
        dead = ~np.isfinite(m.astype(np.float64))
        ms = np.where(dead, dtype(0), m)
        e = np.where(dead[:, None], dtype(1), np.exp(lwp - ms[:, None]))
        norm = ms + np.log(e.sum(axis=1))
        new = np.where(dead[:, None], dtype(neg_ln(P, dtype)), np.where(present[:, None], lwp - norm[:, None], lw))
        loglik = np.where(present & ~dead, norm - dtype(0.5) * lnr, dtype(0))
    return dict(lw=new, e=e, loglik=loglik, dead=dead, present=present)


def quantise(e):
    """wq = (uint32) rint(e 2^24)"""
    return np.rint(np.asarray(e, np.float64) * float(WQ_ONE)).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# everything downstream of the integer weights: exact
# ---------------------------------------------------------------------------------------------------------------------
def integer_step(wq, u, ess_frac):
    """wq [N,P] integers, u [N] in [0, 2^16).  Returns dict: S1, S2 (Python ints per env), ess [N] float64, resampled
    [N] bool, best [N], anc [N,P] (the identity where the step does not resample)."""
    wq = np.asarray(wq).astype(np.int64)
    n, P = wq.shape
    S1 = wq.sum(axis=1)                                   # <= 2^34
    S2 = (wq * wq).sum(axis=1)                            # <= 2^58
    s1d, s2d = S1.astype(np.float64), S2.astype(np.float64)
    ess = s1d * s1d / s2d
    resampled = s1d * s1d < (float(ess_frac) * float(P)) * s2d
    best = np.argmax(wq, axis=1)                          # (the first of equal maxima)
    anc = np.tile(np.arange(P), (n, 1))
    for e in np.flatnonzero(resampled):
        anc[e] = ancestors(wq[e], int(u[e]))
    return dict(S1=S1, S2=S2, ess=ess, resampled=resampled, best=best, anc=anc)


def ancestors(wq, u):
    """systematic resampling of one env: the ancestor of slot j is the smallest p with C_p (P << 16) > ((j << 16) + u) S1;
    both sides in uint64 (asserted to fit)"""
    wq = np.asarray(wq).astype(np.uint64)
    P = wq.shape[0]
    C = np.cumsum(wq, dtype=np.uint64)
    S1 = int(C[-1])
    assert S1 * (P << 16) < 1 << 64 and (((P - 1) << 16) + u) * S1 < 1 << 64
    lhs = C * np.uint64(P << 16)
    rhs = ((np.arange(P, dtype=np.uint64) << np.uint64(16)) + np.uint64(u)) * np.uint64(S1)
    return np.searchsorted(lhs, rhs, side="right")        # the first index with lhs > rhs


def estimate(X, wq, dtype=np.float64):
    """xhat [N,12], var [N,12], cov [N,12,12] of the weighted particles; weight-0 particles left out"""
    X = np.asarray(X).astype(dtype)
    w = np.asarray(wq).astype(dtype)
    S1 = w.sum(axis=1)
    Xz = np.where(w[:, :, None] != 0, X, dtype(0))
    xh = np.einsum("np,npj->nj", w, Xz) / S1[:, None]
    d = np.where(w[:, :, None] != 0, X - xh[:, None, :], dtype(0))
    var = np.einsum("np,npj->nj", w, d * d) / S1[:, None]
    cov = np.einsum("np,npi,npj->nij", w, d, d) / S1[:, None, None]
    return xh, var, cov


def scaled(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    e = np.where((got == ref) | (np.isnan(got) & np.isnan(ref)), 0.0, e)
    return float(np.max(e)) if e.size else 0.0


def bar(ref64, refld):
    """100 x the float64 reference's own distance from its longdouble twin, floored at FLOOR (section 19's bar)"""
    return max(100.0 * scaled(ref64, np.asarray(refld).astype(np.float64)), FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# the chained filter over any step function (CPU checks only: a device may resample where this does not)
# ---------------------------------------------------------------------------------------------------------------------
def gaussian_start(seed, g, nonce, x0, L0, P):
    """particles [N,P,12] = xhat_0 + L0 eps(k = 0, p); x0 [12,N]; L0 [N,12,12] or None"""
    X = np.repeat(np.asarray(x0, np.float64).T[:, None, :], P, axis=1)
    if L0 is not None:
        X = X + colour(L0, eps_block(seed, g, nonce, 0, P))
    return X


def run(step, seed, g, nonce, X, status, lw, actions, z, H, r, Lq, ess_frac=0.5, first_step=1):
    """K steps from particles X [N,P,12], status [N,P], lw [N,P]; step(k, X, status) -> (X, status) is the physics of
    step k (no noise).  Returns dict of x, var, ess, resampled, best, loglik, ok and the carried state."""
    n, P = lw.shape
    K = np.asarray(z).shape[0]
    g = np.asarray(g, np.int64)
    out = {k: [] for k in ("x", "var", "ess", "resampled", "best", "status")}
    loglik, ok = np.zeros(n), np.ones(n, bool)
    for k in range(K):
        kg = first_step + k
        X, status = step(k, X, status)
        X = X + colour(Lq, eps_block(seed, g, nonce, kg, P))
        w = weight_step(lw, X, H, r, z[k])
        lw, loglik, ok = w["lw"], loglik + w["loglik"], ok & ~w["dead"]
        wq = quantise(w["e"])
        it = integer_step(wq, resample_u(seed, g, nonce, kg), ess_frac)
        xh, var, _ = estimate(X, wq)
        rows = np.arange(n)
        for key, v in (("x", xh), ("var", var), ("ess", it["ess"]), ("resampled", it["resampled"]),
                       ("best", it["best"]), ("status", status[rows, it["best"]])):
            out[key].append(v)
        X = np.take_along_axis(X, it["anc"][:, :, None], axis=1)
        status = np.take_along_axis(status, it["anc"], axis=1)
        lw = np.where(it["resampled"][:, None], neg_ln(P), lw)
    res = {k: np.array(v) for k, v in out.items()}
    res.update(loglik=loglik, ok=ok, part=X, pstatus=status, lw=lw)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the application (Hover3D with section 19's sensors and P0): its inputs
# ---------------------------------------------------------------------------------------------------------------------
APP_N, APP_K, APP_P = 32, 32, 1024
APP_SEED, APP_NONCE, APP_Z_SEED = 3, 0, 2
# The process noise of the application, variances per step: positions 1e-3, velocities 1e-1, angles 1e-5, rates 2e-3.
# This is roughening, not a model of the vehicle: 1 024 bootstrap particles in 12 dimensions under section 19's P0 (1 m/s
# and 0.2 rad/s of prior spread) and sensors (1 cm, 0.01 rad) collapse to a handful of survivors in the first steps, and
# the unmeasured velocities are recovered only as far as fresh noise keeps proposing them.  Chosen on the CPU
# (tests/test_rollout_pf_cpu.py) so that the filter is calibrated in every slot; with 1e-6 everywhere the ratios below
# reach 500.
APP_CPU_MARGIN = 1.53      # the particle filter's position RMSE over the EKF's on the CPU oracle (test_rollout_pf_cpu.py)
APP_Q = np.array([1e-3, 1e-1, 1e-3, 1e-1, 1e-3, 1e-1, 1e-5, 2e-3, 1e-5, 2e-3, 1e-5, 2e-3])


def app_inputs(hover, seed=1):
    """(actions [K,N,4] float32, true start x0 [12,N], filter start xhat0 [12,N], H [6,12], r [6]) from NumPy seed
    `seed`: ekf_ref.app_inputs' construction at this module's N and K"""
    import ekf_ref
    rng = np.random.default_rng(seed)
    n, K = APP_N, APP_K
    a = (hover + 0.02 * rng.standard_normal((K, n, 4))).astype(np.float32)
    x0 = np.zeros((12, n))
    x0[4] = -10.0
    x0[[1, 3, 5]] = 0.5 * rng.standard_normal((3, n))
    x0[[6, 8]] = 0.05 * rng.standard_normal((2, n))
    xhat0 = x0 + np.sqrt(np.diag(ekf_ref.APP_P0))[:, None] * rng.standard_normal((12, n))
    H = np.zeros((6, 12))
    H[np.arange(6), ekf_ref.APP_SLOTS] = 1.0
    return a, x0, xhat0, H, ekf_ref.APP_SIGMA ** 2


def app_measurements(truth, H, r):
    """z [K,N,6] = H truth + sqrt(r) N(0, 1) from NumPy seed APP_Z_SEED"""
    rng = np.random.default_rng(APP_Z_SEED)
    return np.asarray(truth, np.float64) @ H.T + np.sqrt(r) * rng.standard_normal((APP_K, APP_N, H.shape[0]))


def app_conditions(x_last, var_last, truth_last):
    """the two conditions of the application after the last step: the position RMSE below the sensor's sigma, and per
    slot RMSE / sqrt(mean var) within [0.5, 2]; returns (rmse [12], ratio [12]) (asserts inside)"""
    import ekf_ref
    err = np.asarray(x_last) - np.asarray(truth_last)
    rmse = np.sqrt(np.mean(err ** 2, axis=0))
    ratio = rmse / np.sqrt(np.mean(np.asarray(var_last), axis=0))
    assert np.all(rmse[[0, 2, 4]] < ekf_ref.APP_SIGMA[0]), rmse[[0, 2, 4]]
    assert np.all((ratio >= 0.5) & (ratio <= 2.0)), ratio
    return rmse, ratio


def position_rmse(rmse):
    return float(np.sqrt(np.mean(np.asarray(rmse)[[0, 2, 4]] ** 2)))


# ---------------------------------------------------------------------------------------------------------------------
# the problem of the GPU tests: five envs, one per situation
# ---------------------------------------------------------------------------------------------------------------------
TEST_N, TEST_K = 5, 12
AIRBORNE_, CRASHED_, LANDED_ = 3, 0, 1


def test_problem(rng, A, hover, M=6, dense=True):
    """(x0 [12,N], status0 [N], P0 [N,12,12], actions [K,N,A] float32, H [M,12], r [M]) for N = 5 envs:
      0  a high hover under a wide P0: the weights degenerate, the filter resamples, some wq are 0
      1  a descent 4 cm above the ground at 1 m/s with the altitude and the descent rate uncertain: inside the horizon
         some particles crash (dz > 1 at contact), some level and land, some still fly
      2  a LANDED start      3  a CRASHED start
      4  motors outside [0, 1] on both sides under a tight P0"""
    n, K = TEST_N, TEST_K
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[1], x[3] = rng.uniform(-0.3, 0.3, (2, n))
    x[4] = rng.uniform(-8, -4, n)
    x[5] = rng.uniform(-0.5, 0.5, n)
    x[6], x[8] = rng.uniform(-0.05, 0.05, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-0.3, 0.3, (4, n))
    st = np.full(n, AIRBORNE_, np.uint8)
    x[4, 1], x[5, 1] = -0.04, 1.0
    x[4, 2], x[5, 2], st[2] = 0.0, 0.0, LANDED_
    st[3] = CRASHED_
    m = rng.standard_normal((n, 12, 12))
    P0 = 0.5 * (m @ np.swapaxes(m, 1, 2) / 12 + 0.2 * np.eye(12))
    P0 = (P0 + np.swapaxes(P0, 1, 2)) / 2
    P0[1] = np.diag([1e-4] * 4 + [0.03 ** 2, 0.5 ** 2] + [1e-4] * 6)
    P0[2:] *= 2e-4
    a = hover * rng.uniform(0.8, 1.2, (K, n, A))
    a[:, 4] = np.where(rng.uniform(size=(K, A)) < 0.5, rng.uniform(-0.4, -0.01, (K, A)), a[:, 4])
    a[0, 4, A - 1] = 1.2
    if dense:
        H = rng.standard_normal((M, 12)) / np.sqrt(12)
    else:
        H = np.zeros((M, 12))
        H[np.arange(M), rng.permutation(12)[:M]] = 1.0
    return x, st, P0, a.astype(np.float32), H, rng.uniform(0.01, 0.1, M)


test_problem.__test__ = False
