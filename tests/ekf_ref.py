"""A plain NumPy restatement of one step of the extended Kalman filter of cs_rollout_ekf (include/copterstep.h): the
covariance prediction P- = A P A^T + Q from a given step Jacobian, and the sequential scalar measurement updates, batched
over envs, in float64 or numpy.longdouble.  The GPU tests hold the kernel to it one step at a time on the kernel's own
tapes (the Jacobian depends on the filter's own mean, so a reference chained over K steps could take another branch than
the device at a touchdown); tests/test_rollout_ekf_cpu.py checks it against the joint-form update and the dense Gaussian
log-density.  Also the bar of those comparisons and the application of the issue's section 6 on the CPU oracle."""
import numpy as np

FLOOR = 1e-12      # scaled (gpu_util.scaled_err's scaling): one step is ~300 operations per entry
LOG_2PI = np.log(2 * np.pi)


def mirror_upper(P):
    """the symmetric matrix with P's upper triangle: what the kernel keeps and writes"""
    up = np.triu(P)
    return up + np.swapaxes(np.triu(P, 1), -1, -2)


def predict_cov(A, P, Q, dtype=np.float64):
    """P- = A P A^T + Q, [N,12,12]; the upper triangle mirrored"""
    A, P, Q = (np.asarray(m).astype(dtype) for m in (A, P, Q))
    W = np.einsum("nij,njk->nik", A, P)
    return mirror_upper(np.einsum("nij,nkj->nik", W, A) + Q)


def sequential_update(x, P, H, r, z, dtype=np.float64):
    """The M scalar updates of one step, in order, a NaN z skipped.  x [N,12], P [N,12,12], H [M,12], r [M], z [N,M].
    Returns (x, P (upper triangle mirrored), nis [N], loglik [N] (the step's term), ok [N])."""
    x, P, H, r = (np.array(m).astype(dtype) for m in (x, P, H, r))
    z = np.asarray(z, np.float64)
    n = x.shape[0]
    nis, ll, ok = np.zeros(n, dtype), np.zeros(n, dtype), np.ones(n, bool)
    two_pi = dtype(2) * np.arccos(dtype(-1))
    for i in range(H.shape[0]):
        use = ~np.isnan(z[:, i])
        if not use.any():
            continue
        h = H[i]
        p = P @ h
        s = p @ h + r[i]
        zi = np.where(use, z[:, i], 0.0).astype(dtype)
        nu = zi - x @ h
        with np.errstate(divide="ignore", invalid="ignore"):
            g = p / s[:, None]
            e = nu * nu / s
            term = (e + np.log(two_pi * s)) / dtype(2)
        ok &= ~use | (np.isfinite(s.astype(np.float64)) & (s > 0))
        m = use[:, None]
        x = np.where(m, x + g * nu[:, None], x)
        P = np.where(m[:, :, None], P - g[:, :, None] * p[:, None, :], P)
        nis = np.where(use, nis + e, nis)
        ll = np.where(use, ll - term, ll)
    return x, mirror_upper(P), nis, ll, ok


def one_step(A, P_prev, x_pred, Q, H, r, z, dtype=np.float64):
    """one filter step from the device's own inputs: dict of P_pred, x, P, var, nis, loglik (the step's term), ok"""
    Pm = predict_cov(A, P_prev, Q, dtype)
    x, P, nis, ll, ok = sequential_update(x_pred, Pm, H, r, z, dtype)
    return dict(P_pred=Pm, x=x, P=P, var=np.diagonal(P, axis1=1, axis2=2), nis=nis, loglik=ll, ok=ok)


def joint_update(x, P, H, r, z):
    """the joint form for one env, no missing rows: K = P H^T (H P H^T + R)^-1 (numpy.linalg.solve); returns (x, P, nis,
    loglik term, cond(S))"""
    S = H @ P @ H.T + np.diag(r)
    nu = z - H @ x
    K = np.linalg.solve(S, H @ P).T
    sol = np.linalg.solve(S, nu)
    _, logdet = np.linalg.slogdet(S)
    nis = nu @ sol
    return x + K @ nu, P - K @ H @ P, nis, -0.5 * (nis + logdet + len(z) * LOG_2PI), np.linalg.cond(S)


def scaled(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    e = np.where(np.isnan(got) & np.isnan(ref), 0.0, e)
    return float(np.max(e)) if e.size else 0.0


def bars(ref64, refld, keys=("x", "P", "var", "nis", "loglik")):
    """per output: 100 x the float64 reference's own distance from the longdouble one, floored at FLOOR"""
    return {k: max(100.0 * scaled(ref64[k], np.asarray(refld[k]).astype(np.float64)), FLOOR) for k in keys}


def test_Q():
    """the process noise of the tests: diag(1e-4 .. 1e-3, distinct per slot) plus small off-diagonals, every entry far
    above the floor"""
    i = np.arange(12)
    Q = 1e-6 * (1.0 + 0.5 * np.cos(i[:, None] + i[None, :]))
    Q[i, i] = np.linspace(1e-4, 1e-3, 12)
    assert np.array_equal(Q, Q.T) and np.linalg.eigvalsh(Q).min() > 0
    return Q


test_Q.__test__ = False


# ---------------------------------------------------------------------------------------------------------------------
# the application (Hover3D, section 6 of the issue): its inputs, and the filter restated on the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
APP_N, APP_K = 300, 48
APP_SLOTS = (0, 2, 4, 6, 8, 10)
APP_SIGMA = np.array([0.1, 0.1, 0.1, 0.01, 0.01, 0.01])
APP_P0 = np.diag([0.01, 1.0, 0.01, 1.0, 0.01, 1.0, 0.01, 0.04, 0.01, 0.04, 0.01, 0.04])
APP_Q = 1e-8 * np.eye(12)


def app_inputs(hover, seed=1):
    """(actions [K,N,4] float32, true start x0 [12,N], filter start xhat0 [12,N], H [6,12], r [6]) from NumPy seed `seed`"""
    rng = np.random.default_rng(seed)
    n, K = APP_N, APP_K
    a = (hover + 0.02 * rng.standard_normal((K, n, 4))).astype(np.float32)
    x0 = np.zeros((12, n))
    x0[4] = -10.0
    x0[[1, 3, 5]] = 0.5 * rng.standard_normal((3, n))
    x0[[6, 8]] = 0.05 * rng.standard_normal((2, n))
    xhat0 = x0 + np.sqrt(np.diag(APP_P0))[:, None] * rng.standard_normal((12, n))
    H = np.zeros((6, 12))
    H[np.arange(6), APP_SLOTS] = 1.0
    return a, x0, xhat0, H, APP_SIGMA ** 2


def app_conditions(x, P_diag_last, nis, truth, rmse0_vel):
    """the four conditions of the application on a filter's result: x [K,N,12], the last posterior's diagonal [N,12], nis
    [K,N], truth [K,N,12]; returns the figures (asserts inside)"""
    mean_nis = float(np.mean(nis))
    assert abs(mean_nis - 6.0) <= 0.3, mean_nis
    err = x[-1] - truth[-1]
    rmse = np.sqrt(np.mean(err ** 2, axis=0))
    sd = np.sqrt(np.mean(P_diag_last, axis=0))
    ratio = rmse / sd
    assert np.all((ratio >= 0.8) & (ratio <= 1.25)), ratio
    assert np.all(rmse[[0, 2, 4]] < 0.5 * 0.1), rmse[[0, 2, 4]]
    assert np.all(rmse[[1, 3, 5]] < 0.2 * rmse0_vel), (rmse[[1, 3, 5]], rmse0_vel)
    return dict(mean_nis=mean_nis, rmse=rmse, sd=sd, ratio=ratio)
