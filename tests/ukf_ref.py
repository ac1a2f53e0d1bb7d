"""A plain NumPy restatement of one step of the unscented Kalman filter of cs_rollout_ukf (include/copterstep.h), batched
over envs, in float64 or numpy.longdouble: the weights of the scaled transform, the Cholesky factor (restating
rts_solve.h's rts_cholesky), the 25 sigma points, the weighted moments of the propagated points, and ekf_ref's sequential
scalar updates.  In float64 it follows gym_copter_amd/csrc/ukf_points.h operation by operation, so that the host build of
that header (tests/host/ukf_points_host) agrees with it bit for bit:

  factor   column j = 0 .. 11: for i < j  s = P[i][j]; s -= U[k][i] * U[k][j], k = 0 .. i-1; U[i][j] = s * inv[i];
           then d = P[j][j]; d -= U[k][j] * U[k][j], k = 0 .. j-1; inv[j] = 1 / sqrt(d).  ok: every d > 0 and finite.
  points   L = U^T with L[j][j] = 1 / inv[j]; point 0 = x, point 1+j = x + gamma * L[:,j], point 13+j = x - gamma * L[:,j]
           for the entries a >= j, x's own above them.
  moments  about y0 over the points 1 .. 24 IN THIS ORDER, from zero: sy += y_i; d_i = y_i - y0; S += d_i d_i^T.
           x- = wm0 * y0 + wi * sy;  m = x- - y0;  c2 = 2 - (wc0 + 24 * wi);
           P- = (wi * S - c2 * (m m^T)) + Q, the upper triangle mirrored.
  landed   x- = x, P- = P + Q.

The GPU tests hold the kernel to it one step at a time on the kernel's own tapes (tests/test_gpu_rollout_ukf.py);
tests/test_rollout_ukf_cpu.py checks it against the linear and the quadratic case.  Also the filter restated over the
float64 oracle's step, for the starts and the application of the GPU tests."""
import numpy as np

import ekf_ref

FLOOR = ekf_ref.FLOOR
NP = 25
SETTINGS = ((1.0, 0.0, 1.0), (0.5, 2.0, 0.0), (1.0, 0.0, 0.0))     # (alpha, beta, kappa) of the tests


def weights(alpha=1.0, beta=0.0, kappa=1.0, dtype=np.float64):
    """(gamma, wm0, wc0, wi) in dtype, in gym_copter_amd.ukf.weights' order of operations"""
    a, b, k = dtype(alpha), dtype(beta), dtype(kappa)
    lam = a * a * (dtype(12) + k) - dtype(12)
    c = dtype(12) + lam
    wm0 = lam / c
    return np.sqrt(c), wm0, wm0 + dtype(1) - a * a + b, dtype(1) / (dtype(2) * c)


def cholesky(P, dtype=np.float64):
    """rts_cholesky, batched: P [N,12,12] (upper triangle read) -> (U [N,12,12] upper with inv[j] on the diagonal, ok [N])"""
    P = np.asarray(P).astype(dtype)
    n = P.shape[0]
    U = np.zeros((n, 12, 12), dtype)
    ok = np.ones(n, bool)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(12):
            for i in range(j):
                s = P[:, i, j].copy()
                for k in range(i):
                    s = s - U[:, k, i] * U[:, k, j]
                U[:, i, j] = s * U[:, i, i]
            d = P[:, j, j].copy()
            for k in range(j):
                d = d - U[:, k, j] * U[:, k, j]
            d64 = d.astype(np.float64)
            ok &= (d > 0) & np.isfinite(d64)
            U[:, j, j] = dtype(1) / np.sqrt(d)
    return U, ok


def points(x, P, gamma, dtype=np.float64):
    """x [N,12], P [N,12,12] -> (points [N,25,12], ok [N] of the factor, U)"""
    x = np.asarray(x).astype(dtype)
    U, ok = cholesky(P, dtype)
    n = x.shape[0]
    pts = np.repeat(x[:, None, :], NP, axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for j in range(12):
            for a in range(j, 12):
                t = dtype(gamma) * (dtype(1) / U[:, j, j] if a == j else U[:, j, a])
                pts[:, 1 + j, a] = x[:, a] + t
                pts[:, 13 + j, a] = x[:, a] - t
    assert pts.shape == (n, NP, 12)
    return pts, ok, U


def moments(y, w, Q, dtype=np.float64):
    """y [N,25,12] the propagated points, w = (gamma, wm0, wc0, wi), Q [12,12] -> (x- [N,12], P- [N,12,12])"""
    y, Q = np.asarray(y).astype(dtype), np.asarray(Q).astype(dtype)
    _, wm0, wc0, wi = (dtype(v) for v in w)
    y0 = y[:, 0]
    sy = np.zeros_like(y0)
    S = np.zeros((y.shape[0], 12, 12), dtype)
    for i in range(1, NP):
        d = y[:, i] - y0
        sy = sy + y[:, i]
        S = S + d[:, :, None] * d[:, None, :]
    xm = wm0 * y0 + wi * sy
    m = xm - y0
    c2 = dtype(2) - (wc0 + dtype(24) * wi)
    Pm = (wi * S - c2 * (m[:, :, None] * m[:, None, :])) + Q
    return xm, ekf_ref.mirror_upper(Pm)


def moments_two_pass(y, w, Q):
    """the textbook form: x- = sum wm_i y_i, P- = sum wc_i (y_i - x-)(y_i - x-)^T + Q, in longdouble"""
    y = np.asarray(y).astype(np.longdouble)
    _, wm0, wc0, wi = (np.longdouble(v) for v in w)
    wm = np.full(NP, wi)
    wc = wm.copy()
    wm[0], wc[0] = wm0, wc0
    xm = np.einsum("i,nij->nj", wm, y)
    d = y - xm[:, None]
    return xm, np.einsum("i,nia,nib->nab", wc, d, d) + np.asarray(Q).astype(np.longdouble)


def one_step(y, landed, x_prev, P_prev, w, Q, H, r, z, dtype=np.float64):
    """One filter step from the propagated points y [N,25,12]: the moments (for the lanes of `landed` [N] bool:
    x- = x_prev, P- = P_prev + Q) and the sequential update.  Returns dict of x_pred, P_pred, x, P, var, nis, loglik (the
    step's term), ok (the update's)."""
    xm, Pm = moments(y, w, Q, dtype)
    landed = np.asarray(landed, bool)
    Pl = ekf_ref.mirror_upper(np.asarray(P_prev).astype(dtype) + np.asarray(Q).astype(dtype))
    xm = np.where(landed[:, None], np.asarray(x_prev).astype(dtype), xm)
    Pm = np.where(landed[:, None, None], Pl, Pm)
    x, P, nis, ll, ok = ekf_ref.sequential_update(xm, Pm, H, r, z, dtype)
    return dict(x_pred=xm, P_pred=Pm, x=x, P=P, var=np.diagonal(P, axis1=1, axis2=2), nis=nis, loglik=ll, ok=ok)


def bars(ref64, refld, keys):
    """per output: 100 x the float64 reference's own distance from the longdouble one, floored at FLOOR"""
    return ekf_ref.bars(ref64, refld, keys)


# ---------------------------------------------------------------------------------------------------------------------
# the filter over the float64 oracle's step (CPU): what the GPU tests' inputs are checked on before a device sees them
# ---------------------------------------------------------------------------------------------------------------------
def oracle_filter(task, actions, z, H, r, Q, x0, P0, status0, setting=SETTINGS[0], substeps=1):
    """K steps of the restated filter with every point propagated by the float64 oracle (branch_fd.run_rollout from the
    explicit start (point, status of the mean)).  actions [K,N,A], z [K,N,M], x0 [12,N], P0 [N,12,12], status0 [N].
    Returns dict of x [K,N,12], P (last), nis [K,N], status [K,N], spread [K,N], point_status [K,N,25], ok [N]."""
    from branch_fd import run_rollout
    from oracle.refcpu import LANDED
    w = weights(*setting)
    K, n = actions.shape[:2]
    x, P, st = np.asarray(x0, np.float64).T.copy(), np.asarray(P0, np.float64).copy(), np.asarray(status0).copy()
    out = dict(x=[], nis=[], status=[], spread=[], point_status=[])
    ok = np.ones(n, bool)
    for k in range(K):
        landed = st == LANDED
        pts, okf, _ = points(x, P, w[0])
        ok &= okf | landed
        flat = pts.reshape(n * NP, 12)
        tape, _ = run_rollout(task, flat.T, np.repeat(st, NP), np.repeat(actions[k].astype(np.float64), NP, axis=0)[None],
                              substeps=substeps)
        y = tape["x"][0].reshape(n, NP, 12)
        ps = tape["status"][0].reshape(n, NP).astype(np.uint8)
        ps = np.where(landed[:, None], np.uint8(LANDED), ps)
        step = one_step(y, landed, x, P, w, Q, H, r, z[k])
        ok &= step["ok"]
        x, P, st = step["x"], step["P"], ps[:, 0].copy()
        out["x"].append(x)
        out["nis"].append(step["nis"])
        out["status"].append(st)
        out["spread"].append(np.where(landed, 0, (ps != ps[:, :1]).sum(axis=1)))
        out["point_status"].append(ps)
    res = {k: np.array(v) for k, v in out.items()}
    res.update(P=P, ok=ok)
    return res
