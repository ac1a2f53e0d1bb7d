"""A plain NumPy restatement of one backward step of the Rauch-Tung-Striebel smoother of cs_rollout_rts
(include/copterstep.h), batched over envs, in float64 or numpy.longdouble: the prediction P- = A P_f A^T + Q from a given
step Jacobian, then the arithmetic of gym_copter_amd/csrc/rts_solve.h in its order -- the Cholesky factor with
reciprocal pivots, the two substitutions per column of G = P-^-1 W, the smoothed mean and covariance -- with explicit
loops, so that tests/host/rts_solve_host gives the same bits in float64.  The GPU tests hold the kernel to it one step at
a time on the kernel's own next row; tests/test_rollout_rts_cpu.py checks it against the textbook form and the
conditional Gaussian of a linear system's joint density.  Also the bar of those comparisons."""
import numpy as np

import ekf_ref

FLOOR = ekf_ref.FLOOR
EPS = np.finfo(np.float64).eps
COND_MAX = 1e8


def factor(Pm, dtype=np.float64):
    """P- [N,12,12] (upper triangle read) = U^T U: returns (U [N,12,12] strictly upper, inv [N,12] = 1 / sqrt(pivot),
    ok [N]: every pivot > 0 and finite); carried through regardless"""
    P = np.array(Pm).astype(dtype)
    n = P.shape[0]
    U, inv, ok = np.zeros_like(P), np.zeros((n, 12), dtype), np.ones(n, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for j in range(12):
            for i in range(j):
                s = P[:, i, j].copy()
                for k in range(i):
                    s = s - U[:, k, i] * U[:, k, j]
                U[:, i, j] = s * inv[:, i]
            d = P[:, j, j].copy()
            for k in range(j):
                d = d - U[:, k, j] * U[:, k, j]
            ok &= (d > 0) & np.isfinite(d.astype(np.float64))
            inv[:, j] = dtype(1) / np.sqrt(d)
    return U, inv, ok


def solve(U, inv, W):
    """G = P-^-1 W [N,12,12]: per column a forward substitution with U^T, then a backward one with U"""
    with np.errstate(invalid="ignore", over="ignore"):
        Y = np.zeros_like(W)
        for i in range(12):
            s = W[:, i, :].copy()
            for k in range(i):
                s = s - U[:, k, i, None] * Y[:, k, :]
            Y[:, i, :] = s * inv[:, i, None]
        G = np.zeros_like(W)
        for i in range(11, -1, -1):
            s = Y[:, i, :].copy()
            for k in range(i + 1, 12):
                s = s - U[:, i, k, None] * G[:, k, :]
            G[:, i, :] = s * inv[:, i, None]
    return G


def smooth_mean(G, xf, dx):
    """x_f + G^T dx, the sum over rows of G in order from its first term"""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = G[:, 0, :] * dx[:, 0, None]
        for r in range(1, 12):
            acc = acc + G[:, r, :] * dx[:, r, None]
        return xf + acc


def smooth_cov(G, D, Pf):
    """P_f + G^T D G: T = D G, then G^T T, both sums in index order from their first term; upper triangle mirrored"""
    with np.errstate(invalid="ignore", over="ignore"):
        T = D[:, :, 0, None] * G[:, None, 0, :]
        for k in range(1, 12):
            T = T + D[:, :, k, None] * G[:, None, k, :]
        acc = G[:, 0, :, None] * T[:, 0, None, :]
        for r in range(1, 12):
            acc = acc + G[:, r, :, None] * T[:, r, None, :]
        return ekf_ref.mirror_upper(Pf + acc)


def algebra(Pm, W, D, Pf, xf, dx, dtype=np.float64):
    """what tests/host/rts_solve_host computes: dict of U, inv, ok, G, x, P"""
    Pm, W, D, Pf, xf, dx = (np.array(m).astype(dtype) for m in (Pm, W, D, Pf, xf, dx))
    U, inv, ok = factor(Pm, dtype)
    G = solve(U, inv, W)
    return dict(U=U, inv=inv, ok=ok, G=G, x=smooth_mean(G, xf, dx), P=smooth_cov(G, ekf_ref.mirror_upper(D), Pf))


def one_step(A, Pf, xf, x_pred_next, xs_next, Ps_next, Q, dtype=np.float64):
    """one backward step from the filter's tapes and the smoother's next row: A [N,12,12] the step Jacobian at the
    filter's row j, Pf [N,12,12] and xf [N,12] that row, x_pred_next [N,12] the prior of row j + 1, (xs_next, Ps_next)
    the smoothed row j + 1.  Returns dict of x, P, var, ok, P_pred, G."""
    A, Pf, xf, x_pred_next, xs_next, Ps_next, Q = (np.array(m).astype(dtype) for m in
                                                   (A, Pf, xf, x_pred_next, xs_next, Ps_next, Q))
    Pf = ekf_ref.mirror_upper(Pf)
    W = np.einsum("nij,njk->nik", A, Pf)
    Pm = ekf_ref.mirror_upper(np.einsum("nij,nkj->nik", W, A) + Q)
    D = ekf_ref.mirror_upper(Ps_next) - Pm
    out = algebra(Pm, W, D, Pf, xf, xs_next - x_pred_next, dtype)
    return dict(x=out["x"], P=out["P"], var=np.diagonal(out["P"], axis1=1, axis2=2), ok=out["ok"], P_pred=Pm, G=out["G"])


def textbook_step(A, Pf, xf, x_pred_next, xs_next, Ps_next, Q):
    """the same step for one env in its textbook form, numpy.linalg.solve: C = P_f A^T P-^-1, x_f + C (x_s' - x-'),
    P_f + C (P_s' - P-) C^T; returns (x, P, cond(P-))"""
    Pm = A @ Pf @ A.T + Q
    C = np.linalg.solve(Pm, A @ Pf).T
    return xf + C @ (xs_next - x_pred_next), Pf + C @ (Ps_next - Pm) @ C.T, np.linalg.cond(Pm)


def scaled_env(got, ref):
    """per env: the largest |got - ref| / max(|ref|, 1) over its entries, [N] (NaN where both are NaN counts as 0)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)
    e = np.where(np.isnan(got) & np.isnan(ref), 0.0, e)
    return e.reshape(e.shape[0], -1).max(axis=1)


def cond(Pm):
    """kappa_2 of every env's P-, [N]"""
    w = np.linalg.eigvalsh(np.asarray(Pm, np.float64))
    return w[:, -1] / w[:, 0]


def bars(ref64, refld, keys=("x", "P", "var")):
    """per output and env [N]: 100 x the float64 reference's own distance from the longdouble one, floored at the larger
    of FLOOR (scaled) and 12 eps kappa_2(P-) of that env -- the forward bound of a backward-stable 12 x 12 solve.
    kappa_2 <= COND_MAX is asserted for every env: none is left out."""
    kappa = cond(ref64["P_pred"])
    assert np.all(np.isfinite(kappa)) and kappa.min() > 0 and kappa.max() <= COND_MAX, kappa.max()
    floor = np.maximum(FLOOR, 12 * EPS * kappa)
    return {k: np.maximum(100.0 * scaled_env(ref64[k], np.asarray(refld[k]).astype(np.float64)), floor) for k in keys}


# ---------------------------------------------------------------------------------------------------------------------
# the application (Hover3D, ekf_ref.app_inputs): what the smoothed estimates must satisfy
# ---------------------------------------------------------------------------------------------------------------------
def app_conditions(xs, var_s, x0_s, var0_s, xf, var_f, truth, x0_true, rmse0_vel):
    """the conditions of the application on a smoother's result: xs, var_s [K,N,12] the smoothed tape and its variances,
    (x0_s, var0_s) [N,12] the smoothed starting point, xf, var_f [K,N,12] the filter's, truth [K,N,12], x0_true [N,12];
    returns the figures (asserts inside)"""
    K = xs.shape[0]
    measured = list(ekf_ref.APP_SLOTS)
    hidden = [s for s in range(12) if s not in measured]
    rm_s = np.sqrt(np.mean((xs[1:] - truth[1:]) ** 2, axis=(0, 1)))
    rm_f = np.sqrt(np.mean((xf[1:] - truth[1:]) ** 2, axis=(0, 1)))
    gain = rm_s / rm_f
    assert np.all(gain[measured] <= 0.6), gain[measured]
    assert np.all(gain[hidden] <= 0.3), gain[hidden]
    rm0 = np.sqrt(np.mean((x0_s - x0_true) ** 2, axis=0))
    assert np.all(rm0[[0, 2, 4]] < 0.04), rm0[[0, 2, 4]]
    assert np.all(rm0[[1, 3, 5]] < 0.15 * rmse0_vel), (rm0[[1, 3, 5]], rmse0_vel)
    # rows -1 .. K-2: the starting point and every row but the last, which is the filter's
    err = np.concatenate([(x0_s - x0_true)[None], xs[:K - 1] - truth[:K - 1]])
    var = np.concatenate([var0_s[None], var_s[:K - 1]])
    ratio = np.sqrt(np.mean(err ** 2, axis=(0, 1))) / np.sqrt(np.mean(var, axis=(0, 1)))
    assert np.all((ratio >= 0.8) & (ratio <= 1.25)), ratio
    assert np.all(var_s <= var_f * (1 + 1e-9)), float(np.max(var_s / var_f))
    return dict(measured=float(gain[measured].max()), hidden=float(gain[hidden].max()), pos0=float(rm0[[0, 2, 4]].max()),
                vel0=float((rm0[[1, 3, 5]] / rmse0_vel).max()), ratio=(float(ratio.min()), float(ratio.max())))
