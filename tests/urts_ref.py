"""A plain NumPy restatement of one backward step of the unscented Rauch-Tung-Striebel smoother of cs_urts_smooth
(include/copterstep.h), batched over envs, in float64 or numpy.longdouble: the cross-covariance of
gym_copter_amd/csrc/urts_cross.h in its order, on ukf_ref's factor and moments and rts_ref's algebra, so that
tests/host/urts_cross_host gives the same bits in float64:

  pairs    dY[a][c] = y(1 + c)[a] - y(13 + c)[a], one subtraction
  diag     L[c][c] = 1 / inv[c];  L[c][j] = U[j][c] for j < c
  scale    s = wi * gamma
  row      acc = dY[i][0] * L[c][0];  acc += dY[i][j] * L[c][j], j = 1 .. c in order;  W[i][c] = s * acc
  landed   W = P_f mirrored, P- = P_f + Q

W[i][c] pairs component i after the step with component c before it: it stands where rts_ref's W = A P_f stands.  The GPU
tests hold the kernel to it one step at a time on the kernel's own next row and the filter's own point tape;
tests/test_urts_cpu.py checks it against the textbook sum over the 25 weighted points, against rts_ref for a linear map
and against the conditional Gaussian of a linear system's joint density.  Also the filter and the smoother restated over
the float64 oracle's step, for the conditions of the GPU tests' inputs."""
import numpy as np

import ekf_ref
import rts_ref
import ukf_ref

NP = ukf_ref.NP


def cross(y, U, w, dtype=np.float64):
    """W [N,12,12] from the propagated points y [N,25,12], ukf_ref.cholesky's U [N,12,12] (the reciprocal roots of the
    pivots on its diagonal) and w = (gamma, wm0, wc0, wi)"""
    y, U = np.asarray(y).astype(dtype), np.asarray(U).astype(dtype)
    gamma, _, _, wi = (dtype(v) for v in w)
    n = y.shape[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dY = np.swapaxes(y[:, 1:13] - y[:, 13:25], 1, 2)          # dY[n, a, c]
        diag = dtype(1) / np.diagonal(U, axis1=1, axis2=2)
        s = wi * gamma
        W = np.zeros((n, 12, 12), dtype)
        for c in range(12):
            acc = dY[:, :, 0] * (diag[:, 0] if c == 0 else U[:, 0, c])[:, None]
            for j in range(1, c + 1):
                acc = acc + dY[:, :, j] * (diag[:, c] if j == c else U[:, j, c])[:, None]
            W[:, :, c] = s * acc
    return W


def textbook_cross(pts, y, w):
    """the textbook form in longdouble: W = C^T with C = sum_i wc_i (chi_i - xhat)(y_i - x-)^T, xhat = point 0 and
    x- = sum_i wm_i y_i; pts, y [N,25,12]"""
    pts, y = np.asarray(pts).astype(np.longdouble), np.asarray(y).astype(np.longdouble)
    _, wm0, wc0, wi = (np.longdouble(v) for v in w)
    wm = np.full(NP, wi)
    wc = wm.copy()
    wm[0], wc[0] = wm0, wc0
    xm = np.einsum("i,nij->nj", wm, y)
    C = np.einsum("i,nia,nib->nab", wc, pts - pts[:, :1], y - xm[:, None])
    return np.swapaxes(C, 1, 2)


def one_step(y, landed, Pf, xf, x_pred_next, xs_next, Ps_next, w, Q, dtype=np.float64):
    """one backward step from the filter's tapes and the smoother's next row: y [N,25,12] the propagated points of the
    filter's step j + 2 (ignored for the lanes of `landed` [N] bool), Pf [N,12,12] and xf [N,12] the filter's row j,
    x_pred_next [N,12] the prior of row j + 1, (xs_next, Ps_next) the smoothed row j + 1, w = (gamma, wm0, wc0, wi).
    Returns dict of x, P, var, ok (both factorisations), ok_factor, P_pred, W, G."""
    Pf, xf, x_pred_next, xs_next, Ps_next, Q = (np.array(m).astype(dtype) for m in
                                                (Pf, xf, x_pred_next, xs_next, Ps_next, Q))
    w = tuple(dtype(v) for v in w)
    landed = np.asarray(landed, bool)
    Pf = ekf_ref.mirror_upper(Pf)
    U, okf = ukf_ref.cholesky(Pf, dtype)
    _, Pm = ukf_ref.moments(y, w, Q, dtype)
    W = cross(y, U, w, dtype)
    W = np.where(landed[:, None, None], Pf, W)
    Pm = np.where(landed[:, None, None], ekf_ref.mirror_upper(Pf + Q), Pm)
    D = ekf_ref.mirror_upper(Ps_next) - Pm
    out = rts_ref.algebra(Pm, W, D, Pf, xf, xs_next - x_pred_next, dtype)
    okf = okf | landed
    return dict(x=out["x"], P=out["P"], var=np.diagonal(out["P"], axis1=1, axis2=2), ok=out["ok"] & okf, ok_factor=okf,
                ok_solve=out["ok"], P_pred=Pm, W=W, G=out["G"])


def bars(ref64, refld, keys=("x", "P", "var")):
    """rts_ref's bar: per output and env, 100 x the float64 reference's distance from the longdouble one, floored at the
    larger of 1e-12 scaled and 12 eps kappa_2(P-); kappa_2 <= 1e8 is asserted for every env"""
    return rts_ref.bars(ref64, refld, keys)


def smoother(tapes, x0, P0, st0, w, Q, landed_code, dtype=np.float64):
    """the whole backward recursion over a filter's tapes (dict of x, x_pred, P_tape, status [K,...] and y [K,N,25,12],
    the propagated points) from the start (x0 [N,12], P0, st0): dict of x [K,N,12], P [K,N,12,12], x0, P0, ok, and per
    backward step j = K-2 .. -1 the lists P_pred and steps (one_step's results)"""
    K = tapes["x"].shape[0]
    xs, Ps = [tapes["x"][-1].astype(dtype)], [ekf_ref.mirror_upper(tapes["P_tape"][-1].astype(dtype))]
    ok = np.ones(tapes["x"].shape[1], bool)
    steps = []
    for j in range(K - 2, -2, -1):
        xf, Pf, st = (tapes["x"][j], tapes["P_tape"][j], tapes["status"][j]) if j >= 0 else (x0, P0, st0)
        r = one_step(tapes["y"][j + 1], np.asarray(st) == landed_code, Pf, xf, tapes["x_pred"][j + 1], xs[0], Ps[0], w, Q,
                     dtype)
        ok &= r["ok"]
        steps.append(r)
        xs.insert(0, r["x"])
        Ps.insert(0, r["P"])
    return dict(x=np.array(xs[1:]), P=np.array(Ps[1:]), x0=xs[0], P0=Ps[0], ok=ok, steps=steps)


# ---------------------------------------------------------------------------------------------------------------------
# the filter over the float64 oracle's step with the tapes the smoother reads (CPU): what the GPU tests' inputs are
# checked on before a device sees them
# ---------------------------------------------------------------------------------------------------------------------
def oracle_filter_tapes(task, actions, z, H, r, Q, x0, P0, status0, setting=ukf_ref.SETTINGS[0], substeps=1):
    """ukf_ref.oracle_filter keeping what the smoother reads: dict of x, x_pred [K,N,12], P_tape [K,N,12,12], var, status,
    spread [K,N], y [K,N,25,12] (the propagated points; the mean 25 times on a LANDED step), ok [N]"""
    from branch_fd import run_rollout
    from oracle.refcpu import LANDED
    w = ukf_ref.weights(*setting)
    K, n = actions.shape[:2]
    x, P, st = np.asarray(x0, np.float64).T.copy(), np.asarray(P0, np.float64).copy(), np.asarray(status0).copy()
    out = dict(x=[], x_pred=[], P_tape=[], var=[], status=[], spread=[], y=[])
    ok = np.ones(n, bool)
    for k in range(K):
        landed = st == LANDED
        pts, okf, _ = ukf_ref.points(x, P, w[0])
        ok &= okf | landed
        flat = pts.reshape(n * NP, 12)
        tape, _ = run_rollout(task, flat.T, np.repeat(st, NP), np.repeat(actions[k].astype(np.float64), NP, axis=0)[None],
                              substeps=substeps)
        y = tape["x"][0].reshape(n, NP, 12)
        y = np.where(landed[:, None, None], x[:, None, :], y)
        ps = tape["status"][0].reshape(n, NP).astype(np.uint8)
        ps = np.where(landed[:, None], np.uint8(LANDED), ps)
        step = ukf_ref.one_step(y, landed, x, P, w, Q, H, r, z[k])
        ok &= step["ok"]
        x, P, st = step["x"], step["P"], ps[:, 0].copy()
        for key, v in (("x", x), ("x_pred", step["x_pred"]), ("P_tape", P), ("var", step["var"]), ("status", st),
                       ("spread", np.where(landed, 0, (ps != ps[:, :1]).sum(axis=1))), ("y", y)):
            out[key].append(v)
    res = {k: np.array(v) for k, v in out.items()}
    res["ok"] = ok
    return res
