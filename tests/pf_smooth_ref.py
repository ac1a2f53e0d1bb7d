"""A plain NumPy restatement of the backward-simulation particle smoother of cs_pf_smooth (include/copterstep.h), written
from the contract in the header: the inverse of the noise factor, the whitening and log beta in float64 in the stated
order (or numpy.longdouble), the integer weights (pf_ref.quantise), the draw in exact integer arithmetic (uint64 with
the fit asserted), the estimates, and a chained smoother over any step function for the CPU checks.  The GPU tests hold
the kernel to it one row at a time on the kernel's own tapes.  The Philox words are pf_ref's."""
import numpy as np

import pf_ref

DRAW_SLOT = 13
DRAW_BITS = 24


# ---------------------------------------------------------------------------------------------------------------------
# the inputs the host side makes
# ---------------------------------------------------------------------------------------------------------------------
def noise_inverse(Q):
    """Linv = Lq^-1 by forward substitution, one column at a time, sums in ascending order (what
    gym_copter_amd.pf.noise_inverse uploads)"""
    L = pf_ref.factor_q(Q)
    X = np.zeros((12, 12))
    for c in range(12):
        X[c, c] = 1.0 / L[c, c]
        for r in range(c + 1, 12):
            acc = 0.0
            for j in range(c, r):
                acc = acc + L[r, j] * X[j, c]
            X[r, c] = -acc / L[r, r]
    return X


def whiten(Linv, X, dtype=np.float64):
    """Linv x in the kernel's order: row r = sum_{j <= r} Linv[r][j] x_j, j ascending, the first term starting the sum.
    X [...,12] -> [...,12]"""
    Linv, X = np.asarray(Linv).astype(dtype), np.asarray(X).astype(dtype)
    out = np.empty(X.shape, dtype)
    for r in range(12):
        acc = Linv[r, 0] * X[..., 0]
        for j in range(1, r + 1):
            acc = acc + Linv[r, j] * X[..., j]
        out[..., r] = acc
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one backward step
# ---------------------------------------------------------------------------------------------------------------------
def log_beta(lw, Y, sigma, Yt, st, dtype=np.float64):
    """lw [N,P], Y [N,P,12] = Linv mu, sigma [N,P] (the statuses after the step), Yt [N,S,12] = Linv x~, st [N,S].
    Returns logb [N,S,P]: lw + (-0.5 d2) where sigma == st, else -inf; non-finite values count as -inf."""
    lw, Y, Yt = (np.asarray(v).astype(dtype) for v in (lw, Y, Yt))
    with np.errstate(invalid="ignore", over="ignore"):
        t = Yt[:, :, None, 0] - Y[:, None, :, 0]
        d2 = t * t
        for j in range(1, 12):
            t = Yt[:, :, None, j] - Y[:, None, :, j]
            d2 = d2 + t * t
        v = lw[:, None, :] + (dtype(-0.5) * d2)
        v = np.where(np.asarray(sigma)[:, None, :] == np.asarray(st)[:, :, None], v, -np.inf)
        return np.where(np.isfinite(v.astype(np.float64)), v, -np.inf)


def weights(logb):
    """(e [..,P] = exp(logb - max), or 1 everywhere on a row whose maximum is -inf; dead [..])"""
    logb = np.asarray(logb)
    mx = logb.max(axis=-1)
    dead = ~np.isfinite(mx.astype(np.float64))
    with np.errstate(invalid="ignore"):
        e = np.exp(logb - np.where(dead, 0, mx)[..., None])
    return np.where(dead[..., None], 1.0, e), dead


quantise = pf_ref.quantise


def draw_u(seed, g, nonce, kg, m):
    """u of (global env id, nonce, global row kg, path m): the top 24 bits of the first word of slot 13; broadcasts"""
    return pf_ref.words(seed, g, nonce, kg, m, DRAW_SLOT)[0] >> (32 - DRAW_BITS)


def draw_index(w, u):
    """the smallest p with (C[p] << 24) > u S1, C the inclusive cumulative sum of the integer weights w [..,P], S1 =
    C[P-1], u [..]; P - 1 if none passes.  Exact: uint64, the fit asserted."""
    w = np.asarray(w)
    assert w.min() >= 0 and w.max() <= pf_ref.WQ_ONE
    C = np.cumsum(w.astype(np.uint64), axis=-1, dtype=np.uint64)
    S1 = C[..., -1]
    u = np.asarray(u).astype(np.uint64)
    assert int(S1.max()) << DRAW_BITS < 1 << 64 and int(u.max()) < 1 << DRAW_BITS
    hit = (C << np.uint64(DRAW_BITS)) > (u * S1)[..., None]
    return np.where(hit.any(axis=-1), hit.argmax(axis=-1), w.shape[-1] - 1)


def estimate(X, idx, dtype=np.float64):
    """the mean [N,12] and the variance about it [N,12] of the drawn particles X [N,P,12][idx [N,S]], equal weights"""
    Xd = np.take_along_axis(np.asarray(X).astype(dtype), np.asarray(idx)[:, :, None], axis=1)
    S = dtype(Xd.shape[1])
    mean = Xd.sum(axis=1) / S
    d = Xd - mean[:, None, :]
    return mean, (d * d).sum(axis=1) / S


def backward_step(seed, g, nonce, kg, lw, mu, sigma, Xt, st, Linv):
    """one row: lw [N,P], (mu [N,P,12], sigma [N,P]) the propagated particles, (Xt [N,S,12], st [N,S]) the paths' next
    points.  Returns (idx [N,S], logb [N,S,P], bwq [N,S,P], dead [N,S])."""
    S = Xt.shape[1]
    logb = log_beta(lw, whiten(Linv, mu), sigma, whiten(Linv, Xt), st)
    e, dead = weights(logb)
    bwq = quantise(e)
    u = draw_u(seed, np.asarray(g, np.int64)[:, None], nonce, kg, np.arange(S)[None, :])
    return draw_index(bwq, u), logb, bwq, dead


# ---------------------------------------------------------------------------------------------------------------------
# the chained smoother over any step function (CPU checks)
# ---------------------------------------------------------------------------------------------------------------------
def run(step, seed, g, nonce, part, pstatus, lw, wq, Linv, S, first_step=1, end_idx=None, start=None, keep_tapes=False):
    """K backward steps over the tapes part [K,N,P,12], pstatus [K,N,P], lw [K,N,P], wq [K,N,P]; step(k, X, status) ->
    (mu, sigma) is the physics of the step that leads to row k (no noise).  start: (part, pstatus, lw) of the row before
    row 0.  Returns dict of idx [K,N,S], idx0 (or None), ok [N], x, var [K,N,12] and, with keep_tapes, logb and bwq
    [K,N,S,P] (row K-1: lw and wq of that row when drawn, else zeros)."""
    K, n, P = lw.shape
    g = np.asarray(g, np.int64)
    idx = np.zeros((K, n, S), np.int64)
    ok = np.ones(n, bool)
    logbs = np.zeros((K, n, S, P)) if keep_tapes else None
    bwqs = np.zeros((K, n, S, P), np.int64) if keep_tapes else None
    if end_idx is not None:
        idx[K - 1] = np.asarray(end_idx) % P
    else:
        u = draw_u(seed, g[:, None], nonce, first_step + K - 1, np.arange(S)[None, :])
        idx[K - 1] = draw_index(np.repeat(np.asarray(wq[K - 1])[:, None, :], S, axis=1), u)
        if keep_tapes:
            logbs[K - 1] = np.asarray(lw[K - 1])[:, None, :]
            bwqs[K - 1] = np.asarray(wq[K - 1])[:, None, :]
    idx0 = None
    for k in range(K - 2, -2 if start is not None else -1, -1):
        Xk, sk, lwk = (part[k], pstatus[k], lw[k]) if k >= 0 else start
        mu, sigma = step(k + 1, Xk, sk)
        Xt = np.take_along_axis(part[k + 1], idx[k + 1][:, :, None], axis=1)
        st = np.take_along_axis(pstatus[k + 1], idx[k + 1], axis=1)
        b, logb, bwq, dead = backward_step(seed, g, nonce, first_step + k, lwk, mu, sigma, Xt, st, Linv)
        ok &= ~dead.any(axis=1)
        if k >= 0:
            idx[k] = b
            if keep_tapes:
                logbs[k], bwqs[k] = logb, bwq
        else:
            idx0 = b
    est = [estimate(part[k], idx[k]) for k in range(K)]
    return dict(idx=idx, idx0=idx0, ok=ok, x=np.array([e[0] for e in est]), var=np.array([e[1] for e in est]),
                logb=logbs, bwq=bwqs)


def filter_tapes(step, seed, g, nonce, X, status, lw, z, H, r, Lq, ess_frac=0.5, first_step=1):
    """pf_ref.run's loop with the tapes cs_rollout_pf writes kept: dict of x [K,N,12] (the filtered means) and part_tape,
    pstatus_tape, lw_tape, wq_tape"""
    n, P = lw.shape
    g = np.asarray(g, np.int64)
    out = {k: [] for k in ("x", "part_tape", "pstatus_tape", "lw_tape", "wq_tape")}
    for k in range(np.asarray(z).shape[0]):
        kg = first_step + k
        X, status = step(k, X, status)
        X = X + pf_ref.colour(Lq, pf_ref.eps_block(seed, g, nonce, kg, P))
        w = pf_ref.weight_step(lw, X, H, r, z[k])
        lw = w["lw"]
        wq = pf_ref.quantise(w["e"])
        it = pf_ref.integer_step(wq, pf_ref.resample_u(seed, g, nonce, kg), ess_frac)
        for key, v in (("x", pf_ref.estimate(X, wq)[0]), ("part_tape", X), ("pstatus_tape", status), ("lw_tape", lw),
                       ("wq_tape", wq)):
            out[key].append(v)
        X = np.take_along_axis(X, it["anc"][:, :, None], axis=1)
        status = np.take_along_axis(status, it["anc"], axis=1)
        lw = np.where(it["resampled"][:, None], pf_ref.neg_ln(P), lw)
    return {k: np.array(v) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# the application (pf_ref's Hover3D problem, smoothed with S = 256 paths)
# ---------------------------------------------------------------------------------------------------------------------
APP_S, APP_SMOOTH_NONCE = 256, 0
APP_VEL_SLOTS = (1, 3, 5)          # the unmeasured velocities dX, dY, dZ (the sensors see positions and angles)
APP_INTERIOR = slice(1, -1)        # rows 1 .. K-2: the last row is the filter's own, the first has the least to gain
# smoothed RMSE / filtered RMSE of the velocity slots over the interior rows on the CPU oracle
# (tests/test_pf_smooth_cpu.py::test_application_improves_the_velocities_on_the_oracle); the device may be worse by 25 %
APP_CPU_RATIO = 0.905


def app_ratio(x_s, x_f, truth, slots=APP_VEL_SLOTS):
    """(smoothed RMSE, filtered RMSE) of `slots` over the interior rows, each pooled over rows, envs and slots"""
    sl = list(slots)
    es = (np.asarray(x_s)[APP_INTERIOR] - np.asarray(truth)[APP_INTERIOR])[..., sl]
    ef = (np.asarray(x_f)[APP_INTERIOR] - np.asarray(truth)[APP_INTERIOR])[..., sl]
    return float(np.sqrt(np.mean(es ** 2))), float(np.sqrt(np.mean(ef ** 2)))
