"""A NumPy restatement of the box-constrained quadratic programme of cs_ilqr_box_backward
(gym_copter_amd/csrc/boxqp_solve.h), operation for operation: minimise 1/2 x^T H x + g^T x over l <= x <= u by
projected Newton steps on lqr_ref's Cholesky.  Batched over problems (finished problems are frozen while the others go
on); the working dtype is a parameter (float64, or numpy.longdouble for the reference's own error).  brute_force
enumerates the 3^A active sets of one problem: what the iteration is held to."""
import itertools

import numpy as np

import lqr_ref

ITERS = 16
TRIALS = 30


def clamp(v, l, u):
    """v < l ? l : (v > u ? u : v): a NaN stays a NaN"""
    return np.where(v < l, l, np.where(v > u, u, v))


def times(H, x):
    """(Hx)_a = sum_b H_ab x_b, from 0 in index order"""
    A = x.shape[-1]
    out = np.zeros_like(x)
    for a in range(A):
        acc = np.zeros_like(x[..., 0])
        for b in range(A):
            acc = acc + H[..., a, b] * x[..., b]
        out[..., a] = acc
    return out


def value(hx, g, x):
    """f(x) = sum_a x_a (0.5 (Hx)_a + g_a), from 0 in index order"""
    half = x.dtype.type(0.5)
    f = np.zeros_like(x[..., 0])
    for a in range(x.shape[-1]):
        f = f + x[..., a] * (half * hx[..., a] + g[..., a])
    return f


def _bits(mask):
    return (mask.astype(np.int64) << np.arange(mask.shape[-1])).sum(-1)


def solve(H, g, l, u, max_iters=ITERS, dtype=np.float64):
    """boxqp_solve for H [N,A,A] (full, symmetric), g, l, u [N,A]; max_iters an int or [N] (0: the clamped start only).
    Returns dict(x [N,A], fac [N,A,A] (the lower triangle of the last masked factor), lower, upper [N] (bit masks),
    clamped [N,A] bool, iters [N], ok [N], pd [N]: lqr_cholesky's verdict on H itself)."""
    H, g = np.asarray(H, dtype), np.asarray(g, dtype)
    l, u = np.asarray(l, dtype), np.asarray(u, dtype)
    N, A = g.shape
    c = lambda v: dtype(v)
    eye = np.broadcast_to(np.eye(A, dtype=dtype), (N, A, A))
    with np.errstate(all="ignore"):
        fach, pd = lqr_ref.cholesky(H)
        start = -lqr_ref.chol_solve(fach, g)
        lo = start < l
        up = ~lo & (start > u)
        x = clamp(start, l, u)
        fac = eye.copy()
        iters = np.zeros(N, np.int64)
        ok = np.ones(N, bool)
        cap = np.broadcast_to(np.asarray(max_iters), (N,))
        done = cap <= 0
        alive = ~done
        for it in range(ITERS):
            alive = alive & (it < cap)
            if not alive.any():
                break
            iters[alive] = it + 1
            hx = times(H, x)
            gr = g + hx
            nlo = (x <= l) & (gr > 0)
            nup = ~nlo & (x >= u) & (gr < 0)
            lo[alive], up[alive] = nlo[alive], nup[alive]
            cl = nlo | nup
            fac[alive] = eye[alive]
            none_free = cl.all(-1)
            done |= alive & none_free
            alive = alive & ~none_free
            free = ~cl
            M = np.where(free[:, :, None] & free[:, None, :], H, eye)
            L, pdm = lqr_ref.cholesky(M)
            fac[alive] = L[alive]
            ok[alive] &= pdm[alive]
            t = g.copy()
            for b in range(A):
                t = np.where(cl[:, b, None], t + H[:, :, b] * x[:, b, None], t)
            sol = lqr_ref.chol_solve(L, np.where(cl, c(0.0), -t))
            s = np.where(cl, c(0.0), sol - x)
            ms, mx = np.zeros(N, dtype), np.ones(N, dtype)
            for a in range(A):
                vs, vx = np.abs(s[:, a]), np.abs(x[:, a])
                ms = np.where(vs > ms, vs, ms)
                mx = np.where(vx > mx, vx, mx)
            small = ms <= c(1e-14) * mx
            done |= alive & small
            alive = alive & ~small
            gs = np.zeros(N, dtype)
            for a in range(A):
                gs = gs + gr[:, a] * s[:, a]
            f0 = value(hx, g, x)
            step = np.ones(N, dtype)
            accepted = np.zeros(N, bool)
            searching = alive.copy()
            xc = x.copy()
            for _ in range(TRIALS):
                if not searching.any():
                    break
                cand = clamp(x + step[:, None] * s, l, u)
                df = value(times(H, cand), g, cand) - f0
                good = searching & (df <= c(0.1) * step * gs)
                xc[good] = cand[good]
                accepted |= good
                searching = searching & ~good
                step = np.where(searching, c(0.6) * step, step)
            alive = alive & accepted          # (no trial accepted: the iteration could only repeat itself; not done)
            x[alive] = xc[alive]
        ok &= done
    return dict(x=x, fac=fac, lower=_bits(lo), upper=_bits(up), clamped=lo | up, iters=iters, ok=ok, pd=pd)


def gain(sol, kk):
    """boxqp_gain: the free rows of -(H_ff)^-1 kk_f by the factor solve() left, 0 on the clamped rows.  kk [N,A]."""
    cl = sol["clamped"]
    zero = sol["x"].dtype.type(0.0)
    with np.errstate(all="ignore"):
        out = lqr_ref.chol_solve(sol["fac"], np.where(cl, zero, np.asarray(kk, sol["x"].dtype)))
    return np.where(cl, zero, -out)


def brute_force(H, g, l, u):
    """One problem's minimiser by enumeration of the 3^A active sets (each control free, at l or at u): the KKT point
    of least value.  Returns (x [A], state [A] (0 free, -1 at l, +1 at u), multipliers [A]: |gradient| on the clamped
    controls, 0 on the free ones)."""
    H, g, l, u = (np.asarray(v, np.float64) for v in (H, g, l, u))
    A = g.shape[0]
    scale = max(1.0, np.abs(l[np.isfinite(l)]).max(initial=0.0), np.abs(u[np.isfinite(u)]).max(initial=0.0))
    best = None
    for state in itertools.product((0, -1, 1), repeat=A):
        st = np.array(state)
        if (np.isinf(l) & (st == -1)).any() or (np.isinf(u) & (st == 1)).any():
            continue
        x = np.where(st == -1, l, np.where(st == 1, u, 0.0))
        fr = st == 0
        if fr.any():
            x[fr] = np.linalg.solve(H[np.ix_(fr, fr)], -(g[fr] + H[np.ix_(fr, ~fr)] @ x[~fr]))
        gr = g + H @ x
        tol = 1e-11 * scale
        if (x < l - tol).any() or (x > u + tol).any():
            continue
        gtol = 1e-11 * max(1.0, np.abs(g).max())
        if (gr[st == -1] < -gtol).any() or (gr[st == 1] > gtol).any():
            continue
        f = 0.5 * x @ H @ x + g @ x
        if best is None or f < best[0]:
            best = (f, np.clip(x, l, u), st, np.where(fr, 0.0, np.abs(gr)))
    assert best is not None, "no KKT point among the active sets"
    return best[1], best[2], best[3]
