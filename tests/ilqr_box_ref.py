"""A NumPy restatement of the control-limited iLQR backward pass (cs_ilqr_box_backward) from explicit Jacobian blocks:
lqr_ref.lqr_backward with the step's A x A solve replaced by boxqp_ref's box-constrained programme, and the float32
clamp of the forward pass (cs_ilqr_box_forward).  Batched over envs; the working dtype is a parameter."""
import numpy as np

import boxqp_ref
import lqr_ref


def lqr_box_backward(Ab, Bb, Q, R, abar, lo, hi, q=None, r=None, Q_final=None, mu=0.0, dtype=np.float64,
                     resetting=None):
    """lqr_ref.lqr_backward's recursion with d_k the minimiser of 1/2 d^T (Quu + mu I) d + Qu^T d over lo - abar_k <= d
    <= hi - abar_k and the gains of boxqp_ref.gain.  abar [K,N,A] float32: the nominal actions; lo, hi [A] float32;
    resetting [N] bool (None: nobody): the lanes whose first step is a NEXT_STEP reset (no iteration there).
    Returns lqr_backward's dict plus clamped [K,N] (the device's byte), iters [K,N], and what a comparison needs to
    choose its envs: mult [K,N] = the least |Qu + H d| over the clamped controls relative to max(1, |Qu|_inf) (inf where
    none is clamped) and gap [K,N] = the least distance of a free control from its bounds relative to max(1, |l|, |u|
    finite) (inf where none is free)."""
    Ab, Bb = np.asarray(Ab, dtype), np.asarray(Bb, dtype)
    K, N, _, A = Bb.shape
    Q, R = np.asarray(Q, dtype), np.asarray(R, dtype)
    Qf = Q if Q_final is None else np.asarray(Q_final, dtype)
    q = np.zeros((K, N, 12), dtype) if q is None else np.asarray(q, dtype)
    r = np.zeros((K, N, A), dtype) if r is None else np.asarray(r, dtype)
    mu = dtype(mu)
    abar = np.asarray(abar, np.float32).astype(dtype)
    lo = np.broadcast_to(np.asarray(lo, np.float32), (A,)).astype(dtype)
    hi = np.broadcast_to(np.asarray(hi, np.float32), (A,)).astype(dtype)
    S, s = np.zeros((N, 12, 12), dtype), np.zeros((N, 12), dtype)
    Ks, ds = np.zeros((K, N, A, 12), dtype), np.zeros((K, N, A), dtype)
    clamped, iters = np.zeros((K, N), np.uint8), np.zeros((K, N), np.uint8)
    mult, gap = np.full((K, N), np.inf), np.full((K, N), np.inf)
    dV = np.zeros((N, 2), dtype)
    ok = np.ones(N, bool)
    T = lambda m: np.swapaxes(m, -1, -2)
    mv = lambda m, v: np.einsum("nij,nj->ni", m, v)
    half = dtype(0.5)
    for k in range(K - 1, -1, -1):
        Am, Bm = Ab[k], Bb[k]
        V = S + (Qf if k == K - 1 else Q)
        v = s + q[k]
        Qx, Qu = mv(T(Am), v), r[k] + mv(T(Bm), v)
        Qxx, Qux, Quu = T(Am) @ V @ Am, T(Bm) @ V @ Am, R + T(Bm) @ V @ Bm
        H = Quu + mu * np.eye(A, dtype=dtype)
        l, u = lo - abar[k], hi - abar[k]
        cap = boxqp_ref.ITERS
        if k == 0 and resetting is not None:
            cap = np.where(resetting, 0, boxqp_ref.ITERS)
        sol = boxqp_ref.solve(H, Qu, l, u, cap, dtype)
        ok &= sol["pd"] & sol["ok"]
        dk = sol["x"]
        Kk = np.stack([boxqp_ref.gain(sol, Qux[..., j]) for j in range(12)], axis=-1)
        S = Qxx + T(Kk) @ Quu @ Kk + T(Kk) @ Qux + T(Qux) @ Kk
        S = np.triu(S) + T(np.triu(S, 1))
        s = Qx + mv(T(Kk), mv(Quu, dk)) + mv(T(Kk), Qu) + mv(T(Qux), dk)
        dV[:, 0] += np.einsum("ni,ni->n", dk, Qu)
        dV[:, 1] += half * np.einsum("ni,ni->n", dk, mv(Quu, dk))
        Ks[k], ds[k] = Kk, dk
        clamped[k] = (sol["lower"] | (sol["upper"] << 4)).astype(np.uint8)
        iters[k] = sol["iters"].astype(np.uint8)
        cl = sol["clamped"]
        with np.errstate(all="ignore"):
            gr = np.abs((Qu + mv(H, dk)).astype(np.float64)) / np.maximum(1.0, np.abs(Qu).max(-1))[:, None].astype(np.float64)
            mult[k] = np.where(cl, gr, np.inf).min(-1)
            fin = lambda b: np.where(np.isfinite(b), np.abs(b), 0.0).astype(np.float64)
            scale = np.maximum(1.0, np.maximum(fin(l), fin(u)))
            dist = np.minimum(np.abs(dk - l), np.abs(u - dk)).astype(np.float64) / scale
            gap[k] = np.where(cl, np.inf, dist).min(-1)
    return dict(K=Ks, d=ds, dV=dV, S0=S, s0=s, ok=ok, clamped=clamped, iters=iters, mult=mult, gap=gap)


def clamp_actions(a, lo, hi):
    """The forward's clamp of a float32 action tape [..., A] and its flag bytes [...]: a < lo ? lo : (a > hi ? hi : a),
    bit c where the clamp raised action c, bit 4 + c where it lowered it."""
    a = np.asarray(a, np.float32)
    A = a.shape[-1]
    lo = np.broadcast_to(np.asarray(lo, np.float32), (A,))
    hi = np.broadcast_to(np.asarray(hi, np.float32), (A,))
    below, above = a < lo, ~(a < lo) & (a > hi)
    out = np.where(below, lo, np.where(above, hi, a)).astype(np.float32)
    w = 1 << np.arange(A)
    return out, ((below * w).sum(-1) + ((above * w).sum(-1) << 4)).astype(np.uint8)
