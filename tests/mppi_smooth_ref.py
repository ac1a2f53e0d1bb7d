"""NumPy restatement of the smooth MPPI entry points (include/copterstep.h: cs_rollout_mppi_costs_ex /
cs_rollout_mppi_update_ex / cs_rollout_mppi_temperature): the knot table, the blended noise, the sample actions, the
update with a temperature per env and the bisection of that temperature.  Written from the contract in the header; the
draw, the weights and the white update are tests/mppi_ref.py's."""
import numpy as np

import mppi_ref

BISECTIONS = 48


def knots(K, hold):
    """(knot [K] int64, w [K,2] float32): knot[k] = (k - 1) // hold + 1, t = ((k - 1) % hold) / hold,
    w = fl32((1 - t, t) / sqrt((1 - t)^2 + t^2)), computed in float64 and rounded once."""
    k0 = np.arange(K, dtype=np.int64)
    t = (k0 % hold) / np.float64(hold)
    norm = np.sqrt((1.0 - t) * (1.0 - t) + t * t)
    w = np.stack([(1.0 - t) / norm, t / norm], axis=1)
    return k0 // hold + 1, w.astype(np.float32)


def blend(w0, e0, w1, e1):
    """fl32(fl32(w0 e0) + fl32(w1 e1)), no fma; the second term left out altogether where w1 == 0.  Broadcasts."""
    w0, e0, w1, e1 = (np.asarray(v, dtype=np.float32) for v in (w0, e0, w1, e1))
    a = (w0 * e0).astype(np.float32)
    b = (w1 * e1).astype(np.float32)
    return np.where(w1 == 0, a, (a + b).astype(np.float32)).astype(np.float32)


def noise(seed, env_id, stream, knot, w0, w1, p, j):
    """eps~ of (global env id, nonce, the step's knot number and weights, sample p, component j), float32; the arguments
    broadcast."""
    knot = np.asarray(knot, dtype=np.int64)
    return blend(w0, mppi_ref.noise(seed, env_id, stream, knot, p, j), w1,
                 mppi_ref.noise(seed, env_id, stream, knot + 1, p, j))


def perturbation(sigma, seed, env_ids, stream, table, p, A):
    """sigma[j] * eps~(p, k, j) as float32 [K,N,A] (zero for sample 0); table = (knot [K], w [K,2])."""
    knot, w = table
    knot, w = np.asarray(knot, dtype=np.int64), np.asarray(w, dtype=np.float32)
    env_ids = np.asarray(env_ids, dtype=np.int64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (A,))
    K = knot.shape[0]
    if p == 0:
        return np.zeros((K, env_ids.shape[0], A), np.float32)
    eps = noise(seed, env_ids[None, :, None], stream, knot[:, None, None], w[:, 0][:, None, None],
                w[:, 1][:, None, None], p, np.arange(A)[None, None, :])
    return (sigma[None, None, :] * eps).astype(np.float32)


def sample_actions(abar, sigma, seed, env_ids, stream, table, p):
    """a(p) [K,N,A] float32 = abar + sigma eps~, one float32 multiply and one add; sample 0 is abar itself."""
    abar = np.asarray(abar, dtype=np.float32)
    if p == 0:
        return abar.copy()
    return (abar + perturbation(sigma, seed, env_ids, stream, table, p, abar.shape[2])).astype(np.float32)


def update(abar, costs, sigma, lam, seed, env_ids, stream, table, dtype=np.float64):
    """(actions_out [K,N,A] float32, ess [N], cost_min [N]) of cs_rollout_mppi_update_ex: mppi_ref.update with eps~ and
    lam a scalar or [N]; an env whose lam is not finite and > 0 keeps its plan and reports ess = 0 (cost_min is beta as
    ever)."""
    abar = np.asarray(abar, dtype=np.float32)
    K, N, A = abar.shape
    costs = np.asarray(costs, dtype=dtype)
    P = costs.shape[0]
    lam = np.broadcast_to(np.asarray(lam, dtype=dtype), (N,))
    warm = np.isfinite(lam) & (lam > 0)
    fin = np.isfinite(costs)
    any_ = fin.any(0)
    beta = np.where(fin, costs, np.inf).min(0)
    safe = np.where(warm, lam, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(fin, np.exp(-(np.where(fin, costs, 0) - np.where(any_, beta, 0)) / safe[None, :]), 0).astype(dtype)
    eta, eta2 = np.zeros(N, dtype), np.zeros(N, dtype)
    acc = np.zeros((K, N, A), dtype)
    for p in range(P):
        eta = eta + w[p]
        eta2 = eta2 + w[p] * w[p]
        if p:
            acc = acc + w[p][None, :, None] * perturbation(sigma, seed, env_ids, stream, table, p, A).astype(dtype)
    move = any_ & warm
    with np.errstate(invalid="ignore", divide="ignore"):
        new = (abar.astype(dtype) + (dtype(1) / eta)[None, :, None] * acc).astype(np.float32)
        ess = np.where(move, eta * eta / eta2, 0)
    out = np.where(move[None, :, None], np.clip(new, np.float32(0), np.float32(1)), abar).astype(np.float32)
    return out, ess, np.where(any_, beta, np.inf)


def ess_at(costs, lam, dtype=np.float64):
    """E(lam) [N] = (sum_p w_p)^2 / sum_p w_p^2 over the finite costs, sums over p ascending in `dtype`; lam a scalar or
    [N]; 0 for an env without a finite cost."""
    costs = np.asarray(costs, dtype=dtype)
    P, N = costs.shape
    lam = np.broadcast_to(np.asarray(lam, dtype=dtype), (N,))
    fin = np.isfinite(costs)
    any_ = fin.any(0)
    beta = np.where(any_, np.where(fin, costs, np.inf).min(0), 0)
    eta, eta2 = np.zeros(N, dtype), np.zeros(N, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            w = np.where(fin[p], np.exp(-(np.where(fin[p], costs[p], 0) - beta) / lam), 0).astype(dtype)
            eta = eta + w
            eta2 = eta2 + w * w
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(any_, eta * eta / eta2, 0)


def temperature(costs, ess_target, lam_min, lam_max):
    """(lam [N], E(lam) [N]) of cs_rollout_mppi_temperature, float64: 48 bisections of u = ln lam, u_lo = u where
    E(exp u) < target, else u_hi = u; lam = exp(u_hi); lam_max where E(lam_max) < target; lam_min where E(lam_min) >=
    target; lam_max and E = 0 for an env without a finite cost."""
    costs = np.asarray(costs, dtype=np.float64)
    N = costs.shape[1]
    target = np.float64(ess_target)
    any_ = np.isfinite(costs).any(0)
    e_hi, e_lo = ess_at(costs, lam_max), ess_at(costs, lam_min)
    lo, hi = np.full(N, np.log(np.float64(lam_min))), np.full(N, np.log(np.float64(lam_max)))
    for _ in range(BISECTIONS):
        u = 0.5 * (lo + hi)
        below = ess_at(costs, np.exp(u)) < target
        lo, hi = np.where(below, u, lo), np.where(below, hi, u)
    lam = np.exp(hi)
    at_max = ~any_ | (e_hi < target)
    at_min = ~at_max & (e_lo >= target)
    lam = np.where(at_max, np.float64(lam_max), np.where(at_min, np.float64(lam_min), lam))
    return lam, ess_at(costs, lam)
