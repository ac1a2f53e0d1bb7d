"""NumPy restatement of the MPPI entry points (include/copterstep.h: cs_rollout_mppi_costs / cs_rollout_mppi_update):
the noise draw, the sample actions, the cost of a rolled-out sample and the weighted update.  Written from the contract
in the header; the Philox round function and the seed mix are the oracle's."""
import numpy as np

from oracle.refvec import philox2x32_10, splitmix64

NOISE_SCALE = np.float32(np.float32(np.sqrt(3.0)) * np.float32(2.0 ** -16))     # fl32(sqrt(3) 2^-16)
assert float(NOISE_SCALE) == float.fromhex("0x1.bb67aep-16")


def noise_key(seed):
    """lo32(splitmix64(splitmix64(seed)))."""
    return np.uint32(splitmix64(splitmix64(int(seed) & ((1 << 64) - 1))) & 0xFFFFFFFF)


def noise(seed, env_id, stream, k, p, j):
    """eps of (global env id, nonce, step k >= 1, sample p, component j), float32; the arguments broadcast."""
    env_id, stream, k, p, j = (np.asarray(v, dtype=np.int64) for v in (env_id, stream, k, p, j))
    key = (int(noise_key(seed)) + (((k - 1) << 16) + p) * 4 + j) & 0xFFFFFFFF
    env_id, stream, key = np.broadcast_arrays(env_id & 0xFFFFFFFF, stream & 0xFFFFFFFF, key)
    r0, r1 = philox2x32_10(env_id.astype(np.uint32), stream.astype(np.uint32), key.astype(np.uint32))
    r0, r1 = r0.astype(np.int64), r1.astype(np.int64)
    t = (r0 >> 16) + (r0 & 0xFFFF) + (r1 >> 16) + (r1 & 0xFFFF) - 131070
    return t.astype(np.float32) * NOISE_SCALE


def perturbation(sigma, seed, env_ids, stream, K, p, A):
    """sigma[j] * eps(p, k, j) as float32 [K,N,A]: the float32 product both kernels form (zero for sample 0)."""
    env_ids = np.asarray(env_ids, dtype=np.int64)
    sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float32), (A,))
    if p == 0:
        return np.zeros((K, env_ids.shape[0], A), np.float32)
    eps = noise(seed, env_ids[None, :, None], stream, np.arange(1, K + 1)[:, None, None], p, np.arange(A)[None, None, :])
    return (sigma[None, None, :] * eps).astype(np.float32)


def sample_actions(abar, sigma, seed, env_ids, stream, p):
    """a(p) [K,N,A] float32 = abar + sigma eps, one float32 multiply and one add; sample 0 is abar itself."""
    abar = np.asarray(abar, dtype=np.float32)
    if p == 0:
        return abar.copy()
    K, _, A = abar.shape
    return (abar + perturbation(sigma, seed, env_ids, stream, K, p, A)).astype(np.float32)


def cost_terms(x, reward, a, x_ref, Q, R, Q_final=None, a_ref=None, reward_weight=0.0, dtype=np.float64):
    """The 3 K terms of S per env, [3K, N] in `dtype`: state, action and reward term of every step."""
    x, reward, Q, R = (np.asarray(v, dtype=dtype) for v in (x, reward, Q, R))
    a = np.asarray(a, dtype=np.float32).astype(dtype)
    K = x.shape[0]
    dx = x - np.asarray(x_ref, dtype=dtype)
    da = a - (0 if a_ref is None else np.asarray(a_ref, dtype=dtype))
    Qk = np.broadcast_to(Q, (K, 12, 12)).copy()
    if Q_final is not None:
        Qk[-1] = np.asarray(Q_final, dtype=dtype)
    half = dtype(0.5)
    lx = half * np.einsum("kni,kij,knj->kn", dx, Qk, dx)
    la = half * np.einsum("kni,ij,knj->kn", da, R, da)
    return np.concatenate([lx, la, -dtype(reward_weight) * reward])


def cost_magnitude(x, reward, a, x_ref, Q, R, Q_final=None, a_ref=None, reward_weight=0.0):
    """(T, M [N]): the number of elementary products S is a sum of -- K (144 + A^2 + 1) -- and the sum of their absolute
    values per env: any order of summation in float64 is within (T - 1) 2^-53 M of the exact sum, to first order."""
    x, reward, Q, R = (np.asarray(v, dtype=np.float64) for v in (x, reward, Q, R))
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    K, _, A = a.shape
    dx = np.abs(x - np.asarray(x_ref, dtype=np.float64))
    da = np.abs(a - (0 if a_ref is None else np.asarray(a_ref, dtype=np.float64)))
    Qk = np.broadcast_to(np.abs(Q), (K, 12, 12)).copy()
    if Q_final is not None:
        Qk[-1] = np.abs(np.asarray(Q_final, dtype=np.float64))
    m = 0.5 * np.einsum("kni,kij,knj->n", dx, Qk, dx) + 0.5 * np.einsum("kni,ij,knj->n", da, np.abs(R), da)
    return K * (144 + A * A + 1), m + np.abs(reward_weight * reward).sum(0)


def cost(*args, **kwargs):
    """S [N] of a rolled-out sample (cost_terms summed)."""
    return cost_terms(*args, **kwargs).sum(0)


def weights(costs, lam, dtype=np.float64):
    """(w [P,N], beta [N], any [N]): w_p = exp(-(S_p - beta) / lam) for finite S_p, else 0; beta = the minimum finite
    cost (inf where none)."""
    costs = np.asarray(costs, dtype=dtype)
    fin = np.isfinite(costs)
    beta = np.where(fin, costs, np.inf).min(0)
    any_ = fin.any(0)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(fin, np.exp(-(np.where(fin, costs, 0) - np.where(any_, beta, 0)) / dtype(lam)), 0).astype(dtype)
    return w, beta, any_


def update(abar, costs, sigma, lam, seed, env_ids, stream, dtype=np.float64):
    """(actions_out [K,N,A] float32, ess [N], cost_min [N]) of cs_rollout_mppi_update; sums over p ascending in `dtype`
    (np.longdouble: the brute-force evaluation the float64 one is tested against)."""
    abar = np.asarray(abar, dtype=np.float32)
    K, N, A = abar.shape
    P = np.asarray(costs).shape[0]
    w, beta, any_ = weights(costs, lam, dtype)
    eta, eta2 = np.zeros(N, dtype), np.zeros(N, dtype)
    acc = np.zeros((K, N, A), dtype)
    for p in range(P):
        eta = eta + w[p]
        eta2 = eta2 + w[p] * w[p]
        if p:
            acc = acc + w[p][None, :, None] * perturbation(sigma, seed, env_ids, stream, K, p, A).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        new = (abar.astype(dtype) + (dtype(1) / eta)[None, :, None] * acc).astype(np.float32)
        ess = np.where(any_, eta * eta / eta2, 0)
    out = np.where(any_[None, :, None], np.clip(new, np.float32(0), np.float32(1)), abar).astype(np.float32)
    return out, ess, np.where(any_, beta, np.inf)


def best(costs):
    """The arg-min over each env's finite costs, the lowest index on ties, -1 if none is finite."""
    costs = np.asarray(costs, dtype=np.float64)
    fin = np.isfinite(costs)
    return np.where(fin.any(0), np.where(fin, costs, np.inf).argmin(0), -1).astype(np.int32)
