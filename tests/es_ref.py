"""NumPy restatement of the population and evolution-strategies entry points (include/copterstep.h:
cs_rollout_mlp_population / cs_es_perturb / cs_es_gradient): the noise draw, the mirrored table, the search gradient,
and a population's returns, lengths, flags and status built from the tapes of rollout_mlp_states.  Written from the
contract in the header; the Philox round function and the seed mix are the oracle's, the Irwin-Hall scale mppi_ref's."""
import numpy as np

from mppi_ref import NOISE_SCALE
from oracle.refvec import philox2x32_10, splitmix64

PAIR_CHUNK = 32                                                # CS_ES_PAIR_CHUNK


def noise_key(seed):
    """lo32(splitmix64(splitmix64(splitmix64(seed))))."""
    return np.uint32(splitmix64(splitmix64(splitmix64(int(seed) & ((1 << 64) - 1)))) & 0xFFFFFFFF)


def noise(seed, pair, stream, p):
    """eps of (global pair index, nonce, parameter index p), float32; the arguments broadcast."""
    pair, stream, p = (np.asarray(v, dtype=np.int64) for v in (pair, stream, p))
    key = (int(noise_key(seed)) + p) & 0xFFFFFFFF
    pair, stream, key = np.broadcast_arrays(pair & 0xFFFFFFFF, stream & 0xFFFFFFFF, key)
    r0, r1 = philox2x32_10(pair.astype(np.uint32), stream.astype(np.uint32), key.astype(np.uint32))
    r0, r1 = r0.astype(np.int64), r1.astype(np.int64)
    t = (r0 >> 16) + (r0 & 0xFFFF) + (r1 >> 16) + (r1 & 0xFFFF) - 131070
    return t.astype(np.float32) * NOISE_SCALE


def pair_noise(seed, stream, pairs, P, pair_base=0):
    """eps [pairs, P] float32 of the pairs pair_base .. pair_base + pairs - 1."""
    return noise(seed, (pair_base + np.arange(pairs))[:, None], stream, np.arange(P)[None, :])


def perturb(theta, sigma, members, seed, stream, pair_base=0):
    """table [M,P] float32: rows 2i / 2i+1 = theta +- sigma eps_i, one float32 multiply and one add each."""
    theta = np.asarray(theta, dtype=np.float32)
    d = (np.float32(sigma) * pair_noise(seed, stream, members // 2, theta.shape[0], pair_base)).astype(np.float32)
    table = np.empty((members, theta.shape[0]), np.float32)
    table[0::2] = theta[None, :] + d
    table[1::2] = theta[None, :] - d
    return table


def gradient(weights, P, seed, stream, pair_base=0, dtype=np.float64):
    """(g [P], magnitude [P]): g[p] = sum_i (w[2i] - w[2i+1]) eps_i[p] in `dtype`, in the kernel's order for float64
    (chunks of PAIR_CHUNK pairs, i ascending inside, then the chunks in order), and the sum of the terms' absolute
    values: any order of summation in float64 is within (terms - 1) 2^-53 x magnitude of the exact sum."""
    w = np.asarray(weights, dtype=dtype)
    pairs = w.shape[0] // 2
    eps = pair_noise(seed, stream, pairs, P, pair_base).astype(dtype)
    terms = (w[0::2] - w[1::2])[:, None] * eps
    g = np.zeros(P, dtype)
    for c0 in range(0, pairs, PAIR_CHUNK):
        part = np.zeros(P, dtype)
        for i in range(c0, min(c0 + PAIR_CHUNK, pairs)):
            part = part + terms[i]
        g = g + part
    return g, np.abs(terms).sum(0).astype(np.float64)


def returns_from_tapes(reward, terminated, truncated, status, gamma):
    """(returns [N] float64, lengths [N] int32, end_flags [N] uint8, end_status [N] uint8) of cs_rollout_mlp_population
    from rollout_mlp_states' [K,N] tapes: d = the first step with a flag (K if none), returns = sum_{k<=d} disc_k
    reward_k with k ascending, disc_1 = 1, disc_{k+1} = disc_k gamma, each product and sum a float64 operation."""
    reward = np.asarray(reward, dtype=np.float64)
    term, trunc = np.asarray(terminated).astype(bool), np.asarray(truncated).astype(bool)
    status = np.asarray(status)
    K, N = reward.shape
    done = term | trunc
    d = np.where(done.any(0), done.argmax(0) + 1, K)
    ret, disc = np.zeros(N), np.float64(1.0)
    for k in range(K):
        live = k < d
        ret = np.where(live, ret + disc * reward[k], ret)
        disc = disc * np.float64(gamma)
    at = (d - 1, np.arange(N))
    flags = term[at].astype(np.uint8) | (trunc[at].astype(np.uint8) << 1)
    return ret, d.astype(np.int32), flags, status[at].astype(np.uint8)


def member_mean(returns, E):
    """member_returns [M] in the kernel's order: lane l adds returns[m E + l + 64 t], t ascending; then the tree of
    offsets 32 .. 1; lane 0's sum / E."""
    r = np.asarray(returns, dtype=np.float64).reshape(-1, E // 64, 64)
    v = np.zeros((r.shape[0], 64))
    for t in range(r.shape[1]):
        v = v + r[:, t]
    off = 32
    while off >= 1:
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
        off //= 2
    return v[:, 0] / np.float64(E)
