"""NumPy restatement of the actor-critic collection and GAE entry points (include/copterstep.h: cs_rollout_actor_critic /
cs_gae): the noise draw, the log-probability, the live mask and the advantages.  Written from the contract in the
header; the Philox round function and the seed mix are the oracle's."""
import numpy as np

from oracle.refvec import philox2x32_10, splitmix64

TWO_PI_F32 = np.float32(6.2831854820251465)                    # fl32(2 pi), 0x1.921fb6p+2


def noise_key(seed):
    """lo32(splitmix64^4(seed))."""
    z = int(seed) & ((1 << 64) - 1)
    for _ in range(4):
        z = splitmix64(z)
    return np.uint32(z & 0xFFFFFFFF)


def uniforms(seed, g, nonce, k, pair):
    """(u1, u2) float32 of (global env id, nonce, step k = 1.., pair of components); the arguments broadcast.  Bit for
    bit what the kernel's header computes: integer arithmetic, then two float32 operations each."""
    g, nonce, k, pair = (np.asarray(v, dtype=np.int64) for v in (g, nonce, k, pair))
    key = (int(noise_key(seed)) + 2 * k + pair) & 0xFFFFFFFF
    g, nonce, key = np.broadcast_arrays(g & 0xFFFFFFFF, nonce & 0xFFFFFFFF, key)
    r0, r1 = philox2x32_10(g.astype(np.uint32), nonce.astype(np.uint32), key.astype(np.uint32))
    m1 = (np.asarray(r0, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)
    u1 = (m1 * np.float32(2.0 ** -24)).astype(np.float32)
    u2 = ((np.asarray(r1, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return u1, u2


def box_muller(u1, u2, dtype=np.float64):
    """(eps_even, eps_odd, R) of the exact float32 bits u1, u2, evaluated in `dtype` with the true 2 pi."""
    u1, u2 = np.asarray(u1).astype(dtype), np.asarray(u2).astype(dtype)
    two_pi = dtype(2) * (np.arctan(dtype(1)) * dtype(4))
    r = np.sqrt(dtype(-2) * np.log(u1))
    t = two_pi * u2
    return r * np.cos(t), r * np.sin(t), r


def noise(seed, g, nonce, k, c, dtype=np.float64):
    """eps of (global env id, nonce, step k = 1.., action component c) in float64 (the reference the kernel's float32
    value is compared with); the arguments broadcast."""
    c = np.asarray(c, dtype=np.int64)
    u1, u2 = uniforms(seed, g, nonce, k, c >> 1)
    even, odd, _ = box_muller(u1, u2, dtype)
    return np.where(np.broadcast_to(c & 1, even.shape) == 0, even, odd)


def noise_radius(seed, g, nonce, k, c):
    """R = sqrt(-2 ln u1) of the same draw, float64: the scale of eps' error."""
    u1, u2 = uniforms(seed, g, nonce, k, np.asarray(c, dtype=np.int64) >> 1)
    return box_muller(u1, u2)[2]


def logp(actions, means, log_std, dtype=np.float64):
    """-1/2 sum_c z_c^2 - sum_c log_std[c] - (A/2) ln 2 pi in `dtype` from the float32 tapes, c ascending."""
    a, mu, ls = (np.asarray(v, dtype=np.float32).astype(dtype) for v in (actions, means, log_std))
    A = a.shape[-1]
    zz, sl = np.zeros(a.shape[:-1], dtype), dtype(0)
    for c in range(A):
        z = (a[..., c] - mu[..., c]) * np.exp(-ls[c])
        zz = zz + z * z
        sl = sl + ls[c]
    pi = np.arctan(dtype(1)) * dtype(4)
    return (dtype(-0.5) * zz - sl) - dtype(A) * (np.log(dtype(2) * pi) / dtype(2))


def live(terminated, truncated, pending0, next_step):
    """live [K,N] bool: under next_step auto-reset step k is a reset step, live = False, where the step before it ended
    an episode -- for the call's first step: where a reset was pending in the stored state; True everywhere in the other
    modes."""
    done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
    out = np.ones(done.shape, bool)
    if next_step:
        out[0] = ~np.asarray(pending0).astype(bool)
        out[1:] = ~done[:-1]
    return out


def gae(reward, values, terminated, truncated, gamma, lam):
    """(advantages, returns) [K,N] float32, the kernel's arithmetic operation for operation: float32, k descending,
    every product and sum rounded on its own."""
    f = np.float32
    r, v = np.asarray(reward, dtype=f), np.asarray(values, dtype=f)
    done = np.asarray(terminated).astype(bool) | np.asarray(truncated).astype(bool)
    K = r.shape[0]
    g = f(gamma)
    gl = f(g * f(lam))
    nd = np.where(done, f(0), f(1)).astype(f)
    adv, ret = np.empty_like(r), np.empty_like(r)
    nxt = np.zeros(r.shape[1:], f)
    for k in range(K - 1, -1, -1):
        boot = ((g * v[k + 1]).astype(f) * nd[k]).astype(f)
        delta = ((r[k] + boot).astype(f) - v[k]).astype(f)
        carry = ((gl * nd[k]).astype(f) * nxt).astype(f)
        nxt = (delta + carry).astype(f)
        adv[k] = nxt
        ret[k] = (nxt + v[k]).astype(f)
    return adv, ret
