"""CPU-side checks of cs_rollout_mlp_population / cs_es_perturb / cs_es_gradient: the entry
points declared, exported and bound, the ctypes structs mirroring the header; bad argument blocks refused without
touching a device; the noise draw of tests/es_ref.py against the kernels' own header compiled for the host
(tests/host/es_noise_host), bit for bit, and its moments; es_ref's gradient against a scalar loop in longdouble.
(N = members x envs_per_member needs the context's N: tests/test_gpu_rollout_es.py checks that refusal.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import es_ref
import mppi_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "es_noise_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors
# ---------------------------------------------------------------------------------------------------------------------
def _check_mirror(struct, mirror, expect_size):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [f for _, f in decls] == [f for f, _ in mirror._fields_]
    # offsets from the header's declarations: natural alignment, as the C compiler lays the struct out
    size = {"uint32_t": 4, "int32_t": 4, "float": 4, "double": 8}
    at = 0
    for (ctype, field), (name, _) in zip(decls, mirror._fields_):
        w = 8 if "*" in ctype else size[ctype.strip()]
        at = (at + w - 1) // w * w
        assert getattr(mirror, name).offset == at and getattr(mirror, name).size == w, field
        at += w
    assert C.sizeof(mirror) == (at + 7) // 8 * 8 == expect_size
    assert decls[0][1] == "struct_size"


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_rollout_mlp_population\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, "
                     r"const cs_rollout_population_io\* \w+,\s*void\* stream\);", HEADER)
    for name in ("cs_es_perturb", "cs_es_gradient"):
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_es_io\* \w+,\s*void\* stream\);" % name, HEADER)
        assert getattr(lib, name).argtypes[1] is C.POINTER(_lib.EsIO)
    for name in ("cs_rollout_mlp_population", "cs_es_perturb", "cs_es_gradient"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.cs_rollout_mlp_population.argtypes[2] is C.POINTER(_lib.RolloutPopulationIO)
    _check_mirror("cs_rollout_population_io", _lib.RolloutPopulationIO, 16 + 8 + 6 * 8)
    _check_mirror("cs_es_io", _lib.EsIO, 24 + 4 * 8)
    assert lib.cs_version() == 5 == _lib.ABI_VERSION and re.search(r"#define CS_ABI_VERSION 5\b", HEADER)
    for macro, value in (("CS_ES_PAIR_CHUNK", _lib.ES_PAIR_CHUNK), ("CS_ES_MAX_MEMBERS", _lib.ES_MAX_MEMBERS),
                         ("CS_ES_MAX_PARAMS", _lib.ES_MAX_PARAMS)):
        assert int(re.search(r"#define %s (\d+)" % macro, HEADER).group(1)) == value
    assert _lib.ES_PAIR_CHUNK == es_ref.PAIR_CHUNK
    assert _lib.ES_MAX_PARAMS == 64 * 13 + 4 * 65                # Hover3D, hidden = 64: the largest policy


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _pio(**kw):
    pio = _lib.RolloutPopulationIO()
    pio.struct_size = C.sizeof(pio)
    pio.hidden, pio.members, pio.envs_per_member, pio.gamma = 8, 4, 64, 1.0
    pio.params_table_dev, pio.returns_dev = 0x2000, 0x3000
    for k, v in kw.items():
        setattr(pio, k, v)
    return pio


def _eio(**kw):
    eio = _lib.EsIO()
    eio.struct_size = C.sizeof(eio)
    eio.members, eio.num_params, eio.sigma = 4, 10, 0.1
    eio.params_dev, eio.table_dev, eio.weights_dev, eio.grad_dev = 0x2000, 0x3000, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(eio, k, v)
    return eio


def test_population_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_mlp_population
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null pio" in lib.cs_last_error()
    for delta in (-8, 8):
        bad = _pio(struct_size=C.sizeof(_lib.RolloutPopulationIO) + delta)
        assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in lib.cs_last_error()
    bad = _io(struct_size=C.sizeof(_lib.RolloutIO) - 8)
    assert fn(None, C.byref(bad), C.byref(_pio()), None) == _lib.ERR_ABI and b"struct_size" in lib.cs_last_error()
    for H in (-1, _lib.MLP_MAX_HIDDEN + 1):
        assert fn(None, C.byref(_io()), C.byref(_pio(hidden=H)), None) == _lib.ERR_ARG
        assert b"hidden" in lib.cs_last_error()
    for E in (0, -64, 1, 63, 65, 96, 100):
        assert fn(None, C.byref(_io()), C.byref(_pio(envs_per_member=E)), None) == _lib.ERR_ARG
        assert b"is not a positive multiple of 64" in lib.cs_last_error()
    for M in (0, -2):
        assert fn(None, C.byref(_io()), C.byref(_pio(members=M)), None) == _lib.ERR_ARG
        assert b"members must be >= 1" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_pio(members=1 << 26, envs_per_member=64)), None) == _lib.ERR_ARG
    assert b"does not fit" in lib.cs_last_error()
    for g in (float("inf"), float("nan")):
        assert fn(None, C.byref(_io()), C.byref(_pio(gamma=g)), None) == _lib.ERR_ARG
        assert b"gamma must be finite" in lib.cs_last_error()
    for key in ("params_table_dev", "returns_dev"):
        assert fn(None, C.byref(_io()), C.byref(_pio(**{key: None})), None) == _lib.ERR_ARG
        assert b"required" in lib.cs_last_error()
    assert fn(None, C.byref(_io(actions_dev=0x1000)), C.byref(_pio()), None) == _lib.ERR_ARG
    assert b"actions_dev must be NULL" in lib.cs_last_error()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_pio()), None) == _lib.ERR_ARG
    assert b"num_steps" in lib.cs_last_error()
    assert fn(None, C.byref(_io(start_status_dev=0x1000)), C.byref(_pio()), None) == _lib.ERR_ARG
    assert b"start_x_dev is required" in lib.cs_last_error()
    # ... as far as the context (where N = members x envs_per_member is checked): the optional outputs may be NULL
    for ok in (_pio(), _pio(hidden=0, members=1, envs_per_member=128, gamma=0.0), _pio(hidden=64, gamma=-0.5)):
        assert fn(None, C.byref(_io()), C.byref(ok), None) == _lib.ERR_ARG and lib.cs_last_error() == b"null context"


@pytest.mark.parametrize("name", ["cs_es_perturb", "cs_es_gradient"])
def test_es_calls_refuse_bad_arguments_without_a_device(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    assert fn(None, None, None) == _lib.ERR_ARG and b"null eio" in lib.cs_last_error()
    for delta in (-8, 8):
        bad = _eio(struct_size=C.sizeof(_lib.EsIO) + delta)
        assert fn(None, C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in lib.cs_last_error()
    for M in (0, 1, 3, 5, -2, _lib.ES_MAX_MEMBERS + 2):
        assert fn(None, C.byref(_eio(members=M)), None) == _lib.ERR_ARG
        assert b"is not an even number in [2, 65536]" in lib.cs_last_error()
    for P in (0, -1, _lib.ES_MAX_PARAMS + 1):
        assert fn(None, C.byref(_eio(num_params=P)), None) == _lib.ERR_ARG
        assert b"num_params" in lib.cs_last_error()
    mine = ("params_dev", "table_dev") if name == "cs_es_perturb" else ("weights_dev", "grad_dev")
    other = ("weights_dev", "grad_dev") if name == "cs_es_perturb" else ("params_dev", "table_dev")
    for key in mine:
        assert fn(None, C.byref(_eio(**{key: None})), None) == _lib.ERR_ARG and b"required" in lib.cs_last_error()
    for s in (-1e-30, float("inf"), float("nan")):
        rc = fn(None, C.byref(_eio(sigma=s)), None)
        assert rc == _lib.ERR_ARG
        if name == "cs_es_perturb":
            assert b"sigma must be" in lib.cs_last_error()
        else:                                                           # (sigma is the perturbation's alone)
            assert lib.cs_last_error() == b"null context"
    for ok in (_eio(**{k: None for k in other}), _eio(members=2, num_params=1, sigma=0.0),
               _eio(members=_lib.ES_MAX_MEMBERS, num_params=_lib.ES_MAX_PARAMS, noise_stream=(1 << 32) - 1,
                    pair_base=(1 << 32) - 1)):
        assert fn(None, C.byref(ok), None) == _lib.ERR_ARG and lib.cs_last_error() == b"null context"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the noise: the kernels' header on the host against the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def _host(*args):
    out = subprocess.run([HOST] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split()
    return np.array([int(v, 16) for v in out], dtype=np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_noise_key_is_a_fourth_mix_of_the_seed():
    from oracle.refvec import splitmix64
    for seed in (0, 1, 7, 0xFFFFFFFF, 1 << 32, (1 << 64) - 1, 0x0123456789ABCDEF):
        key = int(_host("key", seed)[0])
        assert key == int(es_ref.noise_key(seed))
        h = splitmix64(seed)
        assert key == splitmix64(splitmix64(h)) & 0xFFFFFFFF
        assert key not in (h & 0xFFFFFFFF, h >> 32, int(mppi_ref.noise_key(seed)))


def test_noise_points_match_bit_for_bit():
    """A grid of (seed, pair, nonce, p) with pair indices and nonces at the 2^32 wrap; the key wraps too: key_es + p
    passes 2^32 for the large p (p >= 2^32 - key_es), whatever the seed's key is."""
    top = (1 << 32) - 1
    seeds = [0, 7, (1 << 64) - 1]
    for seed in seeds:
        key = int(es_ref.noise_key(seed))
        assert key + top > top and 0 < (1 << 32) - key <= top                  # (some p of the grid wraps the key)
    pts = [(seed, g, s, p) for seed in seeds for g in (0, 1, 31, 32, 1000003, top - 1, top) for s in (0, 1, top)
           for p in (0, 1, 63, 64, 1000, 1091, top - int(es_ref.noise_key(seed)), top + 1 - int(es_ref.noise_key(seed)),
                     top)]
    got = np.concatenate([_host("point", *[v for pt in pts[a:a + 100] for v in pt]) for a in range(0, len(pts), 100)])
    want = np.concatenate([_bits(es_ref.noise(*pt)).ravel() for pt in pts])
    assert got.shape == want.shape == (len(pts),) and np.array_equal(got, want)
    arr = np.array(pts, dtype=object)                                    # and vectorised, as the tests call it
    for seed in seeds:
        rows = arr[arr[:, 0] == seed]
        v = es_ref.noise(seed, *(rows[:, c].astype(np.int64) for c in range(1, 4)))
        assert np.array_equal(_bits(v), got[(arr[:, 0] == seed).nonzero()[0]])
        assert len(set(_bits(v).tolist())) > 0.9 * len(rows)           # (distinct (counter, key) within a seed)
    # the pair index wraps as the kernel's uint32 does: pair_base + i past 2^32 is pair (pair_base + i) mod 2^32
    assert np.array_equal(_bits(es_ref.pair_noise(7, 3, 4, 5, pair_base=top - 1)),
                          _bits(es_ref.noise(7, np.array([top - 1, top, 0, 1])[:, None], 3, np.arange(5)[None, :])))


def test_noise_bulk_order_and_moments():
    """2^20 draws (1024 pairs from an index just below 2^32, P = 1024): the restatement matches all of them, the values
    lie on the grid T x c with |T| <= 131 070, and the sample mean and variance lie within four standard errors of 0 and
    1 - 2^-32: s.e.(mean) = 1 / sqrt(n) = 2^-10; s.e.(variance) = sqrt((kappa - 1) / n) with the kurtosis of Irwin-Hall
    of order 4, kappa = 3 - 6 / (5 x 4) = 2.7."""
    seed, pair0, stream, pairs, P = 11, (1 << 32) - 40, 3, 1024, 1024
    got = _host("bulk", seed, pair0, stream, pairs, P)
    n = pairs * P
    assert n == 1 << 20 and got.shape == (n,)
    want = es_ref.pair_noise(seed, stream, pairs, P, pair_base=pair0)
    assert want.shape == (pairs, P) and want.dtype == np.float32
    assert np.array_equal(_bits(want).ravel(), got)
    eps = got.view(np.float32).astype(np.float64)
    t = np.round(eps / float(mppi_ref.NOISE_SCALE))
    assert np.array_equal(t.astype(np.float32) * mppi_ref.NOISE_SCALE, got.view(np.float32))
    assert np.abs(t).max() <= 131070 and np.abs(eps).max() <= 3.4642
    mean, var = eps.mean(), eps.var()
    se_mean, se_var = 2.0 ** -10, np.sqrt((2.7 - 1.0) / n)
    print("noise over 2^20 draws: mean %.3e (s.e. %.3e), variance - 1 %.3e (s.e. %.3e)" % (mean, se_mean, var - 1, se_var))
    assert abs(mean) <= 4 * se_mean
    assert abs(var - (1.0 - 2.0 ** -32)) <= 4 * se_var
    # a pure function of (seed, nonce, pair, p): a smaller population, fewer parameters and another base give the same
    small = _host("bulk", seed, pair0 + 5, stream, 3, 8).reshape(3, 8)
    assert np.array_equal(small, got.reshape(pairs, P)[5:8, :8])
    # another nonce, another seed: other noise
    assert not np.array_equal(_host("bulk", seed, pair0 + 5, stream + 1, 3, 8).reshape(3, 8), small)
    assert not np.array_equal(_host("bulk", seed + 1, pair0 + 5, stream, 3, 8).reshape(3, 8), small)


def test_es_draws_differ_from_the_mppi_draws_of_the_same_seed():
    """The same seed, counter words and key offset under the MPPI key give other bits: (env id, nonce, k = 1, p = 0, j)
    has the key key_noise + j, the ES draw (pair, nonce, p = j) the key key_es + j."""
    seed, stream = 11, 3
    ids, j = np.arange(64)[:, None], np.arange(4)[None, :]
    a = es_ref.noise(seed, ids, stream, j)
    b = mppi_ref.noise(seed, ids, stream, 1, 0, j)
    assert a.shape == b.shape == (64, 4)
    assert np.mean(_bits(a) == _bits(b)) < 0.01
    assert int(es_ref.noise_key(seed)) != int(mppi_ref.noise_key(seed))


def test_perturb_restatement():
    rng = np.random.default_rng(0)
    P, M, seed, stream, base = 13, 6, 9, 2, 5
    theta = rng.standard_normal(P).astype(np.float32)
    table = es_ref.perturb(theta, 0.25, M, seed, stream, base)
    assert table.dtype == np.float32 and table.shape == (M, P)
    for i in range(M // 2):
        for p in range(P):
            d = np.float32(np.float32(0.25) * es_ref.noise(seed, base + i, stream, p))
            assert table[2 * i, p] == np.float32(theta[p] + d) and table[2 * i + 1, p] == np.float32(theta[p] - d)
    assert np.array_equal(_bits(es_ref.perturb(theta, 0.0, M, seed, stream)), _bits(np.tile(theta, (M, 1))))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the gradient against a scalar loop in longdouble; the return and the member mean against scalar loops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 10, 64, 66, 200])
def test_gradient_against_a_longdouble_loop(M):
    """float64 sums of M/2 terms in the kernel's order against scalar longdouble loops written from the formula: within
    (M/2 + 1) 2^-53 x the sum of the terms' absolute values (each term one rounded difference and one rounded product,
    then M/2 - 1 additions and the chunk sums)."""
    L = np.longdouble
    rng = np.random.default_rng(M)
    P, seed, stream, base = 7, 5, 4, (1 << 32) - 3
    w = rng.standard_normal(M)
    g, mag = es_ref.gradient(w, P, seed, stream, base)
    assert g.dtype == np.float64 and g.shape == mag.shape == (P,)
    for p in range(P):
        s, a = L(0), L(0)
        for i in range(M // 2):
            term = (L(w[2 * i]) - L(w[2 * i + 1])) * L(es_ref.noise(seed, base + i, stream, p))
            s += term
            a += abs(term)
        assert abs(L(g[p]) - s) <= (M // 2 + 1) * 2.0 ** -53 * float(a) + 1e-300
        assert abs(mag[p] - float(a)) <= 1e-12 * float(a)
    gl, _ = es_ref.gradient(w, P, seed, stream, base, dtype=np.longdouble)
    assert gl.dtype == np.longdouble and np.all(np.abs(gl - g) <= (M // 2 + 1) * 2.0 ** -53 * mag)
    # equal weights inside every pair: exactly zero
    same = np.repeat(rng.standard_normal(M // 2), 2)
    assert np.array_equal(es_ref.gradient(same, P, seed, stream, base)[0], np.zeros(P))


def test_returns_and_member_mean_restatements():
    rng = np.random.default_rng(4)
    K, N, gamma = 9, 128, 0.97
    reward = rng.standard_normal((K, N))
    term = rng.uniform(size=(K, N)) < 0.08
    trunc = rng.uniform(size=(K, N)) < 0.04
    status = rng.integers(0, 4, (K, N)).astype(np.uint8)
    ret, d, flags, st = es_ref.returns_from_tapes(reward, term, trunc, status, gamma)
    assert d.dtype == np.int32 and flags.dtype == st.dtype == np.uint8
    for i in range(N):
        s, disc, di = 0.0, 1.0, K
        for k in range(K):
            s = s + disc * reward[k, i]
            disc = disc * gamma
            if term[k, i] or trunc[k, i]:
                di = k + 1
                break
        assert ret[i] == s and d[i] == di
        assert flags[i] == int(term[di - 1, i]) + 2 * int(trunc[di - 1, i]) and st[i] == status[di - 1, i]
    assert (d < K).any() and (d == K).any() and np.all(flags[d < K] != 0)
    ret1 = es_ref.returns_from_tapes(reward, term, trunc, status, 1.0)[0]
    assert np.allclose(ret1, [reward[:d[i], i].sum() for i in range(N)], rtol=0, atol=1e-12)
    for E in (64, 128):
        mean = es_ref.member_mean(ret, E)
        exact = ret.astype(np.longdouble).reshape(-1, E).mean(1)
        bound = (2 * E + 64) * 2.0 ** -53 * np.abs(ret).reshape(-1, E).sum(1)
        assert mean.shape == (N // E,) and np.all(np.abs(mean - exact) <= bound)


def test_centred_ranks_of_the_driver():
    """gym_copter_amd.es's shaping: rank / (M - 1) - 1/2, ties in index order, a fitness that is not finite below every
    finite one; the weights sum to zero."""
    import torch
    from gym_copter_amd.es import shape_fitness
    f = torch.tensor([3.0, float("nan"), 1.0, 7.0, float("inf"), 1.0], dtype=torch.float64)
    w = shape_fitness(f)
    assert w.dtype == torch.float64
    assert torch.equal(w, torch.tensor([4, 0, 2, 5, 1, 3], dtype=torch.float64) / 5 - 0.5)
    assert abs(float(w.sum())) < 1e-15
    assert torch.equal(shape_fitness(torch.tensor([2.0, 5.0], dtype=torch.float64)), torch.tensor([-0.5, 0.5], dtype=torch.float64))
