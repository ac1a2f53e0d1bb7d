"""CPU-side checks of cs_rollout_mppi_costs / cs_rollout_mppi_update: both entry points declared, exported and bound,
the ctypes struct mirroring the header; bad argument blocks refused without touching a device; the noise draw of
tests/mppi_ref.py against the kernels' own header compiled for the host (tests/host/mppi_noise_host), bit for bit, and
its moments; mppi_ref's update against a brute-force evaluation in longdouble; the explicit starts of the GPU cases under
non-default vehicle models (tests/model_variants.py) replayed through the oracle: no env may terminate."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mppi_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "mppi_noise_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    struct, mirror = "cs_rollout_mppi_io", _lib.RolloutMppiIO
    for name in ("cs_rollout_mppi_costs", "cs_rollout_mppi_update"):
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const %s\* \w+,\s*void\* stream\);"
                         % (name, struct), HEADER)
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes[2] is C.POINTER(mirror)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [f for _, f in decls] == [f for f, _ in mirror._fields_]
    # offsets from the header's declarations: natural alignment, as the C compiler lays the struct out
    size = {"uint32_t": 4, "int32_t": 4, "double": 8}
    at = 0
    for (ctype, field), (name, _) in zip(decls, mirror._fields_):
        w = 8 if "*" in ctype else size[ctype.strip()]
        at = (at + w - 1) // w * w
        assert getattr(mirror, name).offset == at and getattr(mirror, name).size == w, field
        at += w
    assert C.sizeof(mirror) == (at + 7) // 8 * 8 == 16 + 2 * 8 + 11 * 8
    assert lib.cs_version() == 5 == _lib.ABI_VERSION and re.search(r"#define CS_ABI_VERSION 5\b", HEADER)
    assert int(re.search(r"#define CS_MPPI_MAX_SAMPLES (\d+)", HEADER).group(1)) == _lib.MPPI_MAX_SAMPLES
    scale = re.search(r"#define CS_MPPI_NOISE_SCALE (\S+)f\b", HEADER).group(1)
    assert float.fromhex(scale) == float(mppi_ref.NOISE_SCALE)


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev = 0x1000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _mio(**kw):
    mio = _lib.RolloutMppiIO()
    mio.struct_size = C.sizeof(mio)
    mio.num_samples, mio.lam = 8, 1.0
    mio.sigma_dev, mio.x_ref_dev, mio.Q_dev, mio.R_dev, mio.costs_dev = 0x2000, 0x3000, 0x4000, 0x5000, 0x6000
    mio.actions_out_dev = 0x7000
    for k, v in kw.items():
        setattr(mio, k, v)
    return mio


@pytest.mark.parametrize("name", ["cs_rollout_mppi_costs", "cs_rollout_mppi_update"])
def test_shared_argument_checks_without_a_device(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in lib.cs_last_error()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_mio()), None) == _lib.ERR_ARG
    assert b"actions_dev" in lib.cs_last_error()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_mio()), None) == _lib.ERR_ARG
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null mio" in lib.cs_last_error()
    for delta in (-8, 8):
        bad = _mio(struct_size=C.sizeof(_lib.RolloutMppiIO) + delta)
        assert fn(None, C.byref(_io()), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in lib.cs_last_error()
    for P in (0, -1, _lib.MPPI_MAX_SAMPLES + 1):
        assert fn(None, C.byref(_io()), C.byref(_mio(num_samples=P)), None) == _lib.ERR_ARG
        assert b"num_samples must be in [1, 65535]" in lib.cs_last_error()
    for key in ("sigma_dev", "costs_dev"):
        assert fn(None, C.byref(_io()), C.byref(_mio(**{key: None})), None) == _lib.ERR_ARG
        assert b"required" in lib.cs_last_error()
    for P in (1, _lib.MPPI_MAX_SAMPLES):                                              # ... as far as the context
        assert fn(None, C.byref(_io()), C.byref(_mio(num_samples=P)), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"


def test_costs_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_mppi_costs
    for key in ("x_ref_dev", "Q_dev", "R_dev"):
        assert fn(None, C.byref(_io()), C.byref(_mio(**{key: None})), None) == _lib.ERR_ARG
        assert b"required" in lib.cs_last_error()
    for w in (-1e-300, -1.0, float("inf"), float("nan")):
        assert fn(None, C.byref(_io()), C.byref(_mio(reward_weight=w)), None) == _lib.ERR_ARG
        assert b"reward_weight must be" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_mio(x_ref_steps=2)), None) == _lib.ERR_ARG
    assert b"x_ref_steps" in lib.cs_last_error()
    # lambda and actions_out_dev are the update's: not looked at here
    ok = _mio(lam=0.0, actions_out_dev=None, reward_weight=2.0, x_ref_steps=1, a_ref_dev=None, best_dev=None)
    assert fn(None, C.byref(_io()), C.byref(ok), None) == _lib.ERR_ARG and lib.cs_last_error() == b"null context"


def test_update_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_mppi_update
    for lam in (0.0, -1.0, float("inf"), float("nan")):
        assert fn(None, C.byref(_io()), C.byref(_mio(lam=lam)), None) == _lib.ERR_ARG
        assert b"lambda must be" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_mio(actions_out_dev=None)), None) == _lib.ERR_ARG
    assert b"actions_out_dev is required" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_mio(actions_out_dev=0x1000)), None) == _lib.ERR_ARG
    assert b"alias" in lib.cs_last_error()
    assert fn(None, C.byref(_io(num_steps=_lib.MPPI_MAX_SAMPLES + 1)), C.byref(_mio()), None) == _lib.ERR_ARG
    assert b"num_steps must be <=" in lib.cs_last_error()
    # the costs' inputs are not the update's
    ok = _mio(x_ref_dev=None, Q_dev=None, R_dev=None, reward_weight=-1.0, ess_dev=None, cost_min_dev=None)
    assert fn(None, C.byref(_io()), C.byref(ok), None) == _lib.ERR_ARG and lib.cs_last_error() == b"null context"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the noise: the kernels' header on the host against the NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def _host(*args):
    out = subprocess.run([HOST] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split()
    return np.array([int(v, 16) for v in out], dtype=np.uint32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_noise_key_is_a_third_mix_of_the_seed():
    from oracle.refvec import splitmix64
    for seed in (0, 1, 7, 0xFFFFFFFF, 1 << 32, (1 << 64) - 1, 0x0123456789ABCDEF):
        key = int(_host("key", seed)[0])
        assert key == int(mppi_ref.noise_key(seed))
        h = splitmix64(seed)
        assert key == splitmix64(h) & 0xFFFFFFFF and key not in (h & 0xFFFFFFFF, h >> 32)


def test_noise_points_match_bit_for_bit():
    """A grid of (seed, env id, stream, k, p, j) with ids, nonces and keys near 2^32 (the key wraps: k = 16 384 shifts
    to 2^30, times 4)."""
    top = (1 << 32) - 1
    pts = [(seed, g, s, k, p, j)
           for seed in (0, 7, (1 << 64) - 1)
           for g in (0, 1, 63, 64, 1000003, top - 1, top)
           for s in (0, 1, top)
           for (k, p, j) in ((1, 0, 0), (1, 1, 3), (2, 255, 1), (64, 1023, 2), (16384, 65534, 3), (16384, 1, 0))]
    got = np.concatenate([_host("point", *[v for pt in pts[a:a + 60] for v in pt]) for a in range(0, len(pts), 60)])
    want = np.concatenate([_bits(mppi_ref.noise(*pt)).ravel() for pt in pts])
    assert got.shape == want.shape == (len(pts),) and np.array_equal(got, want)
    # and vectorised, as the tests call it
    arr = np.array(pts, dtype=object)
    for seed in (0, 7, (1 << 64) - 1):
        rows = arr[arr[:, 0] == seed]
        v = mppi_ref.noise(seed, *(rows[:, c].astype(np.int64) for c in range(1, 6)))
        assert np.array_equal(_bits(v), got[(arr[:, 0] == seed).nonzero()[0]])
    assert len(set(got.tolist())) > 0.9 * len(pts)


def test_noise_bulk_order_and_moments():
    """2^20 draws (64 envs from an id just below 2^32, K = 16, P = 256, A = 4): the restatement matches all of them, the
    values lie on the grid T x c with |T| <= 131 070, and the sample mean and variance lie within four standard errors
    of 0 and 1 - 2^-32: s.e.(mean) = 1 / sqrt(n) = 2^-10; s.e.(variance) = sqrt((kappa - 1) / n) with the kurtosis of
    Irwin-Hall of order 4, kappa = 3 - 6 / (5 x 4) = 2.7."""
    seed, id0, stream, envs, K, P, A = 11, (1 << 32) - 40, 3, 64, 16, 256, 4
    got = _host("bulk", seed, id0, stream, envs, K, P, A)
    n = envs * K * P * A
    assert n == 1 << 20 and got.shape == (n,)
    ids = (id0 + np.arange(envs))[:, None, None, None]
    want = mppi_ref.noise(seed, ids, stream, np.arange(1, K + 1)[None, :, None, None],
                          np.arange(P)[None, None, :, None], np.arange(A)[None, None, None, :])
    assert want.shape == (envs, K, P, A) and want.dtype == np.float32
    assert np.array_equal(_bits(want).ravel(), got)
    eps = got.view(np.float32).astype(np.float64)
    t = np.round(eps / float(mppi_ref.NOISE_SCALE))                 # (the one float32 multiply rounds: eps = fl32(T c))
    assert np.array_equal(t.astype(np.float32) * mppi_ref.NOISE_SCALE, got.view(np.float32))
    assert np.abs(t).max() <= 131070 and np.abs(eps).max() <= 3.4642
    mean, var = eps.mean(), eps.var()
    se_mean, se_var = 2.0 ** -10, np.sqrt((2.7 - 1.0) / n)
    print("noise over 2^20 draws: mean %.3e (s.e. %.3e), variance - 1 %.3e (s.e. %.3e)" % (mean, se_mean, var - 1, se_var))
    assert abs(mean) <= 4 * se_mean
    assert abs(var - (1.0 - 2.0 ** -32)) <= 4 * se_var
    # the first samples of a larger P are those of a smaller one: the key does not depend on P
    small = _host("bulk", seed, id0, stream, 2, 2, 8, A).reshape(2, 2, 8, A)
    assert np.array_equal(small, got.reshape(envs, K, P, A)[:2, :2, :8])
    # another nonce, another seed: other noise
    assert not np.array_equal(_host("bulk", seed, id0, stream + 1, 1, 1, 8, A), small[0, 0].ravel())
    assert not np.array_equal(_host("bulk", seed + 1, id0, stream, 1, 1, 8, A), small[0, 0].ravel())


def test_sample_actions():
    rng = np.random.default_rng(0)
    K, N, A, seed, stream = 3, 5, 4, 9, 2
    ids = 100 + np.arange(N)
    abar = rng.uniform(0, 1, (K, N, A)).astype(np.float32)
    sigma = np.array([0.1, 0.0, 0.25, 1.0], np.float32)
    assert np.array_equal(_bits(mppi_ref.sample_actions(abar, sigma, seed, ids, stream, 0)), _bits(abar))
    a = mppi_ref.sample_actions(abar, sigma, seed, ids, stream, 5)
    assert a.dtype == np.float32 and np.array_equal(a[..., 1], abar[..., 1]) and np.all(a[..., 0] != abar[..., 0])
    for k in range(K):
        for i in range(N):
            for j in range(A):
                eps = mppi_ref.noise(seed, ids[i], stream, k + 1, 5, j)
                assert a[k, i, j] == np.float32(abar[k, i, j] + np.float32(sigma[j] * eps))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the update against a brute-force evaluation in longdouble
# ---------------------------------------------------------------------------------------------------------------------
def _brute_update(abar, costs, sigma, lam, seed, ids, stream):
    """Scalar loops in longdouble, written from the formula: (unclipped new action as longdouble, ess, beta)."""
    L = np.longdouble
    K, N, A = abar.shape
    P = costs.shape[0]
    new, ess, beta = np.zeros((K, N, A), L), np.zeros(N, L), np.full(N, np.inf)
    for i in range(N):
        fin = [p for p in range(P) if np.isfinite(costs[p, i])]
        if not fin:
            new[:, i] = abar[:, i].astype(L)
            continue
        b = min(L(costs[p, i]) for p in fin)
        w = {p: np.exp(-(L(costs[p, i]) - b) / L(lam)) for p in fin}
        eta = sum(w.values(), L(0))
        ess[i], beta[i] = eta * eta / sum((v * v for v in w.values()), L(0)), float(b)
        for k in range(K):
            for j in range(A):
                s = L(0)
                for p in fin:
                    if p:
                        s += w[p] * L(np.float32(np.float32(sigma[j]) * mppi_ref.noise(seed, ids[i], stream, k + 1, p, j)))
                new[k, i, j] = L(abar[k, i, j]) + s / eta
    return new, ess, beta


@pytest.mark.parametrize("P,lam", [(1, 1.0), (3, 0.5), (7, 1.0), (33, 0.05), (33, 50.0)])
def test_update_against_longdouble_brute_force(P, lam):
    """Columns: ordinary costs; one with +inf and NaN entries; one with every cost non-finite (where P allows); ties.
    float64 sums over <= 33 terms of magnitude <= 3.5 sigma: the new action agrees with the longdouble value rounded
    to float32 except where that value lies within the float64 error (1e-13) of a rounding boundary -- one float32 ulp
    at most -- and ess / cost_min to 1e-13 relative."""
    rng = np.random.default_rng(100 + P)
    K, N, A, seed, stream = 3, 6, 2, 5, 4
    ids = (1 << 32) - 3 + np.arange(N)                 # (the global id wraps as the kernel's uint32 does)
    abar = rng.uniform(-0.1, 1.1, (K, N, A)).astype(np.float32)
    sigma = np.array([0.2, 0.05], np.float32)
    costs = rng.uniform(10.0, 14.0, (P, N))
    if P > 1:
        costs[0, 1], costs[P - 1, 1] = np.inf, np.nan
        costs[:, 2] = [np.nan, -np.inf, np.inf][:min(P, 3)] + [np.nan] * max(P - 3, 0)
        costs[:, 3] = costs[0, 3]                        # all tied: the plain mean
    else:
        costs[0, 2] = np.nan
    out, ess, cmin = mppi_ref.update(abar, costs, sigma, lam, seed, ids, stream)
    new, bess, beta = _brute_update(abar, costs, sigma, lam, seed, ids, stream)
    want = np.clip(new.astype(np.float32), np.float32(0), np.float32(1))
    want[:, 2] = abar[:, 2]                                   # (no finite cost: the plan is kept as it is, unclipped)
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(2.0 ** -20)))
    assert out.dtype == np.float32 and np.all(np.abs(out.astype(np.float64) - want) <= ulp)
    assert np.mean(out == want) > 0.99
    assert np.array_equal(_bits(out[:, 2]), _bits(abar[:, 2])) and ess[2] == 0 and cmin[2] == np.inf
    live = np.arange(N) != 2
    assert np.max(np.abs(ess[live] / bess[live].astype(np.float64) - 1)) < 1e-13
    assert np.array_equal(cmin[live], beta[live])
    assert np.all(ess[live] >= 1 - 1e-13) and np.all(ess[live] <= P + 1e-9)
    if P > 1:
        assert abs(ess[3] - P) < 1e-9 and abs(ess[1] - bess[1]) < 1e-9 and ess[1] <= P - 2 + 1e-9
        mean = sum(mppi_ref.perturbation(sigma, seed, ids[3:4], stream, K, p, A).astype(np.float64) for p in range(P)) / P
        assert np.allclose(out[:, 3:4], np.clip(abar[:, 3:4] + mean, 0, 1), rtol=0, atol=1e-6)
    else:
        assert np.array_equal(out[:, live], np.clip(abar[:, live], 0, 1)) and np.all(ess[live] == 1)
    assert np.array_equal(mppi_ref.best(costs)[[1, 2]], [int(np.nanargmin(np.where(np.isfinite(costs[:, 1]), costs[:, 1],
                                                                                    np.nan))), -1])


def test_cost_restatement():
    """cost_terms against scalar loops, and its longdouble form."""
    rng = np.random.default_rng(3)
    K, N, A = 4, 3, 2
    x, xr = rng.standard_normal((K, N, 12)), rng.standard_normal((K, N, 12))
    a = rng.uniform(0, 1, (K, N, A)).astype(np.float32)
    rew = rng.standard_normal((K, N))
    m = rng.standard_normal((12, 12))
    Q, Qf, R, ar = m @ m.T, np.eye(12) * 3, np.diag([1.0, 0.0]), np.array([0.5, 0.25])
    S = mppi_ref.cost(x, rew, a, xr, Q, R, Q_final=Qf, a_ref=ar, reward_weight=0.7)
    for i in range(N):
        s = 0.0
        for k in range(K):
            dx, da = x[k, i] - xr[k, i], a[k, i].astype(np.float64) - ar
            s += 0.5 * dx @ (Qf if k == K - 1 else Q) @ dx + 0.5 * da @ R @ da - 0.7 * rew[k, i]
        assert abs(S[i] - s) <= 1e-12 * abs(s)
    Sl = mppi_ref.cost(x, rew, a, xr, Q, R, Q_final=Qf, a_ref=ar, reward_weight=0.7, dtype=np.longdouble)
    assert Sl.dtype == np.longdouble and np.max(np.abs(Sl - S)) < 1e-11
    assert np.array_equal(mppi_ref.cost(x, rew, a, xr[0], Q, R), mppi_ref.cost(x, rew, a, np.broadcast_to(xr[0], x.shape), Q, R))


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases under non-default vehicle models keep every sample of their explicit start airborne
# ---------------------------------------------------------------------------------------------------------------------
def test_variant_cost_cases_terminate_nowhere_in_the_oracle():
    """tests/test_gpu_rollout_mppi.py::test_costs_under_model_variants asserts that no sample of its explicit start
    terminates (expect_quiet).  The same problem through VecOracle with the variant's vehicle, world and thrust law, in
    the case's storage mode: samples 0, 3 and P - 1 stay airborne, inside the bounds and below the tilt limit.  (The
    oracle has no float32 motor law: act_f32 is replayed on the float64 one, 1e-7 relative away.)"""
    import model_variants
    import test_gpu_rollout_mppi as gpu
    from oracle.refcpu import AIRBORNE
    from rollout_fd import oracle_rollout
    ids = gpu.VARIANT_BASE + np.arange(gpu.VARIANT_N)
    for variant, task, mode, substeps in gpu.VARIANT_COST_CASES:
        _, installed, abar, sigma, state = gpu._variant_problem(variant, task, mode, substeps)
        model = model_variants.oracle_model(None if variant == "act_f32" else variant, installed)
        for p in (0, 3, gpu.VARIANT_P - 1):
            a = mppi_ref.sample_actions(abar, sigma, gpu.VARIANT_SEED, ids, gpu.VARIANT_STREAM, p)
            xs, _, term, trunc, orc = oracle_rollout(task, state["x"], state["status"], a, force=state["force"],
                                                     substeps=substeps, store_mode=mode, **model)
            assert not term.any() and not trunc.any(), (variant, task, p)
            assert np.all(orc.status == AIRBORNE) and xs[..., 4].max() < -4.0, (variant, task, p)
            assert np.abs(xs[..., [6, 8]]).max() < 0.7 and np.abs(xs[..., [0, 2]]).max() < 6.0, (variant, task, p)
