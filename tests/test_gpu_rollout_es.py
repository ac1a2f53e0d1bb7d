"""cs_rollout_mlp_population / cs_es_perturb / cs_es_gradient on the GPU: a population's returns,
lengths, flags and status against the tapes of the existing rollout_mlp_states run once per member; the mirrored table
and the search gradient against tests/es_ref.py; determinism, no side effects; the es driver; plumbing.  The population
also under the non-default vehicle models of tests/model_variants.py."""
import zlib

import numpy as np
import pytest

import es_ref
import model_variants
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASK_SHAPE = {"lander3d": (10, 4), "hover3d": (12, 4), "lander2d": (6, 2), "hover1d": (2, 1)}
AH = hover_action()


def _env(task, n, mode="float32", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _num_params(task, H):
    from gym_copter_amd import mlp
    return mlp.num_params(TASK_SHAPE[task][0], TASK_SHAPE[task][1], H)


def _low_starts(n, rng):
    """tests/test_gpu_rollout_mppi.py's low-start recipe: 0.05-1.5 m up and descending at up to 4 m/s, so that within
    K = 24 steps (0.24 s: a fall of 0.3 m plus up to 1 m of descent) a good part of the lanes touches down or crashes and
    a good part stays up (asserted on the reference tapes where it is used)."""
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    x[1], x[3] = rng.uniform(-2, 2, (2, n))
    x[4] = rng.uniform(-1.2, -0.05, n)
    x[5] = rng.uniform(0.0, 4.0, n)
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    x[10] = rng.uniform(-1, 1, n)
    x[7], x[9], x[11] = rng.uniform(-1, 1, (3, n))
    return x, np.full(n, AIRBORNE, np.uint8)


def _table(task, M, H, rng, ah=AH):
    """M parameter vectors that act differently: every member's output bias is its own multiple of the hover motor value
    (0.6 .. 1.25 from the first member to the last, +-3 % per motor), the other weights nn.Linear-sized draws with a
    small output layer."""
    obs, A = TASK_SHAPE[task]
    rows = []
    for m in range(M):
        bias = ah * (0.6 + 0.65 * (m + 0.5) / M) * rng.uniform(0.97, 1.03, A)
        if H == 0:
            parts = [rng.uniform(-1, 1, (A, obs)) * 0.0002, bias]
        else:
            parts = [rng.uniform(-1, 1, (H, obs)) / np.sqrt(obs), rng.uniform(-1, 1, H) / np.sqrt(obs),
                     rng.uniform(-1, 1, (A, H)) * 0.001 / np.sqrt(H), bias]
        rows.append(np.concatenate([p.ravel() for p in parts]))
    table = np.stack(rows).astype(np.float32)
    assert table.shape == (M, _num_params(task, H))
    return table


def _reference(env, table, K, H, E, gamma, state):
    """What cs_rollout_mlp_population must give, from the existing closed-loop forward: rollout_mlp_states once per
    member with theta = table[m], that member's lanes of its tapes, and es_ref.returns_from_tapes.  Also (a) whether
    the members act differently: in every lane that starts airborne the action of step 1 under the next member's theta
    differs in bits from its own member's; (b) the shares of lanes with d < K and d = K."""
    M = table.shape[0]
    n = M * E
    cols = {k: [] for k in ("reward", "terminated", "truncated", "status")}
    first = []
    for m in range(M):
        ro = env.rollout_mlp_states(_dev(table[m], env), K, H, state=state)
        first.append(to_np(ro.actions[0]).copy())
        for k in cols:
            cols[k].append(to_np(getattr(ro, k))[:, m * E:(m + 1) * E].copy())
    tapes = {k: np.concatenate(v, axis=1) for k, v in cols.items()}
    ret, d, flags, status = es_ref.returns_from_tapes(tapes["reward"], tapes["terminated"], tapes["truncated"],
                                                      tapes["status"], gamma)
    differ = np.ones(n, bool)
    for m in range(M if M > 1 else 0):
        lanes = slice(m * E, (m + 1) * E)
        a, b = first[m][lanes], first[(m + 1) % M][lanes]
        differ[lanes] = np.any(a.view(np.uint32) != b.view(np.uint32), axis=1)
    return (ret, d, flags, status), differ, tapes


def _check_population(name, env, table, K, H, E, gamma, state, expect_events=True, airborne=None):
    """torch.equal on all four outputs against _reference (the arithmetic is fixed: equality is the bar), member_returns
    within (2E + 64) 2^-53 sum|returns| of NumPy's mean (any summation order of E terms and the division), and both bit
    for bit the same on a second call."""
    import torch
    M = table.shape[0]
    want, differ, tapes = _reference(env, table, K, H, E, gamma, state)
    ret, d, flags, status = want
    if airborne is None:
        airborne = np.ones(M * E, bool)
    if M > 1:
        assert np.all(differ[airborne]), (name, "members act alike in %d airborne lanes" % int((~differ & airborne).sum()))
    early, full = float(np.mean(d < K)), float(np.mean(d == K))
    print("%s: d < K in %.0f %% of the lanes, d = K in %.0f %%; terminated %d, truncated %d; end status %s"
          % (name, 100 * early, 100 * full, int((flags & 1).sum()), int((flags >> 1).sum()),
             np.bincount(status, minlength=4).tolist()))
    if expect_events and K > 1:
        assert early >= 0.25 and full >= 0.25, (name, early, full)
    kw = dict(state=state)
    pop = env.rollout_mlp_population(_dev(table, env), K, H, E, gamma, **kw)
    got = [t.clone() for t in pop]
    assert got[0].dtype == torch.float64 and got[1].dtype == torch.int32 and got[2].dtype == got[3].dtype == torch.uint8
    assert got[4].dtype == torch.float64 and tuple(got[4].shape) == (M,) and tuple(got[0].shape) == (M * E,)
    for g, w, what in zip(got[:4], (ret, d, flags, status), ("returns", "lengths", "end_flags", "end_status")):
        w = torch.from_numpy(np.ascontiguousarray(w))
        g = g.cpu()
        if what == "returns":                                     # (bits: a NaN return compares equal to itself)
            g, w = g.view(torch.int64), w.view(torch.int64)
        bad = (g != w).nonzero().flatten()[:8].tolist()
        assert torch.equal(g, w), (name, what, bad, [to_np(got[k])[bad].tolist() for k in range(4)], d[bad].tolist())
    mean = ret.astype(np.longdouble).reshape(M, E).mean(1).astype(np.float64)
    bound = (2 * E + 64) * 2.0 ** -53 * np.abs(ret).reshape(M, E).sum(1)
    fin = np.isfinite(mean)
    assert np.array_equal(np.isfinite(to_np(got[4])), fin), name
    assert np.all(np.abs(to_np(got[4])[fin] - mean[fin]) <= bound[fin]), name
    assert np.array_equal(to_np(got[4])[fin], es_ref.member_mean(ret, E)[fin]), name       # (the documented order)
    again = env.rollout_mlp_population(_dev(table, env), K, H, E, gamma, **kw)
    for g, a in zip(got, again):
        assert torch.equal(g.view(torch.uint8), a.view(torch.uint8)), name
    return got, want, tapes


# ---------------------------------------------------------------------------------------------------------------------
# 1. the population's returns
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [0, 1, 32, 64])
@pytest.mark.parametrize("M,E", [(4, 64), (3, 128), (1, 64)])
def test_population_equals_the_tapes_of_rollout_mlp_states(M, E, H):
    """Lander3D, float32 storage, low explicit starts: (M, E) = (4, 64); (3, 128), where indexing by tile in place of by
    env would pick the wrong member; (1, 64), the shared-theta kernel itself.  K in {1, 24}, gamma in {1, 0.97}."""
    rng = np.random.default_rng(zlib.crc32(repr((M, E, H)).encode()))
    n = M * E
    env = _env("lander3d", n, "float32", seed=5)
    try:
        env.reset()
        x0, st = _low_starts(n, rng)
        state = {"x": x0, "status": st}
        table = _table("lander3d", M, H, rng)
        for K in (1, 24):
            for gamma in (1.0, 0.97):
                _check_population("lander3d M %d E %d H %d K %d gamma %g" % (M, E, H, K, gamma), env, table, K, H, E,
                                  gamma, state)
    finally:
        env.close()


@pytest.mark.parametrize("task,mode,substeps", [("hover3d", "float32", 1), ("lander2d", "float32", 10),
                                                 ("hover1d", "float32", 1), ("lander3d", "float32_rn", 1),
                                                 ("lander3d", "float64", 1)])
def test_population_on_the_other_tasks_and_storage_modes(task, mode, substeps):
    """Hover3D, Lander2D x 10 substeps (ten physics calls of a tenth of the step's time), Hover1D; Lander3D in the other
    two storage modes.  M = 3, E = 128, K = 24, gamma = 0.97, H in {32, 0}; the same low explicit starts."""
    M, E, K = 3, 128, 24
    rng = np.random.default_rng(zlib.crc32(repr((task, mode, substeps)).encode()))
    n = M * E
    env = _env(task, n, mode, seed=6, substeps=substeps)
    try:
        env.reset()
        x0, st = _low_starts(n, rng)
        state = {"x": x0, "status": st}
        for H in (32, 0):
            _check_population("%s/%s/%d H %d" % (task, mode, substeps, H), env, _table(task, M, H, rng), K, H, E, 0.97,
                              state)
    finally:
        env.close()


def test_population_from_the_stored_start():
    """The stored start: low states installed with set_state (so that episodes end inside the horizon) with a pending
    explicit force, then the start of a fresh reset() -- its Philox perturbation pending, nobody near the ground."""
    M, E, K, H = 4, 64, 24, 32
    rng = np.random.default_rng(77)
    n = M * E
    env = _env("lander3d", n, "float32", seed=8)
    try:
        env.reset()
        table = _table("lander3d", M, H, rng)
        _check_population("stored start after reset()", env, table, K, H, E, 0.97, None, expect_events=False)
        x0, st = _low_starts(n, rng)
        env.set_state(x=x0, status=st, force=rng.uniform(-20, 20, (3, n)), flags=np.full(n, 1 | 4, np.uint8))
        _check_population("stored low starts", env, table, K, H, E, 0.97, None)
    finally:
        env.close()


@pytest.mark.parametrize("truncates", [True, False])
def test_population_with_a_time_limit(truncates):
    """A step limit of 20 inside the horizon of 24: the lanes that are still flying then are truncated (bit 1 of
    end_flags) or, without time_limit_truncates, terminated; nobody reaches K."""
    M, E, K, H = 4, 64, 24, 32
    rng = np.random.default_rng(78)
    n = M * E
    env = _env("lander3d", n, "float32", seed=8, max_steps=20, time_limit_truncates=truncates)
    try:
        env.reset()
        x0, st = _low_starts(n, rng)
        got, want, _ = _check_population("time limit, truncates %s" % truncates, env, _table("lander3d", M, H, rng), K, H,
                                         E, 0.97, {"x": x0, "status": st}, expect_events=False)
        flags, d = want[2], want[1]
        assert d.max() < K and (d < d.max()).sum() >= n // 8 and (d == d.max()).sum() >= n // 8
        at_limit = 2 if truncates else 1                  # (a lane that ends at the limit step by itself is terminated)
        assert (flags[d == d.max()] == at_limit).sum() >= n // 8 and np.all(flags[d < d.max()] == 1)
        assert np.all(d[flags == 2] == d.max()) and (truncates or not np.any(flags == 2))
    finally:
        env.close()


def test_population_with_next_step_resets_pending():
    """A next_step env with resets pending at the start: those lanes reset in step 1 (reward 0, no flag) and go on with
    the new episode, as in rollout_mlp_states."""
    M, E, K, H = 8, 128, 16, 16
    n = M * E
    rng = np.random.default_rng(41)
    env = _env("lander3d", n, "float32", autoreset="next_step", seed=13)
    try:
        env.reset()
        pend = np.zeros(n, bool)
        for _ in range(300):
            _, _, term, trunc, _ = env.step(_dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env))
            pend = to_np(term | trunc).astype(bool)
            if pend.sum() >= 32:
                break
        assert pend.sum() >= 8
        table = _table("lander3d", M, H, rng)
        airborne = (env.get_state()["status"] == AIRBORNE) & ~pend
        got, want, tapes = _check_population("next_step resets", env, table, K, H, E, 0.97, None, expect_events=False,
                                             airborne=airborne)
        assert np.all(tapes["reward"][0, pend] == 0.0) and np.all(want[1][pend] > 1)
        assert np.isfinite(to_np(got[0])[pend]).all()
    finally:
        env.close()


def test_population_has_no_side_effects():
    M, E, K, H = 4, 64, 24, 32
    n = M * E
    rng = np.random.default_rng(23)
    envs = [_env("lander3d", n, "float32", autoreset="next_step", seed=3) for _ in range(2)]
    try:
        for e in envs:
            e.reset()
        warm = _dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), envs[0])
        for e in envs:
            e.step(warm)
        env, twin = envs
        before = env.get_state()
        table = _dev(_table("lander3d", M, H, rng), env)
        env.rollout_mlp_population(table, K, H, E, 0.97)
        x0, st = _low_starts(n, rng)
        env.rollout_mlp_population(table, K, H, E, 1.0, start_x=x0)
        w = env.es_perturb(table[0], 0.01, M, 1)
        env.es_gradient(_dev(rng.standard_normal(M), env), 1, int(w.shape[1]))
        after = env.get_state()
        assert set(before) == set(after)
        for k in before:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), k
        for _ in range(3):
            a = _dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env)
            for u, v in zip(env.step(a)[:4], twin.step(a)[:4]):
                assert np.array_equal(to_np(u), to_np(v))
    finally:
        for e in envs:
            e.close()


@pytest.mark.parametrize("variant,task,mode", [("mars_gyro", "lander3d", "float32"), ("vehicles", "lander3d", "float64")])
def test_population_under_model_variants(variant, task, mode):
    """The comparison under two non-default vehicle models (the rotor-gyro branch of rollout_step with the lift law; the
    per-env coefficient load), on the condition that the default model gives another return in every airborne lane."""
    M, E, K, H = 3, 128, 24, 32
    n = M * E
    rng = np.random.default_rng(zlib.crc32(repr((variant, task, mode)).encode()))
    installed = model_variants.draw(variant, rng, n)
    x0, st = _low_starts(n, rng)
    state = {"x": x0, "status": st}
    table = _table(task, M, H, rng, ah=model_variants.hover(variant))
    env = _env(task, n, mode, seed=9, **model_variants.env_kwargs(variant))
    try:
        model_variants.install_same(env, installed)
        env.reset()
        got, _, _ = _check_population("%s %s/%s" % (variant, task, mode), env, table, K, H, E, 0.97, state)
    finally:
        env.close()
    ref = _env(task, n, mode, seed=9)
    try:
        ref.reset()
        assert not ref.config.rotor_gyro and ref.config.thrust_model == 0
        plain = ref.rollout_mlp_population(_dev(table, ref), K, H, E, 0.97, state=state).returns
        same = to_np(plain).view(np.uint64) == to_np(got[0]).view(np.uint64)
        assert not np.any(same & (st == AIRBORNE)), (variant, int(same.sum()))
    finally:
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the mirrored population
# ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(to_np(a), dtype=np.float32).view(np.uint32)


def test_perturb_equals_the_restatement_bit_for_bit():
    seed, nonce = 17, 5
    rng = np.random.default_rng(3)
    env = _env("lander3d", 64, "float32", seed=seed)
    try:
        for H in (0, 1, 33, 64):
            P = _num_params("hover3d", H)                                # (H = 64: 1092, the largest policy)
            theta = rng.standard_normal(P).astype(np.float32)
            for M in (2, 10):
                for sigma, base in ((0.05, 0), (1.5, (1 << 32) - 2)):
                    got = env.es_perturb(_dev(theta, env), sigma, M, nonce, pair_base=base)
                    assert tuple(got.shape) == (M, P)
                    assert np.array_equal(_bits(got), _bits(es_ref.perturb(theta, sigma, M, seed, nonce, base))), (H, M)
        theta = rng.standard_normal(44).astype(np.float32)
        th = _dev(theta, env)
        ten = env.es_perturb(th, 0.1, 10, nonce).clone()
        assert np.all(_bits(ten[0::2]) != _bits(ten[1::2]), axis=1).all() and len(np.unique(_bits(ten), axis=0)) == 10
        # pair_base shifts the members: the pairs of (base 3, M 4) are pairs 3 and 4 of (base 0, M 10)
        four = env.es_perturb(th, 0.1, 4, nonce, pair_base=3).clone()
        assert np.array_equal(_bits(four), _bits(ten[6:10]))
        # another nonce, another seed: other noise; sigma = 0: every row is theta
        other = env.es_perturb(th, 0.1, 10, nonce + 1).clone()
        assert np.mean(_bits(other) == _bits(ten)) < 0.01
        env.seed(seed + 1)
        assert np.array_equal(_bits(env.es_perturb(th, 0.1, 10, nonce)), _bits(es_ref.perturb(theta, 0.1, 10, seed + 1, nonce)))
        assert np.array_equal(_bits(env.es_perturb(th, 0.0, 10, nonce)), _bits(np.tile(theta, (10, 1))))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the search gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 10, 64, 66, 200, 4096])
def test_gradient_equals_the_restatement(M):
    """M = 2; one chunk of 32 pairs exactly, and one pair more; several chunks; 64 chunks.  Against es_ref.gradient in
    longdouble within (2M + 64) 2^-53 sum|terms| per parameter (M/2 differences, products and sums, and the chunk sums:
    any order is inside it); the float64 restatement in the kernel's order gives the same bits."""
    import torch
    seed, nonce, base = 23, (1 << 32) - 1, 7
    rng = np.random.default_rng(M)
    env = _env("lander3d", 64, "float32", seed=seed)
    try:
        for P in (1092, 44, 1):
            w = rng.standard_normal(M)
            g = env.es_gradient(_dev(w, env), nonce, P, pair_base=base)
            first = g.clone()
            assert first.dtype == torch.float64 and tuple(first.shape) == (P,)
            want, mag = es_ref.gradient(w, P, seed, nonce, base, dtype=np.longdouble)
            err = np.abs(to_np(first).astype(np.longdouble) - want).astype(np.float64)
            assert np.all(err <= (2 * M + 64) * 2.0 ** -53 * mag), (M, P, float((err / mag).max()))
            assert np.array_equal(to_np(first), es_ref.gradient(w, P, seed, nonce, base)[0])
            g.fill_(float("nan"))                                        # written, not accumulated
            again = env.es_gradient(_dev(w, env), nonce, P, pair_base=base)
            assert again.data_ptr() == g.data_ptr() and torch.equal(again, first)
            # equal weights within each pair: exactly zero
            same = np.repeat(rng.standard_normal(M // 2), 2)
            zero = env.es_gradient(_dev(same, env), nonce, P, pair_base=base)
            assert torch.equal(zero, torch.zeros_like(zero)) and not torch.signbit(zero).any()
        # the gradient of a table's own noise: w = (+1, -1) per pair gives 2 sum_i eps_i
        P = 44
        w = np.tile([1.0, -1.0], M // 2)
        g = to_np(env.es_gradient(_dev(w, env), nonce, P, pair_base=base))
        eps = es_ref.pair_noise(seed, nonce, M // 2, P, base).astype(np.float64)
        assert np.allclose(g, 2 * eps.sum(0), rtol=0, atol=1e-9)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the driver
# ---------------------------------------------------------------------------------------------------------------------
DRIVER = dict(task="lander3d", H=16, pairs=64, E=64, K=64, iterations=30, sigma=0.002, lr=0.001)


def driver_problem(env_seed=2):
    """Lander3D: 64 common start points 0.6-1.1 m up, descending at 2.5-3.5 m/s, slightly off the centre.  The initial policy
    -- mlp.init with the hover motor value as its output bias and a small output layer -- holds hover thrust, arrives far
    above the landing limit and crashes everywhere (asserted)."""
    import torch
    from gym_copter_amd import mlp
    rng = np.random.default_rng(5)
    E = DRIVER["E"]
    x0 = np.zeros((12, E))
    x0[0], x0[2] = rng.uniform(-0.5, 0.5, (2, E))
    x0[4] = -rng.uniform(0.6, 1.1, E)
    x0[5] = rng.uniform(2.5, 3.5, E)
    gen = torch.Generator().manual_seed(11)
    theta0 = mlp.init(10, 4, DRIVER["H"], generator=gen, out_bias=float(AH), out_scale=0.01)
    return x0, theta0


def evaluate(env, theta, x0):
    """theta itself on the common starts: (mean return, landed share, crashed share), every member the same policy."""
    d = DRIVER
    M = 2 * d["pairs"]
    pop = env.rollout_mlp_population(theta.to(env.device)[None, :].repeat(M, 1), d["K"], d["H"], d["E"], 1.0,
                                     start_x=np.tile(x0, (1, M)))
    status = to_np(pop.end_status)[:d["E"]]
    return float(to_np(pop.member_returns)[0]), float(np.mean(status == LANDED)), float(np.mean(status == CRASHED))


def test_es_driver_improves_the_landers_return():
    """gym_copter_amd.es on the descent above: 64 pairs x 64 envs, K = 64, H = 16, sigma = 0.002, lr = 0.001, 30
    iterations.  The returned history is what the calls produce (iteration 0 recomputed here), theta moved, and the mean
    return of theta itself on the 64 starts rises by at least DRIVER_BAR.  The trajectory is printed.  Measured on an
    MI355X: the initial policy crashes everywhere, return 12.21; after 30 iterations 117.64 with
    67.2 % of the starts landed and none crashed; the population mean went 21.35 -> 88.21."""
    import gym_copter_amd
    d = DRIVER
    M = 2 * d["pairs"]
    env = _env(d["task"], M * d["E"], "float32", seed=2)
    try:
        env.reset()
        x0, theta0 = driver_problem()
        r0, landed0, crashed0 = evaluate(env, theta0, x0)
        assert crashed0 == 1.0, (r0, landed0, crashed0)
        res = gym_copter_amd.es(env, theta0, d["H"], d["K"], d["pairs"], d["sigma"], d["lr"], d["iterations"],
                                envs_per_member=d["E"], start_x=x0)
        hist = to_np(res.history)
        r1, landed1, crashed1 = evaluate(env, res.params, x0)
        print("es driver: initial policy return %.3f (landed %.0f %%, crashed %.0f %%); after %d iterations %.3f (landed "
              "%.0f %%, crashed %.0f %%); population mean per iteration %s"
              % (r0, 100 * landed0, 100 * crashed0, d["iterations"], r1, 100 * landed1, 100 * crashed1,
                 " ".join("%.2f" % v for v in hist)))
        assert hist.shape == (d["iterations"],) and np.isfinite(hist).all()
        assert tuple(res.params.shape) == tuple(theta0.shape) and not np.array_equal(to_np(res.params), to_np(theta0))
        # iteration 0 of the history is what the calls produce
        table = env.es_perturb(theta0.to(env.device), d["sigma"], M, 0)
        pop = env.rollout_mlp_population(table, d["K"], d["H"], d["E"], 1.0, start_x=np.tile(x0, (1, M)))
        assert float(to_np(pop.member_returns.mean())) == hist[0]
        assert r1 - r0 >= DRIVER_BAR, (r0, r1)
    finally:
        env.close()


# half the improvement of the mean return measured on this problem (12.21 -> 117.64): half, because
# the noise and Adam's path make the endpoint vary
DRIVER_BAR = 0.5 * (117.64 - 12.21)


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib
    M, E, K, H = 2, 64, 4, 8
    n = M * E
    rng = np.random.default_rng(2)
    env = _env("lander3d", n, "float64", seed=1)
    try:
        env.reset()
        table = _dev(_table("lander3d", M, H, rng), env)
        x0, st = _low_starts(n, rng)
        good = dict(table=table, K=K, hidden=H, envs_per_member=E)
        for kw, match in ((dict(envs_per_member=32), "multiple of 64"), (dict(envs_per_member=96), "multiple of 64"),
                          (dict(envs_per_member=128), "is not num_envs"), (dict(table=table[:1]), "is not num_envs"),
                          (dict(table=table.double()), "table must be"), (dict(table=table[:, :-1]), "table must be"),
                          (dict(table=to_np(table)), "table must be"), (dict(hidden=65), "hidden must be"),
                          (dict(hidden=9), "table must be"), (dict(K=0), "K must be"), (dict(K=2.0), "K must be"),
                          (dict(gamma=float("nan")), "gamma must be"), (dict(start_status=st), "start_x is required"),
                          (dict(start_x=x0[:, :-1]), "must have shape"),
                          (dict(start_x=x0, state={"x": x0, "status": st}), "not both")):
            args = dict(good)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_mlp_population(**args)
        theta = table[0]
        for kw, match in ((dict(members=3), "members must be"), (dict(members=0), "members must be"),
                          (dict(members=65538), "members must be"), (dict(sigma=-1.0), "sigma must be"),
                          (dict(sigma=float("inf")), "sigma must be"), (dict(nonce=-1), "nonce must be"),
                          (dict(nonce=1 << 32), "nonce must be"), (dict(pair_base=1 << 32), "pair_base must be"),
                          (dict(params=theta.double()), "params must be"), (dict(params=table), "params must be"),
                          (dict(params=torch.zeros(1093)), "num_params must be")):
            args = dict(params=theta, sigma=0.1, members=4, nonce=0)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.es_perturb(**args)
        w = _dev(rng.standard_normal(4), env)
        for kw, match in ((dict(weights=w[:3]), "members must be"), (dict(weights=w.float()), "weights must be"),
                          (dict(weights=to_np(w)), "weights must be"), (dict(num_params=0), "num_params must be"),
                          (dict(num_params=1093), "num_params must be"), (dict(nonce=0.5), "nonce must be")):
            args = dict(weights=w, nonce=0, num_params=10)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.es_gradient(**args)
        # the C ABI with a live context: N != M E is CS_ERR_ARG, a wrong struct_size CS_ERR_ABI
        returns = torch.empty(n, dtype=torch.float64, device=env.device)
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), K
        pio = _lib.RolloutPopulationIO()
        pio.struct_size, pio.hidden, pio.members, pio.envs_per_member, pio.gamma = C.sizeof(pio), H, M, E, 1.0
        pio.params_table_dev, pio.returns_dev = table.data_ptr(), returns.data_ptr()
        fn = env._lib.cs_rollout_mlp_population
        for m, e in ((M + 1, E), (M, 2 * E), (1, E)):
            pio.members, pio.envs_per_member = m, e
            assert fn(env._ctx, C.byref(io), C.byref(pio), None) == _lib.ERR_ARG
            assert b"is not the context's 128 envs" in env._lib.cs_last_error()
        pio.members, pio.envs_per_member = M, E
        assert fn(env._ctx, C.byref(io), C.byref(pio), None) == 0              # the optional outputs may all be NULL
        want = env.rollout_mlp_population(table, K, H, E).returns
        assert torch.equal(returns.view(torch.int64), want.view(torch.int64))
        pio.struct_size += 8
        assert fn(env._ctx, C.byref(io), C.byref(pio), None) == _lib.ERR_ABI
        eio = _lib.EsIO()
        eio.struct_size = C.sizeof(eio) + 8
        assert env._lib.cs_es_perturb(env._ctx, C.byref(eio), None) == _lib.ERR_ABI
        assert env._lib.cs_es_gradient(env._ctx, C.byref(eio), None) == _lib.ERR_ABI
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_mlp_population(table, K, H, E)
            with pytest.raises(CopterStepError, match="serv"):
                env.es_perturb(theta, 0.1, 4, 0)
            with pytest.raises(CopterStepError, match="serv"):
                env.es_gradient(w, 0, 10)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_mlp_population(table, K, H, E)
    with pytest.raises(RuntimeError, match="closed"):
        env.es_perturb(theta, 0.1, 4, 0)
    with pytest.raises(RuntimeError, match="closed"):
        env.es_gradient(w, 0, 10)
