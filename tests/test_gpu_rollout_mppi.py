"""cs_rollout_mppi_costs / cs_rollout_mppi_update on the GPU: the costs against the existing
rollout_states fed the sample actions tests/mppi_ref.py rebuilds; the update against mppi_ref on the kernel's own costs;
determinism, shard invariance, no side effects; the mppi driver; plumbing.  The costs also under the non-default vehicle
models of tests/model_variants.py."""
import zlib

import numpy as np
import pytest

import model_variants
import mppi_ref
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASKS = ["lander3d", "hover3d", "lander2d", "lander1d", "hover2d", "hover1d"]
TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover1d": 1, "lander1d": 1, "hover2d": 2}
AH = hover_action()


def _env(task, n, mode="float64", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _random_point(n, rng, low=False):
    """Airborne starts at 5-20 m: 16 steps are 0.16 s, in which an env falls less than 1 m, turns less than 0.2 rad and
    drifts less than 0.4 m, so no sample of the main comparison can touch down, tilt out or leave the bounds (asserted
    where it is used).  low=True: 0.05-1.5 m up and descending, so that many samples touch down or crash."""
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    x[1], x[3], x[5] = rng.uniform(-2, 2, (3, n))
    x[4] = rng.uniform(-20, -5, n)
    x[6], x[8] = rng.uniform(-0.4, 0.4, (2, n))
    x[10] = rng.uniform(-1, 1, n)
    x[7], x[9], x[11] = rng.uniform(-1, 1, (3, n))
    if low:
        x[4] = rng.uniform(-1.5, -0.05, n)
        x[5] = rng.uniform(0.0, 4.0, n)
        x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    return x, np.full(n, AIRBORNE, np.uint8)


def _cost_model(rng, A, n, K=None):
    m = rng.standard_normal((12, 12))
    Q = m @ m.T / 12 + 0.1 * np.eye(12)
    m = rng.standard_normal((12, 12))
    Qf = m @ m.T / 12 + 0.5 * np.eye(12)
    m = rng.standard_normal((A, A))
    R = m @ m.T / A                                         # (positive semidefinite is enough here)
    shape = (n, 12) if K is None else (K, n, 12)
    x_ref = rng.standard_normal(shape)
    x_ref[..., 4] -= 10.0
    return Q, Qf, R, x_ref, rng.uniform(0.3, 0.7, A)


def _check_costs(name, env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, wr, stream, state, samples, ids, seed,
                 expect_quiet=True):
    """costs[p] against S evaluated in NumPy on rollout_states(a(p)), a(p) rebuilt by mppi_ref.  The bar per env is
    max(100 x |S_float64 - S_longdouble|, T 2^-52 M): DESIGN section 13's rule (a multiple of the float64 reference's
    own error) with the floor mppi_ref.cost_magnitude derives (any summation order of the T elementary products, whose
    absolute values sum to M, is within (T - 1) 2^-53 M of the exact sum; twice that, because both sides round).
    Prints and returns the worst ratio error / bar."""
    res = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, reward_weight=wr, stream=stream,
                                 state=state)
    costs, best = to_np(res.costs).copy(), to_np(res.best).copy()
    assert costs.shape == (P, env.num_envs) and best.dtype == np.int32
    worst, events = 0.0, 0
    for p in samples:
        a = mppi_ref.sample_actions(to_np(abar), sigma, seed, ids, stream, p)
        ro = env.rollout_states(_dev(a, env), state)
        x, rew = to_np(ro.x), to_np(ro.reward)
        events += int(to_np(ro.terminated | ro.truncated).any(axis=0).sum())
        kw = dict(Q_final=Qf, a_ref=a_ref, reward_weight=wr)
        S = mppi_ref.cost(x, rew, a, x_ref, Q, R, **kw)
        Sl = mppi_ref.cost(x, rew, a, x_ref, Q, R, dtype=np.longdouble, **kw)
        T, M = mppi_ref.cost_magnitude(x, rew, a, x_ref, Q, R, **kw)
        bar = np.maximum(100 * np.abs(S - Sl).astype(np.float64), T * 2.0 ** -52 * M)
        fin = np.isfinite(S)
        assert np.array_equal(np.isfinite(costs[p]), fin), (name, p)
        ratio = np.abs(costs[p][fin] - S[fin]) / bar[fin]
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        assert np.all(ratio <= 1.0), (name, p, float(ratio.max()))
    if expect_quiet:
        assert events == 0, (name, events)
    assert np.array_equal(best, mppi_ref.best(costs)), name
    print("%s: worst |costs - S| / bar %.3g over samples %s (%d finished envs)" % (name, worst, list(samples), events))
    return costs, events


# ---------------------------------------------------------------------------------------------------------------------
# 1. the action tape and the cost
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("mode", ["float32", "float32_rn", "float64"])
@pytest.mark.parametrize("task", TASKS)
def test_costs_equal_the_cost_of_rollout_states_on_the_sample_actions(task, mode, substeps):
    """N = 300 (a partial wavefront), K = 16, P = 7, both start forms: the stored start right after reset() (its
    perturbation pending) and an explicit one; x_ref per env and per step; samples 0, 3 and P - 1; the Landers with
    their reward in the cost.  costs[0] is the cost of rollout_states(actions)."""
    n, K, P, A = 300, 16, 7, TASK_A[task]
    seed, base = 21, 1000
    rng = np.random.default_rng(TASKS.index(task) * 10 + substeps)
    env = _env(task, n, mode, substeps=substeps, seed=seed, env_id_base=base)
    try:
        env.reset()
        ids = base + np.arange(n)
        abar = _dev((AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32), env)
        sigma = (0.05 * AH * rng.uniform(0.5, 2.0, A)).astype(np.float32)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        wr = 0.5 if "lander" in task else 0.0
        _check_costs("%s/%s/%d stored" % (task, mode, substeps), env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, wr, 3,
                     None, (0, 3, P - 1), ids, seed, expect_quiet=False)
        x0, st = _random_point(n, rng)
        state = {"x": x0, "status": st, "force": rng.uniform(-1, 1, (3, n))}
        _, _, _, x_ref_k, _ = _cost_model(rng, A, n, K)
        _check_costs("%s/%s/%d explicit" % (task, mode, substeps), env, abar, sigma, P, x_ref_k, Q, R, None, None, wr,
                     (1 << 32) - 1, state, (0, 1, P - 1), ids, seed)
    finally:
        env.close()


VARIANT_COST_CASES = [("mars_gyro", "lander3d", "float32", 1), ("mars_gyro", "hover3d", "float64", 1),
                      ("vehicles", "lander2d", "float32_rn", 10), ("vehicles_mars_gyro", "lander3d", "float64", 1),
                      ("act_f32", "lander3d", "float32", 1)]


VARIANT_N, VARIANT_K, VARIANT_P, VARIANT_SEED, VARIANT_BASE, VARIANT_STREAM = 300, 16, 7, 21, 1000, (1 << 32) - 1


def _variant_problem(variant, task, mode, substeps):
    """the generator of a case under a model variant and what it draws first: the per-env table, the nominal tape
    centred on the variant's hover value, sigma and the 5-20 m explicit start.  tests/test_rollout_mppi_cpu.py replays
    samples 0, 3 and P - 1 of every case through VecOracle with the variant's model: no env terminates inside the
    horizon (the per-env vehicles hover within 0.6-1.5 x the value the tape is centred on, and 0.16 s at up to twice
    hover thrust leave the starts far from the ground, the bounds and the tilt limit)."""
    n, K, A = VARIANT_N, VARIANT_K, TASK_A[task]
    rng = np.random.default_rng(zlib.crc32(repr((variant, task, mode, substeps)).encode()))
    ah = model_variants.hover(variant)
    installed = model_variants.draw(variant, rng, n)
    abar = (ah * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32)
    sigma = (0.05 * ah * rng.uniform(0.5, 2.0, A)).astype(np.float32)
    x0, st = _random_point(n, rng)
    return rng, installed, abar, sigma, {"x": x0, "status": st, "force": rng.uniform(-1, 1, (3, n))}


@pytest.mark.parametrize("variant,task,mode,substeps", VARIANT_COST_CASES)
def test_costs_under_model_variants(variant, task, mode, substeps):
    """The comparison above under the non-default vehicle models of tests/model_variants.py (the rotor-gyro branch of the
    sample loop, its float32 motor law, the lift law, the per-env coefficient load): N = 300, K = 16, P = 7, both start
    forms, samples 0, 3 and P - 1, the same bar; no sample of the explicit start may terminate, and the nominal's x tape
    differs from the default model's in every lane."""
    n, K, P, A = VARIANT_N, VARIANT_K, VARIANT_P, TASK_A[task]
    seed, base = VARIANT_SEED, VARIANT_BASE
    rng, installed, a0, sigma, state = _variant_problem(variant, task, mode, substeps)
    env = _env(task, n, mode, substeps=substeps, seed=seed, env_id_base=base, **model_variants.env_kwargs(variant))
    try:
        model_variants.install_same(env, installed)
        env.reset()
        ids = base + np.arange(n)
        abar = _dev(a0, env)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        wr = 0.5 if "lander" in task else 0.0
        name = "%s %s/%s/%d" % (variant, task, mode, substeps)
        _check_costs(name + " stored", env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, wr, 3, None, (0, 3, P - 1), ids,
                     seed, expect_quiet=False)
        _, _, _, x_ref_k, _ = _cost_model(rng, A, n, K)
        _check_costs(name + " explicit", env, abar, sigma, P, x_ref_k, Q, R, None, None, wr, VARIANT_STREAM, state,
                     (0, 3, P - 1), ids, seed)
        model_variants.assert_differs_from_default(variant, env.rollout_states(abar, state).x, task, mode, substeps,
                                                   state, abar)
    finally:
        env.close()


def test_costs_with_next_step_resets_pending():
    """A next_step env (float32 storage) with resets pending at the start: those envs reset in step 1 and the new
    episode's perturbation enters step 2, in every sample as in rollout_states."""
    n, K, P, A, seed = 1024, 16, 5, 4, 13
    rng = np.random.default_rng(41)
    env = _env("lander3d", n, "float32", autoreset="next_step", seed=seed)
    try:
        env.reset()
        pend = np.zeros(n, bool)
        for _ in range(300):
            _, _, term, trunc, _ = env.step(_dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env))
            pend = to_np(term | trunc).astype(bool)
            if pend.sum() >= 32:
                break
        assert pend.sum() >= 8
        abar = _dev((AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32), env)
        sigma = np.full(A, 0.1 * AH, np.float32)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        costs, _ = _check_costs("next_step resets", env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, 1.0, 0, None, range(P),
                                np.arange(n), seed, expect_quiet=False)
        assert np.isfinite(costs[:, pend]).all()
    finally:
        env.close()


def test_costs_through_touchdowns_and_crashes():
    """Low, descending starts: many samples touch down or crash inside the horizon, differently from sample to sample
    (sigma is large).  Every sample's cost still is that of rollout_states, and best is NumPy's arg-min."""
    n, K, P, A, seed = 512, 16, 12, 4, 5
    rng = np.random.default_rng(8)
    for task, mode in (("lander3d", "float32"), ("hover3d", "float64")):
        env = _env(task, n, mode, seed=seed)
        try:
            env.reset()
            x0, st = _random_point(n, rng, low=True)
            state = {"x": x0, "status": st}
            abar = _dev((AH * rng.uniform(0.2, 1.2, (K, n, A))).astype(np.float32), env)
            sigma = np.full(A, 0.5 * AH, np.float32)
            Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
            costs, events = _check_costs("%s low starts" % task, env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, 1.0, 9,
                                         state, range(P), np.arange(n), seed, expect_quiet=False)
            ro = env.rollout_states(abar, state)
            final = to_np(ro.status)[-1]
            print("  nominal plan: %d crashed, %d landed, %d airborne of %d" % ((final == CRASHED).sum(),
                  (final == LANDED).sum(), (final == AIRBORNE).sum(), n))
            assert events > 0 and (final == CRASHED).sum() > 10 and (final != CRASHED).sum() > 10
            assert len(np.unique(to_np(env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, state=state).best))) > 3
        finally:
            env.close()


def test_costs_through_touchdowns_and_crashes_under_per_env_mars_vehicles():
    """The low, descending starts above under vehicles_mars_gyro (Lander3D, float32 storage): crashes and landings under
    per-env coefficients, the lift law and the rotor-gyro term."""
    variant, task, mode = "vehicles_mars_gyro", "lander3d", "float32"
    n, K, P, A, seed = 512, 16, 12, 4, 5
    rng = np.random.default_rng(88)
    ah = model_variants.hover(variant)
    env = _env(task, n, mode, seed=seed, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        x0, st = _random_point(n, rng, low=True)
        state = {"x": x0, "status": st}
        abar = _dev((ah * rng.uniform(0.2, 1.2, (K, n, A))).astype(np.float32), env)
        sigma = np.full(A, 0.5 * ah, np.float32)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        costs, events = _check_costs("%s %s low starts" % (variant, task), env, abar, sigma, P, x_ref, Q, R, Qf, a_ref,
                                     1.0, 9, state, range(P), np.arange(n), seed, expect_quiet=False)
        ro = env.rollout_states(abar, state)
        final = to_np(ro.status)[-1]
        print("  nominal plan: %d crashed, %d landed, %d airborne of %d" % ((final == CRASHED).sum(),
              (final == LANDED).sum(), (final == AIRBORNE).sum(), n))
        assert events > 0 and (final == CRASHED).sum() > 10 and (final != CRASHED).sum() > 10
        model_variants.assert_differs_from_default(variant, ro.x, task, mode, 1, state, abar)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the update
# ---------------------------------------------------------------------------------------------------------------------
def _ulps(got, want, scale):
    """|got - want| in float32 ulps of max(|want|, scale): the rounding of fl32(abar + delta) is relative to the larger of
    the two operands and the result; the float64 sums behind delta are ~1e-9 ulp."""
    ulp = np.spacing(np.maximum(np.abs(want), np.abs(scale)).astype(np.float32))
    return float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp))


@pytest.mark.parametrize("task,mode", [("lander3d", "float32"), ("hover2d", "float64"), ("lander1d", "float32_rn")])
def test_update_equals_the_restatement_on_the_kernels_costs(task, mode):
    import torch
    n, K, P, A, seed, base, stream = 300, 16, 37, TASK_A[task], 17, (1 << 32) - 300, 6
    rng = np.random.default_rng(70 + A)
    env = _env(task, n, mode, seed=seed, env_id_base=base)
    try:
        env.reset()
        ids = base + np.arange(n)
        x0, st = _random_point(n, rng)
        state = {"x": x0, "status": st}
        a0 = (AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32)
        a0[:, :8] = rng.uniform(-0.2, 1.2, (K, 8, A))                # (some actions outside [0, 1]: the result is clipped)
        abar = _dev(a0, env)
        sigma = (0.1 * AH * rng.uniform(0.5, 2.0, A)).astype(np.float32)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        costs = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, stream=stream,
                                       state=state).costs.clone()
        assert bool(torch.isfinite(costs).all())
        spread = float(costs.std(dim=0).median())               # (a temperature on the scale of the costs' differences)
        # injected non-finite costs: envs 0-3 some, env 4 all of them, env 5 all but one
        costs[1, 0], costs[P - 1, 1], costs[0, 2] = float("inf"), float("nan"), float("-inf")
        costs[::2, 3] = float("nan")
        costs[:, 4] = torch.tensor([float("nan"), float("inf")] * P, device=env.device)[:P].double()
        costs[:, 5] = float("inf")
        costs[11, 5] = 3.0
        ch = to_np(costs)
        for lam in (spread, 0.1 * spread):
            up = env.rollout_mppi_update(abar, costs, sigma, lam, stream=stream)
            got, ess, cmin = to_np(up.actions).copy(), to_np(up.ess).copy(), to_np(up.cost_min).copy()
            want, wess, wmin = mppi_ref.update(a0, ch, sigma, lam, seed, ids, stream)
            u = _ulps(got, want, a0)
            live = np.arange(n) != 4
            rel = float(np.max(np.abs(ess[live] / wess[live] - 1)))
            print("%s lam %.3g: actions within %.2f ulp, ess within %.2e relative; ess median %.1f of %d"
                  % (task, lam, u, rel, np.median(ess), P))
            assert u <= 2.0 and rel <= 1e-12 and np.array_equal(cmin, wmin)
            assert got[:, live].min() >= 0.0 and got[:, live].max() <= 1.0
            assert np.array_equal(got[:, 4].view(np.uint32), a0[:, 4].view(np.uint32))       # all non-finite: the input bits
            assert ess[4] == 0.0 and cmin[4] == np.inf
            assert ess[5] == 1.0 and cmin[5] == 3.0
            assert _ulps(got[:, 5], np.clip(mppi_ref.sample_actions(a0, sigma, seed, ids, stream, 11)[:, 5], 0, 1),
                         a0[:, 5]) <= 2.0
            again = env.rollout_mppi_update(abar, costs, sigma, lam, stream=stream)
            for s, t in zip(again, (got, ess, cmin)):
                assert np.array_equal(to_np(s).view(np.uint8), t.view(np.uint8))          # the same bits on every call
        # lambda -> large: every finite sample weighs 1 exactly (exp(-tiny) rounds to 1): the plain mean
        clean = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, stream=stream,
                                       state=state).costs.clone()
        up = env.rollout_mppi_update(abar, clean, sigma, 1e30, stream=stream)
        pert = sum(mppi_ref.perturbation(sigma, seed, ids, stream, K, p, A).astype(np.float64) for p in range(P)) / P
        mean = np.clip((a0.astype(np.float64) + pert).astype(np.float32), 0, 1)
        assert _ulps(to_np(up.actions), mean, a0) <= 2.0 and np.all(to_np(up.ess) == P)
        # lambda -> small: the best sample's tape
        up = env.rollout_mppi_update(abar, clean, sigma, 1e-12, stream=stream)
        best = mppi_ref.best(to_np(clean))
        tape = np.stack([mppi_ref.sample_actions(a0[:, i:i + 1], sigma, seed, ids[i:i + 1], stream, int(best[i]))[:, 0]
                         for i in range(n)], axis=1)
        assert _ulps(to_np(up.actions), np.clip(tape, 0, 1), a0) <= 2.0 and np.all(to_np(up.ess) == 1.0)
        assert np.array_equal(to_np(up.cost_min), to_np(clean).min(axis=0))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. determinism, invariance, no side effects
# ---------------------------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_the_batch_split_and_of_P():
    import torch
    n, K, P, A, seed = 300, 16, 9, 4, 4
    rng = np.random.default_rng(15)
    x0, st = _random_point(n, rng)
    a0 = (AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32)
    Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
    sigma = 0.1 * AH

    def run(lo, hi, samples=P, stream=2, base=0):
        env = _env("lander3d", hi - lo, "float32", seed=seed, env_id_base=base + lo)
        try:
            env.reset()
            state = {"x": x0[:, lo:hi], "status": st[lo:hi]}
            acts = _dev(a0[:, lo:hi], env)
            kw = dict(Q_final=Qf, a_ref=a_ref, reward_weight=0.3, stream=stream, state=state)
            c = env.rollout_mppi_costs(acts, sigma, samples, x_ref[lo:hi], Q, R, **kw)
            c = type(c)(*(t.clone() for t in c))
            c2 = env.rollout_mppi_costs(acts, sigma, samples, x_ref[lo:hi], Q, R, **kw)
            assert torch.equal(c.costs.view(torch.int64), c2.costs.view(torch.int64)) and torch.equal(c.best, c2.best)
            up = env.rollout_mppi_update(acts, c.costs, sigma, 2.0, stream=stream)
            return to_np(c.costs), to_np(up.actions).copy(), to_np(up.ess).copy()
        finally:
            env.close()
    whole = run(0, n)
    for lo, hi in ((0, 128), (128, 300), (37, 101)):
        part = run(lo, hi)
        assert np.array_equal(part[0], whole[0][:, lo:hi]) and np.array_equal(part[1], whole[1][:, lo:hi])
        assert np.array_equal(part[2], whole[2][lo:hi])
    assert np.array_equal(run(0, n, samples=4)[0], whole[0][:4])          # the first samples of a larger P
    other = run(0, n, stream=3)
    assert np.array_equal(other[0][0], whole[0][0]) and np.all(other[0][1:] != whole[0][1:])   # sample 0 has no noise
    shifted = run(0, n, base=1)
    assert np.array_equal(shifted[0][0], whole[0][0]) and np.all(shifted[0][1:] != whole[0][1:])
    assert not np.array_equal(shifted[1], whole[1])                      # (other global ids: other noise)


def test_no_side_effects():
    n, K, P, A = 300, 8, 6, 4
    rng = np.random.default_rng(23)
    envs = [_env("lander3d", n, "float32", autoreset="next_step", seed=3) for _ in range(2)]
    try:
        for e in envs:
            e.reset()
        warm = _dev(rng.uniform(0, 1, (n, A)).astype(np.float32), envs[0])
        for e in envs:
            e.step(warm)
        env, twin = envs
        before = env.get_state()
        abar = _dev((AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32), env)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        c = env.rollout_mppi_costs(abar, 0.05, P, x_ref, Q, R, Q_final=Qf, reward_weight=1.0, stream=1)
        env.rollout_mppi_update(abar, c.costs, 0.05, 1.0, stream=1)
        after = env.get_state()
        assert set(before) == set(after)
        for k in before:
            assert np.array_equal(np.asarray(before[k]), np.asarray(after[k]), equal_nan=True), k
        for _ in range(3):
            a = _dev(rng.uniform(0, 1, (n, A)).astype(np.float32), env)
            for u, v in zip(env.step(a)[:4], twin.step(a)[:4]):
                assert np.array_equal(to_np(u), to_np(v))
    finally:
        for e in envs:
            e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the driver
# ---------------------------------------------------------------------------------------------------------------------
def _tracking(rng, n):
    """DESIGN section 13's application: starts near 5 m, a setpoint 1 m above the start, velocity and rate weights."""
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-0.5, 0.5, (2, n))
    x[4] = -5.0 + rng.uniform(-0.5, 0.5, n)
    x[5] = rng.uniform(-1.0, 1.0, n)
    x = x.astype(np.float32).astype(np.float64)
    x_ref = np.zeros((n, 12))
    x_ref[:, 0], x_ref[:, 2], x_ref[:, 4] = x[0], x[2], x[4] - 1.0            # (z points down)
    Q = np.diag([1.0, 0.1, 1.0, 0.1, 1.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    return x, x_ref, Q, np.eye(4)


def test_mppi_on_hover3d_tracking():
    """4 096 Hover3D envs, K = 64, from constant hover motors, the setpoint 1 m above the start: test_gpu_rollout_lqr's
    application with the same starts.  Every env's cost history is non-increasing (exact: a candidate is taken only
    where it is cheaper) and the batch mean strictly decreases; the final cost is that of rollout_states on the
    result.  No improvement ratio is required; the trajectory is printed.  Measured: 34.66 -> 28.64
    after 8 iterations, at a median effective sample size of 1.0."""
    import torch
    import gym_copter_amd
    from gym_copter_amd.ilqr import tracking_cost
    n, K, iters = 4096, 64, 8
    rng = np.random.default_rng(61)
    env = _env("hover3d", n, "float32", seed=1)
    try:
        env.reset()
        x0, x_ref, Q, R = _tracking(rng, n)
        state = {"x": _dev(x0, env), "status": np.full(n, AIRBORNE, np.uint8)}
        a0 = torch.full((K, n, 4), float(np.float32(AH)), dtype=torch.float32, device=env.device)
        res = gym_copter_amd.mppi(env, a0, x_ref, Q, R, a_ref=AH, samples=256, sigma=0.02, lam=0.5, iters=iters,
                                  state=state)
        hist, ess = to_np(res.cost), to_np(res.ess)
        assert hist.shape == (iters + 1, n) and ess.shape == (iters, n) and np.isfinite(hist).all()
        assert res.actions.shape == (K, n, 4) and res.actions.dtype == torch.float32
        print("hover3d tracking, MPPI P = 256: batch-mean cost per iteration %s; median ess %s"
              % (" ".join("%.4f" % v for v in hist.mean(axis=1)), " ".join("%.1f" % v for v in np.median(ess, axis=1))))
        assert np.all(hist[1:] <= hist[:-1])
        assert np.all(np.diff(hist.mean(axis=1)) < 0)
        assert np.all((ess >= 1.0) & (ess <= 256.0))
        check = env.rollout_states(res.actions, state)
        want = tracking_cost(check.x, res.actions, _dev(x_ref, env), torch.tensor(AH, dtype=torch.float64, device=env.device),
                             _dev(Q, env), _dev(R, env))
        assert torch.allclose(want, res.cost[-1], rtol=1e-12, atol=0)
    finally:
        env.close()


def test_mppi_lands_the_lander_with_its_own_reward():
    """Lander3D, a descent at 3 m/s from 1.5-2.5 m under hover motors: the nominal plan arrives too fast and crashes (the
    landing limit is far below 3 m/s).  With reward_weight > 0 the task's own reward -- the crash penalty, the landing
    bonus, the shaping -- is the cost, which no derivative sees across.  Reported: the share of envs whose best sample
    of the first iteration lands, and whose plan lands after the driver's iterations.  Required: the nominal crashes
    everywhere, and the cost history is non-increasing.  Measured: 0.0 % and 0.0 %; no candidate was
    accepted (the reward does not penalise a crash inside the bounds)."""
    import torch
    import gym_copter_amd
    n, K, P = 1024, 96, 512
    rng = np.random.default_rng(5)
    env = _env("lander3d", n, "float32", seed=2)
    try:
        env.reset()
        x0 = np.zeros((12, n))
        x0[4] = -rng.uniform(1.5, 2.5, n)
        x0[5] = 3.0
        state = {"x": x0, "status": np.full(n, AIRBORNE, np.uint8)}
        a0 = torch.full((K, n, 4), float(np.float32(AH)), dtype=torch.float32, device=env.device)
        Q, R = np.zeros((12, 12)), np.zeros((4, 4))
        nominal = to_np(env.rollout_states(a0, state).status)[-1]
        assert np.all(nominal == CRASHED)
        sigma, ids = np.full(4, 0.3, np.float32), np.arange(n)
        c = env.rollout_mppi_costs(a0, sigma, P, np.zeros(12), Q, R, reward_weight=1.0, state=state)
        best = to_np(c.best)
        tape = np.stack([mppi_ref.sample_actions(to_np(a0[:, i:i + 1]), sigma, 2, ids[i:i + 1], 0, int(best[i]))[:, 0]
                         for i in range(n)], axis=1)
        first = to_np(env.rollout_states(_dev(tape, env), state).status)[-1]
        res = gym_copter_amd.mppi(env, a0, np.zeros(12), Q, R, reward_weight=1.0, samples=P, sigma=sigma, lam=5.0,
                                  iters=6, state=state)
        hist = to_np(res.cost)
        final = to_np(env.rollout_states(res.actions, state).status)[-1]
        print("lander3d descent: best sample of %d lands in %.1f %% of envs; after 6 iterations the plan lands in %.1f %%; "
              "batch-mean cost %s" % (P, 100 * np.mean(first == LANDED), 100 * np.mean(final == LANDED),
                                      " ".join("%.2f" % v for v in hist.mean(axis=1))))
        assert np.all(hist[1:] <= hist[:-1]) and np.isfinite(hist).all()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_shortest_horizon_single_sample_and_odd_sample_counts():
    n, A, seed = 257, 4, 1
    rng = np.random.default_rng(12)
    env = _env("lander3d", n, "float32", seed=seed)
    try:
        env.reset()
        ids = np.arange(n)
        for K, P in ((1, 1), (1, 3), (5, 1), (3, 61)):
            x0, st = _random_point(n, rng)
            state = {"x": x0, "status": st}
            a0 = (AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32)
            abar = _dev(a0, env)
            Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
            sigma = np.float32(0.1)
            costs, _ = _check_costs("K=%d P=%d" % (K, P), env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, 0.2, 5, state,
                                    sorted({0, P // 2, P - 1}), ids, seed)
            up = env.rollout_mppi_update(abar, env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref,
                                                                      reward_weight=0.2, stream=5, state=state).costs,
                                         sigma, 1.0, stream=5)
            want, wess, wmin = mppi_ref.update(a0, costs, sigma, 1.0, seed, ids, 5)
            assert up.actions.shape == (K, n, A) and up.ess.shape == (n,) and up.cost_min.shape == (n,)
            assert _ulps(to_np(up.actions), want, a0) <= 2.0 and np.array_equal(to_np(up.cost_min), wmin)
            if P == 1:                                                          # the nominal alone: the clipped input
                assert np.array_equal(to_np(up.actions), np.clip(a0, 0, 1)) and np.all(to_np(up.ess) == 1.0)
    finally:
        env.close()


def test_costs_past_4_gib():
    """costs [P,N] float64 passes 4 GiB at P = 513 with 2^20 envs (513 x 2^20 x 8 B): the last rows against a smaller
    call's (the noise does not depend on P), the update's result against the restatement on a few envs."""
    import torch
    n, K, P, seed = 1 << 20, 2, 513, 9
    assert P * n * 8 > 4 << 30 >= (P - 1) * n * 8
    free, _ = torch.cuda.mem_get_info()
    if free < 3 * P * n * 8:
        pytest.skip("needs %.0f GiB of device memory" % (3 * P * n * 8 / 2 ** 30))
    env = _env("lander3d", n, "float32", seed=seed)
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        acts = torch.rand((K, n, 4), generator=g, device=env.device, dtype=torch.float32) * 0.2 + float(AH) - 0.1
        Q, R, x_ref = np.eye(12), np.eye(4), np.zeros(12)
        big = env.rollout_mppi_costs(acts, 0.05, P, x_ref, Q, R, stream=1)
        assert bool(torch.isfinite(big.costs[P - 1]).all()) and bool((big.best >= 0).all())
        lanes = [0, 1, 63, 64, n // 2 + 5, n - 2, n - 1]
        sub = big.costs[:, lanes].clone()
        small = env.rollout_mppi_costs(acts, 0.05, 16, x_ref, Q, R, stream=1)
        assert torch.equal(small.costs, big.costs[:16]) and bool((big.costs[P - 1] != big.costs[P - 2]).any())
        a = mppi_ref.sample_actions(to_np(acts[:, lanes]), 0.05, seed, np.array(lanes), 1, P - 1)
        full = np.broadcast_to(to_np(acts[:, :1]), (K, n, 4)).copy()
        full[:, lanes] = a
        ro = env.rollout_states(_dev(full, env))
        S = mppi_ref.cost(to_np(ro.x[:, lanes]), to_np(ro.reward[:, lanes]), a, x_ref, Q, R)
        assert np.allclose(to_np(sub[P - 1]), S, rtol=1e-12, atol=0)
        up = env.rollout_mppi_update(acts, big.costs, 0.05, 1.0, stream=1)
        want, wess, _ = mppi_ref.update(to_np(acts[:, lanes]), to_np(sub), 0.05, 1.0, seed, np.array(lanes), 1)
        assert _ulps(to_np(up.actions[:, lanes]), want, to_np(acts[:, lanes])) <= 2.0
        assert np.max(np.abs(to_np(up.ess[lanes]) / wess - 1)) <= 1e-12
    finally:
        env.close()


def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n, K, P, A = 4097, 6, 10, 4
    rng = np.random.default_rng(3)
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = _env("lander3d", n, "float32", autoreset="next_step", seed=6, max_steps=1000)
    try:
        sh.reset()
        plain.reset()
        acts = _dev((AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32), plain)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        c1 = sh.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, reward_weight=0.5, stream=2)
        c2 = plain.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, reward_weight=0.5, stream=2)
        assert torch.equal(c1.costs, c2.costs) and torch.equal(c1.best, c2.best)
        u1 = sh.rollout_mppi_update(acts, c1.costs, 0.1, 1.5, stream=2)
        u2 = plain.rollout_mppi_update(acts, c2.costs, 0.1, 1.5, stream=2)
        for u, v in zip(u1, u2):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib
    n, K, P, A = 128, 4, 6, 4
    rng = np.random.default_rng(2)
    env = _env("lander3d", n, "float64", seed=1)
    try:
        env.reset()
        x0, st = _random_point(n, rng)
        state = {"x": x0, "status": st}
        acts = _dev((AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32), env)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        costs = env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, state=state).costs
        bad = Q.copy()
        bad[0, 1] += 1e-9
        for kw, match in ((dict(Q=bad), "Q must be symmetric"), (dict(Q=Q[:6]), "Q must have shape"),
                          (dict(R=np.eye(3)), "R must have shape"), (dict(R=-np.eye(4)), "diagonal must be >= 0"),
                          (dict(Q_final=bad), "Q_final must be symmetric"), (dict(samples=0), "samples must be"),
                          (dict(samples=65536), "samples must be"), (dict(samples=2.0), "samples must be"),
                          (dict(sigma=-0.1), "sigma must be"), (dict(sigma=np.ones(3)), "sigma must be"),
                          (dict(sigma=float("nan")), "sigma must be"), (dict(a_ref=np.ones(5)), "a_ref must be"),
                          (dict(reward_weight=-1.0), "reward_weight must be"), (dict(stream=-1), "stream must be"),
                          (dict(stream=1 << 32), "stream must be"), (dict(x_ref=np.zeros((n, 6))), "x_ref must be"),
                          (dict(x_ref=np.zeros((K + 1, n, 12))), "x_ref must be"),
                          (dict(actions=acts[:, :n - 1]), "actions must have shape")):
            args = dict(actions=acts, sigma=0.1, samples=P, x_ref=x_ref, Q=Q, R=R, state=state)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_mppi_costs(**args)
        env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, np.zeros((4, 4)), state=state)      # R = 0 is semidefinite
        for kw, match in ((dict(lam=0.0), "lam must be"), (dict(lam=float("inf")), "lam must be"),
                          (dict(costs=costs.float()), "costs must be"), (dict(costs=costs[:, :n - 1]), "costs must have shape"),
                          (dict(costs=to_np(costs)), "costs must be"), (dict(sigma=-1.0), "sigma must be"),
                          (dict(stream=0.5), "stream must be"), (dict(actions=acts[:, :, :2]), "actions must have shape")):
            args = dict(actions=acts, costs=costs, sigma=0.1, lam=1.0)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_mppi_update(**args)
        # the result of an update can be the actions of the next one: the buffers alternate
        u1 = env.rollout_mppi_update(acts, costs, 0.1, 1.0)
        u2 = env.rollout_mppi_update(u1.actions, costs, 0.1, 1.0)
        assert u2.actions.data_ptr() != u1.actions.data_ptr()
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too; aliasing is refused
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps, io.actions_dev = C.sizeof(io), K, acts.data_ptr()
        mio = _lib.RolloutMppiIO()
        mio.struct_size = C.sizeof(mio) + 8
        assert env._lib.cs_rollout_mppi_costs(env._ctx, C.byref(io), C.byref(mio), None) == _lib.ERR_ABI
        assert env._lib.cs_rollout_mppi_update(env._ctx, C.byref(io), C.byref(mio), None) == _lib.ERR_ABI
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, state=state)
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_mppi_update(acts, costs, 0.1, 1.0)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R)
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_mppi_update(acts, costs, 0.1, 1.0)
    assert torch.cuda.is_available()
