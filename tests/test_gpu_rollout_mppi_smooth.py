"""cs_rollout_mppi_costs_ex / cs_rollout_mppi_update_ex / cs_rollout_mppi_temperature on the GPU:
the white table against the entry points of section 14, bit for bit; the smooth costs against rollout_states fed the
sample actions tests/mppi_smooth_ref.py rebuilds; the update, with a temperature per env, against the restatement on the
kernel's own costs; the solved temperature against E(lambda) in longdouble; determinism, shard invariance, no side
effects; plumbing; the mppi driver with smooth noise on the two problems of section 14."""
import numpy as np
import pytest

import mppi_ref
import mppi_smooth_ref as ref
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE, CRASHED, LANDED
from test_gpu_rollout_mppi import AH, TASK_A, TASKS, _cost_model, _dev, _env, _random_point, _tracking, _ulps

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]


def _knots(K, hold):
    import gym_copter_amd
    return gym_copter_amd.mppi_knots(K, hold)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the white table is section 14's noise
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["lander1d", "lander2d", "lander3d"])
def test_white_table_gives_the_bits_of_the_old_entry_points(task):
    """A = 1, 2 and 4; N = 300, K = 16, P = 7: knots = mppi_knots(K, 1) goes through the _ex calls and the new kernels."""
    import torch
    n, K, P, A, seed, base, stream = 300, 16, 7, TASK_A[task], 21, 1000, 4
    rng = np.random.default_rng(300 + A)
    env = _env(task, n, "float32", seed=seed, env_id_base=base)
    try:
        env.reset()
        abar = _dev((AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32), env)
        sigma = (0.05 * AH * rng.uniform(0.5, 2.0, A)).astype(np.float32)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        x0, st = _random_point(n, rng)
        white = _knots(K, 1)
        for state in (None, {"x": x0, "status": st, "force": rng.uniform(-1, 1, (3, n))}):
            kw = dict(Q_final=Qf, a_ref=a_ref, reward_weight=0.5, stream=stream, state=state)
            old = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, **kw)
            old = type(old)(*(t.clone() for t in old))
            new = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, knots=white, **kw)
            assert torch.equal(old.costs.view(torch.int64), new.costs.view(torch.int64)) and torch.equal(old.best, new.best)
            lam = float(old.costs.std(dim=0).median())
            uo = env.rollout_mppi_update(abar, old.costs, sigma, lam, stream=stream)
            uo = type(uo)(*(t.clone() for t in uo))
            un = env.rollout_mppi_update(abar, old.costs, sigma, lam, stream=stream, knots=white)
            assert torch.equal(uo.actions.view(torch.int32), un.actions.view(torch.int32))
            assert torch.equal(uo.ess.view(torch.int64), un.ess.view(torch.int64)) and torch.equal(uo.cost_min, un.cost_min)
            # ... and with the temperature as an [N] tensor of one value
            ul = env.rollout_mppi_update(abar, old.costs, sigma, torch.full((n,), lam, dtype=torch.float64, device=env.device),
                                         stream=stream)
            assert torch.equal(uo.actions.view(torch.int32), ul.actions.view(torch.int32))
            assert torch.equal(uo.ess.view(torch.int64), ul.ess.view(torch.int64))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the smooth costs
# ---------------------------------------------------------------------------------------------------------------------
def _check_costs(name, env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, wr, stream, state, samples, ids, seed, table,
                 expect_quiet=True):
    """costs[p] against S evaluated in NumPy on rollout_states(a(p)), a(p) rebuilt by mppi_smooth_ref.  The bar per env
    is tests/test_gpu_rollout_mppi.py's: max(100 x |S_float64 - S_longdouble|, T 2^-52 M)."""
    res = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, reward_weight=wr, stream=stream,
                                 state=state, knots=table)
    costs, best = to_np(res.costs).copy(), to_np(res.best).copy()
    assert costs.shape == (P, env.num_envs) and best.dtype == np.int32
    worst, events = 0.0, 0
    for p in samples:
        a = ref.sample_actions(to_np(abar), sigma, seed, ids, stream, table, p)
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


@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("mode", ["float32", "float32_rn", "float64"])
@pytest.mark.parametrize("task", TASKS)
def test_smooth_costs_equal_the_cost_of_rollout_states_on_the_sample_actions(task, mode, substeps):
    """N = 300 (a partial wavefront), K = 16, P = 7, samples 0, 3 and 6; hold 3 (K is no multiple: the last hold is cut
    short) and hold 16 (one knot pair over the horizon), each from the stored start right after reset() (its perturbation
    pending) and from an explicit one; the Landers with their reward in the cost.  Smooth and white costs differ."""
    n, K, P, A = 300, 16, 7, TASK_A[task]
    seed, base = 21, 1000
    rng = np.random.default_rng(1000 + TASKS.index(task) * 10 + substeps)
    env = _env(task, n, mode, substeps=substeps, seed=seed, env_id_base=base)
    try:
        env.reset()
        ids = base + np.arange(n)
        abar = _dev((AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32), env)
        sigma = (0.05 * AH * rng.uniform(0.5, 2.0, A)).astype(np.float32)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        wr = 0.5 if "lander" in task else 0.0
        x0, st = _random_point(n, rng)
        state = {"x": x0, "status": st, "force": rng.uniform(-1, 1, (3, n))}
        _, _, _, x_ref_k, _ = _cost_model(rng, A, n, K)
        for hold in (3, 16):
            table = _knots(K, hold)
            name = "%s/%s/%d hold %d" % (task, mode, substeps, hold)
            c1, _ = _check_costs(name + " stored", env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, wr, 3, None, (0, 3, P - 1),
                                 ids, seed, table, expect_quiet=False)
            _check_costs(name + " explicit", env, abar, sigma, P, x_ref_k, Q, R, None, None, wr, (1 << 32) - 1, state,
                         (0, 3, P - 1), ids, seed, table)
            white = to_np(env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, reward_weight=wr,
                                                 stream=3).costs)
            assert np.array_equal(white[0], c1[0]) and np.all(white[1:] != c1[1:])        # sample 0 has no noise
    finally:
        env.close()


def test_smooth_costs_with_next_step_resets_pending():
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
        costs, _ = _check_costs("next_step resets, hold 3", env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, 1.0, 0, None,
                                range(P), np.arange(n), seed, _knots(K, 3), expect_quiet=False)
        assert np.isfinite(costs[:, pend]).all()
    finally:
        env.close()


def test_smooth_costs_through_touchdowns_and_crashes():
    """Low, descending starts: many samples touch down or crash inside the horizon, differently from sample to sample."""
    n, K, P, A, seed = 512, 16, 12, 4, 5
    rng = np.random.default_rng(8)
    for task, mode, hold in (("lander3d", "float32", 16), ("hover3d", "float64", 3)):
        env = _env(task, n, mode, seed=seed)
        try:
            env.reset()
            x0, st = _random_point(n, rng, low=True)
            state = {"x": x0, "status": st}
            abar = _dev((AH * rng.uniform(0.2, 1.2, (K, n, A))).astype(np.float32), env)
            sigma = np.full(A, 0.5 * AH, np.float32)
            Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
            table = _knots(K, hold)
            costs, events = _check_costs("%s low starts, hold %d" % (task, hold), env, abar, sigma, P, x_ref, Q, R, Qf,
                                         a_ref, 1.0, 9, state, range(P), np.arange(n), seed, table, expect_quiet=False)
            final = to_np(env.rollout_states(abar, state).status)[-1]
            assert events > 0 and (final == CRASHED).sum() > 10 and (final != CRASHED).sum() > 10
            assert len(np.unique(to_np(env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, state=state,
                                                              knots=table).best))) > 3
        finally:
            env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the update and the temperature
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,mode,hold", [("lander3d", "float32", 3), ("hover2d", "float64", 16),
                                            ("lander1d", "float32_rn", 3)])
def test_smooth_update_equals_the_restatement_on_the_kernels_costs(task, mode, hold):
    """N = 300, K = 16, P = 37, global ids that wrap past 2^32.  A scalar temperature; the same value as an [N] tensor
    (the same bits); a random temperature per env with bad entries (NaN, 0, negative, inf), which keep the plan."""
    import torch
    n, K, P, A, seed, base, stream = 300, 16, 37, TASK_A[task], 17, (1 << 32) - 300, 6
    rng = np.random.default_rng(170 + A)
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
        table = _knots(K, hold)
        costs = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, stream=stream, state=state,
                                       knots=table).costs.clone()
        assert bool(torch.isfinite(costs).all())
        spread = float(costs.std(dim=0).median())
        costs[1, 0], costs[P - 1, 1], costs[0, 2] = float("inf"), float("nan"), float("-inf")
        costs[::2, 3] = float("nan")
        costs[:, 4] = torch.tensor([float("nan"), float("inf")] * P, device=env.device)[:P].double()
        costs[:, 5] = float("inf")
        costs[11, 5] = 3.0
        ch = to_np(costs)
        live = np.arange(n) != 4

        def compare(what, up, lam):
            got, ess, cmin = to_np(up.actions).copy(), to_np(up.ess).copy(), to_np(up.cost_min).copy()
            want, wess, wmin = ref.update(a0, ch, sigma, lam, seed, ids, stream, table)
            moved = wess > 0
            u = _ulps(got, want, a0)
            rel = float(np.max(np.abs(ess[moved] / wess[moved] - 1)))
            print("%s hold %d, %s: actions within %.2f ulp, ess within %.2e relative; ess median %.1f of %d"
                  % (task, hold, what, u, rel, np.median(ess), P))
            assert u <= 2.0 and rel <= 1e-12 and np.array_equal(cmin, wmin)
            assert np.array_equal(ess == 0, ~moved)
            assert np.array_equal(got[:, ~moved].view(np.uint32), a0[:, ~moved].view(np.uint32))   # the input bits
            assert got[:, moved].min() >= 0.0 and got[:, moved].max() <= 1.0
            return got, ess, cmin

        for lam in (spread, 0.1 * spread):
            first = compare("lam %.3g" % lam, env.rollout_mppi_update(abar, costs, sigma, lam, stream=stream, knots=table), lam)
            assert first[1][4] == 0.0 and first[2][4] == np.inf and first[1][5] == 1.0 and first[2][5] == 3.0
            best5 = np.clip(ref.sample_actions(a0, sigma, seed, ids, stream, table, 11)[:, 5], 0, 1)
            assert _ulps(first[0][:, 5], best5, a0[:, 5]) <= 2.0
            filled = torch.full((n,), lam, dtype=torch.float64, device=env.device)
            for again in (env.rollout_mppi_update(abar, costs, sigma, lam, stream=stream, knots=table),
                          env.rollout_mppi_update(abar, costs, sigma, filled, stream=stream, knots=table)):
                for s, t in zip(again, first):
                    assert np.array_equal(to_np(s).view(np.uint8), t.view(np.uint8))        # the same bits
        # the smooth update is not the white one
        white = env.rollout_mppi_update(abar, costs, sigma, spread, stream=stream)
        assert not np.array_equal(to_np(white.actions)[:, live], first[0][:, live])
        # a temperature per env
        lam_n = spread * np.exp(rng.uniform(-3, 3, n))
        lam_n[[7, 8, 9, 10]] = [np.nan, 0.0, -1.0, np.inf]
        got, ess, _ = compare("lam per env", env.rollout_mppi_update(abar, costs, sigma, _dev(lam_n, env), stream=stream,
                                                                    knots=table), lam_n)
        assert np.all(ess[[4, 7, 8, 9, 10]] == 0) and np.all(ess[11:] >= 1.0)
        for kw, match in ((dict(lam=_dev(lam_n[:-1], env)), "lam must have shape"),
                          (dict(lam=_dev(lam_n, env).float()), "lam must be"),
                          (dict(knots=_knots(K + 1, 3)), "knots must be"), (dict(knots=(table[0],)), "knots must be"),
                          (dict(knots=(table[0] * 0, table[1])), "knot numbers must"),
                          (dict(knots=(table[0], table[1] * np.nan)), "knot weights must")):
            args = dict(actions=abar, costs=costs, sigma=sigma, lam=1.0, knots=table)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_mppi_update(**args)
    finally:
        env.close()


def _ld_ess(costs, lam):
    return ref.ess_at(costs, np.asarray(lam, dtype=np.longdouble), dtype=np.longdouble)


@pytest.mark.parametrize("P,target", [(37, 8.0), (256, 8.0), (7, 1.0), (7, 40.0), (1, 1.0)])
def test_temperature_solves_the_effective_sample_size(P, target):
    """N = 300 on the kernel's own smooth costs with injected non-finite entries.  Inside the bracket, E at the kernel's
    lambda in longdouble is as close to the target as 100 x the float64 restatement's own distance (floored at 1e-9
    relative); at the edges the rules hold exactly; the kernel's own E is printed and is the longdouble one to 1e-10;
    two calls give the same bits."""
    import torch
    n, K, A, seed, stream = 300, 16, 4, 17, 6
    lam_min, lam_max = 1e-6, 1e6
    rng = np.random.default_rng(500 + P)
    env = _env("lander3d", n, "float32", seed=seed)
    try:
        env.reset()
        x0, st = _random_point(n, rng)
        abar = _dev((AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32), env)
        Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
        costs = env.rollout_mppi_costs(abar, 0.1 * AH, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, stream=stream,
                                       state={"x": x0, "status": st}, knots=_knots(K, 3)).costs.clone()
        costs[:, 4] = float("nan")                              # no finite cost
        costs[:, 5] = float("inf")
        costs[P // 2, 5] = 3.0                                  # one finite cost: E = 1 at every lambda
        costs[:, 6] = 2.5                                       # all tied: E = P at every lambda
        if P > 2:
            costs[0, 0], costs[P - 1, 1], costs[1, 2] = float("inf"), float("nan"), float("-inf")
            costs[:, 7] *= 1e6                                  # E(lam_max) < target for a large target
            costs[:, 8] *= 1e-9                                 # E(lam_min) close to P
        ch = to_np(costs)
        res = env.rollout_mppi_temperature(costs, target, lam_min, lam_max)
        lam, ess = to_np(res.lam).copy(), to_np(res.ess).copy()
        again = env.rollout_mppi_temperature(costs, target, lam_min, lam_max)
        assert np.array_equal(to_np(again.lam).view(np.uint64), lam.view(np.uint64))
        assert np.array_equal(to_np(again.ess).view(np.uint64), ess.view(np.uint64))
        wlam, _ = ref.temperature(ch, target, lam_min, lam_max)
        e_min, e_max = _ld_ess(ch, lam_min), _ld_ess(ch, lam_max)
        none = ~np.isfinite(ch).any(0)
        at_max = none | (e_max < target)
        at_min = ~at_max & (e_min >= target)
        inside = ~at_max & ~at_min
        # (an env whose E(lam_min) or E(lam_max) is within rounding of the target may fall on either side: none here)
        # (E >= 1 in any arithmetic, so a target of 1 is met at lam_min by every env)
        assert target == 1.0 or np.min(np.abs(np.stack([e_min, e_max])[:, ~none] / target - 1)) > 1e-9
        assert np.all(lam[at_max] == lam_max) and np.all(lam[at_min] == lam_min)
        assert none[4] and ess[4] == 0.0 and ess[5] == 1.0 and ess[6] == P
        assert lam[5] == (lam_min if target <= 1.0 else lam_max) and lam[6] == (lam_min if target <= P else lam_max)
        e_kernel = _ld_ess(ch, lam)
        rel = np.abs(ess[~none] / e_kernel[~none].astype(np.float64) - 1)
        assert rel.max() <= 1e-10
        if inside.any():
            dist_ref = np.abs(_ld_ess(ch, wlam)[inside] / target - 1).astype(np.float64)
            dist = np.abs(e_kernel[inside] / target - 1).astype(np.float64)
            bar = 100 * np.maximum(dist_ref, 1e-9)
            print("temperature P %d target %g: %d envs inside, E(lam) / target - 1: kernel max %.2e, restatement max %.2e; "
                  "kernel's own E within %.1e of longdouble; lam %.3g .. %.3g; %d at lam_max, %d at lam_min"
                  % (P, target, inside.sum(), dist.max(), dist_ref.max(), rel.max(), lam[inside].min(),
                     lam[inside].max(), at_max.sum(), at_min.sum()))
            assert np.all(dist <= bar)
            assert np.all((lam[inside] > lam_min) & (lam[inside] < lam_max))
        assert inside.sum() > 250 if target == 8.0 else inside.sum() == 0
        # the solved temperature in the update gives that effective sample size
        up = env.rollout_mppi_update(abar, costs, 0.1 * AH, res.lam, stream=stream, knots=_knots(K, 3))
        assert np.allclose(to_np(up.ess), ess, rtol=1e-12, atol=0)
        for kw, match in ((dict(ess_target=0.5), "ess_target must be"), (dict(lam_min=0.0), "lam_min < lam_max"),
                          (dict(lam_min=2.0, lam_max=1.0), "lam_min < lam_max"), (dict(costs=costs.float()), "costs must be"),
                          (dict(costs=costs[:, :n - 1]), "costs must have shape")):
            args = dict(costs=costs, ess_target=target, lam_min=lam_min, lam_max=lam_max)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_mppi_temperature(**args)
        assert torch.cuda.is_available()
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism, invariance, no side effects
# ---------------------------------------------------------------------------------------------------------------------
def test_smooth_costs_independent_of_the_batch_split_and_of_P():
    n, K, P, A, seed = 300, 16, 9, 4, 4
    rng = np.random.default_rng(15)
    x0, st = _random_point(n, rng)
    a0 = (AH * rng.uniform(0.7, 1.3, (K, n, A))).astype(np.float32)
    Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
    sigma, table = 0.1 * AH, _knots(K, 3)

    def run(lo, hi, samples=P, stream=2, base=0):
        import torch
        env = _env("lander3d", hi - lo, "float32", seed=seed, env_id_base=base + lo)
        try:
            env.reset()
            state = {"x": x0[:, lo:hi], "status": st[lo:hi]}
            acts = _dev(a0[:, lo:hi], env)
            kw = dict(Q_final=Qf, a_ref=a_ref, reward_weight=0.3, stream=stream, state=state, knots=table)
            c = env.rollout_mppi_costs(acts, sigma, samples, x_ref[lo:hi], Q, R, **kw).costs.clone()
            c2 = env.rollout_mppi_costs(acts, sigma, samples, x_ref[lo:hi], Q, R, **kw).costs
            assert torch.equal(c.view(torch.int64), c2.view(torch.int64))
            up = env.rollout_mppi_update(acts, c, sigma, 2.0, stream=stream, knots=table)
            t = env.rollout_mppi_temperature(c, 3.0)
            return to_np(c), to_np(up.actions).copy(), to_np(up.ess).copy(), to_np(t.lam).copy()
        finally:
            env.close()
    whole = run(0, n)
    for lo, hi in ((0, 128), (128, 300), (37, 101)):
        part = run(lo, hi)
        assert np.array_equal(part[0], whole[0][:, lo:hi]) and np.array_equal(part[1], whole[1][:, lo:hi])
        assert np.array_equal(part[2], whole[2][lo:hi])
    assert np.array_equal(run(0, n, samples=4)[0], whole[0][:4])          # the first samples of a larger P
    other = run(0, n, stream=3)
    assert np.array_equal(other[0][0], whole[0][0]) and np.all(other[0][1:] != whole[0][1:])
    shifted = run(0, n, base=1)
    assert np.array_equal(shifted[0][0], whole[0][0]) and np.all(shifted[0][1:] != whole[0][1:])


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
        table = _knots(K, 3)
        c = env.rollout_mppi_costs(abar, 0.05, P, x_ref, Q, R, Q_final=Qf, reward_weight=1.0, stream=1, knots=table)
        t = env.rollout_mppi_temperature(c.costs, 2.0)
        env.rollout_mppi_update(abar, c.costs, 0.05, t.lam, stream=1, knots=table)
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
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_shortest_horizon_and_single_sample():
    n, A, seed = 257, 4, 1
    rng = np.random.default_rng(12)
    env = _env("lander3d", n, "float32", seed=seed)
    try:
        env.reset()
        ids = np.arange(n)
        for K, P, hold in ((1, 1, 16), (1, 3, 2), (5, 1, 2), (3, 61, 2)):
            x0, st = _random_point(n, rng)
            state = {"x": x0, "status": st}
            a0 = (AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32)
            abar = _dev(a0, env)
            Q, Qf, R, x_ref, a_ref = _cost_model(rng, A, n)
            sigma, table = np.float32(0.1), _knots(K, hold)
            costs, _ = _check_costs("K=%d P=%d hold %d" % (K, P, hold), env, abar, sigma, P, x_ref, Q, R, Qf, a_ref, 0.2,
                                    5, state, sorted({0, P // 2, P - 1}), ids, seed, table)
            cd = env.rollout_mppi_costs(abar, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref, reward_weight=0.2, stream=5,
                                        state=state, knots=table).costs
            t = env.rollout_mppi_temperature(cd, 1.5)
            up = env.rollout_mppi_update(abar, cd, sigma, t.lam, stream=5, knots=table)
            wlam = to_np(t.lam)
            want, wess, wmin = ref.update(a0, costs, sigma, wlam, seed, ids, 5, table)
            assert up.actions.shape == (K, n, A) and t.lam.shape == (n,) and t.ess.shape == (n,)
            assert _ulps(to_np(up.actions), want, a0) <= 2.0 and np.array_equal(to_np(up.cost_min), wmin)
            if P == 1:                                                # the nominal alone: E = 1 < 1.5, so lam_max
                assert np.array_equal(to_np(up.actions), np.clip(a0, 0, 1)) and np.all(to_np(up.ess) == 1.0)
                assert np.all(wlam == 1e6) and np.all(to_np(t.ess) == 1.0)
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
        table = _knots(K, 4)
        kw = dict(Q_final=Qf, a_ref=a_ref, reward_weight=0.5, stream=2, knots=table)
        c1 = sh.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, **kw)
        c2 = plain.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, **kw)
        assert torch.equal(c1.costs, c2.costs) and torch.equal(c1.best, c2.best)
        t1, t2 = sh.rollout_mppi_temperature(c1.costs, 3.0, 1e-3, 1e3), plain.rollout_mppi_temperature(c2.costs, 3.0, 1e-3, 1e3)
        assert torch.equal(t1.lam, t2.lam) and torch.equal(t1.ess, t2.ess)
        u1 = sh.rollout_mppi_update(acts, c1.costs, 0.1, t1.lam, stream=2, knots=table)
        u2 = plain.rollout_mppi_update(acts, c2.costs, 0.1, t2.lam, stream=2, knots=table)
        for u, v in zip(u1, u2):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_errors_and_an_open_serve_session():
    import ctypes as C
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
        table = _knots(K, 2)
        costs = env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, state=state, knots=table).costs
        for bad, match in ((_knots(K + 1, 2), "knots must be"), (3, "knots must be"),
                           ((table[0].astype(np.float32), table[1]), "knots must be"),
                           ((table[0] + 16383, table[1]), "knot numbers must")):
            with pytest.raises(ValueError, match=match):
                env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, state=state, knots=bad)
        # the C ABI with a live context: a wrong struct_size of the new block is CS_ERR_ABI; a lone table pointer CS_ERR_ARG
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps, io.actions_dev = C.sizeof(io), K, acts.data_ptr()
        mio = _lib.RolloutMppiIO()
        mio.struct_size, mio.num_samples = C.sizeof(mio), P
        mio.sigma_dev = mio.x_ref_dev = mio.Q_dev = mio.R_dev = mio.costs_dev = costs.data_ptr()
        ext = _lib.RolloutMppiExt()
        ext.struct_size = C.sizeof(ext) + 8
        assert env._lib.cs_rollout_mppi_costs_ex(env._ctx, C.byref(io), C.byref(mio), C.byref(ext), None) == _lib.ERR_ABI
        assert env._lib.cs_rollout_mppi_temperature(env._ctx, C.byref(mio), C.byref(ext), None) == _lib.ERR_ABI
        ext.struct_size, ext.knot_dev = C.sizeof(ext), costs.data_ptr()
        assert env._lib.cs_rollout_mppi_costs_ex(env._ctx, C.byref(io), C.byref(mio), C.byref(ext), None) == _lib.ERR_ARG
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_mppi_costs(acts, 0.1, P, x_ref, Q, R, state=state, knots=table)
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_mppi_update(acts, costs, 0.1, 1.0, knots=table)
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_mppi_temperature(costs, 2.0)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_mppi_temperature(costs, 2.0)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the driver
# ---------------------------------------------------------------------------------------------------------------------
def test_mppi_with_smooth_noise_lands_the_lander():
    """tests/test_gpu_rollout_mppi.py's descent -- 1 024 Lander3D envs at 3 m/s from 1.5-2.5 m under hover motors, the
    task's own reward as the cost, K = 96, P = 512 -- at sigma = 0.006 (a third of the hover motor value), lam = 5, 6
    iterations, with white noise (hold 1) and with smooth noise (hold 16).  Required: the nominal crashes everywhere;
    both cost histories are non-increasing; the share of envs whose best first-iteration sample lands at hold 16 is at
    least twice that at hold 1; the final plan lands in more envs at hold 16 than at hold 1.  CPU measurements
    (tests/test_rollout_mppi_smooth_cpu.py): 56/64 against 13/64 for the best sample; 1.00 against
    0.62 for the plan on 32 envs."""
    import torch
    import gym_copter_amd
    n, K, P, seed = 1024, 96, 512, 2
    rng = np.random.default_rng(5)
    env = _env("lander3d", n, "float32", seed=seed)
    try:
        env.reset()
        x0 = np.zeros((12, n))
        x0[4] = -rng.uniform(1.5, 2.5, n)
        x0[5] = 3.0
        state = {"x": x0, "status": np.full(n, AIRBORNE, np.uint8)}
        a0 = torch.full((K, n, 4), float(np.float32(AH)), dtype=torch.float32, device=env.device)
        Q, R = np.zeros((12, 12)), np.zeros((4, 4))
        assert np.all(to_np(env.rollout_states(a0, state).status)[-1] == CRASHED)
        sigma, ids, a0_np = np.full(4, 0.006, np.float32), np.arange(n), to_np(a0)
        first, final = {}, {}
        for hold in (1, 16):
            table = _knots(K, hold)
            c = env.rollout_mppi_costs(a0, sigma, P, np.zeros(12), Q, R, reward_weight=1.0, state=state, knots=table)
            best = to_np(c.best)
            tape = np.empty((K, n, 4), np.float32)
            for p in np.unique(best):                                 # the best samples' tapes, one sample index at a time
                at = np.flatnonzero(best == p)
                tape[:, at] = ref.sample_actions(a0_np[:, at], sigma, seed, ids[at], 0, table, int(p))
            first[hold] = float(np.mean(to_np(env.rollout_states(_dev(tape, env), state).status)[-1] == LANDED))
            res = gym_copter_amd.mppi(env, a0, np.zeros(12), Q, R, reward_weight=1.0, samples=P, sigma=sigma, lam=5.0,
                                      iters=6, state=state, hold=hold)
            hist = to_np(res.cost)
            final[hold] = float(np.mean(to_np(env.rollout_states(res.actions, state).status)[-1] == LANDED))
            print("lander3d descent, hold %2d: best sample of %d lands in %.1f %% of envs; after 6 iterations the plan lands "
                  "in %.1f %%; batch-mean cost %s; median ess %s"
                  % (hold, P, 100 * first[hold], 100 * final[hold], " ".join("%.2f" % v for v in hist.mean(axis=1)),
                     " ".join("%.1f" % v for v in np.median(to_np(res.ess), axis=1))))
            assert np.all(hist[1:] <= hist[:-1]) and np.isfinite(hist).all()
        assert first[16] >= 2 * first[1] and first[16] > 0
        assert final[16] > final[1]
    finally:
        env.close()


def test_mppi_with_smooth_noise_on_hover3d_tracking():
    """tests/test_gpu_rollout_mppi.py's tracking problem -- 4 096 Hover3D envs, K = 64, P = 256, lam = 0.5, 8 iterations
    from constant hover motors.  Required: at sigma = 0.004 the final batch-mean cost with hold 8 is at most 0.9 x the
    white one's (CPU, 16 envs: 18.02 against 22.41, a ratio of 0.80; the bar leaves half the gap) and below that of
    today's setting (white, sigma = 0.02); every history is non-increasing, that of ess_target = 8 included, of which
    nothing else is required."""
    import torch
    import gym_copter_amd
    n, K, iters, P = 4096, 64, 8, 256
    rng = np.random.default_rng(61)
    env = _env("hover3d", n, "float32", seed=1)
    try:
        env.reset()
        x0, x_ref, Q, R = _tracking(rng, n)
        state = {"x": _dev(x0, env), "status": np.full(n, AIRBORNE, np.uint8)}
        a0 = torch.full((K, n, 4), float(np.float32(AH)), dtype=torch.float32, device=env.device)
        final = {}
        for name, kw in (("white sigma 0.02", dict(sigma=0.02)), ("white sigma 0.004", dict(sigma=0.004)),
                         ("hold 8 sigma 0.004", dict(sigma=0.004, hold=8)),
                         ("hold 8 sigma 0.004 ess_target 8", dict(sigma=0.004, hold=8, ess_target=8.0))):
            res = gym_copter_amd.mppi(env, a0, x_ref, Q, R, a_ref=AH, samples=P, lam=0.5, iters=iters, state=state, **kw)
            hist, ess = to_np(res.cost), to_np(res.ess)
            print("hover3d tracking, %s: batch-mean cost per iteration %s; median ess %s"
                  % (name, " ".join("%.4f" % v for v in hist.mean(axis=1)), " ".join("%.1f" % v for v in np.median(ess, axis=1))))
            assert hist.shape == (iters + 1, n) and np.isfinite(hist).all() and np.all(hist[1:] <= hist[:-1])
            assert np.all((ess >= 1.0 - 1e-9) & (ess <= P + 1e-9))
            final[name] = float(hist[-1].mean())
        assert final["hold 8 sigma 0.004"] <= 0.9 * final["white sigma 0.004"]
        assert final["hold 8 sigma 0.004"] < final["white sigma 0.02"]
    finally:
        env.close()
