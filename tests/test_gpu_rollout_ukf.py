"""The unscented Kalman filter on the device (cs_rollout_ukf, CopterVecEnv.rollout_ukf, gym_copter_amd.ukf): every step
of the kernel's recursion against the NumPy restatement (tests/ukf_ref.py) on the kernel's OWN tapes, with points=True --
one step at a time no branch can be taken differently by the reference, and by induction over k the whole recursion is
verified.  For step k (_check_steps):

  1. points        points[k] against the reference's points from the device's posterior k - 1, within the bar
  2. propagation   points_pred[k] and point_status[k] equal, bit for bit, a K = 1 rollout_states on a second env of 25 N
                   lanes started explicitly from points[k] and status[k - 1] (float32 storage: within 2^-23 max(1, |v|),
                   as section 19 holds x_pred: rollout_states rounds its stored words once, the filter does not)
  3. status        status[k] is point 0's; spread[k] counts the points whose status differs from it
  4. posterior     the reference's moments of the device's points_pred[k] plus its sequential update, against x_pred, x,
                   P_tape, var and nis within the bar; loglik against the sum of the steps' terms, bars summed
  5. Q             its share of every entry of P- is >= 1 000 x the bar (on the reference): a dropped Q cannot pass

The bar per output is section 19's: 100 x the float64 reference's own distance from the same step in numpy.longdouble,
floored at 1e-12 scaled.  The induction runs under three weight settings -- (1, 0, 1); (0.5, 2, 0) with wm0 = -3 and
wc0 = -0.25; (1, 0, 0), the cubature rule, wm0 = 0 -- so that swapped or dropped centre weights fail.  The inputs are
NumPy's (inputs()): tests/test_rollout_ukf_cpu.py runs them through the restated filter on the float64 oracle first."""
import zlib

import numpy as np
import pytest

import ekf_ref
import test_gpu_rollout_ekf as E
import ukf_ref
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE, CRASHED, LANDED, LEVELING

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K = E.N, E.K         # 300 (four whole wavefronts and one of 44 lanes), 16
NP = ukf_ref.NP
TAPES = ("x", "x_pred", "var", "nis", "status", "spread", "P_tape", "points", "points_pred", "point_status")


def inputs(task, n, steps, seed, M=6, dense=True, missing=0.0, ah=E.AH):
    """The filter's inputs as NumPy arrays (no device): section 19's starts of every branch (test_gpu_rollout_ekf._points),
    its model, a random SPD P0 per env (small for the lanes whose motor is driven past 1), section 19's Q, and the
    measurement noise (already scaled by sqrt(r); NaN where a Bernoulli(missing) draw says "no measurement") that is added
    to H x of the true rollout from the same starts."""
    rng = np.random.default_rng(seed)
    x0, st0, acts, grp = E._points(n, steps, E.TASK_A[task], rng, ah)
    H, r = E._model(rng, M, dense)
    P0 = E._spd(rng, n)
    P0[grp == "clip_hi"] *= 1e-4
    noise = np.sqrt(r) * rng.standard_normal((steps, n, M))
    if missing > 0.0:
        noise[rng.uniform(size=noise.shape) < missing] = np.nan
    return dict(x0=x0, st0=st0, acts=acts, grp=grp, H=H, r=r, P0=P0, Q=ekf_ref.test_Q(), noise=noise)


def _problem(env, p):
    """inputs() on env's device, with z = H x + noise on the rollout_states tape of the same starts"""
    import torch
    acts = E._dev(p["acts"], env)
    truth = env.rollout_states(acts, state={"x": p["x0"], "status": p["st0"]}).x
    z = truth.to(torch.float64) @ E._dev(p["H"], env).T + E._dev(p["noise"], env)
    return dict(p, acts=acts, z=z, x0=E._dev(p["x0"], env), P0=E._dev(p["P0"], env), st0=E._dev(p["st0"], env))


def _run(env, p, setting=ukf_ref.SETTINGS[0], **kw):
    a, b, k = setting
    return env.rollout_ukf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], status0=p["st0"], alpha=a, beta=b,
                           kappa=k, **kw)


def _clone(res):
    return type(res)(*[None if t is None else t.clone() for t in res])


def _pair(task, n, mode="float64", **kw):
    """the filter's env and the env of 25 n lanes that propagates its points one by one"""
    return E._env(task, n, mode, seed=3, **kw), E._env(task, NP * n, mode, seed=3, **kw)


WORST = {}


def _check_steps(name, env, penv, p, res, setting, exact=True):
    """every step of res (a tape=True, points=True result, cloned) against one reference step from the device's own
    tapes; returns the point statuses [K,n,25]"""
    import torch
    steps, n = res.x.shape[:2]
    w, wl = ukf_ref.weights(*setting), ukf_ref.weights(*setting, dtype=np.longdouble)
    Q, H, r = p["Q"], p["H"], p["r"]
    xprev, Pprev, sprev = to_np(p["x0"]).T.copy(), to_np(p["P0"]), p["st0"]
    ok = np.ones(n, bool)
    ll64, llbar = 0.0, 0.0
    worst = {}
    assert torch.equal(res.P, res.P_tape[-1])
    assert torch.equal(res.var, torch.diagonal(res.P_tape, dim1=2, dim2=3))
    assert torch.equal(res.P_tape, res.P_tape.transpose(2, 3))

    def hold(key, got, ref, bar, k):
        e = ekf_ref.scaled(got, ref)
        worst[key] = max(worst.get(key, 0.0), e / bar)
        assert e <= bar, (name, key, k, e, bar)

    for k in range(steps):
        landed = to_np(sprev) == LANDED
        # 1. the points from the device's posterior k - 1
        pts64, okf, _ = ukf_ref.points(xprev, Pprev, w[0])
        ptsld, _, _ = ukf_ref.points(xprev, Pprev, wl[0], dtype=np.longdouble)
        pts64 = np.where(landed[:, None, None], xprev[:, None, :], pts64)
        ptsld = np.where(landed[:, None, None], xprev[:, None, :].astype(np.longdouble), ptsld)
        ok &= okf | landed
        bar = max(100.0 * ekf_ref.scaled(pts64, ptsld.astype(np.float64)), ukf_ref.FLOOR)
        pts = to_np(res.points[k])
        hold("points", pts, pts64, bar, k)
        assert np.array_equal(pts[:, 0], xprev), (name, k)                  # point 0 is the mean itself
        # 2. each point through rollout_states from (the point, the status of the mean)
        start = {"x": res.points[k].reshape(n * NP, 12).T.contiguous(), "status": sprev.repeat_interleave(NP)}
        one = penv.rollout_states(p["acts"][k:k + 1].repeat_interleave(NP, dim=1), state=start)
        want_y = torch.where(torch.as_tensor(landed, device=env.device)[:, None, None], res.points[k],
                             one.x[0].to(torch.float64).reshape(n, NP, 12))
        want_s = one.status[0].reshape(n, NP).clone()
        want_s[torch.as_tensor(landed, device=env.device)] = LANDED
        if exact:
            assert torch.equal(res.points_pred[k], want_y), (name, k)
        else:
            wy = to_np(want_y)
            err = np.abs(to_np(res.points_pred[k]) - wy) / np.maximum(1.0, np.abs(wy))
            worst["points_pred / 2^-23"] = max(worst.get("points_pred / 2^-23", 0.0), float(err.max()) * 2.0 ** 23)
            assert np.all(err <= 2.0 ** -23), (name, k, float(err.max()) * 2.0 ** 23)
        assert torch.equal(res.point_status[k], want_s), (name, k)
        # 3. the status of the mean and the spread
        ps = to_np(res.point_status[k])
        assert np.array_equal(to_np(res.status[k]), ps[:, 0]), (name, k)
        assert np.array_equal(to_np(res.spread[k]), (ps != ps[:, :1]).sum(axis=1)), (name, k)
        assert not to_np(res.spread[k])[landed].any()
        # 4. the moments of the device's propagated points and the update
        y, zk = to_np(res.points_pred[k]), to_np(p["z"][k])
        r64 = ukf_ref.one_step(y, landed, xprev, Pprev, w, Q, H, r, zk)
        rld = ukf_ref.one_step(y, landed, xprev, Pprev, wl, Q, H, r, zk, dtype=np.longdouble)
        ok &= r64["ok"]
        bars = ukf_ref.bars(r64, rld, ("x_pred", "P_pred", "x", "P", "var", "nis", "loglik"))
        # 5. Q's share of every entry of P- is far above the bar: a dropped Q cannot pass
        share = np.abs(Q)[None] / np.maximum(1.0, np.abs(r64["P_pred"]))
        fin = np.isfinite(r64["P_pred"]).all(axis=(1, 2))
        assert share[fin].min() >= 1e3 * max(bars["P_pred"], bars["P"]), (name, k, share[fin].min(), bars)
        got = dict(x_pred=to_np(res.x_pred[k]), x=to_np(res.x[k]), P=to_np(res.P_tape[k]), var=to_np(res.var[k]),
                   nis=to_np(res.nis[k]))
        for key, g in got.items():
            hold(key, g, r64[key], bars[key], k)
        ll64 = ll64 + r64["loglik"]
        llbar += bars["loglik"]
        xprev, Pprev, sprev = got["x"], got["P"], res.status[k]
    e = ekf_ref.scaled(to_np(res.loglik), ll64)
    worst["loglik"] = e / llbar
    assert e <= llbar, (name, "loglik", e, llbar)
    assert np.array_equal(to_np(res.ok), ok)
    WORST[name] = worst
    print("%s: worst ratio to the bar " % name + " ".join("%s %.4f" % kv for kv in worst.items()))
    return to_np(res.point_status)


# ---------------------------------------------------------------------------------------------------------------------
# 1. through every branch, under the three weight settings
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ukf_ref.SETTINGS, ids=lambda s: "a%g-b%g-k%g" % s)
@pytest.mark.parametrize("substeps", [1, 10])
def test_every_step_through_every_branch(substeps, setting):
    import torch
    env, penv = _pair("lander3d", N, substeps=substeps)
    try:
        env.reset()
        penv.reset()
        p = _problem(env, inputs("lander3d", N, K, seed=700 + substeps))
        res = _clone(_run(env, p, setting, tape=True, points=True))
        ps = _check_steps("lander3d substeps=%d %r" % (substeps, setting), env, penv, p, res, setting)
        spread = to_np(res.spread)
        share = float((spread > 0).mean())
        shares = {nm: float((ps == s).mean()) for nm, s in (("AIRBORNE", AIRBORNE), ("LEVELING", LEVELING),
                                                             ("LANDED", LANDED), ("CRASHED", CRASHED))}
        print("spread > 0 in %.3f of the (k, env) pairs, at most %d; point statuses: %s" % (
            share, spread.max(), " ".join("%s %.3f" % kv for kv in shares.items())))
        assert share >= 0.01, share
        assert all(v > 0 for v in shares.values()), shares
        # every group of section 19's starts is there ("clip_hi": the third of the clip group driven past 1)
        for g in E.GROUPS:
            assert np.char.startswith(p["grp"], g).sum() >= N // 12, g
        # the same bits in every other output without the tapes, and on a second call
        plain = _run(env, p, setting)
        assert plain.P_tape is None and plain.points is None and plain.points_pred is None and plain.point_status is None
        for a, b in zip(plain[:9], res[:9]):
            assert torch.equal(a, b)
        again = _run(env, p, setting, tape=True, points=True)
        for a, b in zip(again, res):
            assert torch.equal(a, b)
    finally:
        env.close()
        penv.close()


@pytest.mark.parametrize("task,mode,M", [("hover3d", "float32", 6), ("lander2d", "float64", 1), ("hover1d", "float64", 12)])
def test_every_step_for_other_tasks_storage_modes_and_measurement_counts(task, mode, M):
    seed = zlib.crc32(repr((task, mode, M)).encode())
    env, penv = _pair(task, N, mode)
    try:
        env.reset()
        penv.reset()
        p = _problem(env, inputs(task, N, K, seed=seed, M=M))
        for setting in ukf_ref.SETTINGS[:2]:
            res = _clone(_run(env, p, setting, tape=True, points=True))
            _check_steps("%s %s M=%d %r" % (task, mode, M, setting), env, penv, p, res, setting, exact=mode == "float64")
    finally:
        env.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. missing measurements
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_measurements_are_skipped():
    import torch
    env, penv = _pair("lander3d", N)
    try:
        env.reset()
        penv.reset()
        p = _problem(env, inputs("lander3d", N, K, seed=31, dense=False, missing=0.3))
        p["z"][3] = float("nan")                       # steps without a measurement for any env
        p["z"][K - 1] = float("nan")
        gone = torch.isnan(p["z"])
        assert 0.25 < float(gone[[0, 1, 2, 4]].double().mean()) < 0.35
        blind = gone.all(dim=2).all(dim=1)
        assert blind.tolist() == [k in (3, K - 1) for k in range(K)]
        res = _clone(_run(env, p, tape=True, points=True))
        _check_steps("lander3d 30% missing", env, penv, p, res, ukf_ref.SETTINGS[0])
        for k in (3, K - 1):
            assert torch.equal(res.x[k], res.x_pred[k])
            assert bool((res.nis[k] == 0).all())
    finally:
        env.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact statements
# ---------------------------------------------------------------------------------------------------------------------
def test_landed_filter_without_measurements_adds_q_exactly():
    import torch
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, inputs("lander3d", N, K, seed=42))
        p["st0"] = torch.full((N,), int(LANDED), dtype=torch.uint8, device=env.device)
        p["z"] = torch.full_like(p["z"], float("nan"))
        res = _run(env, p, tape=True, points=True)
        want = to_np(p["P0"]).copy()
        for k in range(K):
            want = want + p["Q"]                       # (((P0 + Q) + Q) + ...), in this order
            assert torch.equal(res.x[k], p["x0"].T), k
            assert np.array_equal(to_np(res.P_tape[k]), want), k
            assert torch.equal(res.points[k], p["x0"].T[:, None, :].expand(N, NP, 12)), k
            assert torch.equal(res.points_pred[k], res.points[k]), k
        assert bool((res.status == int(LANDED)).all()) and bool(res.ok.all()) and bool((res.spread == 0).all())
        assert bool((res.point_status == int(LANDED)).all())
        assert bool((res.nis == 0).all()) and bool((res.loglik == 0).all())
    finally:
        env.close()


def test_crashed_filter_without_measurements_keeps_the_mean_and_adds_q():
    """a CRASHED point is held by the physics, so the propagated points are the points: x stays xhat0 and P_tape[k] is
    P0 + k Q to the rounding of the factorisation and the moments.  The bar is that of the same recursion restated with
    the identity for the physics, float64 against longdouble, 100 x, floored at 1e-12."""
    import torch
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, inputs("lander3d", N, K, seed=43))
        p["st0"] = torch.full((N,), int(CRASHED), dtype=torch.uint8, device=env.device)
        p["z"] = torch.full_like(p["z"], float("nan"))
        res = _run(env, p, tape=True, points=True)
        assert bool((res.status == int(CRASHED)).all()) and bool(res.ok.all()) and bool((res.spread == 0).all())
        assert torch.equal(res.points_pred, res.points)
        x0, P0, Q = to_np(p["x0"]).T, to_np(p["P0"]), p["Q"]
        w, wl = ukf_ref.weights(), ukf_ref.weights(dtype=np.longdouble)
        x64, P64, xld, Pld = x0, P0, x0.astype(np.longdouble), P0.astype(np.longdouble)
        worst = 0.0
        for k in range(K):
            x64, P64 = ukf_ref.moments(ukf_ref.points(x64, P64, w[0])[0], w, Q)
            xld, Pld = ukf_ref.moments(ukf_ref.points(xld, Pld, wl[0], dtype=np.longdouble)[0], wl, Q, dtype=np.longdouble)
            for got, ref64, refld, exact in ((to_np(res.x[k]), x64, xld, x0),
                                             (to_np(res.P_tape[k]), P64, Pld, P0 + (k + 1) * Q)):
                bar = max(100.0 * ekf_ref.scaled(ref64, refld.astype(np.float64)), ukf_ref.FLOOR)
                e = ekf_ref.scaled(got, exact)
                worst = max(worst, e / bar)
                assert e <= bar, (k, e, bar)
        print("CRASHED start: worst ratio to the bar %.4f" % worst)
    finally:
        env.close()


def test_a_covariance_that_is_not_positive_definite_clears_ok_for_that_env_only():
    import torch
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, inputs("lander3d", N, K, seed=44, dense=False))
        good = _clone(_run(env, p, tape=True, points=True))
        assert bool(good.ok.all())
        bad_env = 72                                   # a hover start: its covariance is factored at every step
        assert p["grp"][bad_env] == "hover"
        p["P0"] = p["P0"].clone()
        p["P0"][bad_env] = -torch.eye(12, dtype=torch.float64, device=env.device)
        res = _run(env, p, tape=True, points=True)
        ok = to_np(res.ok)
        assert not ok[bad_env] and ok.sum() == N - 1
        others = torch.arange(N, device=env.device) != bad_env
        for a, b in zip(res, good):
            sel = (lambda t: t[others]) if a.shape[0] == N else (lambda t: t[:, others])
            assert torch.equal(sel(a), sel(b))
            assert bool(torch.isfinite(sel(a).double()).all())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. chunking
# ---------------------------------------------------------------------------------------------------------------------
def test_chunked_filter_is_the_single_call_bit_for_bit():
    import torch
    from gym_copter_amd import ukf
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, inputs("lander3d", N, K, seed=51, missing=0.1))
        setting = ukf_ref.SETTINGS[1]
        one = _clone(_run(env, p, setting, tape=True, points=True))
        args = (env, p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"])
        a, b, kp = setting
        for chunk in (5, None, 1):
            got = ukf(*args, status0=p["st0"], alpha=a, beta=b, kappa=kp, chunk=chunk, points=True)
            for name in TAPES + ("P", "ok"):
                assert torch.equal(getattr(got, name), getattr(one, name)), (chunk, name)
            assert torch.allclose(got.loglik, one.loglik, rtol=1e-13, atol=1e-12)
        got = ukf(*args, status0=p["st0"], alpha=a, beta=b, kappa=kp, chunk=7)
        assert got.points is None and torch.equal(got.P_tape, one.P_tape)
        with pytest.raises(ValueError, match="chunk must be"):
            ukf(*args, chunk=0)
        with pytest.raises(ValueError, match="z must be a tensor"):
            ukf(env, p["acts"], p["z"][:3], p["H"], p["r"], p["Q"], p["x0"], p["P0"])
    finally:
        env.close()
    # K = 1 and N = 1 pass the one-step checks
    env, penv = _pair("lander3d", 1)
    try:
        env.reset()
        penv.reset()
        p = _problem(env, inputs("lander3d", 1, 1, seed=52))
        res = _clone(_run(env, p, tape=True, points=True))
        assert res.x.shape == (1, 1, 12) and res.P_tape.shape == (1, 1, 12, 12) and res.points.shape == (1, 1, NP, 12)
        _check_steps("N=1 K=1", env, penv, p, res, ukf_ref.SETTINGS[0])
    finally:
        env.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. application
# ---------------------------------------------------------------------------------------------------------------------
def test_hover_tracking_is_consistent():
    """Section 19's Hover3D case (300 envs, 48 steps, positions and angles measured) with the default weights: the
    inputs of test_rollout_ukf_cpu.py::test_application_conditions_hold_on_the_oracle_restatement -- the same actions,
    starts and noise draws -- which satisfy the same four conditions on the float64 oracle."""
    import torch
    a, x0, xhat0, H, r = ekf_ref.app_inputs(E.AH, seed=1)
    n, steps = ekf_ref.APP_N, ekf_ref.APP_K
    env = E._env("hover3d", n, seed=3)
    try:
        env.reset()
        acts = E._dev(a, env)
        ro = env.rollout_states(acts, state={"x": x0, "status": np.full(n, AIRBORNE, np.uint8)})
        truth = ro.x.clone()
        assert bool((ro.status == AIRBORNE).all())
        noise = np.sqrt(r) * np.random.default_rng(2).standard_normal((steps, n, 6))
        z = truth @ E._dev(H, env).T + E._dev(noise, env)
        P0 = np.repeat(ekf_ref.APP_P0[None], n, axis=0)
        res = env.rollout_ukf(acts, z, H, r, ekf_ref.APP_Q, E._dev(xhat0, env), E._dev(P0, env))
        assert bool(res.ok.all()) and bool((res.spread == 0).all())
        rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
        fig = ekf_ref.app_conditions(to_np(res.x), to_np(torch.diagonal(res.P, dim1=1, dim2=2)), to_np(res.nis),
                                     to_np(truth), rmse0)
        print("mean NIS %.3f rmse %s sd %s" % (fig["mean_nis"], np.round(fig["rmse"], 4), np.round(fig["sd"], 4)))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_float32_outputs_overwrite_and_no_state_change():
    import torch
    n = 257
    env = E._env("lander3d", n, "float32", seed=3)
    try:
        env.reset()
        before = env.get_state()
        p = _problem(env, inputs("lander3d", n, K, seed=71, missing=0.2))
        r64 = _clone(_run(env, p, tape=True, points=True))
        for t in _run(env, p, tape=True, points=True):   # the env's buffers: poison them, then run again
            t.fill_(float("nan") if t.dtype.is_floating_point else 1)
        again = _run(env, p, tape=True, points=True)
        for a, b in zip(again, r64):
            assert torch.equal(a, b)                     # NaN-filled outputs are overwritten, the same bits on every call
        r32 = _run(env, p, tape=True, points=True, dtype=torch.float32)
        for name in ("P", "var", "nis", "loglik", "P_tape"):
            assert getattr(r32, name).dtype == torch.float32
            assert torch.equal(getattr(r32, name), getattr(r64, name).float()), name
        for name in ("x", "x_pred", "status", "spread", "ok", "points", "points_pred", "point_status"):
            assert getattr(r32, name).dtype == getattr(r64, name).dtype
            assert torch.equal(getattr(r32, name), getattr(r64, name)), name
        assert r32.ok.dtype == torch.bool and r32.points.dtype == torch.float64
        assert not any(t.requires_grad for t in r32)
        # status0 defaults to AIRBORNE
        air = dict(p, st0=torch.full((n,), AIRBORNE, dtype=torch.uint8, device=env.device))
        for a, b in zip(_clone(_run(env, dict(p, st0=None))), _run(env, air)):
            assert a is None or torch.equal(a, b)
        after = env.get_state()
        assert sorted(before) == sorted(after)
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]), equal_nan=True), key
    finally:
        env.close()


def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n = 4097
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = E._env("lander3d", n, "float32", seed=6)
    try:
        sh.reset()
        plain.reset()
        p = _problem(plain, inputs("lander3d", n, 4, seed=72))
        a = sh.rollout_ukf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], status0=p["st0"], alpha=0.5,
                           beta=2.0, kappa=0.0, tape=True, points=True)
        b = _run(plain, p, ukf_ref.SETTINGS[1], tape=True, points=True)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib
    n = 128
    env = E._env("lander3d", n, seed=1)
    try:
        env.reset()
        p = _problem(env, inputs("lander3d", n, 4, seed=74))
        base = dict(actions=p["acts"], z=p["z"], H=p["H"], r=p["r"], Q=p["Q"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        env.rollout_ukf(**base)
        badQ = p["Q"].copy()
        badQ[0, 1] += 1e-9
        nanr = p["r"].copy()
        nanr[0] = np.nan
        for kw, match in ((dict(actions=p["acts"][:, :n - 1]), "actions must have shape"),
                          (dict(z=p["z"][:2]), "z must have shape"), (dict(z=p["z"].cpu()), "z must be on"),
                          (dict(z=p["z"].long()), "z must be a floating-point"),
                          (dict(H=np.zeros((13, 12))), "H must have shape"), (dict(H=np.zeros((0, 12))), "H must have shape"),
                          (dict(H=p["H"][:, :11]), "H must have shape"), (dict(H=p["H"] * np.inf), "H must be finite"),
                          (dict(r=p["r"][:3]), "r must have shape"), (dict(r=-p["r"]), "r must be positive"),
                          (dict(r=p["r"] * 0), "r must be positive"), (dict(r=nanr), "r must be finite"),
                          (dict(Q=badQ), "Q must be symmetric"), (dict(Q=p["Q"][:6]), "Q must have shape"),
                          (dict(Q=p["Q"] * np.nan), "Q must be finite"),
                          (dict(x0=p["x0"][:6]), "x0 must have shape"), (dict(x0=p["x0"].cpu()), "x0 must be on"),
                          (dict(P0=p["P0"][:, :6]), "P0 must have shape"), (dict(P0=p["P0"].cpu()), "P0 must be on"),
                          (dict(P0=p["P0"].long()), "P0 must be a floating-point"),
                          (dict(status0=p["st0"][:5]), "status0"), (dict(dtype=torch.float16), "dtype must be"),
                          (dict(kappa=-12.0), r"12 \+ lambda"), (dict(alpha=0.0), r"12 \+ lambda"),
                          (dict(kappa=-20.0), r"12 \+ lambda"), (dict(beta=float("nan")), "must be finite")):
            args = dict(base)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_ukf(**args)
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), 4
        io.actions_dev, io.start_x_dev, io.start_status_dev = p["acts"].data_ptr(), p["x0"].data_ptr(), p["st0"].data_ptr()
        uio = _lib.RolloutUkfIO()
        uio.struct_size = C.sizeof(uio) + 8
        assert env._lib.cs_rollout_ukf(env._ctx, C.byref(io), C.byref(uio), None) == _lib.ERR_ABI
        # refused while a serve session is open
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_ukf(**base)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_ukf(**base)
    f32 = E._env("lander3d", n, seed=1, action_arith="float32")
    try:
        f32.reset()
        with pytest.raises(CopterStepError, match="float32 motor model"):
            f32.rollout_ukf(**base)
    finally:
        f32.close()
