"""The unscented Rauch-Tung-Striebel smoother on the device (cs_urts_smooth, CopterVecEnv.rollout_urts,
gym_copter_amd.smooth) over the tapes of a real rollout_ukf(..., tape=True, points=True) call: every backward step of the
kernel against the NumPy restatement (tests/urts_ref.py) on the kernel's OWN next row, which is section 19's rule.  For
row j the reference takes the device's x_s[j+1] and P_s[j+1], the filter's x, x_pred and P_tape, and the filter's own
points_pred[j+1] tape as the propagated points -- tests/test_gpu_rollout_ukf.py holds those to rollout_states bit for
bit, so the reference needs no physics; by induction from the given row K-1 down to the starting point the whole
recursion is verified.

The bar is section 20's: per output and env 100 x the float64 reference's own distance from the same step in
numpy.longdouble, floored at the larger of 1e-12 scaled and 12 eps kappa_2(P-) of that env; kappa_2 <= 1e8 is asserted for
every compared env, and Q's share of every env's x_s and P_s is asserted to be >= 1 000 x its bar, so that a dropped Q
cannot pass.  tests/test_urts_cpu.py runs the main case's inputs through the restatement on the float64 oracle first.  The
worst measured ratios to the bar are in DESIGN.md section 25."""
import zlib

import numpy as np
import pytest

import ekf_ref
import model_variants
import rts_ref
import test_gpu_rollout_ekf as E          # section 19's starts of every branch and the env helpers
import test_gpu_rollout_ukf as U          # the unscented filter's inputs and runs
import ukf_ref
import urts_ref
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K = E.N, E.K          # 300 envs: four whole wavefronts and one of 44 lanes; 16 steps
WORST = {}


def main_inputs(substeps):
    """the main case's inputs (NumPy only): section 19's starts, M = 6 measurements, 30 % of them missing"""
    return U.inputs("lander3d", N, K, seed=900 + substeps, M=6, missing=0.3)


def _filter(env, p, setting=ukf_ref.SETTINGS[0], **kw):
    return U._clone(U._run(env, p, setting, tape=True, points=True, **kw))


def _urts(env, p, filt, setting=ukf_ref.SETTINGS[0], **kw):
    a, b, k = setting
    return env.rollout_urts(p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], alpha=a, beta=b, kappa=k, **kw)


def _check_rows(name, p, filt, res, setting, lanes=None, end=None, share=True):
    """every backward step of res (a tape=True result, cloned) against one reference step from the filter's tapes (its
    propagated points among them) and the device's own next row"""
    import torch
    steps, n = res.x.shape[:2]
    lanes = slice(None) if lanes is None else lanes
    Q = p["Q"]
    w, wl = ukf_ref.weights(*setting), ukf_ref.weights(*setting, dtype=np.longdouble)
    if end is None:
        assert torch.equal(res.x[-1], filt.x[-1]) and torch.equal(res.P_tape[-1], filt.P_tape[-1])
    else:
        up = torch.triu(end[1])
        assert torch.equal(res.x[-1], end[0].T) and torch.equal(res.P_tape[-1], up + torch.triu(end[1], 1).transpose(1, 2))
    assert torch.equal(res.var, torch.diagonal(res.P_tape, dim1=2, dim2=3))
    assert torch.equal(res.P_tape, res.P_tape.transpose(2, 3)) and torch.equal(res.P0, res.P0.transpose(1, 2))
    ok = np.ones(n, bool)[lanes]
    worst, least, kmax = {}, {}, 0.0
    for j in range(steps - 2, -2, -1):
        if j >= 0:
            xf, Pf, st = to_np(filt.x[j][lanes]), to_np(filt.P_tape[j][lanes]), to_np(filt.status[j][lanes])
            got = dict(x=to_np(res.x[j][lanes]), P=to_np(res.P_tape[j][lanes]), var=to_np(res.var[j][lanes]))
        else:
            xf, Pf, st = to_np(p["x0"].T[lanes]), to_np(p["P0"][lanes]), to_np(p["st0"][lanes])
            got = dict(x=to_np(res.x0.T[lanes]), P=to_np(res.P0[lanes]))
            got["var"] = np.diagonal(got["P"], axis1=1, axis2=2)
        landed = st == LANDED
        y = to_np(filt.points_pred[j + 1][lanes])
        nxt = (to_np(filt.x_pred[j + 1][lanes]), to_np(res.x[j + 1][lanes]), to_np(res.P_tape[j + 1][lanes]))
        r64 = urts_ref.one_step(y, landed, Pf, xf, *nxt, w, Q)
        rld = urts_ref.one_step(y, landed, Pf, xf, *nxt, wl, Q, dtype=np.longdouble)
        ok &= r64["ok"]
        bar = urts_ref.bars(r64, rld)                    # (asserts kappa_2(P-) <= 1e8 for every env)
        kmax = max(kmax, float(rts_ref.cond(r64["P_pred"]).max()))
        if share:                                        # Q's share of every env's row is far above its bar
            noq = urts_ref.one_step(y, landed, Pf, xf, *nxt, w, 0.0 * np.asarray(Q))
            for key in ("x", "P"):
                with np.errstate(invalid="ignore"):
                    s = rts_ref.scaled_env(noq[key], r64[key])
                s = np.where(np.isnan(s), np.inf, s)
                least[key] = min(least.get(key, np.inf), float(np.min(s / bar[key])))
                assert np.all(s >= 1e3 * bar[key]), (name, key, j, float(np.min(s / bar[key])))
        for key, g in got.items():
            e = rts_ref.scaled_env(g, r64[key])
            worst[key] = max(worst.get(key, 0.0), float(np.max(e / bar[key])))
            assert np.all(e <= bar[key]), (name, key, j, int(np.argmax(e / bar[key])), float(np.max(e / bar[key])))
    assert np.array_equal(to_np(res.ok[lanes]), ok)
    WORST[name] = worst
    print("%s: worst error / bar " % name + " ".join("%s %.3g" % kv for kv in worst.items()) +
          "; kappa_2(P-) <= %.1e; Q's least share / bar " % kmax + " ".join("%s %.1e" % kv for kv in least.items()))


def _same(a, b):
    import torch
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. through every branch under the three weight settings, and the exact statements
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ukf_ref.SETTINGS, ids=lambda s: "a%g-b%g-k%g" % s)
@pytest.mark.parametrize("substeps", [1, 10])
def test_every_row_through_every_branch(substeps, setting):
    import torch
    env = E._env("lander3d", N, substeps=substeps, seed=3)
    try:
        env.reset()
        before = env.get_state()
        p = U._problem(env, main_inputs(substeps))
        assert 0.25 < float(torch.isnan(p["z"]).double().mean()) < 0.35
        filt = _filter(env, p, setting)
        assert bool(filt.ok.all())
        res = U._clone(_urts(env, p, filt, setting))
        _check_rows("lander3d substeps=%d %r" % (substeps, setting), p, filt, res, setting)
        spread, landed = float((filt.spread > 0).double().mean()), float((filt.status == LANDED).double().mean())
        print("spread > 0 in %.3f and LANDED rows %.3f of the (j, env) pairs" % (spread, landed))
        assert spread >= 0.01 and landed >= 0.01
        for g in E.GROUPS:
            assert np.char.startswith(p["grp"], g).sum() >= N // 12, g
        assert bool(res.ok.all())
        # the same bits in every other output without the tape, and on every call over NaN-filled buffers
        plain = _urts(env, p, filt, setting, tape=False)
        assert plain.P_tape is None
        assert _same([t for t, nm in zip(plain, plain._fields) if nm != "P_tape"],
                     [t for t, nm in zip(res, res._fields) if nm != "P_tape"])
        for t in _urts(env, p, filt, setting):
            t.fill_(float("nan") if t.dtype.is_floating_point else 1)
        assert _same(_urts(env, p, filt, setting), res)
        # float32 outputs are the float64 ones rounded
        r32 = _urts(env, p, filt, setting, dtype=torch.float32)
        for nm in ("P_tape", "var", "P0"):
            assert getattr(r32, nm).dtype == torch.float32 and torch.equal(getattr(r32, nm), getattr(res, nm).float()), nm
        for nm in ("x", "x0", "ok"):
            assert torch.equal(getattr(r32, nm), getattr(res, nm)), nm
        assert r32.ok.dtype == torch.bool and not any(t.requires_grad for t in r32)
        after = env.get_state()
        assert sorted(before) == sorted(after)
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]), equal_nan=True), key
    finally:
        env.close()


def test_a_given_end_row_is_written_out_and_smoothed_from():
    import torch
    rng = np.random.default_rng(911)
    setting = ukf_ref.SETTINGS[1]
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = U._problem(env, main_inputs(1))
        filt = _filter(env, p, setting)
        end = (filt.x[-1].T.contiguous() + 0.01 * E._dev(rng.standard_normal((12, N)), env),
               0.5 * filt.P_tape[-1] + E._dev(np.repeat(ekf_ref.test_Q()[None], N, axis=0), env))
        end[1][:, 5, 2] = 77.0                           # (below the diagonal: not read)
        res = U._clone(_urts(env, p, filt, setting, end=end))
        _check_rows("lander3d end=", p, filt, res, setting, end=end)
        assert not torch.equal(res.x[0], _urts(env, p, filt, setting).x[0])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. no measurements: the smoother returns the filter; rows the physics holds: the extended smoother's with A = I
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ukf_ref.SETTINGS[:2], ids=lambda s: "a%g-b%g-k%g" % s)
def test_without_measurements_the_smoothed_tape_is_the_filters(setting):
    """z all NaN: P_f[j+1] is the filter's prior, which the smoother makes again bit for bit from the same points, so D
    and the mean's increment are exact zeros (numeric equality: a zero's sign is free).  LANDED and CRASHED starts are
    among the envs."""
    import torch
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = U._problem(env, main_inputs(1))
        p["z"] = torch.full_like(p["z"], float("nan"))
        assert int((p["st0"] == LANDED).sum()) > 0 and int((p["st0"] == CRASHED).sum()) > 0
        filt = _filter(env, p, setting)
        res = _urts(env, p, filt, setting)
        assert bool(res.ok.all())
        assert bool((res.x == filt.x).all()) and bool((res.P_tape == filt.P_tape).all())
        assert bool((res.var == filt.var).all())
        assert bool((res.x0 == p["x0"]).all())
        up = torch.triu(p["P0"])
        assert bool((res.P0 == up + torch.triu(p["P0"], 1).transpose(1, 2)).all())
    finally:
        env.close()


def test_rows_the_physics_holds_are_the_extended_smoothers_with_the_identity():
    """where all 25 points of a step stayed CRASHED the physics is the identity: 2 wi gamma^2 = 1 makes W = P_f and
    P- = P_f + Q to the points' rounding (eps |x| / (gamma L) <~ 1e-13 for these P0), so x_s and P_s agree with rts_ref
    under A = I to 1e-9 scaled; a wrong weight or column order shows at order 1."""
    setting = ukf_ref.SETTINGS[1]
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = U._problem(env, main_inputs(1))
        filt = _filter(env, p, setting)
        res = U._clone(_urts(env, p, filt, setting))
        eye = np.eye(12)[None]
        rows, worst = 0, 0.0
        for j in range(K - 2, -2, -1):
            held = to_np((filt.point_status[j + 1] == CRASHED).all(dim=1))
            if j >= 0:
                held &= to_np(filt.status[j]) == CRASHED
                xf, Pf, got = to_np(filt.x[j]), to_np(filt.P_tape[j]), (to_np(res.x[j]), to_np(res.P_tape[j]))
            else:
                held &= to_np(p["st0"]) == CRASHED
                xf, Pf, got = to_np(p["x0"].T), to_np(p["P0"]), (to_np(res.x0.T), to_np(res.P0))
            assert held.sum() >= N // 12, (j, held.sum())
            ref = rts_ref.one_step(np.repeat(eye, int(held.sum()), axis=0), Pf[held], xf[held], to_np(filt.x_pred[j + 1])[held],
                                   to_np(res.x[j + 1])[held], to_np(res.P_tape[j + 1])[held], p["Q"])
            for g, key in zip(got, ("x", "P")):
                worst = max(worst, float(rts_ref.scaled_env(g[held], ref[key]).max()))
            rows += int(held.sum())
        print("%d rows held by the physics: worst scaled distance from A = I %.2e" % (rows, worst))
        assert worst <= 1e-9
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. chunking
# ---------------------------------------------------------------------------------------------------------------------
def test_chunked_smoother_is_the_single_call_bit_for_bit():
    from gym_copter_amd import smooth
    setting = ukf_ref.SETTINGS[1]
    a, b, kp = setting
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs("lander3d", N, K, seed=931, missing=0.1))
        filt = _filter(env, p, setting)
        one = U._clone(_urts(env, p, filt, setting))
        for chunk in (5, 1, None):
            got = smooth(env, p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], chunk=chunk, alpha=a, beta=b,
                         kappa=kp)
            assert _same(got, one), chunk
    finally:
        env.close()
    # N = 1 with K = 1 runs and passes the one-step bar for the smoothed starting point
    env = E._env("lander3d", 1, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs("lander3d", 1, 1, seed=932))
        filt = _filter(env, p)
        res = U._clone(_urts(env, p, filt))
        assert res.x.shape == (1, 1, 12) and res.P_tape.shape == (1, 1, 12, 12) and res.x0.shape == (12, 1)
        _check_rows("N=1 K=1", p, filt, res, ukf_ref.SETTINGS[0])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. ok
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["P_tape", "P0"])
def test_a_nonpositive_pivot_clears_ok_for_that_env_only(where):
    import torch
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = U._problem(env, main_inputs(1))
        filt = _filter(env, p)
        good = U._clone(_urts(env, p, filt))
        assert bool(good.ok.all())
        bad_env, row = 72, 6                             # a hover start: its covariance is factored in every row
        assert p["grp"][bad_env] == "hover" and int(filt.status[row, bad_env]) == AIRBORNE
        minus = -torch.eye(12, dtype=torch.float64, device=env.device)
        if where == "P_tape":
            tape = filt.P_tape.clone()
            tape[row, bad_env] = minus
            res = _urts(env, p, filt._replace(P_tape=tape))
        else:                                            # the factorisation of the starting point's covariance
            P0 = p["P0"].clone()
            P0[bad_env] = minus
            res = _urts(env, dict(p, P0=P0), filt)
        ok = to_np(res.ok)
        assert not ok[bad_env] and ok.sum() == N - 1
        others = torch.arange(N, device=env.device) != bad_env
        for a, b in zip(res, good):
            sel = (lambda t: t[others]) if a.shape[0] == N else (lambda t: t[:, others])
            assert torch.equal(sel(a), sel(b))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. shapes and models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,mode,M", [("hover3d", "float32", 6), ("lander2d", "float64", 1), ("hover1d", "float64", 12)])
def test_every_row_for_other_tasks_storage_modes_and_measurement_counts(task, mode, M):
    seed = zlib.crc32(repr((task, mode, M, "urts")).encode())
    setting = ukf_ref.SETTINGS[seed % 2]
    env = E._env(task, N, mode, seed=3)
    try:
        env.reset()
        p = U._problem(env, U.inputs(task, N, K, seed=seed, M=M))
        filt = _filter(env, p, setting)
        res = U._clone(_urts(env, p, filt, setting))
        _check_rows("%s %s M=%d %r" % (task, mode, M, setting), p, filt, res, setting)
    finally:
        env.close()


@pytest.mark.parametrize("variant", ["vehicles", "mars_gyro"])
def test_every_row_under_model_variants(variant):
    rng = np.random.default_rng(zlib.crc32((variant + " urts").encode()))
    setting = ukf_ref.SETTINGS[0]
    env = E._env("lander3d", N, seed=3, **model_variants.env_kwargs(variant))
    ref = E._env("lander3d", N, seed=3)
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        ref.reset()
        p = U._problem(env, U.inputs("lander3d", N, K, seed=int(rng.integers(1 << 30)), ah=model_variants.hover(variant)))
        filt = _filter(env, p, setting)
        res = U._clone(_urts(env, p, filt, setting))
        _check_rows("lander3d %s" % variant, p, filt, res, setting)
        # the default model gives another x_s, from the same tapes, in every lane that flies
        other = _urts(ref, p, filt, setting)
        same = np.all(to_np(res.x).view(np.uint64) == to_np(other.x).view(np.uint64), axis=(0, 2))
        same &= np.all(to_np(res.x0).view(np.uint64) == to_np(other.x0).view(np.uint64), axis=0)
        flies = np.isin(p["grp"], ("hover", "clip", "clip_hi", "soft_mid", "hard_mid"))
        assert flies.sum() >= N // 3 and not np.any(same & flies), np.flatnonzero(same & flies)[:8]
    finally:
        env.close()
        ref.close()


def test_offsets_past_4_gib():
    """the tapes [K,N,12,12] float64 are 4.8 GB at K = 4 with 2^20 envs, and the filter's point tapes 10 GB; the last
    1 000 envs pass the one-step bar."""
    import torch
    from gym_copter_amd import measure
    n, steps, M = 1 << 20, 4, 6
    assert steps * n * 144 * 8 > 4 << 30 > (steps - 1) * n * 144 * 8
    rng = np.random.default_rng(973)
    setting = ukf_ref.SETTINGS[0]
    env = E._env("lander3d", n, seed=9)
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        ah = float(E.AH)
        acts = torch.rand((steps, n, 4), generator=g, device=env.device, dtype=torch.float32) * 0.2 * ah + 0.9 * ah
        x0 = torch.randn((12, n), generator=g, device=env.device, dtype=torch.float64) * 0.2
        x0[4] -= 6.0
        st0 = torch.full((n,), AIRBORNE, dtype=torch.uint8, device=env.device)
        H, r = E._model(rng, M, True)
        P0 = (torch.eye(12, dtype=torch.float64, device=env.device) * 0.05).expand(n, 12, 12).contiguous()
        P0 = P0 * (1.0 + torch.rand((n, 1, 1), generator=g, device=env.device, dtype=torch.float64))
        truth = env.rollout_states(acts, state={"x": x0, "status": st0}).x
        z = measure(truth, H, r, 7)
        del truth
        p = dict(acts=acts, z=z, H=H, r=r, Q=ekf_ref.test_Q(), x0=x0, P0=P0, st0=st0)
        filt = U._run(env, p, setting, tape=True, points=True)
        res = _urts(env, p, filt, setting)
        assert bool(res.ok.all())
        _check_rows("2^20 envs, last 1000", p, filt, res, setting, lanes=slice(n - 1000, n))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. application
# ---------------------------------------------------------------------------------------------------------------------
def test_hover_smoothing_beats_the_filter_and_is_consistent():
    """Section 20's Hover3D case (300 envs, 48 steps, positions and angles measured) with the unscented filter's inputs
    and noise draws: those of test_urts_cpu.py::test_application_conditions_hold_on_the_oracle_restatement, which meet
    section 20's thresholds on the float64 oracle -- smoothed / filtered RMSE <= 0.6 in the measured and <= 0.3 in the
    unmeasured slots, RMSE / sd in [0.8, 1.25], var_s <= var_f (1 + 1e-9) everywhere -- so they are the device's too."""
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
        P0 = E._dev(np.repeat(ekf_ref.APP_P0[None], n, axis=0), env)
        xh = E._dev(xhat0, env)
        filt = env.rollout_ukf(acts, z, H, r, ekf_ref.APP_Q, xh, P0, tape=True)
        res = env.rollout_urts(acts, filt, ekf_ref.APP_Q, xh, P0)
        assert bool(filt.ok.all()) and bool(res.ok.all())
        rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
        fig = rts_ref.app_conditions(to_np(res.x), to_np(res.var), to_np(res.x0.T),
                                     to_np(torch.diagonal(res.P0, dim1=1, dim2=2)), to_np(filt.x), to_np(filt.var),
                                     to_np(truth), x0.T, rmse0)
        print(fig)
    finally:
        env.close()


def test_report_the_smoothed_start_through_touchdown_beside_the_extended_smoother():
    """Reported, not asserted: Lander3D descents that touch down inside the horizon, a start known to sd 0.1 .. 0.3; the
    RMSE of the smoothed starting point under rollout_ukf + rollout_urts and under rollout_ekf + rollout_rts on the same
    measurements.  Only that both run and say ok is asserted."""
    rng = np.random.default_rng(981)
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = U.inputs("lander3d", N, K, seed=982, dense=False)
        mid = np.isin(p["grp"], ("soft_mid", "hard_mid"))
        P0 = np.repeat(np.diag(np.tile([0.01, 0.09], 6))[None], N, axis=0)
        xhat0 = p["x0"] + np.sqrt(np.diagonal(P0, axis1=1, axis2=2)).T * rng.standard_normal((12, N))
        q = U._problem(env, p)                           # (z from the true starts)
        q.update(x0=E._dev(xhat0, env), P0=E._dev(P0, env))
        fu = U._clone(U._run(env, q, tape=True))
        su = U._clone(_urts(env, q, fu))
        fe = E._clone(E._run(env, q, tape=True))
        se = E._clone(env.rollout_rts(q["acts"], fe, q["Q"], q["x0"], q["P0"], status0=q["st0"]))
        ok = mid & to_np(su.ok) & to_np(se.ok) & to_np(fu.ok) & to_np(fe.ok)
        assert ok.sum() >= mid.sum() // 2
        err = lambda s: np.sqrt(np.mean((to_np(s.x0)[:, ok] - p["x0"][:, ok]) ** 2, axis=1))     # noqa: E731
        print("touchdown lanes %d: smoothed-start RMSE per slot\n  ukf + urts %s\n  ekf + rts  %s\n  prior      %s" % (
            ok.sum(), np.round(err(su), 4), np.round(err(se), 4),
            np.round(np.sqrt(np.mean((xhat0 - p["x0"])[:, ok] ** 2, axis=1)), 4)))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_single_rank_matches_plain_env():
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n = 4097
    setting = ukf_ref.SETTINGS[1]
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = E._env("lander3d", n, "float32", seed=6)
    try:
        sh.reset()
        plain.reset()
        p = U._problem(plain, U.inputs("lander3d", n, 6, seed=972))
        filt = _filter(plain, p, setting)
        a = sh.rollout_urts(p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], alpha=0.5, beta=2.0, kappa=0.0)
        b = _urts(plain, p, filt, setting)
        assert _same(a, b)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib, smooth
    n = 128
    env = E._env("lander3d", n, seed=1)
    try:
        env.reset()
        p = U._problem(env, U.inputs("lander3d", n, 4, seed=974))
        filt = _filter(env, p)
        base = dict(actions=p["acts"], filt=filt, Q=p["Q"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        res = env.rollout_urts(**base)
        # status0 defaults to AIRBORNE
        air = torch.full((n,), AIRBORNE, dtype=torch.uint8, device=env.device)
        assert _same(U._clone(env.rollout_urts(**dict(base, status0=None))), env.rollout_urts(**dict(base, status0=air)))
        # the smoothed starting point of a call may be the `end` of the next, although it is that call's own buffer
        res = env.rollout_urts(**base)
        x0c, P0c = res.x0.clone(), res.P0.clone()
        assert _same(U._clone(env.rollout_urts(**dict(base, end=(res.x0, res.P0)))),
                     env.rollout_urts(**dict(base, end=(x0c, P0c))))
        badQ = p["Q"].copy()
        badQ[0, 1] += 1e-9
        f32 = U._run(env, p, tape=True, dtype=torch.float32)
        f32 = f32._replace(x=f32.x.clone(), x_pred=f32.x_pred.clone(), status=f32.status.clone(),
                           P_tape=f32.P_tape.clone())
        ekf = E._clone(E._run(env, p, tape=True))
        for kw, match in ((dict(actions=p["acts"][:, :n - 1]), "actions must have shape"),
                          (dict(filt=filt._replace(P_tape=None)), "no P_tape"),
                          (dict(filt=f32), "must be float64"),
                          (dict(filt=tuple(filt)), "UkfResult"), (dict(filt=ekf), "UkfResult"),
                          (dict(filt=filt._replace(P_tape=filt.P_tape[:2])), "filt.P_tape must have shape"),
                          (dict(filt=filt._replace(x=filt.x[:, :, :6])), "filt.x must have shape"),
                          (dict(filt=filt._replace(x_pred=filt.x_pred.cpu())), "filt.x_pred must be a contiguous"),
                          (dict(filt=filt._replace(status=filt.status.long())), "filt.status must be a contiguous"),
                          (dict(actions=p["acts"][:2]), "filt.x must have shape"),
                          (dict(Q=badQ), "Q must be symmetric"), (dict(Q=p["Q"][:6]), "Q must have shape"),
                          (dict(Q=p["Q"] * np.nan), "Q must be finite"),
                          (dict(x0=p["x0"][:6]), "x0 must have shape"), (dict(x0=p["x0"].cpu()), "x0 must be on"),
                          (dict(P0=p["P0"][:, :6]), "P0 must have shape"),
                          (dict(P0=p["P0"].long()), "P0 must be a floating-point"),
                          (dict(status0=p["st0"][:5]), "status0"),
                          (dict(end=(p["x0"], None)), "both or neither"), (dict(end=(None, p["P0"])), "both or neither"),
                          (dict(end=(p["x0"],)), "both or neither"),
                          (dict(end=(p["x0"][:6], p["P0"])), "must have shape"),
                          (dict(end=(p["x0"], p["P0"][:, :6])), "must have shape"),
                          (dict(kappa=-12.0), r"12 \+ lambda"), (dict(alpha=0.0), r"12 \+ lambda"),
                          (dict(beta=float("nan")), "must be finite"),
                          (dict(dtype=torch.float16), "dtype must be")):
            args = dict(base)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_urts(**args)
        with pytest.raises(ValueError, match="chunk must be"):
            smooth(env, p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], chunk=0)
        with pytest.raises(ValueError, match="P_tape"):
            smooth(env, p["acts"], filt._replace(P_tape=None), p["Q"], p["x0"], p["P0"], status0=p["st0"])
        with pytest.raises(ValueError, match="EkfResult or a UkfResult"):
            smooth(env, p["acts"], tuple(filt), p["Q"], p["x0"], p["P0"], status0=p["st0"])
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), 4
        io.actions_dev, io.start_x_dev, io.start_status_dev = p["acts"].data_ptr(), p["x0"].data_ptr(), p["st0"].data_ptr()
        sio = _lib.RolloutUrtsIO()
        sio.struct_size = C.sizeof(sio) + 8
        assert env._lib.cs_urts_smooth(env._ctx, C.byref(io), C.byref(sio), None) == _lib.ERR_ABI
        # refused while a serve session is open
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_urts(**base)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_urts(**base)
    f32env = E._env("lander3d", n, seed=1, action_arith="float32")
    try:
        f32env.reset()
        with pytest.raises(ValueError, match="float32"):
            f32env.rollout_urts(**base)
    finally:
        f32env.close()
