"""The Rauch-Tung-Striebel smoother on the device (cs_rollout_rts, CopterVecEnv.rollout_rts, gym_copter_amd.smooth) over
the tapes of a real rollout_ekf call: every backward step of the kernel against the NumPy restatement (tests/rts_ref.py)
on the kernel's OWN next row, which is section 19's rule.  For row j the reference takes the device's x_s[j+1] and
P_s[j+1], the filter's tapes (inputs) and A = step_jacobian(actions[j+1], state = (x_f[j], status_f[j])).dx; by induction
from the given row K-1 down to the starting point the whole recursion is verified.

The bar per output and env is 100 x the float64 reference's own distance from the same step in numpy.longdouble, floored
at the larger of 1e-12 scaled and 12 eps kappa_2(P-) of that env; kappa_2 <= 1e8 is asserted for every compared env, and
Q's share of every env's x_s and P_s is asserted to be >= 1 000 x its bar, so that a dropped Q cannot pass.  The worst
measured ratios to the bar are in DESIGN.md section 20."""
import zlib

import numpy as np
import pytest

import ekf_ref
import model_variants
import rts_ref
import test_gpu_rollout_ekf as E          # its starts of every branch, its problems and its env helpers
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K = E.N, E.K          # 300 envs: four whole wavefronts and one of 44 lanes; 16 steps
WORST = {}


def _filter(env, p, **kw):
    return E._clone(E._run(env, p, tape=True, **kw))


def _rts(env, p, filt, **kw):
    return env.rollout_rts(p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], **kw)


def _check_rows(name, env, p, filt, res, lanes=None, end=None, share=True):
    """every backward step of res (a tape=True result, cloned) against one reference step from the filter's tapes and the
    device's own next row; returns the branch bits step_jacobian reports at the filter's points [K,n] (row j = -1 first)"""
    import torch
    steps, n = res.x.shape[:2]
    lanes = slice(None) if lanes is None else lanes
    acts, Q = p["acts"], p["Q"]
    if end is None:
        assert torch.equal(res.x[-1], filt.x[-1]) and torch.equal(res.P_tape[-1], filt.P_tape[-1])
    else:
        assert torch.equal(res.x[-1], end[0].T) and torch.equal(res.P_tape[-1], end[1])
    assert torch.equal(res.var, torch.diagonal(res.P_tape, dim1=2, dim2=3))
    assert torch.equal(res.P_tape, res.P_tape.transpose(2, 3)) and torch.equal(res.P0, res.P0.transpose(1, 2))
    ok = np.ones(n, bool)[lanes]
    bits, worst, least = [], {}, {}
    for j in range(steps - 2, -2, -1):
        if j >= 0:
            state = {"x": filt.x[j].T.contiguous(), "status": filt.status[j]}
            xf, Pf = to_np(filt.x[j][lanes]), to_np(filt.P_tape[j][lanes])
            got = dict(x=to_np(res.x[j][lanes]), P=to_np(res.P_tape[j][lanes]), var=to_np(res.var[j][lanes]))
        else:
            state = {"x": p["x0"], "status": p["st0"]}
            xf, Pf = to_np(p["x0"].T[lanes]), to_np(p["P0"][lanes])
            got = dict(x=to_np(res.x0.T[lanes]), P=to_np(res.P0[lanes]))
            got["var"] = np.diagonal(got["P"], axis1=1, axis2=2)
        jac = env.step_jacobian(acts[j + 1], state=state)
        A = to_np(jac.dx[lanes]).astype(np.float64)
        bits.append(to_np(jac.branch))
        nxt = (to_np(filt.x_pred[j + 1][lanes]), to_np(res.x[j + 1][lanes]), to_np(res.P_tape[j + 1][lanes]))
        r64 = rts_ref.one_step(A, Pf, xf, *nxt, Q)
        rld = rts_ref.one_step(A, Pf, xf, *nxt, Q, dtype=np.longdouble)
        ok &= r64["ok"]
        bar = rts_ref.bars(r64, rld)                     # (asserts kappa_2(P-) <= 1e8 for every env)
        if share:                                        # Q's share of every env's row is far above its bar
            noq = rts_ref.one_step(A, Pf, xf, *nxt, 0.0 * np.asarray(Q))
            for key in ("x", "P"):
                with np.errstate(invalid="ignore"):
                    s = rts_ref.scaled_env(noq[key], r64[key])
                s = np.where(np.isnan(s), np.inf, s)     # (without Q a LEVELING step's prior is singular)
                least[key] = min(least.get(key, np.inf), float(np.min(s / bar[key])))
                assert np.all(s >= 1e3 * bar[key]), (name, key, j, float(np.min(s / bar[key])))
        for key, g in got.items():
            e = rts_ref.scaled_env(g, r64[key])
            worst[key] = max(worst.get(key, 0.0), float(np.max(e / bar[key])))
            assert np.all(e <= bar[key]), (name, key, j, int(np.argmax(e / bar[key])), float(np.max(e / bar[key])))
    assert np.array_equal(to_np(res.ok[lanes]), ok)
    WORST[name] = worst
    print("%s: worst ratio to the bar " % name + " ".join("%s %.5f" % kv for kv in worst.items()) +
          "; Q's least share / bar " + " ".join("%s %.1e" % kv for kv in least.items()))
    return np.array(bits)


def _same(a, b):
    import torch
    return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. through every branch, and the exact statements
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
def test_every_row_through_every_branch(substeps):
    import torch
    from gym_copter_amd import _lib
    rng = np.random.default_rng(800 + substeps)
    env = E._env("lander3d", N, substeps=substeps, seed=3)
    try:
        env.reset()
        before = env.get_state()
        p = E._problem(env, "lander3d", rng)
        filt = _filter(env, p)
        assert bool(filt.ok.all())
        res = E._clone(_rts(env, p, filt))
        bits = _check_rows("lander3d substeps=%d" % substeps, env, p, filt, res)
        frac = {nm: float(((bits & b) != 0).mean()) for nm, b in (
            ("INTEGRATED", _lib.JAC_INTEGRATED), ("LANDED", _lib.JAC_LANDED), ("CONTACT", _lib.JAC_CONTACT),
            ("CRASHED", _lib.JAC_CRASHED), ("CLIPPED", _lib.JAC_CLIPPED), ("LEVELING", _lib.JAC_LEVELING))}
        print("branch shares of the (j, env) pairs: " + " ".join("%s %.3f" % kv for kv in frac.items()))
        for nm in ("INTEGRATED", "LANDED", "CONTACT", "CRASHED", "CLIPPED"):
            assert frac[nm] >= 0.01, (nm, frac[nm])
        assert bool(res.ok.all())
        # the same bits in every other output without the tape, and on every call over NaN-filled buffers
        plain = _rts(env, p, filt, tape=False)
        assert plain.P_tape is None
        assert _same([t for t, nm in zip(plain, plain._fields) if nm != "P_tape"],
                     [t for t, nm in zip(res, res._fields) if nm != "P_tape"])
        for t in _rts(env, p, filt):
            t.fill_(float("nan") if t.dtype.is_floating_point else 1)
        assert _same(_rts(env, p, filt), res)
        # float32 outputs are the float64 ones rounded
        r32 = _rts(env, p, filt, dtype=torch.float32)
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
    rng = np.random.default_rng(811)
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = E._problem(env, "lander3d", rng)
        filt = _filter(env, p)
        end = (filt.x[-1].T.contiguous() + 0.01 * E._dev(rng.standard_normal((12, N)), env),
               0.5 * filt.P_tape[-1] + E._dev(np.repeat(ekf_ref.test_Q()[None], N, axis=0), env))
        res = E._clone(_rts(env, p, filt, end=end))
        _check_rows("lander3d end=", env, p, filt, res, end=end)
        assert not torch.equal(res.x[0], _rts(env, p, filt).x[0])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. no measurements: the smoother returns the filter
# ---------------------------------------------------------------------------------------------------------------------
def test_without_measurements_the_smoothed_tape_is_the_filters():
    """z all NaN: P_f[j+1] is the filter's prior, which the smoother makes again bit for bit, so D and the mean's
    increment are exact zeros (numeric equality: a zero's sign is free).  LANDED and CRASHED starts are among the envs."""
    import torch
    rng = np.random.default_rng(821)
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = E._problem(env, "lander3d", rng)
        p["z"] = torch.full_like(p["z"], float("nan"))
        assert int((p["st0"] == LANDED).sum()) > 0 and int((p["st0"] == CRASHED).sum()) > 0
        filt = _filter(env, p)
        res = _rts(env, p, filt)
        assert bool(res.ok.all())
        assert bool((res.x == filt.x).all()) and bool((res.P_tape == filt.P_tape).all())
        assert bool((res.var == filt.var).all())
        assert bool((res.x0 == p["x0"]).all())
        up = torch.triu(p["P0"])
        assert bool((res.P0 == up + torch.triu(p["P0"], 1).transpose(1, 2)).all())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. chunking
# ---------------------------------------------------------------------------------------------------------------------
def test_chunked_smoother_is_the_single_call_bit_for_bit():
    from gym_copter_amd import smooth
    rng = np.random.default_rng(831)
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = E._problem(env, "lander3d", rng, missing=0.1)
        filt = _filter(env, p)
        one = E._clone(_rts(env, p, filt))
        for chunk in (5, 1, None):
            got = smooth(env, p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], chunk=chunk)
            assert _same(got, one), chunk
    finally:
        env.close()
    # N = 1 with K = 1 runs and passes the one-step bar for the smoothed starting point
    env = E._env("lander3d", 1, seed=3)
    try:
        env.reset()
        p = E._problem(env, "lander3d", rng, steps=1)
        filt = _filter(env, p)
        res = E._clone(_rts(env, p, filt))
        assert res.x.shape == (1, 1, 12) and res.P_tape.shape == (1, 1, 12, 12) and res.x0.shape == (12, 1)
        _check_rows("N=1 K=1", env, p, filt, res)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. ok
# ---------------------------------------------------------------------------------------------------------------------
def test_a_nonpositive_pivot_clears_ok_for_that_env_only():
    import torch
    rng = np.random.default_rng(841)
    env = E._env("lander3d", N, seed=3)
    try:
        env.reset()
        p = E._problem(env, "lander3d", rng)
        filt = _filter(env, p)
        good = E._clone(_rts(env, p, filt))
        assert bool(good.ok.all())
        bad_env, row = 77, 6                             # (-I + Q: the first pivot is negative under every branch)
        tape = filt.P_tape.clone()
        tape[row, bad_env] = -torch.eye(12, dtype=torch.float64, device=env.device)
        res = _rts(env, p, filt._replace(P_tape=tape))
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
@pytest.mark.parametrize("task,mode", [("hover3d", "float32"), ("lander2d", "float64"), ("hover1d", "float64")])
def test_every_row_for_other_tasks_and_storage_modes(task, mode):
    rng = np.random.default_rng(zlib.crc32(repr((task, mode, "rts")).encode()))
    env = E._env(task, N, mode, seed=3)
    try:
        env.reset()
        p = E._problem(env, task, rng)
        filt = _filter(env, p)
        res = E._clone(_rts(env, p, filt))
        _check_rows("%s %s" % (task, mode), env, p, filt, res)
    finally:
        env.close()


@pytest.mark.parametrize("variant", ["vehicles", "mars_gyro"])
def test_every_row_under_model_variants(variant):
    rng = np.random.default_rng(zlib.crc32((variant + " rts").encode()))
    env = E._env("lander3d", N, seed=3, **model_variants.env_kwargs(variant))
    ref = E._env("lander3d", N, seed=3)
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        ref.reset()
        p = E._problem(env, "lander3d", rng, ah=model_variants.hover(variant))
        filt = _filter(env, p)
        res = E._clone(_rts(env, p, filt))
        _check_rows("lander3d %s" % variant, env, p, filt, res)
        # the default model gives another x_s, from the same tapes, in every lane that flies
        other = _rts(ref, p, filt)
        same = np.all(to_np(res.x).view(np.uint64) == to_np(other.x).view(np.uint64), axis=(0, 2))
        same &= np.all(to_np(res.x0).view(np.uint64) == to_np(other.x0).view(np.uint64), axis=0)
        flies = np.isin(p["grp"], ("hover", "clip", "clip_hi", "soft_mid", "hard_mid"))
        assert flies.sum() >= N // 3 and not np.any(same & flies), np.flatnonzero(same & flies)[:8]
    finally:
        env.close()
        ref.close()


def test_offsets_past_4_gib():
    """the tapes [K,N,12,12] float64 are 4.8 GB at K = 4 with 2^20 envs; the last 1 000 envs pass the one-step bar."""
    import torch
    from gym_copter_amd import measure
    n, steps, M = 1 << 20, 4, 6
    assert steps * n * 144 * 8 > 4 << 30 > (steps - 1) * n * 144 * 8
    rng = np.random.default_rng(873)
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
        filt = E._run(env, p, tape=True)
        res = _rts(env, p, filt)
        assert bool(res.ok.all())
        _check_rows("2^20 envs, last 1000", env, p, filt, res, lanes=slice(n - 1000, n))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. application
# ---------------------------------------------------------------------------------------------------------------------
def test_hover_smoothing_beats_the_filter_and_is_consistent():
    """Hover3D, 300 envs, 48 steps, positions and angles measured: the inputs of
    test_rollout_rts_cpu.py::test_application_conditions_hold_on_the_oracle_restatement, which satisfy the same
    conditions on the float64 oracle (there: smoothed / filtered RMSE 0.523 measured and 0.215 unmeasured slots; the
    smoothed start 0.0275 m and 0.101 of the prior's velocity RMSE; RMSE / sd in [0.932, 1.049])."""
    import torch
    from gym_copter_amd import measure
    a, x0, xhat0, H, r = ekf_ref.app_inputs(E.AH, seed=1)
    n = ekf_ref.APP_N
    env = E._env("hover3d", n, seed=3)
    try:
        env.reset()
        acts = E._dev(a, env)
        ro = env.rollout_states(acts, state={"x": x0, "status": np.full(n, AIRBORNE, np.uint8)})
        truth = ro.x.clone()
        assert bool((ro.status == AIRBORNE).all())
        z = measure(truth, H, r, seed=1)
        P0 = E._dev(np.repeat(ekf_ref.APP_P0[None], n, axis=0), env)
        xh = E._dev(xhat0, env)
        filt = env.rollout_ekf(acts, z, H, r, ekf_ref.APP_Q, xh, P0, tape=True)
        res = env.rollout_rts(acts, filt, ekf_ref.APP_Q, xh, P0)
        assert bool(filt.ok.all()) and bool(res.ok.all())
        rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
        fig = rts_ref.app_conditions(to_np(res.x), to_np(res.var), to_np(res.x0.T),
                                     to_np(torch.diagonal(res.P0, dim1=1, dim2=2)), to_np(filt.x), to_np(filt.var),
                                     to_np(truth), x0.T, rmse0)
        print(fig)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_single_rank_matches_plain_env():
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    rng = np.random.default_rng(872)
    n = 4097
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = E._env("lander3d", n, "float32", seed=6)
    try:
        sh.reset()
        plain.reset()
        p = E._problem(plain, "lander3d", rng, steps=6)
        filt = _filter(plain, p)
        a = sh.rollout_rts(p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"])
        b = _rts(plain, p, filt)
        assert _same(a, b)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib, smooth
    rng = np.random.default_rng(874)
    n = 128
    env = E._env("lander3d", n, seed=1)
    try:
        env.reset()
        p = E._problem(env, "lander3d", rng, steps=4)
        filt = _filter(env, p)
        base = dict(actions=p["acts"], filt=filt, Q=p["Q"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        res = env.rollout_rts(**base)
        # status0 defaults to AIRBORNE
        air = torch.full((n,), AIRBORNE, dtype=torch.uint8, device=env.device)
        assert _same(E._clone(env.rollout_rts(**dict(base, status0=None))), env.rollout_rts(**dict(base, status0=air)))
        # the smoothed starting point of a call may be the `end` of the next, although it is that call's own buffer
        res = env.rollout_rts(**base)
        x0c, P0c = res.x0.clone(), res.P0.clone()
        assert _same(E._clone(env.rollout_rts(**dict(base, end=(res.x0, res.P0)))),
                     env.rollout_rts(**dict(base, end=(x0c, P0c))))
        badQ = p["Q"].copy()
        badQ[0, 1] += 1e-9
        f32 = E._run(env, p, tape=True, dtype=torch.float32)
        f32 = f32._replace(x=f32.x.clone(), x_pred=f32.x_pred.clone(), status=f32.status.clone(),
                           P_tape=f32.P_tape.clone())
        for kw, match in ((dict(actions=p["acts"][:, :n - 1]), "actions must have shape"),
                          (dict(filt=filt._replace(P_tape=None)), "no P_tape"),
                          (dict(filt=f32), "must be float64"),
                          (dict(filt=tuple(filt)), "EkfResult"),
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
                          (dict(dtype=torch.float16), "dtype must be")):
            args = dict(base)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_rts(**args)
        with pytest.raises(ValueError, match="chunk must be"):
            smooth(env, p["acts"], filt, p["Q"], p["x0"], p["P0"], status0=p["st0"], chunk=0)
        with pytest.raises(ValueError, match="P_tape"):
            smooth(env, p["acts"], filt._replace(P_tape=None), p["Q"], p["x0"], p["P0"], status0=p["st0"])
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), 4
        io.actions_dev, io.start_x_dev, io.start_status_dev = p["acts"].data_ptr(), p["x0"].data_ptr(), p["st0"].data_ptr()
        rio = _lib.RolloutRtsIO()
        rio.struct_size = C.sizeof(rio) + 8
        assert env._lib.cs_rollout_rts(env._ctx, C.byref(io), C.byref(rio), None) == _lib.ERR_ABI
        # refused while a serve session is open
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_rts(**base)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_rts(**base)
    f32env = E._env("lander3d", n, seed=1, action_arith="float32")
    try:
        f32env.reset()
        with pytest.raises(ValueError, match="float32"):
            f32env.rollout_rts(**base)
    finally:
        f32env.close()
