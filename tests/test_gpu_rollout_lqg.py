"""Output-feedback rollouts on the device (cs_rollout_lqg, CopterVecEnv.rollout_lqg, gym_copter_amd.lqg), verified by
composition with entry points that are already held to independent references.  By induction over k four exact statements
fix every output of the call:

  1. truth     (x, reward, terminated, truncated, status) == rollout_states(actions_out, state)
  2. measure   z == tests/lqg_ref.py's fixed-order H x + e on the device's own truth tape, NaN where e is NaN
  3. filter    every field of rollout_ekf(actions_out, z, H, r, Q, xhat0, P0, status0, tape=True) == the call's filter tapes
  4. law       actions_out[k] == tests/lqg_ref.py's law at xhat[k-1] (xhat0 for k = 0)

(actions_out[0] is 4. at the caller's inputs; given actions_out[..k], 1. fixes the truth up to k, 2. z[k], 3. the filter up
to k, and 4. actions_out[k+1].)  Every comparison is bit for bit.  The conditions that keep the four from passing
vacuously -- the feedback is active, it acts on the estimate and not on the truth, the filter is told the chosen action,
every branch of the step occurs, an estimate lies on the other side of a touchdown -- are asserted in the same tests."""
import collections
import ctypes as C
import zlib

import numpy as np
import pytest

import ekf_ref
import lqg_ref
import model_variants
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

AH = hover_action()
N, K = 300, 16          # four whole wavefronts and one of 44 lanes
Problem = collections.namedtuple("Problem", "abar gains xbar e H r Q xhat0 P0 fst0 state start_x host")


def _env(task, n, mode="float64", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _problem(env, task, rng, steps=K, M=6, dense=True, missing=0.0, ah=AH, stored=False, nan_steps=(), force=True):
    """lqg_ref.problem on the device.  stored: the truth starts from the env's stored state (the estimate is that state
    plus the problem's error, its status the stored one); else from the problem's explicit start with its pending force.
    The reference tape is the nominal rollout's: its start, then its rows 0 .. K-2."""
    import torch
    n = env.num_envs
    h = lqg_ref.problem(task, n, steps, rng, ah, M=M, dense=dense, missing=missing)
    for k in nan_steps:
        h["e"][k] = np.nan
    if stored:
        s = env.get_state()
        state, start_x, fst0 = None, s["x"], s["status"]
        h["xhat0"] = s["x"] + (h["xhat0"] - h["x0"])
    else:
        state = {"x": _dev(h["x0"], env), "status": _dev(h["st0"], env)}
        if force:
            state["force"] = _dev(h["force"], env)
        start_x, fst0 = h["x0"], h["fst0"]
    abar = _dev(h["abar"], env)
    nominal = env.rollout_states(abar, state=state)
    xbar = torch.cat([_dev(start_x, env).T[None], nominal.x[:-1]]).contiguous()
    return Problem(abar, _dev(h["gains"], env), xbar, _dev(h["e"], env), h["H"], h["r"], h["Q"], _dev(h["xhat0"], env),
                   _dev(h["P0"], env), _dev(fst0, env), state, np.asarray(start_x, np.float64), h)


def _run(env, p, **kw):
    return env.rollout_lqg(p.abar, p.gains, p.xbar, p.e, p.H, p.r, p.Q, p.xhat0, p.P0, status0=p.fst0, state=p.state,
                           **kw)


def _clone(res):
    c = lambda nt: type(nt)(*[None if t is None else t.clone() for t in nt])          # noqa: E731
    return type(res)(c(res.rollout), res.actions.clone(), res.z.clone(), c(res.filter))


def _same_bits(a, b):
    """bit for bit, NaN equal to NaN at the same place (no NaN payload is compared)"""
    a, b = np.ascontiguousarray(to_np(a)), np.ascontiguousarray(to_np(b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))
    return bool(np.array_equal(a, b))


def _assert_filter_equal(name, got, want):
    for field, u, v in zip(got._fields, got, want):
        assert (u is None) == (v is None), (name, field)
        if u is not None:
            assert u.dtype == v.dtype and _same_bits(u, v), (name, "filter." + field)


def check_composition(name, env, p, res):
    """statements 1 to 4 on res (a tape=True result in float64, cloned); returns what the vacuity conditions read: the
    law at the true state, and rollout_ekf's result"""
    import torch
    ro, f = res.rollout, res.filter
    steps = res.actions.shape[0]
    # 1. the truth
    want = env.rollout_states(res.actions, state=p.state)
    for field, u, v in zip(ro._fields, ro, want):
        assert _same_bits(u, v), (name, "truth." + field)
    # 2. the measurement
    x, e = to_np(ro.x), to_np(p.e)
    z = np.array([lqg_ref.measure(p.H, x[k], e[k]) for k in range(steps)])
    assert np.array_equal(np.isnan(to_np(res.z)), np.isnan(e)), name
    assert _same_bits(res.z, z), (name, "z")
    # 3. the filter
    ekf = env.rollout_ekf(res.actions, res.z, p.H, p.r, p.Q, p.xhat0, p.P0, status0=p.fst0, tape=True)
    _assert_filter_equal(name, f, ekf)
    assert torch.equal(f.P, f.P_tape[-1])
    # 4. the law, at the estimate -- and, for the caller, at the truth
    xhat, xbar = to_np(f.x), to_np(p.xbar)
    abar, gains, aout = to_np(p.abar), to_np(p.gains), to_np(res.actions)
    at_truth = np.empty_like(aout)
    for k in range(steps):
        prev = to_np(p.xhat0).T if k == 0 else xhat[k - 1]
        assert _same_bits(aout[k], lqg_ref.law(abar[k], gains[k], prev, xbar[k])), (name, "law", k)
        at_truth[k] = lqg_ref.law(abar[k], gains[k], p.start_x.T if k == 0 else x[k - 1], xbar[k])
    return at_truth, type(ekf)(*[None if t is None else t.clone() for t in ekf])


def assert_feedback_active(name, env, p, res, at_truth):
    """the conditions under which the four statements say something: in the lanes that fly (the truth is AIRBORNE after
    step 1) the law moves >= 90 % of the action entries off the nominal, and >= 90 % of them off what the law gives at
    the TRUE state; the filter told the nominal instead of the chosen action predicts another first mean in every lane
    whose first step integrates under other clipped motors; and the nominal rollout ends elsewhere than the truth."""
    from gym_copter_amd import _lib
    aout, abar = to_np(res.actions), to_np(p.abar)
    flying = to_np(res.rollout.status[0]) == AIRBORNE
    assert flying.sum() >= env.num_envs // 4, (name, int(flying.sum()))
    assert (aout != abar)[:, flying].mean() >= 0.9, name
    assert (aout != at_truth)[:, flying].mean() >= 0.9, name
    told_nominal = env.rollout_ekf(p.abar, res.z, p.H, p.r, p.Q, p.xhat0, p.P0, status0=p.fst0)
    moved = np.any(to_np(told_nominal.x_pred[0]) != to_np(res.filter.x_pred[0]), axis=1)
    other_motors = np.any(np.clip(aout[0], 0, 1) != np.clip(abar[0], 0, 1), axis=1)
    integrates = (to_np(res.filter.branch[0]) & _lib.JAC_INTEGRATED) != 0
    assert (integrates & other_motors).sum() >= env.num_envs // 4, name
    assert moved[integrates & other_motors].all(), (name, np.flatnonzero(~moved & integrates & other_motors)[:8])
    nominal_end = to_np(env.rollout_states(p.abar, state=p.state).x[-1])
    assert np.any(nominal_end != to_np(res.rollout.x[-1]), axis=1)[flying].all(), name


def _fractions(branch):
    from gym_copter_amd import _lib
    bits = to_np(branch)
    return {nm: float(((bits & getattr(_lib, "JAC_" + nm)) != 0).mean())
            for nm in ("INTEGRATED", "LANDED", "CONTACT", "CRASHED", "CLIPPED")}


def assert_every_branch(name, p, res):
    """INTEGRATED, LANDED, CONTACT, CRASHED and CLIPPED each in >= 1 % of the (k, env) pairs of the filter's branch; some
    motors outside [0, 1] come from the gains, not from the nominal; and the filter's status differs from the truth's"""
    frac = _fractions(res.filter.branch)
    differ = to_np(res.filter.status) != to_np(res.rollout.status)
    aout, abar = to_np(res.actions), to_np(p.abar)
    pushed = ((abar >= 0) & (abar <= 1) & ((aout < 0) | (aout > 1))).mean()
    print("%s: branch fractions %s; filter status != truth status in %d pairs (%d envs); pushed outside [0, 1]: %.3f"
          % (name, {k: round(v, 4) for k, v in frac.items()}, differ.sum(), differ.any(axis=0).sum(), pushed))
    for nm, v in frac.items():
        assert v >= 0.01, (name, nm, v)
    assert pushed > 0, name
    assert differ.any(), name


# ---------------------------------------------------------------------------------------------------------------------
# 1. through every branch: Lander3D, float64 storage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
def test_explicit_start_with_a_pending_force(substeps):
    """(seed 901 at substeps = 1 is the case tests/test_rollout_lqg_cpu.py restates on the oracle)"""
    rng = np.random.default_rng(900 + substeps)
    name = "lander3d substeps=%d" % substeps
    env = _env("lander3d", N, substeps=substeps, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        assert p.state["force"] is not None and bool((p.state["force"] != 0).all())
        res = _clone(_run(env, p, tape=True))
        at_truth, _ = check_composition(name, env, p, res)
        assert_feedback_active(name, env, p, res, at_truth)
        assert_every_branch(name, p, res)
        # the pending force enters: without it the first step of every lane that integrates ends elsewhere
        bare = dict(p.state)
        del bare["force"]
        other = _run(env, p._replace(state=bare))
        flew = to_np(res.rollout.status[0]) == AIRBORNE
        assert np.any(to_np(other.rollout.x[0]) != to_np(res.rollout.x[0]), axis=1)[flew].all()
    finally:
        env.close()


def test_stored_start_with_pending_perturbations_and_resets():
    """The stored env after reset(), a state of every branch in which two groups of lanes fly out of bounds at 3 m/s --
    one in the second step, one in the third -- and three steps under NEXT_STEP auto-reset: the first group has reset in
    the third step and carries the new episode's perturbation into the call, the second resets in the call's first step
    (with the draw step() would make)."""
    from oracle.refcpu import TaskParams
    rng = np.random.default_rng(910)
    name = "lander3d stored"
    env = _env("lander3d", N, autoreset="next_step", seed=5)
    try:
        env.reset()
        x, st, a, grp = lqg_ref.points(N, 3, 4, rng, AH)
        hover = np.flatnonzero(grp == "hover")
        for lanes, steps_to_bound in ((hover[0::3], 1.5), (hover[1::3], 2.5)):
            x[1, lanes] = 3.0
            x[0, lanes] = TaskParams().bounds - 3.0 * 0.01 * steps_to_bound
        s0 = env.get_state()
        env.set_state(x=x, status=st, steps=np.ones(N, np.int32), prev_shaping=np.zeros(N), flags=s0["flags"])
        for k in range(3):
            env.step(_dev(a[k], env))
        before = env.get_state()
        flags = before["flags"]
        print("%s: %d envs with a pending perturbation, %d with a pending reset" % (name, (flags & 1).astype(bool).sum(),
                                                                                  (flags & 2).astype(bool).sum()))
        assert (flags & 1).any() and (flags & 2).any()
        p = _problem(env, "lander3d", rng, stored=True)
        assert p.state is None
        res = _clone(_run(env, p, tape=True))
        at_truth, _ = check_composition(name, env, p, res)
        # (a lane that resets in step 1 has the reset state whatever its action: "flying" lanes are judged from step 2 on)
        assert_feedback_active(name, env, p, res, at_truth)
        # the reset lanes start their new episode in step 1: the reset state
        resetting = (flags & 2) != 0
        x1 = to_np(res.rollout.x[0])[resetting]
        assert np.all(x1[:, [0, 1, 2, 3, 5]] == 0) and np.all(x1[:, 4] == x1[0, 4])
        after = env.get_state()
        for key, v in before.items():
            assert np.array_equal(v, after[key], equal_nan=key in ("prev_shaping", "x")), (name, key)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the other tasks, storage modes and vehicle models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,mode,M,dense", [("hover3d", "float32", 6, True), ("lander2d", "float64", 1, True),
                                               ("hover1d", "float64", 12, False)])
def test_other_tasks_and_storage(task, mode, M, dense):
    rng = np.random.default_rng(zlib.crc32(repr((task, mode, M)).encode()))
    name = "%s %s M=%d" % (task, mode, M)
    env = _env(task, N, mode, seed=3)
    try:
        env.reset()
        p = _problem(env, task, rng, M=M, dense=dense)
        assert tuple(p.abar.shape) == (K, N, lqg_ref.TASK_A[task]) and tuple(p.e.shape) == (K, N, M)
        res = _clone(_run(env, p, tape=True))
        at_truth, _ = check_composition(name, env, p, res)
        assert_feedback_active(name, env, p, res, at_truth)
        if mode != "float64":      # the filter's means are not rounded to the storage's words (24 + 5 guard bits here)
            xh = to_np(res.filter.x)
            assert (xh != xh.astype(np.float32).astype(np.float64)).mean() > 0.5
            x = to_np(res.rollout.x)
            assert ((x.view(np.uint64) & np.uint64((1 << 24) - 1)) == 0).all()         # 53 - 29 low bits are zero
            assert ((xh.view(np.uint64) & np.uint64((1 << 24) - 1)) != 0).mean() > 0.5
    finally:
        env.close()


@pytest.mark.parametrize("variant", ["vehicles", "mars_gyro"])
def test_under_other_vehicle_models(variant):
    rng = np.random.default_rng(zlib.crc32(variant.encode()))
    name = "lander3d " + variant
    env = _env("lander3d", N, seed=3, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        p = _problem(env, "lander3d", rng, ah=model_variants.hover(variant))
        res = _clone(_run(env, p, tape=True))
        at_truth, _ = check_composition(name, env, p, res)
        assert_feedback_active(name, env, p, res, at_truth)
        # the variant is in force on both sides of the comparisons: the default model flies the same actions elsewhere
        ref = _env("lander3d", N, seed=3)
        try:
            ref.reset()
            default_x = to_np(ref.rollout_states(res.actions, state=p.state).x)
        finally:
            ref.close()
        flying = to_np(res.rollout.status[0]) == AIRBORNE
        assert np.any(default_x != to_np(res.rollout.x), axis=(0, 2))[flying].all()
    finally:
        env.close()


def test_missing_measurements_and_whole_steps_without_any():
    """30 % of the entries missing, and steps 3 and 9 without any measurement: z is all NaN there, the posterior mean is the
    prior bit for bit and the step's nis is 0"""
    import torch
    rng = np.random.default_rng(930)
    name = "lander3d missing"
    env = _env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, missing=0.3, nan_steps=(3, 9))
        frac = float(torch.isnan(p.e).double().mean())
        assert 0.3 < frac < 0.45
        res = _clone(_run(env, p, tape=True))
        at_truth, _ = check_composition(name, env, p, res)
        assert_feedback_active(name, env, p, res, at_truth)
        for k in (3, 9):
            assert bool(torch.isnan(res.z[k]).all())
            assert torch.equal(res.filter.x[k], res.filter.x_pred[k])
            assert bool((res.filter.nis[k] == 0).all())
        assert bool((res.filter.nis[[0, 1, 2, 4]] > 0).any(dim=1).all())
    finally:
        env.close()


def test_one_env_one_step():
    rng = np.random.default_rng(940)
    env = _env("lander3d", 1, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, steps=1)
        res = _clone(_run(env, p, tape=True))
        assert tuple(res.actions.shape) == (1, 1, 4) and tuple(res.filter.P_tape.shape) == (1, 1, 12, 12)
        at_truth, _ = check_composition("n=1 K=1", env, p, res)
        assert np.any(to_np(res.actions) != to_np(p.abar)) and np.any(to_np(res.actions) != at_truth)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_dtype_determinism_tape_and_state():
    import torch
    rng = np.random.default_rng(950)
    env = _env("lander3d", N, seed=3)
    try:
        env.reset()
        before = env.get_state()
        p = _problem(env, "lander3d", rng)
        a = _clone(_run(env, p, tape=True))
        b = _clone(_run(env, p, tape=True))
        for u, v in zip((*a.rollout, a.actions, a.z, *a.filter), (*b.rollout, b.actions, b.z, *b.filter)):
            assert _same_bits(u, v)
        c = _clone(_run(env, p))                                    # tape=False: the same bits elsewhere
        assert c.filter.P_tape is None
        _assert_filter_equal("tape=False", c.filter._replace(P_tape=a.filter.P_tape), a.filter)
        assert _same_bits(c.actions, a.actions) and _same_bits(c.z, a.z) and _same_bits(c.rollout.x, a.rollout.x)
        d = _clone(_run(env, p, tape=True, dtype=torch.float32))    # float32 outputs: the float64 outputs rounded
        for field in ("P", "var", "nis", "loglik", "P_tape"):
            got, want = getattr(d.filter, field), getattr(a.filter, field)
            assert got.dtype == torch.float32 and torch.equal(got, want.to(torch.float32)), field
        for field in ("x", "x_pred", "status", "branch", "ok"):
            assert _same_bits(getattr(d.filter, field), getattr(a.filter, field)), field
        assert _same_bits(d.actions, a.actions) and _same_bits(d.z, a.z) and _same_bits(d.rollout.x, a.rollout.x)
        assert _same_bits(d.rollout.reward, a.rollout.reward)
        # gains as rollout_lqr's result: its .K is used
        Gains = collections.namedtuple("Gains", "K d")
        g = _clone(env.rollout_lqg(p.abar, Gains(p.gains, None), p.xbar, p.e, p.H, p.r, p.Q, p.xhat0, p.P0,
                                   status0=p.fst0, state=p.state, tape=True))
        assert _same_bits(g.actions, a.actions) and _same_bits(g.filter.x, a.filter.x)
        after = env.get_state()
        for key, v in before.items():
            assert np.array_equal(v, after[key], equal_nan=True), key
    finally:
        env.close()


def test_sharded_single_rank_matches_plain_env():
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    rng = np.random.default_rng(960)
    sh = ShardedCopterVecEnv("lander3d", N, device=0, seed=6, autoreset_mode="next_step")
    plain = _env("lander3d", N, "float32", seed=6)
    try:
        sh.reset()
        plain.reset()
        p = _problem(plain, "lander3d", rng, steps=6)
        a = sh.rollout_lqg(p.abar, p.gains, p.xbar, p.e, p.H, p.r, p.Q, p.xhat0, p.P0, status0=p.fst0, state=p.state,
                           tape=True)
        b = _run(plain, p, tape=True)
        for u, v in zip((*a.rollout, a.actions, a.z, *a.filter), (*b.rollout, b.actions, b.z, *b.filter)):
            assert _same_bits(u, v)
    finally:
        sh.close()
        plain.close()


def test_driver_equals_its_composition():
    """gym_copter_amd.lqg() == rollout_states, rollout_lqr at ilqr.tracking_gradients, the reference tape, the noise
    and rollout_lqg, made by hand -- from the stored state and from an explicit one"""
    import torch
    import gym_copter_amd
    from gym_copter_amd import measurement_noise
    from gym_copter_amd.ilqr import tracking_gradients
    rng = np.random.default_rng(970)
    env = _env("hover3d", N, seed=3)
    try:
        env.reset()
        h = lqg_ref.problem("hover3d", N, K, rng, AH)
        air = h["st0"] == AIRBORNE
        h["x0"][4, ~air], h["st0"][:] = -5.0, AIRBORNE              # (a regular LQR problem in every lane)
        Qc, Rc = np.diag(np.linspace(1.0, 2.0, 12)), 50.0 * np.eye(4)
        x_ref = np.zeros(12)
        x_ref[4] = -5.0
        acts = _dev(h["abar"], env)
        for state in (None, {"x": _dev(h["x0"], env), "status": _dev(h["st0"], env)}):
            got = _clone(gym_copter_amd.lqg(env, acts, x_ref, Qc, Rc, h["H"], h["r"], h["Q"], h["xhat0"], h["P0"], seed=11,
                                            missing=0.1, state=state, Q_final=3.0 * Qc, a_ref=AH))
            nominal = env.rollout_states(acts, state=state)
            q, r = tracking_gradients(nominal.x, acts, _dev(x_ref, env), torch.tensor(AH, device=env.device),
                                      _dev(Qc, env), _dev(Rc, env), _dev(3.0 * Qc, env))
            gains = env.rollout_lqr(acts, nominal, Qc, Rc, q=q, r=r, Q_final=3.0 * Qc, state=state)
            assert bool(gains.ok.all())
            x0 = state["x"] if state is not None else _dev(env.get_state(only=("x",))["x"], env)
            xbar = torch.cat([x0.T[None], nominal.x[:-1]]).contiguous()
            noise = measurement_noise(K, N, h["r"], 11, missing=0.1, device=env.device)
            assert 0.05 < float(torch.isnan(noise).double().mean()) < 0.15
            sd = float((noise[..., 0][~torch.isnan(noise[..., 0])]).std())
            assert abs(sd / np.sqrt(h["r"][0]) - 1) < 0.1
            want = env.rollout_lqg(acts, gains, xbar, noise, h["H"], h["r"], h["Q"], h["xhat0"], h["P0"], state=state)
            for u, v in zip((*got.rollout, got.actions, got.z, *got.filter), (*want.rollout, want.actions, want.z,
                                                                              *want.filter)):
                assert (u is None and v is None) or _same_bits(u, v)
            assert np.any(to_np(got.actions) != to_np(acts))
    finally:
        env.close()


def test_wrapper_errors():
    import torch
    import gym_copter_amd
    from gym_copter_amd import CopterStepError, _lib, measurement_noise
    rng = np.random.default_rng(980)
    env = _env("lander3d", 65, seed=3)
    try:
        env.reset()
        n = 65
        p = _problem(env, "lander3d", rng, steps=4)
        base = dict(actions=p.abar, gains=p.gains, xbar=p.xbar, noise=p.e, H=p.H, r=p.r, Q=p.Q, xhat0=p.xhat0, P0=p.P0,
                    status0=p.fst0, state=p.state)
        env.rollout_lqg(**base)
        bad = [
            (dict(actions=p.abar[:, :, :3]), "actions"),
            (dict(gains=p.gains[:3]), "gains"), (dict(gains=p.gains.float()), "gains"),
            (dict(gains=to_np(p.gains)), "gains"), (dict(gains=p.gains.transpose(2, 3)), "gains"),
            (dict(xbar=p.xbar[:, :, :6]), "xbar"), (dict(xbar=p.xbar.cpu()), "xbar"),
            (dict(noise=p.e[:, :, :5]), "noise"), (dict(noise=p.e.to(torch.int32)), "noise"),
            (dict(noise=p.e.cpu()), "noise"),
            (dict(H=p.H[:, :6]), "H must have shape"), (dict(H=np.zeros((13, 12)), r=np.ones(13)), "H must have shape"),
            (dict(r=p.r[:3]), "r must have shape"), (dict(r=-p.r), "positive"),
            (dict(Q=np.eye(11)), "Q must have shape"), (dict(Q=np.triu(np.ones((12, 12)))), "symmetric"),
            (dict(Q=np.full((12, 12), np.nan)), "finite"),
            (dict(xhat0=p.xhat0.T), "xhat0"), (dict(P0=p.P0[:, :6]), "P0"),
            (dict(status0=p.fst0[:5]), "status0"),
            (dict(state={"x": p.state["x"]}), "state needs"), (dict(state=dict(p.state, wind=1)), "state needs"),
            (dict(dtype=torch.float16), "dtype"),
        ]
        for kw, match in bad:
            with pytest.raises(ValueError, match=match):
                env.rollout_lqg(**dict(base, **kw))
        for kw, match in ((dict(missing=1.5), "probability"), (dict(r=[-1.0]), "positive"), (dict(r=np.ones((2, 2))), "shape"),
                          (dict(K=0), ">= 1")):
            with pytest.raises(ValueError, match=match):
                measurement_noise(**dict(dict(K=4, N=n, r=p.r, seed=1, device=env.device), **kw))
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), 4
        io.actions_dev = p.abar.data_ptr()
        lio = _lib.RolloutLqgIO()
        lio.struct_size = C.sizeof(lio) + 8
        assert env._lib.cs_rollout_lqg(env._ctx, C.byref(io), C.byref(lio), None) == _lib.ERR_ABI
        # refused while a serve session is open
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_lqg(**base)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_lqg(**base)
    f32 = _env("lander3d", n, seed=3, action_arith="float32")
    try:
        f32.reset()
        with pytest.raises(CopterStepError, match="float32 motor model"):
            f32.rollout_lqg(**base)
    finally:
        f32.close()
    assert gym_copter_amd.CopterVecEnv.rollout_lqg.__doc__


# ---------------------------------------------------------------------------------------------------------------------
# 4. the application: Hover3D held at its reference from measured positions and angles
# ---------------------------------------------------------------------------------------------------------------------
def test_application_closing_the_loop_keeps_the_filter_consistent_and_holds_the_position():
    """Hover3D, 300 envs, K = 192 (see lqg_ref.APP_K), positions and angles measured with sigma = 0.1 m and 0.01 rad, P0
    of the filter's application, xhat0 = truth + N(0, P0), starts perturbed in velocity, gains of one host-computed LQR
    recursion at hover -- the inputs of tests/test_rollout_lqg_cpu.py's restatement.  Mean NIS within 6 +- 0.3; final
    position RMSE below 0.5 x the open-loop nominal's from the same starts.

    Measured: the CPU restatement mean NIS 5.978, RMSE 0.170 m against 0.950 m (ratio 0.179); the device (MI355X) mean NIS
    5.978, RMSE 0.170 m against 0.950 m (ratio 0.179)  (DESIGN.md section 22)."""
    env = _env("hover3d", lqg_ref.APP_N, seed=3)
    try:
        env.reset()
        abar, x0, xhat0, xbar, e, H, r = lqg_ref.app_inputs(AH, seed=1)
        n, steps = lqg_ref.APP_N, lqg_ref.APP_K
        gains = np.broadcast_to(lqg_ref.app_gains(AH)[:, None], (steps, n, 4, 12))
        st = np.full(n, AIRBORNE, np.uint8)
        state = {"x": _dev(x0, env), "status": _dev(st, env)}
        P0 = np.repeat(ekf_ref.APP_P0[None], n, axis=0)
        res = env.rollout_lqg(_dev(abar, env), _dev(gains, env), _dev(xbar, env), _dev(e, env), H, r, ekf_ref.APP_Q,
                              _dev(xhat0, env), _dev(P0, env), state=state)
        closed, nis = to_np(res.rollout.x).copy(), to_np(res.filter.nis).copy()
        assert bool(res.filter.ok.all()) and (to_np(res.rollout.status) == AIRBORNE).all()
        opened = to_np(env.rollout_states(_dev(abar, env), state=state).x)
        fig = lqg_ref.app_conditions(nis, closed, opened)
        print("application: mean NIS %.3f rmse closed %.3f open %.3f ratio %.3f"
              % (fig["mean_nis"], fig["rmse_closed"], fig["rmse_open"], fig["ratio"]))
    finally:
        env.close()
