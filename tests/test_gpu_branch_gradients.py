"""The device gradients through the branches of the env step -- touchdowns (soft and hard), LEVELING (and the take-off
after it inside one step at substeps > 1), CRASHED, LANDED starts, clipped motors (both sides, and exactly on the
edges), tilts, out-of-bounds (alone and with a tilt), the |dz| > dz_max penalty, time-limit truncation, and a lane on
the target at the origin -- against the branch-aware central differences of the float64 oracle (tests/branch_fd.py):
step_jacobian, rollout_vjp, rollout_vjp_params and rollout_mlp_vjp.  float64 storage, explicit starts, ragged env
counts.  Lanes where the oracle's run is not smooth under +-h (the stability verdict) are dropped and counted; every
test requires a minimum of kept lanes in each event class it covers, and prints its counts and largest errors."""
import numpy as np
import pytest

from branch_fd import (AIRBORNE, INACTIVE, ROWS, TOOK_OFF, event_classes, fd_mlp, fd_params, fd_rollout, fd_step,
                       run_rollout)
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from mlp_rollout_fd import OBS_SHAPE
from oracle.refcpu import CRASHED, DJI_PHANTOM, G, LANDED, LEVELING, TaskParams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "lander1d": 1}
MARS = dict(thrust_model="lift", rotor_gyro=True, vehicle_params={"C_L": 0.5}, world_params={"rho": 1.0})
BAR = 1e-6
MIN_KEPT = 20
MAX_STEPS = 1000
AH = hover_action()


def _env(task, n, substeps, **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype="float64", autoreset_mode="disabled",
                                       substeps=substeps, **kw)


def _dev(a, env):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def _mars_hover():
    w = DJI_PHANTOM.maxrpm * np.pi / 30
    kl = 0.5 * 1.0 * (0.05 * DJI_PHANTOM.L * 4) * 0.5 * (DJI_PHANTOM.L / 2) ** 2 * w * w
    return np.sqrt(G * DJI_PHANTOM.M / (4 * kl))


def _scaled(got, want, keep=None, axis=None):
    """max |got - want| / max(1, |want|) over the kept envs (env axis `axis`)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if keep is not None:
        got, want = np.compress(keep, got, axis=axis), np.compress(keep, want, axis=axis)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def _report(what, keep, classes, dropped_tape=0, errs=()):
    counts = " ".join("%s=%d/%d" % (k, int((v & keep).sum()), int(v.sum())) for k, v in classes.items() if v.any())
    print("%s: kept %d of %d (tape mismatches %d) | %s | errors %s" % (
        what, int(keep.sum()), keep.size, dropped_tape, counts, " ".join("%s %.2e" % e for e in errs)))


def _check_tapes(r, fd, n):
    """On kept lanes the device's status / terminated / truncated tapes must be the oracle base run's: lanes where
    they differ are dropped (at most 1 %).  Returns the new keep mask and the number dropped."""
    same = np.ones(n, bool)
    for name, t in (("status", r.status), ("terminated", r.terminated), ("truncated", r.truncated)):
        same &= (to_np(t).astype(np.int64) == fd.tape[name].astype(np.int64)).all(axis=0)
    dropped = int((fd.keep & ~same).sum())
    assert dropped <= 0.01 * n, ("device tapes differ from the oracle on %d kept lanes" % dropped)
    return fd.keep & same, dropped


# ---------------------------------------------------------------------------------------------------------------------
# start points, one group of envs per branch
# ---------------------------------------------------------------------------------------------------------------------
def _groups(n, names):
    """env index -> group name, the groups as even as the ragged count allows"""
    return np.array([names[i % len(names)] for i in range(n)])


def _step_points(n, A, rng, ah):
    """One-step points: LANDED, soft / hard contact (at the first call, z > 0, and inside the step), LEVELING below and
    above hover thrust, CRASHED, motors clipped at 0 and at 1, tilted, out of bounds, both, on the target at the
    origin, and free flight."""
    names = ["landed", "soft", "hard", "soft_mid", "hard_mid", "leveling", "leveling_up", "crashed", "clip", "tilt",
             "oob", "oob_tilt", "origin", "flight"]
    grp = _groups(n, names)
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-4, 4, (2, n))
    x[1], x[3] = rng.uniform(-1, 1, (2, n))
    x[4] = rng.uniform(-15, -5, n)
    x[5] = rng.uniform(-1, 1, n)
    x[6], x[8] = rng.uniform(-0.3, 0.3, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-1, 1, (4, n))
    st = np.full(n, AIRBORNE, np.uint8)
    a = ah * rng.uniform(0.5, 1.5, (n, A))

    def g(name):
        return grp == name

    m = g("landed") | g("origin")
    x[4, m], x[5, m], st[m] = 0.0, 0.0, LANDED
    x[:, g("origin")] = 0.0
    for name, dz in (("soft", (0.1, 0.8)), ("hard", (1.5, 3.0)), ("soft_mid", (0.1, 0.8)), ("hard_mid", (1.5, 3.0))):
        m = g(name)
        x[5, m] = rng.uniform(*dz, m.sum())
        x[3, m] = rng.uniform(-1, 1, m.sum())
        if name.endswith("mid"):                         # z reaches 0 inside the step (at 10 substeps)
            x[4, m] = -x[5, m] * rng.uniform(0.1, 0.9, m.sum()) / 100
        else:                                            # z > 0: contact in the first call
            x[4, m] = rng.uniform(1e-3, 0.05, m.sum())
    m = g("leveling") | g("leveling_up")
    x[4, m], st[m] = rng.uniform(-0.01, 0.0, m.sum()), LEVELING
    a[g("leveling")] = ah * rng.uniform(0.3, 0.9, (g("leveling").sum(), A))
    a[g("leveling_up")] = ah * rng.uniform(1.05, 1.4, (g("leveling_up").sum(), A))
    st[g("crashed")] = CRASHED
    m = g("clip")
    k = m.sum()
    a[m, 0] = rng.uniform(-0.5, -0.01, k)
    a[m, A - 1] = np.where(rng.uniform(size=k) < 0.5, rng.uniform(1.01, 1.5, k), a[m, A - 1])
    for name in ("tilt", "oob_tilt"):
        m = g(name)
        x[6, m] = rng.choice([-1, 1], m.sum()) * rng.uniform(0.8, 1.2, m.sum())
    for name in ("oob", "oob_tilt"):
        m = g(name)
        x[0, m] = rng.choice([-1, 1], m.sum()) * rng.uniform(10.2, 11.5, m.sum())
    return x, st, a.astype(np.float32), grp


def _expected_bits(fd, status0, actions):
    """the CS_JAC_* bits of each env from the oracle's per-call record"""
    from gym_copter_amd import _lib
    calls = fd.tape["calls"][0]                                 # [substeps, n]
    act = calls != INACTIVE
    before, after = calls // 4, calls % 4
    bits = np.where((act & (after == AIRBORNE)).any(axis=0), _lib.JAC_INTEGRATED, 0)
    bits |= np.where(np.asarray(status0) == LANDED, _lib.JAC_LANDED, 0)
    contact = act & ((before == AIRBORNE) | (before == LANDED)) & ((after == LEVELING) | (after == CRASHED))
    bits |= np.where(contact.any(axis=0), _lib.JAC_CONTACT, 0)
    bits |= np.where((act & (before == LEVELING)).any(axis=0), _lib.JAC_LEVELING, 0)
    bits |= np.where((act & (before == CRASHED)).any(axis=0), _lib.JAC_CRASHED, 0)
    bits |= np.where(((actions < 0) | (actions > 1)).any(axis=1), _lib.JAC_CLIPPED, 0)
    return bits


# ---------------------------------------------------------------------------------------------------------------------
# 1. step_jacobian at every branch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("task", ["lander3d", "lander2d", "lander1d", "hover3d"])
def test_step_jacobian_at_every_branch(task, substeps):
    n, A = 1000, TASK_A[task]
    rng = np.random.default_rng(100 + 10 * list(TASK_A).index(task) + substeps)
    x, st, a, grp = _step_points(n, A, rng, AH)
    env = _env(task, n, substeps)
    try:
        j = env.step_jacobian(_dev(a, env), state={"x": x, "status": st})
        got = [to_np(t).astype(np.float64) for t in j[:4]]
        branch = to_np(j.branch).astype(np.int64)
    finally:
        env.close()
    fd, dx, du, rdx, rdu = fd_step(task, x, st, a.astype(np.float64), substeps=substeps)
    keep = fd.keep
    classes = {name: grp == name for name in np.unique(grp)}
    errs = [(nm, _scaled(g_, w_, keep, axis=0)) for nm, g_, w_ in zip(("dx", "du", "reward_dx", "reward_du"), got,
                                                                       (dx, du, rdx, rdu))]
    _report("step_jacobian %s substeps=%d" % (task, substeps), keep, classes, errs=errs)
    assert np.array_equal(branch, _expected_bits(fd, st, a)), np.flatnonzero(branch != _expected_bits(fd, st, a))[:8]
    for name, m in classes.items():
        if name == "leveling_up" and substeps == 1:
            continue
        assert (m & keep).sum() >= MIN_KEPT, (name, (m & keep).sum())
    if substeps == 10:                                  # the LEVELING starts above hover take off within the step
        up = classes["leveling_up"] & keep
        assert (fd.tape["calls"][0][:, up] == TOOK_OFF).any(axis=0).all()
    for nm, e in errs:
        assert e <= BAR, (nm, e)


# ---------------------------------------------------------------------------------------------------------------------
# 2. rollout_vjp through the events of a K = 16 horizon
# ---------------------------------------------------------------------------------------------------------------------
ROLLOUT_CLASSES = ("soft_touchdown", "hard_touchdown", "tilt_crossed", "oob_crossed", "dz_crossed", "clipped",
                   "landed_start", "leveling_takeoff", "truncated_mid")


def _rollout_points(n, K, rng, ah, substeps):
    """Mixed starts for a K-step horizon: touchdowns (random and soft-biased), a tilt and a bound approached, a
    descent about to pass |dz| = dz_max, clipped motors, LANDED starts, LEVELING starts above hover, and envs whose
    step counter reaches max_steps inside the horizon."""
    names = ["touchdown", "soft", "soft", "tilt", "oob", "dz", "clip", "landed", "leveling", "trunc"]
    grp = _groups(n, names)
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-4, 4, (2, n))
    x[1], x[3] = rng.uniform(-1, 1, (2, n))
    x[4] = rng.uniform(-8, -3, n)       # (low: |x|, and the rounding of L with it, small; see AGREE in branch_fd.py)
    x[5] = rng.uniform(-1, 1, n)
    x[6], x[8] = rng.uniform(-0.3, 0.3, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-0.5, 0.5, (4, n))
    st = np.full(n, AIRBORNE, np.uint8)
    steps = np.ones(n, np.int32)
    a = ah * rng.uniform(0.5, 1.5, (K, n, 4))

    def g(name):
        m = grp == name
        return m, int(m.sum())

    m, k = g("touchdown")
    x[4, m], x[5, m] = rng.uniform(-0.2, 0.05, k), rng.uniform(0.2, 2.0, k)     # z > 0: contact in the first call
    x[6, m], x[8, m] = rng.uniform(-0.3, 0.3, (2, k))
    a[:, m] = ah * rng.uniform(0.3, 1.3, (K, k, 4))
    m, k = g("soft")
    x[4, m], x[5, m] = rng.uniform(-0.05, -0.005, k), rng.uniform(0.1, 0.6, k)
    x[3, m], x[6, m], x[7, m], x[1, m] = rng.uniform(-0.5, 0.5, (4, k)) * [[1], [0.2], [0.2], [1]]
    a[:, m] = ah * rng.uniform(0.6, 0.95, (K, k, 4))
    m, k = g("tilt")                                     # half tilting over, half recovering from a tilt
    out = rng.uniform(size=k) < 0.5
    x[6, m] = rng.choice([-1, 1], k) * np.where(out, rng.uniform(0.6, 0.75, k), rng.uniform(0.8, 0.9, k))
    x[7, m] = np.sign(x[6, m]) * np.where(out, 1.0, -1.0) * rng.uniform(1.0, 4.0, k)
    m, k = g("oob")
    x[0, m] = rng.choice([-1, 1], k) * rng.uniform(9.6, 9.95, k)
    x[0, m] = np.sign(x[0, m]) * 9.7 + rng.uniform(-0.1, 0.1, k)
    x[1, m] = np.sign(x[0, m]) * rng.uniform(1.0, 3.0, k)
    m, k = g("dz")
    x[5, m] = rng.uniform(9.2, 9.9, k)
    a[:, m] = ah * rng.uniform(0.2, 0.7, (K, k, 4))
    m, k = g("clip")
    a[:, m] = np.where(rng.uniform(size=(K, k, 4)) < 0.3, rng.uniform(-0.4, -0.01, (K, k, 4)), a[:, m])
    top = rng.uniform(size=k) < 0.5                       # full thrust on one motor in the last step only
    a[K - 1, np.flatnonzero(m)[top], 3] = rng.uniform(1.01, 1.3, top.sum())
    m, k = g("landed")
    x[4, m], x[5, m], st[m] = 0.0, 0.0, LANDED
    x[6, m] = np.where(rng.uniform(size=k) < 0.3, 0.9, x[6, m])           # some tilted on the ground
    m, k = g("leveling")
    x[4, m], st[m] = rng.uniform(-0.01, 0.0, k), LEVELING
    a[:, m] = ah * rng.uniform(1.05, 1.4, (K, k, 4)) if substeps > 1 else ah * rng.uniform(0.5, 1.4, (K, k, 4))
    m, k = g("trunc")
    steps[m] = MAX_STEPS - rng.integers(1, K - 1, k)
    a[:, m] = ah * rng.uniform(0.9, 1.1, (K, k, 4))
    return x, st, steps, a.astype(np.float32), grp


def _weights(rng, K, n, grp):
    """cotangents; the |x| of the full-thrust step is ~100: its cotangent small, so that L's rounding stays ~1e-9"""
    gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
    gx[K - 1, grp == "clip"] *= 0.01
    gr[K - 1, grp == "clip"] *= 0.01
    return gx, gr


@pytest.mark.parametrize("substeps,variant", [(1, "force_noprev"), (1, "given_prev"), (1, "force_nan_prev"),
                                              (10, "force_noprev"), (10, "given_prev")])
def test_rollout_vjp_through_events(substeps, variant):
    n, K = 700, 16
    rng = np.random.default_rng(200 + substeps * 7 + len(variant))
    x, st, steps, a, grp = _rollout_points(n, K, rng, AH, substeps)
    gx, gr = _weights(rng, K, n, grp)
    force = rng.uniform(-30, 30, (3, n)) if variant.startswith("force") else None
    prev = {"force_noprev": None, "given_prev": rng.uniform(-400, -50, n),
            "force_nan_prev": np.full(n, np.nan)}[variant]
    state = {"x": x, "status": st}
    if force is not None:
        state["force"] = force
    if prev is not None:
        state["prev_shaping"] = prev
    env = _env("lander3d", n, substeps, max_steps=MAX_STEPS, time_limit_truncates=True)
    try:
        env.set_state(steps=steps)
        acts = _dev(a, env)
        r = env.rollout_states(acts, state=state)
        ga, g0 = env.rollout_vjp(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state)
        ga, g0 = to_np(ga).copy(), to_np(g0).copy()
        fd, wa, w0 = fd_rollout("lander3d", x, st, a.astype(np.float64), gx, gr, force=force, prev_shaping=prev,
                                steps=steps, substeps=substeps, tp=TaskParams(max_steps=MAX_STEPS),
                                time_limit_truncates=True)
        keep, dropped = _check_tapes(r, fd, n)
    finally:
        env.close()
    classes = event_classes(fd.tape, st)
    errs = [("g_actions", _scaled(ga, wa, keep, axis=1)), ("g_x0", _scaled(g0, w0, keep, axis=1))]
    _report("rollout_vjp substeps=%d %s" % (substeps, variant), keep, classes, dropped, errs)
    for name in ROLLOUT_CLASSES:
        if name == "leveling_takeoff" and substeps == 1:
            continue
        assert (classes[name] & keep).sum() >= MIN_KEPT, (name, (classes[name] & keep).sum())
    for nm, e in errs:
        assert e <= BAR, (nm, e)


# ---------------------------------------------------------------------------------------------------------------------
# 3. rollout_vjp_params through the same events
# ---------------------------------------------------------------------------------------------------------------------
def _table(rng, n, mars):
    base = dict(B=5e-3, D=2e-6, M=1.38, L=0.35, Ix=2.0, Iy=2.0, Iz=3.0, Jr=38e-4, maxrpm=15000.0, G=G,
                rho=1.0 if mars else 1.225, C_L=0.5 if mars else 0.0)
    t = np.array([np.full(n, base[k]) for k in ROWS])
    for k, lo, hi in (("M", 0.9, 1.1), ("Ix", 0.9, 1.1), ("Iy", 0.9, 1.1), ("Iz", 0.9, 1.1), ("D", 0.8, 1.2)):
        t[ROWS.index(k)] *= rng.uniform(lo, hi, n)
    return t


@pytest.mark.parametrize("mars", [False, True])
@pytest.mark.parametrize("substeps", [1, 10])
def test_rollout_vjp_params_through_events(substeps, mars):
    n, K = 300, 16
    rng = np.random.default_rng(300 + substeps + 2 * mars)
    ah = _mars_hover() if mars else AH
    x, st, _, a, grp = _rollout_points(n, K, rng, ah, substeps)     # (no time limit here: the "trunc" envs fly)
    gx, gr = _weights(rng, K, n, grp)
    force = rng.uniform(-30, 30, (3, n))
    table = _table(rng, n, mars)
    state = {"x": x, "status": st, "force": force}
    env = _env("lander3d", n, substeps, **(dict(MARS) if mars else {}))
    try:
        acts = _dev(a, env)
        tab = _dev(table, env)
        r = env.rollout_states(acts, state=state, vehicle=tab)
        _, _, gv, gf = env.rollout_vjp_params(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state, vehicle=tab)
        gv, gf = to_np(gv).copy(), to_np(gf).copy()
        fd, wv, wf = fd_params("lander3d", x, st, a.astype(np.float64), table, force, gx, gr, substeps=substeps,
                               mars=mars)
        keep, dropped = _check_tapes(r, fd, n)
    finally:
        env.close()
    classes = {k: v for k, v in event_classes(fd.tape, st).items() if k in ROLLOUT_CLASSES[:-1]}
    errs = [("g_vehicle", _scaled(gv * table, wv * table, keep, axis=1)), ("g_force", _scaled(gf, wf, keep, axis=1))]
    _report("rollout_vjp_params substeps=%d %s" % (substeps, "mars+gyro" if mars else "B law"), keep, classes,
            dropped, errs)
    for name in ("soft_touchdown", "hard_touchdown", "tilt_crossed", "oob_crossed", "clipped", "landed_start"):
        assert (classes[name] & keep).sum() >= MIN_KEPT // 2, (name, (classes[name] & keep).sum())
    froze = np.isin(fd.tape["calls"][0, 0], [AIRBORNE * 4 + LEVELING, AIRBORNE * 4 + CRASHED])
    assert froze.sum() >= 5
    assert not gf[:, froze].any()                        # a force kept pending by a contact freeze never integrates
    for nm, e in errs:
        assert e <= BAR, (nm, e)


# ---------------------------------------------------------------------------------------------------------------------
# 4. rollout_mlp_vjp: a closed loop through touchdowns and a motor that the policy drives across 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [0, 16])
@pytest.mark.parametrize("substeps", [1, 10])
def test_rollout_mlp_vjp_through_events(substeps, hidden):
    import torch
    from gym_copter_amd import mlp
    n, K, A = 100, 16, 4
    rng = np.random.default_rng(400 + substeps + hidden)
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-2, 2, (2, n))     # (small observations: a weight's step moves the action by h |o|)
    x[1], x[3] = rng.uniform(-1, 1, (2, n))
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-0.5, 0.5, (4, n))
    low = np.arange(n) % 2 == 0                           # half of the envs start just above the ground, descending
    x[4] = np.where(low, rng.uniform(-0.3, -0.02, n), rng.uniform(-6, -3, n))
    x[5] = np.where(low, rng.uniform(0.2, 1.5, n), rng.uniform(-1, 1, n))
    st = np.full(n, AIRBORNE, np.uint8)
    p = mlp.init(OBS_SHAPE["lander3d"][1], A, hidden, generator=torch.Generator().manual_seed(5), out_bias=AH,
                 out_scale=0.0005 if hidden else 0.0002)
    p[-A] = 0.0                                          # motor 0 centred on the clip at 0: feedback moves it across
    u = (AH * rng.uniform(-0.2, 0.2, (K, n, A))).astype(np.float32)
    gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
    fd, wp, wu, w0 = fd_mlp("lander3d", x, st, p.double().numpy(), hidden, u.astype(np.float64), gx, gr,
                            substeps=substeps)
    env = _env("lander3d", n, substeps)
    try:
        pd = p.to(env.device)
        state = {"x": x, "status": st}
        r = env.rollout_mlp_states(pd, K, hidden, offsets=_dev(u, env), state=state)
        keep, dropped = _check_tapes(r, fd, n)
        # g_theta sums over envs: the dropped envs' cotangents are zeroed on both sides
        gxk, grk = gx * keep[None, :, None], gr * keep[None, :]
        gp, ga, g0 = env.rollout_mlp_vjp(pd, r, gx=_dev(gxk, env), gr=_dev(grk, env), state=state, hidden=hidden)
        gp, ga, g0 = to_np(gp).copy(), to_np(ga).copy(), to_np(g0).copy()
    finally:
        env.close()
    want_p = (wp * keep[None]).sum(axis=1)
    # g_theta is a sum over envs whose terms cancel (a component of 0.7 from per-env terms of ~100 was seen): its error
    # is the sum of the per-env ones, so it is scaled by the size of what is summed, sum_n |g_theta,n|, not by the sum
    size_p = np.maximum(np.abs(wp * keep[None]).sum(axis=1), 1.0)
    classes = event_classes(fd.tape, st)
    clipped_some = ((fd.tape["actions"][..., 0] < 0).any(axis=0) & (fd.tape["actions"][..., 0] > 0).any(axis=0))
    classes["motor0_crosses_0"] = clipped_some
    errs = [("g_theta", float(np.max(np.abs(gp - want_p) / size_p))), ("g_u", _scaled(ga, wu, keep, axis=1)),
            ("g_x0", _scaled(g0, w0, keep, axis=1))]
    _report("rollout_mlp_vjp substeps=%d H=%d" % (substeps, hidden), keep, classes, dropped, errs)
    assert keep.sum() >= n // 3
    assert (clipped_some & keep).sum() >= 10
    assert ((classes["soft_touchdown"] | classes["hard_touchdown"]) & keep).sum() >= 10
    for nm, e in errs:
        assert e <= 1e-5, (nm, e)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the clip exactly on its edges: the closed interval [0, 1]
# ---------------------------------------------------------------------------------------------------------------------
def _one_sided(f, a, side, h=1e-4):
    """second-order one-sided difference of f at a from inside [0, 1]: side +1 (a = 0, step up), -1 (a = 1, down).
    (h = 1e-4: the truncation error is O(h^2), and the rounding of f (~1e-13) stays far below the bar.)"""
    f0 = f(a)
    return side * (4 * (f(a + side * h) - f0) - (f(a + 2 * side * h) - f0)) / (2 * h)


def test_clip_edges_step_jacobian_and_rollout_vjp():
    """Actions exactly 0.0 and 1.0 (float32-exact) in an otherwise smooth step / rollout: the device derivative is the
    one-sided difference from inside [0, 1].  Under the B law a motor at 0 has derivative 0 either way (2 k m); at 1
    it is the full 2 k."""
    n, K = 96, 3
    rng = np.random.default_rng(500)
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-4, 4, (2, n))
    x[4] = rng.uniform(-8, -5, n)
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    st = np.full(n, AIRBORNE, np.uint8)
    a1 = (AH * rng.uniform(0.8, 1.2, (n, 4))).astype(np.float32)
    a1[:, 0], a1[:, 3] = 0.0, 1.0
    env = _env("lander3d", n, 1)
    try:
        j = env.step_jacobian(_dev(a1, env), state={"x": x, "status": st})
        du, rdu = to_np(j.du).astype(np.float64).copy(), to_np(j.reward_du).astype(np.float64).copy()
        aK = (AH * rng.uniform(0.8, 1.2, (K, n, 4))).astype(np.float32)
        aK[K - 1, :, 0], aK[K - 1, :, 3] = 0.0, 1.0
        aK[0, :, 1] = 0.0
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        gx[K - 1] *= 0.01
        gr[K - 1] *= 0.01
        acts = _dev(aK, env)
        state = {"x": x, "status": st}
        r = env.rollout_states(acts, state=state)
        ga, _ = env.rollout_vjp(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state)
        ga = to_np(ga).copy()
    finally:
        env.close()
    errs = []
    for col, side in ((0, 1.0), (3, -1.0)):
        def f1(v, col=col):
            aa = a1.astype(np.float64).copy()
            aa[:, col] = v
            t, _ = run_rollout("lander3d", x, st, aa[None], prev_shaping=np.zeros(n))
            return np.concatenate([t["x"][0].T, t["reward"]])
        want = _one_sided(f1, float(a1[0, col]), side)          # [13, n]
        errs.append(("du[%d]" % col, _scaled(du[:, :, col].T, want[:12])))
        errs.append(("reward_du[%d]" % col, _scaled(rdu[:, col], want[12])))
    for k, col, side in ((K - 1, 0, 1.0), (K - 1, 3, -1.0), (0, 1, 1.0)):
        def fK(v, k=k, col=col):
            aa = aK.astype(np.float64).copy()
            aa[k, :, col] = v
            t, _ = run_rollout("lander3d", x, st, aa)
            return np.einsum("knj,knj->n", t["x"], gx) + np.einsum("kn,kn->n", t["reward"], gr)
        want = _one_sided(fK, float(aK[k, 0, col]), side)
        errs.append(("g_actions[%d][%d]" % (k, col), _scaled(ga[k, :, col], want)))
    print("clip edges: errors " + " ".join("%s %.2e" % e for e in errs))
    assert np.abs(du[:, :, 3]).max() > 1.0                   # the derivative at 1 is the full one, not 0
    for nm, e in errs:
        assert e <= BAR, (nm, e)
