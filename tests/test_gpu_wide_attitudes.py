"""Every kernel family at attitudes outside the first quadrant (tests/attitude_points.py: all three Euler angles in every
quadrant of either sign, on the edges of the reduction, past the fold at 8e5 rad, lane by lane beside quiet lanes):

1. one step from the installed state against VecOracle -- step(), step_many, rollout_states; substeps 1 and 10; float64
   storage to 1e-13 scaled, the float32 modes to the statement of
   test_a_differing_stored_word_after_one_step_is_a_straddled_rounding_boundary; +-inf and NaN yaws give what the oracle
   gives and disturb nobody;
2. K = 8: step_many and rollout_states bit-identical to eight step() calls;
3. neighbours: a batch of 1024 + 77 envs against the same envs split at 300 + 13, K = 12, bit for bit;
4. step_jacobian and rollout_vjp against central differences of the oracle on the FD point set, with the branch bits
   and the terminated flags the oracle's step gives;
5. yaw periodicity at large magnitude: the derivatives at psi_big against those at its twin psi_red';
6. rollout_mlp_states under a zero policy and the filter's x_pred equal rollout_states at the wide starts, and one run
   each of the step-by-step checks of the filter, the smoother on its tapes, and the particle filter.
The conditions these rest on are checked on the oracle alone by tests/test_wide_attitudes_cpu.py.

Measured on an MI355X (every test prints its own figures; the table is in DESIGN.md section 3): 1. float64 5.4e-15 of
1e-13; float32 1 (one substep) and 6 (ten) of 6 144 words differ, the largest 0.99 of one unit + 1e-10; float32_rn none.
4. step_jacobian dx 3.3e-9, du 4.1e-9, reward rows 1.1e-7 of 1e-6; rollout_vjp 8.1e-8 of 1e-6.  5. 1.4e-15 of 1e-13.
6. the filter's check: x 0.002, nis 0.014, loglik 0.006 of its bars.  The whole file runs in under 5 s.

Mutants this file fails for (uncommitted builds of the library, this file alone): the fold as it was (all three of its
pieces first), the cosine's sign from (q & 2) instead of ((q + 1) & 2), and 0.8 for 0.785 in the fast path's tests."""
import types

import numpy as np
import pytest

import attitude_points as ap
from gpu_util import have_gpu, make_pair, to_np
from jacobian_fd import fd_jacobian
from rollout_fd import fd_rollout_vjp

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

BAR = 1e-6              # derivatives against central differences (tests/test_gpu_jacobian.py, test_gpu_rollout_grad.py)
F64_BAR = 1e-13         # one float64 step against the oracle (tests/test_gpu_numerics.py)


def _env(task, n, mode="float64", substeps=1, **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode="disabled",
                                       substeps=substeps, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(env.device, dtype=dtype)      # (a copy: the points are read-only)


def _install(env, x, status):
    n = env.num_envs
    env.set_state(x=x, status=status, steps=np.ones(n, np.int32), prev_shaping=np.zeros(n), flags=np.zeros(n, np.uint8))


def _same(a, b):
    """bit-for-bit up to the payload of a NaN (tensors or arrays)"""
    a, b = to_np(a), to_np(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def _scaled(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward, one step from the installed state against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _forward_case(mode, substeps):
    """(start as stored, x after one step by each form, flags by each form, the oracle's x, terminated, truncated)"""
    p = ap.points()
    n = ap.N
    env, orc = make_pair("lander3d", n, mode, "disabled", substeps=substeps, seed=1)
    try:
        env.reset()
        orc.reset()
        got = {}
        acts = _dev(p.actions, env)
        with np.errstate(invalid="ignore"):
            for form in ("rollout_states", "step_many", "step"):
                env.set_state(x=p.x, status=p.status, flags=np.zeros(n, np.uint8))
                start = env.get_state(only=("x",))["x"]
                if form == "rollout_states":
                    r = env.rollout_states(acts[None])
                    got[form] = (to_np(r.x[0]).T.copy(), to_np(r.terminated[0]).copy(), to_np(r.truncated[0]).copy(),
                                 to_np(r.status[0]).copy())
                    continue
                out = env.step_many(acts[None]) if form == "step_many" else env.step(acts)
                term, trunc = (to_np(v).reshape(-1).copy() for v in out[2:4])
                s = env.get_state(only=("x", "status"))
                got[form] = (s["x"], term.astype(bool), trunc.astype(bool), s["status"])
            orc.x[:] = start
            orc.pending[:] = False
            _, _, wterm, wtrunc = orc.step(p.actions.astype(np.float64))
        return start, got, orc.x.astype(np.float64).copy(), wterm, wtrunc, orc.status.copy()
    finally:
        env.close()


@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("mode", ["float64", "float32", "float32_rn"])
def test_one_step_from_wide_attitudes_matches_the_oracle(mode, substeps):
    p = ap.points()
    start, got, want, wterm, wtrunc, wstatus = _forward_case(mode, substeps)
    finite = np.ones(ap.N, bool)
    finite[p.nonfinite] = False
    assert np.isnan(want[:, p.nonfinite]).any(axis=0).all()            # the oracle does give NaN there
    for form, (x, term, trunc, status) in got.items():
        assert np.array_equal(term, wterm) and np.array_equal(trunc, wtrunc) and np.array_equal(status, wstatus), form
        # non-finite yaws: NaN where the oracle has NaN, its values elsewhere (the same rule as the finite lanes below)
        assert np.array_equal(np.isnan(x), np.isnan(want)), form
        assert np.array_equal(np.isinf(x), np.isinf(want)) and np.array_equal(x[np.isinf(x)], want[np.isinf(want)]), form
        ok = np.isfinite(want)
        assert ok[:, finite].all()
        if mode == "float64":
            with np.errstate(invalid="ignore"):
                err = np.where(ok, np.abs(x - want) / np.maximum(np.abs(want), 1.0), 0.0)
            lane = int(err.max(axis=0).argmax())
            print("%s %s substeps=%d: scaled error %.2e (%.3f of the bar) at lane %d, group %s" % (
                form, mode, substeps, err.max(), err.max() / F64_BAR, lane, p.group[lane]))
            assert err.max() < F64_BAR, form
        else:
            diff = ok & (x.view(np.int64) != want.view(np.int64))
            bits = 28 if mode == "float32" else 23
            unit = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.where(ok, want, 1.0)), 1e-300))) - bits)
            with np.errstate(invalid="ignore"):
                over = np.where(diff, np.abs(x - want) / (unit + 1e-10), 0.0)
            print("%s %s substeps=%d: %d of %d stored words differ; the largest is %.3f of (one unit + 1e-10)" % (
                form, mode, substeps, diff.sum(), diff.size, over.max()))
            if substeps == 1:                      # x += dt * dx: one fused multiply-add of identical inputs
                assert not diff[[0, 2, 4, 6, 8, 10]].any(), form
            assert over.max() <= 1.0, form
    # the three forms agree with each other bit for bit
    for form in ("step_many", "rollout_states"):
        for a, b in zip(got[form], got["step"]):
            assert _same(a, b), form


# ---------------------------------------------------------------------------------------------------------------------
# 2. K = 8 steps in one launch are eight launches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("mode", ["float32", "float64"])
def test_eight_steps_in_one_launch_are_eight_steps(mode, substeps):
    p = ap.points()
    n, K = ap.N, 8
    rng = np.random.default_rng(8)
    a = np.clip(p.actions[None] * rng.uniform(0.8, 1.2, (K, n, 4)), 0.0, 1.0).astype(np.float32)
    env, twin = _env("lander3d", n, mode, substeps, seed=2), _env("lander3d", n, mode, substeps, seed=2)
    try:
        acts = _dev(a, env)
        for e in (env, twin):
            e.reset()
            _install(e, p.x, p.status)
        roll = [t.clone() for t in env.rollout_states(acts)]
        many = [t.clone() for t in env.step_many(acts)]
        for k in range(K):
            obs, rew, term, trunc, _ = twin.step(acts[k])
            for name, u, v in zip(("obs", "reward", "terminated", "truncated"), many, (obs, rew, term, trunc)):
                assert _same(u[k], v), (name, k)
            s = twin.get_state(only=("x", "status"))
            assert _same(to_np(roll[0][k]).T, s["x"]), k
            assert _same(roll[4][k], s["status"]), k
            assert _same(roll[1][k].float(), rew) and _same(roll[2][k], term) and _same(roll[3][k], trunc), k
        sa, sb = env.get_state(), twin.get_state()
        for key in sa:
            assert _same(np.asarray(sa[key]), np.asarray(sb[key])), key
        # two wavefronts start on the fast path and leave it inside the horizon (their lanes at full motors tumble)
        xs = to_np(roll[0])
        assert ap.wavefronts_in_range(p.x)[:2].all() and not ap.wavefronts_in_range(xs[-1].T)[:2].any()
    finally:
        env.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. neighbours: the same envs in other wavefronts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 3, 10])
@pytest.mark.parametrize("mode", ["float32", "float64"])
def test_an_env_does_not_depend_on_its_wavefronts_neighbours(mode, substeps):
    crossings, regrouped, wide = ap.neighbour_conditions(substeps)          # the ORACLE's tape
    print("oracle tape, substeps %d: %d lane-steps cross 0.785, %d wavefronts regrouped, %.1f %% wide lanes" % (
        substeps, crossings, regrouped, 100 * wide))
    assert crossings >= 32 and regrouped >= 4
    x, st, a = ap.neighbour_points()
    n, cut = ap.NEIGHBOUR_N, ap.NEIGHBOUR_SPLIT

    def run(lo, hi):
        env = _env("lander3d", hi - lo, mode, substeps, seed=4)
        try:
            env.reset()
            _install(env, np.ascontiguousarray(x[:, lo:hi]), st[lo:hi])
            acts = _dev(np.ascontiguousarray(a[:, lo:hi]), env)
            out = [to_np(t).copy() for t in env.rollout_states(acts)]
            out += [to_np(t).copy() for t in env.step_many(acts)]
            s = env.get_state(only=("x", "status", "steps", "prev_shaping"))
            return out + [np.asarray(s[k])[None] if np.asarray(s[k]).ndim == 1 else np.asarray(s[k]).T[None] for k in
                          ("x", "status", "steps", "prev_shaping")]
        finally:
            env.close()

    whole = run(0, n)
    parts = [run(0, cut), run(cut, n)]
    for i, w in enumerate(whole):
        joined = np.concatenate([parts[0][i], parts[1][i]], axis=1)
        assert _same(w, joined), i
    # the device's tape did cross the bound as well (it is the oracle's to the last bits)
    xs = np.concatenate([x.T[None], whole[0]])
    inr = np.array([ap.in_range(s.T) for s in xs])
    assert (inr[:-1] != inr[1:]).sum() >= 32


# ---------------------------------------------------------------------------------------------------------------------
# 4. derivatives against central differences of the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _fd_point(env, mode):
    """the FD point set installed on env; in the float32 modes the point is the decoded state"""
    p = ap.points()
    fd = ap.fd_lanes(p)
    x, st, a = np.ascontiguousarray(p.x[:, fd]), p.status[fd].copy(), p.actions[fd].copy()
    env.reset()
    _install(env, x, st)
    if mode != "float64":
        x = env.get_state(only=("x",))["x"]
    return fd, x, st, a


@pytest.mark.parametrize("mode", ["float64", "float32"])
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("task", ["lander3d", "hover3d"])
def test_step_jacobian_at_wide_attitudes(task, substeps, mode):
    from branch_fd import run_rollout, state_events
    from gym_copter_amd import _lib
    from test_gpu_branch_gradients import _expected_bits
    n = ap.fd_lanes(ap.points()).size
    env = _env(task, n, mode, substeps)
    try:
        fd, x, st, a = _fd_point(env, mode)
        acts = _dev(a, env)
        jac = env.step_jacobian(acts)
        got = [to_np(t).astype(np.float64) for t in jac[:4]]
        branch = to_np(jac.branch).astype(np.int64)
        term = to_np(env.rollout_states(acts[None], state={"x": x, "status": st}).terminated[0]).astype(bool)
    finally:
        env.close()
    want = fd_jacobian(task, x, st, a.astype(np.float64), substeps=substeps)
    worst = {}
    for name, g, w in zip(("dx", "du", "reward_dx", "reward_du"), got, want):
        worst[name] = _scaled(g, w)
    print("step_jacobian %s substeps=%d %s, %d lanes: " % (task, substeps, mode, n) +
          " ".join("%s %.2e" % kv for kv in worst.items()) + " (bar %.0e)" % BAR)
    # the branch bits and the flags of the ORACLE's step: every call integrated, no motor clipped; tilted or not
    tape, _ = run_rollout(task, x, st, a.astype(np.float64)[None], prev_shaping=np.zeros(n), substeps=substeps)
    bits = _expected_bits(types.SimpleNamespace(tape=tape), st, a)
    assert np.all(bits == _lib.JAC_INTEGRATED) and np.array_equal(branch, bits)
    oob, tilt, _, _ = state_events(tape["x"][0].T)
    assert not oob.any() and tilt.sum() >= 50 and (~tilt).sum() >= 50
    if mode == "float64":
        assert np.array_equal(term, tilt) and np.array_equal(term, tape["terminated"][0])
    # the quadrant logic ran for the derivative: yaw and roll / pitch in every residue
    for row in (6, 8, 10):
        q = np.rint(x[row] * (2 / np.pi)).astype(int) % 4
        assert set(q) == {0, 1, 2, 3}, row
    for name, e in worst.items():
        assert e <= BAR, (name, e)


@pytest.mark.parametrize("mode", ["float64", "float32"])
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("task", ["lander3d", "hover3d"])
def test_rollout_vjp_at_wide_attitudes(task, substeps, mode):
    """K = 4, the rollout and cotangents of attitude_points.fd_rollout_case."""
    n, K = ap.fd_lanes(ap.points()).size, ap.FD_ROLLOUT_K
    env = _env(task, n, mode, substeps)
    try:
        fd, x, st, _ = _fd_point(env, mode)
        a, gx, gr = ap.fd_rollout_case(task, substeps)
        state = {"x": x, "status": st}
        acts = _dev(a, env)
        r = env.rollout_states(acts, state=state)
        ga, g0 = env.rollout_vjp(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state)
        ga, g0 = to_np(ga).copy(), to_np(g0).copy()
        tape_x = to_np(r.x).copy()
    finally:
        env.close()
    want_a, want_0 = fd_rollout_vjp(task, x, st, a.astype(np.float64), gx=gx, gr=gr, substeps=substeps)
    ea, e0 = _scaled(ga, want_a), _scaled(g0, want_0)
    print("rollout_vjp %s substeps=%d %s, %d lanes, K = %d: g_actions %.2e g_x0 %.2e (bar %.0e)" % (
        task, substeps, mode, n, K, ea, e0, BAR))
    assert (np.abs(tape_x[..., 6]) > 2.0).any() and (np.abs(tape_x[..., 10]) > 3.0).any()
    assert ea <= BAR and e0 <= BAR, (ea, e0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. yaw periodicity at large magnitude
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task", ["hover3d", "lander3d"])
def test_derivatives_are_periodic_in_a_large_yaw(task):
    """float64, one substep: dx, du and the g_x0, g_actions of a one-step rollout_vjp at psi_big against the same at its
    twin psi_red' (the first half of the batch against the second).  The lander's yaw shaping is not periodic: its
    reward gets no cotangent and its reward rows are not compared."""
    p = ap.points()
    f, xb, xr = ap.twins(p)
    m = f.size
    bar = max(100 * ap.periodicity_distance(task, 1), F64_BAR)
    x = np.concatenate([xb, xr], axis=1)
    st = np.tile(p.status[f], 2)
    a = np.tile(p.actions[f], (2, 1))
    rng = np.random.default_rng(5)
    gx = np.tile(rng.standard_normal((1, m, 12)), (1, 2, 1))
    gr = None if task == "lander3d" else np.tile(rng.standard_normal((1, m)), (1, 2))
    env = _env(task, 2 * m, "float64", 1)
    try:
        env.reset()
        state = {"x": x, "status": st}
        acts = _dev(a, env)
        jac = env.step_jacobian(acts, state=state)
        out = {"dx": to_np(jac.dx).copy(), "du": to_np(jac.du).copy()}
        if task == "hover3d":
            out["reward_dx"], out["reward_du"] = to_np(jac.reward_dx).copy(), to_np(jac.reward_du).copy()
        r = env.rollout_states(acts[None], state=state)
        ga, g0 = env.rollout_vjp(acts[None], r, gx=_dev(gx, env), gr=None if gr is None else _dev(gr, env), state=state)
        out["g_actions"], out["g_x0"] = to_np(ga)[0].copy(), to_np(g0).T.copy()
        assert np.all(to_np(jac.branch) == 1)
    finally:
        env.close()
    worst = {k: _scaled(v[:m], v[m:]) for k, v in out.items()}
    print("%s, %d pairs up to %.1e rad: " % (task, m, np.abs(xb[10]).max()) + " ".join("%s %.2e" % kv for kv in worst.items()) +
          " (bar %.1e)" % bar)
    assert np.abs(out["dx"][:m, :6, 10]).max() > 1e-3             # the yaw column is alive: these lanes fly tilted
    for k, e in worst.items():
        assert e <= bar, (k, e, bar)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the families defined by equality with rollout_states
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["float32", "float64"])
def test_zero_policy_is_the_open_loop_rollout_at_wide_attitudes(mode):
    import torch
    from gym_copter_amd import mlp
    p = ap.points()
    n, K, hidden = ap.N, 8, 32
    rng = np.random.default_rng(6)
    u = np.clip(p.actions[None] * rng.uniform(0.8, 1.2, (K, n, 4)), 0.0, 1.0).astype(np.float32)
    env = _env("lander3d", n, mode, 1, seed=3)
    try:
        env.reset()
        # (finite yaws only: a NaN observation makes the zero policy's action NaN, 0 * NaN, where the open loop keeps its
        # offset -- the two are not the same function there)
        x0 = p.x.copy()
        x0[10, p.nonfinite] = [1e3, -1e3, 2e3]
        _install(env, x0, p.status)
        ud = _dev(u, env)
        p0 = torch.zeros(mlp.num_params(10, 4, hidden), dtype=torch.float32, device=env.device)
        x = env.get_state(only=("x",))["x"]
        for state in (None, {"x": x, "status": p.status.copy()}):
            r = env.rollout_mlp_states(p0, K, hidden, offsets=ud, state=state)
            r = type(r)(*(t.clone() for t in r))
            q = env.rollout_states(ud, state=state)
            for name, a, b in zip(q._fields, r[:5], q):
                bad = np.flatnonzero((to_np(a) != to_np(b)).reshape(K, n, -1).any(axis=(0, 2)))
                assert torch.equal(a, b), (name, state is None, bad[:8], p.group[bad[:8]])
            assert torch.equal(r.actions, ud)
    finally:
        env.close()


def test_the_filter_predicts_with_the_rollouts_step_at_wide_attitudes():
    """cs_rollout_ekf on the wide groups with finite yaws up to 300 rad and motors around hover, K = 4, a small P0: x_pred is
    rollout_states' step bit for bit and every step of the recursion meets the bars of tests/test_gpu_rollout_ekf.py
    (its _check_steps, run once)."""
    import ekf_ref
    from gym_copter_amd import measure
    from test_gpu_rollout_ekf import _check_steps, _clone, _model, _run, _spd
    from test_gpu_rollout_rts import _check_rows, _rts
    p = ap.points()
    sel = np.flatnonzero(np.isin(p.group, [g for g in ap.WIDE_GROUPS if g != "fold"]) & (np.arange(ap.N) % 8 != 0))
    n, K = sel.size, 4
    rng = np.random.default_rng(19)
    env = _env("lander3d", n, "float64", 1, seed=3)
    try:
        env.reset()
        x0, st0 = np.ascontiguousarray(p.x[:, sel]), p.status[sel].copy()
        acts = (p.actions[sel][None] * rng.uniform(0.9, 1.1, (K, n, 4))).astype(np.float32)
        H, r = _model(rng, 6, True)
        acts_d = _dev(acts, env)
        truth = env.rollout_states(acts_d, state={"x": x0, "status": st0}).x.clone()
        prob = dict(acts=acts_d, z=measure(truth, H, r, 5), H=H, r=r, Q=ekf_ref.test_Q(), x0=_dev(x0, env),
                    P0=_dev(1e-4 * _spd(rng, n), env), st0=_dev(st0, env))
        res = _clone(_run(env, prob, tape=True))
        _check_steps("wide attitudes", env, prob, res)
        assert (np.abs(x0[[6, 8]]) > 2.0).any() and (np.abs(x0[10]) > 100).any()
        # the smoother on the same tapes: every backward step at the bars of tests/test_gpu_rollout_rts.py
        smoothed = _clone(_rts(env, prob, res))
        _check_rows("wide attitudes", env, prob, res, smoothed)
    finally:
        env.close()


def test_the_particle_filter_steps_its_particles_at_wide_attitudes():
    """cs_rollout_pf on five lanes of five wide groups (a yaw past 100 rad, a roll or pitch past 2 rad, one at pi/2),
    motors around hover, K = 4, 64 particles from a small P0, float64: every prior particle is rollout_states' step
    from the same point plus the reference's noise bit for bit, and the statuses and everything downstream meet the
    checks of tests/test_gpu_rollout_pf.py (its _check_steps, run once)."""
    import ekf_ref
    import test_gpu_rollout_pf as F
    from test_gpu_rollout_ekf import _model, _spd
    p = ap.points()
    usable = (np.arange(ap.N) % 8 != 0) & np.isfinite(p.x[10])           # motors around hover, a finite yaw
    sel = np.array([np.flatnonzero((p.group == grp) & usable & cond)[0] for grp, cond in (
        ("quadrant", True), ("ymid", np.abs(p.x[10]) > 100), ("r0815", True), ("rpi2", True),
        ("r231", np.abs(p.x[[6, 8]]).max(axis=0) > 2.0))])
    n, K, P = sel.size, 4, 64
    assert n == F.N and len(set(p.group[sel])) == n and "fold" not in p.group[sel] and "nonfinite" not in p.group[sel]
    rng = np.random.default_rng(23)
    env = F._env("lander3d", n)
    penv = F._particle_env("lander3d", P, 1)
    try:
        env.reset()
        x0, st0 = np.ascontiguousarray(p.x[:, sel]), p.status[sel].copy()
        assert (np.abs(x0[[6, 8]]) > 2.0).any() and (np.abs(x0[10]) > 100).any()
        acts = (p.actions[sel][None] * rng.uniform(0.9, 1.1, (K, n, 4))).astype(np.float32)
        H, r = _model(rng, 6, True)
        acts_d = _dev(acts, env)
        truth = to_np(env.rollout_states(acts_d, state={"x": x0, "status": st0}).x).astype(np.float64)
        z = truth @ H.T + np.sqrt(r) * rng.standard_normal((K, n, 6))
        prob = dict(acts=acts_d, z=_dev(z, env), H=H, r=r, Q=ekf_ref.test_Q(), x0=_dev(x0, env),
                    P0=_dev(1e-4 * _spd(rng, n), env), st0=_dev(st0, env), nonce=11, ess_frac=0.5)
        res = F._clone(F._run(env, prob, P))
        F._check_steps("wide attitudes", env, penv, prob, res, P)
        # the particles stayed wide: no lane's cloud was pulled into the first quadrant
        part = to_np(res.part_tape)
        assert (np.abs(part[..., [6, 8]]) > 2.0).any() and (np.abs(part[..., 10]) > 100).any()
    finally:
        env.close()
        penv.close()
