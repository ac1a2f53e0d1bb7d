"""The iLQR backward pass and feedback rollout on the device (cs_rollout_lqr / cs_rollout_feedback_states,
CopterVecEnv.rollout_lqr / rollout_feedback_states, gym_copter_amd.ilqr): the gains against the NumPy recursion
(tests/lqr_ref.py) on the chained step_jacobian blocks, the Cholesky's failure path on the host, the feedback forward
bit for bit, the model's first-order consistency, the iLQR driver against a first-order baseline, and the plumbing;
the gains and the feedback forward also under the non-default vehicle models of tests/model_variants.py."""
import os
import subprocess

import zlib

import numpy as np
import pytest

import model_variants
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from lqr_ref import chol_solve, cholesky, feedback_actions, lqr_backward
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ["lander3d", "hover3d", "lander2d", "lander1d", "hover2d", "hover1d"]
TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover1d": 1, "lander1d": 1, "hover2d": 2}
AH = hover_action()
FLOOR = 1e-9      # the chained-Jacobian anchor of DESIGN section 12, scaled


def _env(task, n, mode="float64", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _random_point(n, rng):
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    x[1], x[3], x[5] = rng.uniform(-2, 2, (3, n))
    x[4] = rng.uniform(-20, -5, n)
    x[6], x[8] = rng.uniform(-0.4, 0.4, (2, n))
    x[10] = rng.uniform(-1, 1, n)
    x[7], x[9], x[11] = rng.uniform(-1, 1, (3, n))
    return x, np.full(n, AIRBORNE, np.uint8)


def _scaled(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def _cost_model(rng, A, K, n, diagonal_R=True):
    m = rng.standard_normal((12, 12))
    Q = m @ m.T / 12 + 0.1 * np.eye(12)
    m = rng.standard_normal((12, 12))
    Qf = m @ m.T / 12 + 0.5 * np.eye(12)
    R = np.diag(rng.uniform(0.5, 2.0, A))
    if not diagonal_R:
        m = rng.standard_normal((A, A))
        R = m @ m.T / A + np.eye(A)
    return Q, Qf, R, rng.standard_normal((K, n, 12)), rng.standard_normal((K, n, A))


def _compare(name, got, blocks, Q, R, q, r, Qf, mu, lanes=None):
    """the kernel's outputs against lqr_ref in float64; the bar per output is 100 x the float64 reference's own error
    (its distance from the same recursion in longdouble), floored at FLOOR; prints and returns the figures"""
    Ab, Bb = blocks
    ref = lqr_backward(Ab, Bb, Q, R, q, r, Q_final=Qf, mu=mu)
    ext = lqr_backward(Ab, Bb, Q, R, q, r, Q_final=Qf, mu=mu, dtype=np.longdouble)
    lanes = slice(None) if lanes is None else lanes
    out = {}
    for key, axis in (("K", 1), ("d", 1), ("dV", 0), ("S0", 0), ("s0", 0)):
        g = to_np(getattr(got, key)).astype(np.float64)
        if key == "s0":
            g = g.T
        pick = (lambda v: v[:, lanes]) if axis == 1 else (lambda v: v[lanes])
        spread = _scaled(pick(ref[key]), pick(ext[key]).astype(np.float64))
        err = _scaled(pick(g), pick(ref[key]))
        out[key] = (spread, err)
    print("%s: " % name + " ".join("%s ref-spread %.2e kernel-err %.2e" % (k, s, e) for k, (s, e) in out.items()))
    assert np.array_equal(to_np(got.ok).astype(bool)[lanes], ref["ok"][lanes])
    for key, (spread, err) in out.items():
        assert err <= max(100.0 * spread, FLOOR), (name, key, spread, err)
    return ref


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gains against the Jacobian chain
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_CASES = [("lander3d", "float64", 1, 0.0), ("lander3d", "float32", 1, 0.3), ("hover3d", "float64", 1, 0.0),
               ("hover3d", "float32", 1, 0.0), ("lander2d", "float64", 10, 0.0), ("hover1d", "float64", 1, 0.0)]


# the same comparison under the non-default vehicle models of tests/model_variants.py: the gyro instantiations of the
# backward kernel, its per-env coefficient load and the lift law's derivative
VARIANT_CHAIN_CASES = [("lander3d", "float64", 1, 0.0, "mars_gyro"), ("lander3d", "float32", 10, 0.3, "mars_gyro"),
                       ("hover3d", "float64", 1, 0.0, "gyro_only"), ("lander3d", "float32", 1, 0.3, "vehicles"),
                       ("hover3d", "float64", 1, 0.0, "vehicles_mars_gyro"), ("lander2d", "float64", 10, 0.0, "vehicles")]


@pytest.mark.parametrize("task,mode,substeps,mu", CHAIN_CASES)
def test_gains_equal_the_recursion_on_chained_step_jacobians(task, mode, substeps, mu):
    """K = 16, 300 envs (four whole wavefronts and a partial one), a stored start with the reset's perturbation pending,
    LANDED and CRASHED lanes and lanes with clipped motors; diagonal R so that a clipped motor's gain row is exact."""
    _gains_against_the_chain(task, mode, substeps, mu, None)


@pytest.mark.parametrize("task,mode,substeps,mu,variant", VARIANT_CHAIN_CASES)
def test_gains_equal_the_recursion_under_model_variants(task, mode, substeps, mu, variant):
    """The case above under a non-default vehicle model, the motors centred on that model's hover value; the bars are
    the same (both sides run the same model), and the x tape differs from the default model's in every airborne lane."""
    _gains_against_the_chain(task, mode, substeps, mu, variant)


def _gains_against_the_chain(task, mode, substeps, mu, variant):
    n, K, A = 300, 16, TASK_A[task]
    if variant is None:
        rng = np.random.default_rng(500 + TASKS.index(task) * 10 + substeps + (mode == "float32"))
    else:
        rng = np.random.default_rng(zlib.crc32(repr((task, mode, substeps, variant)).encode()))
    ah = model_variants.hover(variant)
    env = _env(task, n, mode, seed=4, substeps=substeps, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        x, st = _random_point(n, rng)
        g = n // 8
        x[4, :g], x[5, :g], st[:g] = 0.0, 0.0, LANDED
        st[g:2 * g] = CRASHED
        s0 = env.get_state()
        env.set_state(x=x, status=st, steps=np.ones(n, np.int32), prev_shaping=np.zeros(n), flags=s0["flags"])
        a = ah * rng.uniform(0.5, 1.5, (K, n, A))
        a[:, 2 * g:3 * g] = rng.uniform(-0.3, 1.3, (K, g, A))                 # clipped
        a = a.astype(np.float32)
        acts = _dev(a, env)
        Q, Qf, R, q, r = _cost_model(rng, A, K, n)
        ro = env.rollout_states(acts)
        tape_x, tape_s = to_np(ro.x).copy(), to_np(ro.status).copy()
        if variant is not None:
            model_variants.assert_differs_from_default(variant, tape_x, task, mode, substeps,
                                                       model_variants.stored_start(env), acts)
        got = env.rollout_lqr(acts, ro, Q, R, q=_dev(q, env), r=_dev(r, env), Q_final=Qf, mu=mu)
        Ab, Bb = np.zeros((K, n, 12, 12)), np.zeros((K, n, 12, A))
        for k in range(K):
            jac = env.step_jacobian(acts[k]) if k == 0 else \
                env.step_jacobian(acts[k], state={"x": tape_x[k - 1].T.copy(), "status": tape_s[k - 1]})
            Ab[k], Bb[k] = to_np(jac.dx).astype(np.float64), to_np(jac.du).astype(np.float64)
        assert (tape_s == LANDED).any() and (tape_s == CRASHED).any()
        _compare("%s %s substeps=%d mu=%g%s" % (task, mode, substeps, mu, " " + variant if variant else ""), got,
                 (Ab, Bb), Q, R, q, r, Qf, mu)
        assert to_np(got.ok).all()
        # clipped motors: B's column is zero, so the gain row is exactly 0 and d is -(R + mu I)^-1 r alone
        Kg, d = to_np(got.K), to_np(got.d)
        clipped = (a < 0) | (a > 1)
        assert clipped.sum() > 100
        assert np.all(Kg[clipped] == 0.0)
        l = np.sqrt(np.broadcast_to(np.diag(R) + mu, a.shape))
        assert np.array_equal(d[clipped], -((r / l) / l)[clipped])
    finally:
        env.close()


def test_gains_with_next_step_resets_pending():
    """A next_step env (float32 storage) with resets pending at the start: those envs reset in step 1 (A = B = 0) and
    the new episode's perturbation enters step 2.  The blocks are step_jacobian's at the stored state before each
    step() of the same env afterwards; envs that terminate inside the horizon are left out (the env auto-resets them,
    the rollout does not).  A resetting lane has K_1 = 0 and d_1 = -(R + mu I)^-1 r_1 exactly."""
    n, K, A, mu = 1024, 16, 4, 0.1
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
        a = (AH * rng.uniform(0.5, 1.5, (K, n, 4))).astype(np.float32)
        acts = _dev(a, env)
        Q, Qf, R, q, r = _cost_model(rng, A, K, n, diagonal_R=False)
        ro = env.rollout_states(acts)
        quiet = ~to_np(ro.terminated | ro.truncated).any(axis=0)
        got = env.rollout_lqr(acts, ro, Q, R, q=_dev(q, env), r=_dev(r, env), Q_final=Qf, mu=mu)
        got = type(got)(*(t.clone() for t in got))
        assert (quiet & pend).sum() >= 8
        Ab, Bb = np.zeros((K, n, 12, 12)), np.zeros((K, n, 12, A))
        for k in range(K):
            jac = env.step_jacobian(acts[k])
            Ab[k], Bb[k] = to_np(jac.dx).astype(np.float64), to_np(jac.du).astype(np.float64)
            if k == 0:
                assert np.all(to_np(jac.branch)[pend] & 32)                    # CS_JAC_RESET
            env.step(acts[k])
        _compare("next_step resets", got, (Ab, Bb), Q, R, q, r, Qf, mu, lanes=quiet)
        assert to_np(got.ok).all()
        Kg, d = to_np(got.K), to_np(got.d)
        assert np.all(Kg[0, pend] == 0.0) and np.any(Kg[1, quiet & pend] != 0.0)
        L, ok = cholesky(np.broadcast_to(R + mu * np.eye(A), (int(pend.sum()), A, A)))
        assert ok.all() and np.array_equal(d[0, pend], -chol_solve(L, r[0, pend]))
        assert np.all(to_np(got.S0)[pend] == 0.0) and np.all(to_np(got.s0)[:, pend] == 0.0)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. ok: the Cholesky's failure path, on the host (the same header the kernel compiles)
# ---------------------------------------------------------------------------------------------------------------------
def _host_chol(m, b):
    exe = os.path.join(ROOT, "tests", "host", "lqr_chol_host")
    A = len(b)
    out = subprocess.run([exe, str(A)] + [float(v).hex() for v in np.ravel(m)] + [float(v).hex() for v in b],
                         check=True, capture_output=True, text=True).stdout.split()
    vals = [float.fromhex(v) if "nan" not in v else float("nan") for v in out[2:]]
    return out[1] == "1", np.array(vals[:A * A]).reshape(A, A), np.array(vals[A * A:])


def test_cholesky_reports_matrices_that_are_not_positive_definite():
    rng = np.random.default_rng(8)
    for A in (1, 2, 4):
        m = rng.standard_normal((A, A))
        m = m @ m.T + 0.5 * np.eye(A)
        b = rng.standard_normal(A)
        ok, l, x = _host_chol(m, b)
        L, ok_ref = cholesky(m)
        assert ok and ok_ref and np.array_equal(np.tril(l), L) and np.array_equal(x, chol_solve(L, b))
    assert not _host_chol([[1.0, 2.0], [2.0, 1.0]], [1.0, 1.0])[0]             # indefinite: second pivot -3
    assert not _host_chol([[0.0]], [1.0])[0]                                    # a zero pivot
    assert not _host_chol([[-1.0]], [1.0])[0]
    assert not _host_chol([[float("nan"), 0.0], [0.0, 1.0]], [1.0, 1.0])[0]
    assert not _host_chol([[float("inf"), 0.0], [0.0, 1.0]], [1.0, 1.0])[0]
    m = np.diag([1.0, 1.0, 1.0, -1e-300])
    assert not _host_chol(m, np.ones(4))[0]
    assert _host_chol(np.diag([1.0, 1.0, 1.0, 1e-300]), np.ones(4))[0]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the feedback rollout, exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("mode", ["float32", "float32_rn", "float64"])
@pytest.mark.parametrize("task", TASKS)
def test_feedback_rollout_is_exact(task, mode, substeps):
    _feedback_is_exact(task, mode, substeps, None)


@pytest.mark.parametrize("variant,task,mode", [("mars_gyro", "lander3d", "float32"), ("mars_gyro", "hover3d", "float64"),
                                               ("vehicles", "lander3d", "float64"), ("vehicles", "hover3d", "float32_rn"),
                                               ("act_f32", "lander3d", "float32"), ("act_f32", "hover3d", "float64")])
def test_feedback_rollout_is_exact_under_model_variants(variant, task, mode):
    """The feedback loop's runtime rotor-gyro branch, its float32 motor law, the lift law and its per-env coefficient
    load: the same exact statements, and the x tape differs from the default model's in every lane."""
    _feedback_is_exact(task, mode, 1, variant)


def _feedback_is_exact(task, mode, substeps, variant):
    import torch
    from gym_copter_amd import LqrGains
    n, K, A = 200, 8, TASK_A[task]
    if variant is None:
        rng = np.random.default_rng(900 + TASKS.index(task) * 7 + substeps)
    else:
        rng = np.random.default_rng(zlib.crc32(repr((task, mode, variant)).encode()))
    ah = model_variants.hover(variant)
    env = _env(task, n, mode, seed=2, substeps=substeps, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        x0, st = _random_point(n, rng)
        state = {"x": x0, "status": st}
        abar = _dev((ah * rng.uniform(0.9, 1.1, (K, n, A))).astype(np.float32), env)
        Kg = _dev(0.002 * rng.standard_normal((K, n, A, 12)), env)
        d = _dev(0.01 * rng.standard_normal((K, n, A)), env)
        gains = LqrGains(Kg, d, None, None, None, None)
        # alpha = 0 on its own nominal: the nominal itself, bit for bit
        nom = type(env.rollout_states(abar, state))(*(t.clone() for t in env.rollout_states(abar, state)))
        fro, fa = env.rollout_feedback_states(abar, nom, gains, 0.0, state=state)
        assert torch.equal(fa, abar)
        for u, v in zip(fro, nom):
            assert torch.equal(u, v)
        # a nominal from a perturbed start: a nonzero deviation from step 2 on
        x1 = x0 + 0.05 * rng.standard_normal((12, n))
        off = type(nom)(*(t.clone() for t in env.rollout_states(abar, {"x": x1, "status": st})))
        alpha = rng.uniform(0.0, 1.0, n)
        fro, fa = env.rollout_feedback_states(abar, off, gains, _dev(alpha, env), state=state)
        want = feedback_actions(to_np(abar), alpha, to_np(d), to_np(Kg), to_np(fro.x), to_np(off.x))
        assert np.array_equal(to_np(fa), want)
        assert np.abs(to_np(fro.x)[:-1] - to_np(off.x)[:-1]).max() > 1e-3
        assert np.abs(to_np(fa) - to_np(abar)).max() < 0.06                 # within a few percent of hover
        ro = env.rollout_states(fa, state)
        for u, v in zip(fro, ro):
            assert torch.equal(u, v)
        if variant is not None:
            model_variants.assert_differs_from_default(variant, fro.x, task, mode, substeps, state, fa.clone())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the model's prediction converges to the actual change at first order
# ---------------------------------------------------------------------------------------------------------------------
def _tracking(rng, n, K):
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-0.5, 0.5, (2, n))
    x[4] = -5.0 + rng.uniform(-0.5, 0.5, n)
    x[5] = rng.uniform(-1.0, 1.0, n)
    x = x.astype(np.float32).astype(np.float64)
    x_ref = np.zeros((n, 12))
    x_ref[:, 0], x_ref[:, 2], x_ref[:, 4] = x[0], x[2], x[4] - 1.0            # 1 m above the start (z points down)
    Q = np.diag([1.0, 0.1, 1.0, 0.1, 1.0, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    R = np.eye(4)
    return x, x_ref, Q, R


def test_model_is_consistent_to_first_order():
    """Hover3D, float64 storage, a smooth start, a tracking cost: rho(alpha) = (J(alpha) - J(0)) / (alpha dV1 + alpha^2
    dV2) tends to 1 linearly in alpha (the model drops only the dynamics' second derivatives): |rho - 1| at 1e-3 is at
    most 1/5 of its value at 1e-2, or below the noise floor of the quotient.  The floor is what J itself cannot resolve:
    the float64 evaluation of J (its K (12 + A) terms: K (12 + A) eps J, and whatever J differs by between
    rollout_states and the feedback rollout at alpha = 0) plus the float32 rounding of the actions, to first order
    sum |dJ / da| 2^-24 |a|, over the model's prediction."""
    import torch
    from gym_copter_amd.ilqr import tracking_cost, tracking_gradients
    n, K = 512, 32
    rng = np.random.default_rng(77)
    env = _env("hover3d", n, "float64", seed=3)
    try:
        env.reset()
        x0, x_ref, Q, R = _tracking(rng, n, K)
        state = {"x": x0, "status": np.full(n, AIRBORNE, np.uint8)}
        acts = _dev((AH * rng.uniform(0.97, 1.03, (K, n, 4))).astype(np.float32), env)
        Qd, Rd, xr, ar = _dev(Q, env), _dev(R, env), _dev(x_ref, env), torch.tensor(AH, dtype=torch.float64, device=env.device)
        nom = env.rollout_states(acts, state)
        nom = type(nom)(*(t.clone() for t in nom))
        j_states = tracking_cost(nom.x, acts, xr, ar, Qd, Rd)
        q, r = tracking_gradients(nom.x, acts, xr, ar, Qd, Rd)
        gains = env.rollout_lqr(acts, nom, Q, R, q=q, r=r, state=state)
        assert bool(gains.ok.all())
        ga, _ = env.rollout_vjp(acts, nom, gx=q, state=state)
        dJda = ga + r
        noise_a = (dJda.abs() * acts.abs().double()).sum((0, 2)) * 2.0 ** -24
        fro, fa = env.rollout_feedback_states(acts, nom, gains, 0.0, state=state)
        j0 = tracking_cost(fro.x, fa, xr, ar, Qd, Rd)
        noise_j = (j_states - j0).abs() + K * 16 * np.finfo(np.float64).eps * j0.abs()
        rho = {}
        for alpha in (1e-2, 1e-3):
            fro, fa = env.rollout_feedback_states(acts, nom, gains, alpha, state=state)
            j = tracking_cost(fro.x, fa, xr, ar, Qd, Rd)
            pred = alpha * gains.dV[:, 0] + alpha * alpha * gains.dV[:, 1]
            assert bool((pred < 0).all())
            rho[alpha] = ((j - j0) / pred - 1.0).abs(), (noise_j + noise_a) / pred.abs()
        e2, e3, floor = to_np(rho[1e-2][0]), to_np(rho[1e-3][0]), to_np(rho[1e-3][1])
        print("model consistency: |rho - 1| median %.3e (alpha 1e-2) %.3e (alpha 1e-3); max %.3e %.3e; floor max %.3e; "
              "J(states) - J(feedback, 0) max %.3e" % (np.median(e2), np.median(e3), e2.max(), e3.max(), floor.max(),
                                                       float((j_states - j0).abs().max())))
        assert np.all((e3 <= e2 / 5.0) | (e3 <= floor)), int((~((e3 <= e2 / 5.0) | (e3 <= floor))).sum())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. application: iLQR against a first-order baseline with the same number of rollouts
# ---------------------------------------------------------------------------------------------------------------------
def test_ilqr_beats_adam_on_hover3d_tracking():
    """4 096 Hover3D envs, K = 64, open-loop actions from constant hover motors, tracking a setpoint 1 m above the
    start with velocity and rate weights.  Every accepted step lowers that env's cost (exact, by the line search).  The
    baseline is Adam (the step size of the closed-loop application test, 2e-4) on the same cost through
    differentiable_rollout, given as many kernel launches (forward + backward = 2) as iLQR used.  Measured (DESIGN
    section 13): batch-mean cost 34.66 at the start, iLQR 15.75 after 6 iterations (23 launches), Adam 26.60 after 11
    steps -- a ratio of 0.59.  Required: below 0.8 x the baseline's, a fifth of the baseline's cost as the margin, half
    of the measured gap left as slack for another seed of the starts."""
    import torch
    import gym_copter_amd
    from gym_copter_amd.ilqr import tracking_cost
    n, K = 4096, 64
    rng = np.random.default_rng(61)
    env = _env("hover3d", n, "float32", seed=1)
    try:
        env.reset()
        x0, x_ref, Q, R = _tracking(rng, n, K)
        state = {"x": _dev(x0, env), "status": np.full(n, AIRBORNE, np.uint8)}
        a0 = torch.full((K, n, 4), float(np.float32(AH)), dtype=torch.float32, device=env.device)
        calls = {"n": 0}
        for name in ("rollout_states", "rollout_lqr", "rollout_feedback_states"):
            def counted(*a, _f=getattr(env, name), **kw):
                calls["n"] += 1
                return _f(*a, **kw)
            setattr(env, name, counted)
        res = gym_copter_amd.ilqr(env, a0, x_ref, Q, R, a_ref=AH, iters=6, state=state)
        launches = calls["n"]
        for name in ("rollout_states", "rollout_lqr", "rollout_feedback_states"):
            delattr(env, name)
        hist, alpha = to_np(res.cost), to_np(res.alpha)
        assert hist.shape == (7, n) and alpha.shape == (6, n) and np.isfinite(hist).all()
        assert np.all(hist[1:][alpha > 0] < hist[:-1][alpha > 0]) and np.all(hist[1:][alpha == 0] == hist[:-1][alpha == 0])
        assert (alpha[0] > 0).mean() > 0.99
        Qd, Rd, xr = _dev(Q, env), _dev(R, env), _dev(x_ref, env)
        ar = torch.tensor(AH, dtype=torch.float64, device=env.device)
        check = env.rollout_states(res.actions, state)
        assert torch.allclose(tracking_cost(check.x, res.actions, xr, ar, Qd, Rd), res.cost[-1], rtol=1e-12, atol=0)
        p = a0.clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=2e-4)
        first = None
        for _ in range(launches // 2):
            opt.zero_grad()
            r = gym_copter_amd.differentiable_rollout(env, p, state=state)
            loss = tracking_cost(r.x, p, xr, ar, Qd, Rd).mean()
            loss.backward()
            opt.step()
            first = float(loss.detach()) if first is None else first
        with torch.no_grad():
            adam = float(tracking_cost(env.rollout_states(p.detach(), state).x, p.detach(), xr, ar, Qd, Rd).mean())
        ilqr_cost = float(hist[-1].mean())
        print("hover3d tracking: start %.4f; iLQR %.4f after %d launches (per iteration %s); Adam %.4f after %d steps"
              % (first, ilqr_cost, launches, " ".join("%.4f" % v for v in hist.mean(axis=1)), adam, launches // 2))
        assert ilqr_cost < 0.8 * adam, (ilqr_cost, adam)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _small_problem(env, n, K, A, rng):
    x0, st = _random_point(n, rng)
    state = {"x": x0, "status": st}
    acts = _dev((AH * rng.uniform(0.5, 1.5, (K, n, A))).astype(np.float32), env)
    Q, Qf, R, q, r = _cost_model(rng, A, K, n, diagonal_R=False)
    return state, acts, Q, Qf, R, _dev(q, env), _dev(r, env)


def test_float32_outputs_repeatability_and_one_step():
    import torch
    n, A = 257, 4
    rng = np.random.default_rng(12)
    env = _env("lander3d", n, "float32", seed=1)
    try:
        env.reset()
        for K in (5, 1):
            state, acts, Q, Qf, R, q, r = _small_problem(env, n, K, A, rng)
            ro = env.rollout_states(acts, state)
            g64 = [t.clone() for t in env.rollout_lqr(acts, ro, Q, R, q=q, r=r, Q_final=Qf, mu=0.2, state=state)]
            again = env.rollout_lqr(acts, ro, Q, R, q=q, r=r, Q_final=Qf, mu=0.2, state=state)
            for u, v in zip(g64, again):
                assert torch.equal(u, v)                                   # the same bits on every call
            g32 = env.rollout_lqr(acts, ro, Q, R, q=q, r=r, Q_final=Qf, mu=0.2, state=state, dtype=torch.float32)
            for u, v in zip(g64[:5], g32[:5]):
                assert v.dtype == torch.float32 and torch.equal(v, u.float())
            assert g32.ok.dtype == torch.bool and bool(g32.ok.all())
            assert g32.K.shape == (K, n, A, 12) and g32.d.shape == (K, n, A) and g32.dV.shape == (n, 2)
            assert g32.S0.shape == (n, 12, 12) and g32.s0.shape == (12, n)
            assert not any(t.requires_grad for t in g32)                  # autograd is not involved
        # K = 1 against the one step's blocks (Q_final is the only Hessian in play)
        jac = env.step_jacobian(acts[0], state=state)
        _compare("K=1", type(g32)(*g64), (to_np(jac.dx)[None].astype(np.float64), to_np(jac.du)[None].astype(np.float64)),
                 Q, R, to_np(q), to_np(r), Qf, 0.2)
        fro, fa = env.rollout_feedback_states(acts, ro, type(g32)(*g64), 1.0, state=state)
        want = feedback_actions(to_np(acts), np.ones(n), to_np(g64[1]), to_np(g64[0]), to_np(fro.x), to_np(ro.x))
        assert np.array_equal(to_np(fa), want)
    finally:
        env.close()


def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n, K, A = 4097, 6, 4
    rng = np.random.default_rng(3)
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = _env("lander3d", n, "float32", autoreset="next_step", seed=6, max_steps=1000)
    try:
        sh.reset()
        plain.reset()
        _, acts, Q, Qf, R, q, r = _small_problem(plain, n, K, A, rng)
        r1, r2 = sh.rollout_states(acts), plain.rollout_states(acts)
        g1 = sh.rollout_lqr(acts, r1, Q, R, q=q, r=r, Q_final=Qf)
        g2 = plain.rollout_lqr(acts, r2, Q, R, q=q, r=r, Q_final=Qf)
        for u, v in zip(g1, g2):
            assert torch.equal(u, v)
        (f1, a1), (f2, a2) = sh.rollout_feedback_states(acts, r1, g1, 0.5), plain.rollout_feedback_states(acts, r2, g2, 0.5)
        assert torch.equal(a1, a2)
        for u, v in zip(f1, f2):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_offsets_past_4_gib():
    """K_dev [K,N,A,12] float64 passes 4 GiB at K = 11 with 2^20 envs (11 x 2^20 x 384 B); the float32 output of the same
    call does not, and must hold the same values rounded."""
    import torch
    n, K = 1 << 20, 11
    assert K * n * 48 * 8 > 4 << 30 > (K - 1) * n * 48 * 8
    env = _env("lander3d", n, "float32", seed=9)
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        acts = torch.rand((K, n, 4), generator=g, device=env.device, dtype=torch.float32) * 0.2 + float(AH) - 0.1
        q = torch.randn((K, n, 12), generator=g, device=env.device, dtype=torch.float64)
        Q, R = np.eye(12), np.eye(4)
        ro = env.rollout_states(acts)
        g64 = env.rollout_lqr(acts, ro, Q, R, q=q)
        g32 = env.rollout_lqr(acts, ro, Q, R, q=q, dtype=torch.float32)
        assert bool(g64.ok.all())
        for k in (0, K - 1):
            assert torch.equal(g32.K[k], g64.K[k].float()) and torch.equal(g32.d[k], g64.d[k].float())
        assert bool(torch.isfinite(g64.K[K - 1, n - 1]).all()) and bool((g64.K[K - 1, n - 1] != 0).any())
        fro, fa = env.rollout_feedback_states(acts, ro, g64, 0.0)
        assert torch.equal(fa[K - 1], acts[K - 1]) and torch.equal(fro.x[K - 1], ro.x[K - 1])
    finally:
        env.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import _lib
    n, K, A = 128, 4, 4
    rng = np.random.default_rng(2)
    env = _env("lander3d", n, "float64", seed=1)
    try:
        env.reset()
        state, acts, Q, Qf, R, q, r = _small_problem(env, n, K, A, rng)
        ro = env.rollout_states(acts, state)
        gains = env.rollout_lqr(acts, ro, Q, R, q=q, r=r, state=state)
        bad = Q.copy()
        bad[0, 1] += 1e-9
        for kw, match in ((dict(Q=bad), "Q must be symmetric"), (dict(Q=Q[:6]), "Q must have shape"),
                          (dict(R=np.eye(3)), "R must have shape"), (dict(R=-np.eye(4)), "diagonal must be > 0"),
                          (dict(Q_final=bad), "Q_final must be symmetric"), (dict(mu=-1.0), "mu must be"),
                          (dict(mu=float("nan")), "mu must be"), (dict(q=q[:, :, :6]), "q must have shape"),
                          (dict(r=r[:2]), "r must have shape"), (dict(q=q.cpu()), "q must be on"),
                          (dict(dtype=torch.float16), "dtype must be"),
                          (dict(rollout=ro._replace(x=ro.x.float())), "rollout.x must"),
                          (dict(actions=acts[:, :n - 1]), "actions must have shape")):
            args = dict(actions=acts, rollout=ro, Q=Q, R=R, q=q, r=r, state=state)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_lqr(**args)
        with pytest.raises(ValueError, match="gains.K must"):
            env.rollout_feedback_states(acts, ro, gains._replace(K=gains.K.float()), 1.0, state=state)
        with pytest.raises(ValueError, match="gains.d must have shape"):
            env.rollout_feedback_states(acts, ro, gains._replace(d=gains.d[:2]), 1.0, state=state)
        with pytest.raises(ValueError, match="alpha must"):
            env.rollout_feedback_states(acts, ro, gains, np.ones(n + 1), state=state)
        with pytest.raises(ValueError, match="rollout.x must have shape"):
            env.rollout_feedback_states(acts[:2], ro, gains, 1.0, state=state)
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), K
        io.actions_dev, io.x_dev, io.status_dev = acts.data_ptr(), ro.x.data_ptr(), ro.status.data_ptr()
        lio = _lib.RolloutLqrIO()
        lio.struct_size = C.sizeof(lio) + 8
        assert env._lib.cs_rollout_lqr(env._ctx, C.byref(io), C.byref(lio), None) == _lib.ERR_ABI
        fio = _lib.RolloutFeedbackIO()
        fio.struct_size = C.sizeof(fio) - 8
        assert env._lib.cs_rollout_feedback_states(env._ctx, C.byref(io), C.byref(fio), None) == _lib.ERR_ABI
        # refused while a serve session is open, as every entry point that reads the env state
        env.serve_begin(2)
        try:
            with pytest.raises(gym_copter_error(), match="serv"):
                env.rollout_lqr(acts, ro, Q, R, q=q, r=r, state=state)
            with pytest.raises(gym_copter_error(), match="serv"):
                env.rollout_feedback_states(acts, ro, gains, 1.0, state=state)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_lqr(acts, ro, Q, R)
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_feedback_states(acts, ro, gains, 1.0)


def gym_copter_error():
    from gym_copter_amd import CopterStepError
    return CopterStepError
