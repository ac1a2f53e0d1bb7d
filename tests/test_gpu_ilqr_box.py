"""Control-limited iLQR on the device (cs_ilqr_box_backward / cs_ilqr_box_forward, CopterVecEnv.rollout_lqr_box /
rollout_feedback_box_states, ilqr(bounds=)): the identity with the unconstrained calls under
infinite bounds, the backward pass against tests/ilqr_box_ref.py on chained step_jacobian blocks, its exact statements,
the clamped forward bit for bit, the model's first-order consistency with the box binding, the driver against the
clamped unconstrained one, and the plumbing.  Starts, cost models and the bar are those of tests/test_gpu_rollout_lqr.py
(section 13)."""
import ctypes as C

import numpy as np
import pytest

import ilqr_box_ref
import test_gpu_rollout_lqr as L
from gpu_util import have_gpu, to_np
from lqr_ref import feedback_actions
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

AH = float(L.AH)
INF = float("inf")
BAND = 0.3                  # the box of the chain cases: hover x (1 +- BAND), strictly inside [0, 1]
assert 0.0 < AH * (1 - BAND) and AH * (1 + BAND) < 1.0


def _clone(t):
    return type(t)(*(None if v is None else v.clone() for v in t))


def _popcount(b):
    return np.unpackbits(np.asarray(b, np.uint8)[..., None], axis=-1).sum(-1)


def chain_blocks(env, acts, tape_x, tape_s, stepping=False):
    """step_jacobian's blocks along a tape (stepping: at the stored state before each step() of the env itself)"""
    K, n, A = acts.shape
    Ab, Bb = np.zeros((K, n, 12, 12)), np.zeros((K, n, 12, A))
    branch0 = None
    for k in range(K):
        if stepping or k == 0:
            jac = env.step_jacobian(acts[k])
        else:
            jac = env.step_jacobian(acts[k], state={"x": tape_x[k - 1].T.copy(), "status": tape_s[k - 1]})
        Ab[k], Bb[k] = to_np(jac.dx).astype(np.float64), to_np(jac.du).astype(np.float64)
        if k == 0:
            branch0 = to_np(jac.branch).copy()
        if stepping:
            env.step(acts[k])
    return Ab, Bb, branch0


def compare_box(name, got, blocks, abar, lo, hi, Q, R, q, r, Qf, mu, resetting=None, lanes=None, shares=(0.30, 0.05)):
    """The kernel's outputs against ilqr_box_ref in float64 on the compared envs; the bar per output is section 13's
    (100 x the float64 reference's own distance from longdouble, floored at 1e-9 scaled).  An env is compared only if at
    every step both references agree on the clamp set, every clamped control's multiplier is >= 1e-6 max(1, |Qu|_inf)
    and every free control is >= 1e-9 (scaled) from both bounds; at most 5 % of the envs may be left out, at least
    shares[0] of the compared (k, env) pairs have a clamped control and (A = 4) shares[1] two or more.  Exact on every
    env: clamped rows of K are zero, d lies in [lo - abar, hi - abar], iters < 16, ok = 1.  Prints the worst error-to-bar
    ratio and the shares; returns (ref, compared)."""
    Ab, Bb = blocks
    K, n, A = abar.shape
    kw = dict(q=q, r=r, Q_final=Qf, mu=mu, resetting=resetting)
    ref = ilqr_box_ref.lqr_box_backward(Ab, Bb, Q, R, abar, lo, hi, **kw)
    ext = ilqr_box_ref.lqr_box_backward(Ab, Bb, Q, R, abar, lo, hi, dtype=np.longdouble, **kw)
    lanes = np.ones(n, bool) if lanes is None else lanes
    good = np.ones(n, bool)
    for o in (ref, ext):
        good &= (o["mult"] >= 1e-6).all(0) & (o["gap"] >= 1e-9).all(0)
    good &= (ref["clamped"] == ext["clamped"]).all(0)
    cmp_ = good & lanes
    left_out = 1.0 - cmp_.sum() / lanes.sum()
    pc = _popcount(ref["clamped"][:, cmp_])
    any_share, two_share = float((pc >= 1).mean()), float((pc >= 2).mean())
    worst = 0.0
    figures = {}
    for key, axis in (("K", 1), ("d", 1), ("dV", 0), ("S0", 0), ("s0", 0)):
        g = to_np(getattr(got, key)).astype(np.float64)
        if key == "s0":
            g = g.T
        pick = (lambda v: v[:, cmp_]) if axis == 1 else (lambda v: v[cmp_])
        spread = L._scaled(pick(ref[key]), pick(ext[key]).astype(np.float64))
        err = L._scaled(pick(g), pick(ref[key]))
        figures[key] = (spread, err)
        worst = max(worst, err / max(100.0 * spread, L.FLOOR))
    print("%s: " % name + " ".join("%s ref-spread %.2e kernel-err %.2e" % (k, s, e) for k, (s, e) in figures.items()))
    print("%s: worst error / bar %.3f; left out %.2f %%; pairs clamped %.1f %%, two or more %.1f %%; iters max %d"
          % (name, worst, 100 * left_out, 100 * any_share, 100 * two_share, int(to_np(got.iters).max())))
    assert left_out <= 0.05, left_out
    assert any_share >= shares[0], any_share
    if A == 4:
        assert two_share >= shares[1], two_share
    for key, (spread, err) in figures.items():
        assert err <= max(100.0 * spread, L.FLOOR), (name, key, spread, err)
    flags = to_np(got.clamped)
    assert np.array_equal(flags[:, cmp_], ref["clamped"][:, cmp_])
    assert to_np(got.iters).max() < 16 and to_np(got.ok).all() and ref["ok"].all()
    assert_exact_box_statements(got, abar, lo, hi)
    return ref, cmp_


def assert_exact_box_statements(got, abar, lo, hi):
    """on every env, compared or not: a clamped control's gain row is zero and sits on its bound; d is in the box"""
    K, n, A = abar.shape
    flags, Kg, d = to_np(got.clamped), to_np(got.K), to_np(got.d)
    lo = np.broadcast_to(np.asarray(lo, np.float32), (A,)).astype(np.float64)
    hi = np.broadcast_to(np.asarray(hi, np.float32), (A,)).astype(np.float64)
    l, u = lo - abar.astype(np.float64), hi - abar.astype(np.float64)
    assert ((d >= l) & (d <= u)).all()
    low = (flags[..., None] >> np.arange(A)) & 1 == 1
    upp = (flags[..., None] >> (4 + np.arange(A))) & 1 == 1
    assert not (low & upp).any() and not (flags & ~np.uint8(((1 << A) - 1) * 17)).any()       # no other bit is set
    assert np.all(Kg[low | upp] == 0.0)
    assert np.array_equal(d[low], l[low]) and np.array_equal(d[upp], u[upp])


# ---------------------------------------------------------------------------------------------------------------------
# 1. infinite bounds: the unconstrained calls bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _chain_setup(env, task, rng, n, K, A, ah, nominal=None):
    """section 13's start: LANDED and CRASHED lanes, a stored start with the perturbation pending, and a few lanes whose
    nominal lies partly outside [0, 1] (n // 32 of them: their motors run at up to 60 x the hover value, Qu grows with
    the states they reach, and the comparison's multiplier rule -- relative to |Qu|_inf -- leaves such lanes out; they
    stay under the exact statements)"""
    env.reset()
    x, st = L._random_point(n, rng)
    g = n // 8
    x[4, :g], x[5, :g], st[:g] = 0.0, 0.0, LANDED
    st[g:2 * g] = CRASHED
    s0 = env.get_state()
    env.set_state(x=x, status=st, steps=np.ones(n, np.int32), prev_shaping=np.zeros(n), flags=s0["flags"])
    a = ah * rng.uniform(0.5, 1.5, (K, n, A)) if nominal is None else nominal(rng, (K, n, A))
    c = max(1, n // 32)
    a[:, 2 * g:2 * g + c] = rng.uniform(-0.3, 1.3, (K, c, A))             # partly outside [0, 1]
    return a.astype(np.float32)


@pytest.mark.parametrize("task,mode,substeps", [("lander3d", "float64", 1), ("lander3d", "float32", 10),
                                                ("lander2d", "float64", 1), ("hover1d", "float64", 10)])
def test_infinite_bounds_reproduce_the_unconstrained_calls(task, mode, substeps):
    import torch
    n, K, A = 300, 16, L.TASK_A[task]
    rng = np.random.default_rng(2400 + L.TASKS.index(task) + substeps)
    env = L._env(task, n, mode, seed=4, substeps=substeps)
    try:
        a = _chain_setup(env, task, rng, n, K, A, AH)
        acts = L._dev(a, env)
        Q, Qf, R, q, r = L._cost_model(rng, A, K, n, diagonal_R=False)
        ro = _clone(env.rollout_states(acts))
        kw = dict(q=L._dev(q, env), r=L._dev(r, env), Q_final=Qf, mu=0.1)
        for dtype in (None, torch.float32):
            free = _clone(env.rollout_lqr(acts, ro, Q, R, dtype=dtype, **kw))
            box = env.rollout_lqr_box(acts, ro, Q, R, -INF, INF, dtype=dtype, **kw)
            for key in ("K", "d", "dV", "S0", "s0", "ok"):
                assert torch.equal(getattr(free, key), getattr(box, key)), key
            assert not bool(box.clamped.any()) and bool((box.iters == 1).all())
        free = _clone(env.rollout_lqr(acts, ro, Q, R, **kw))
        alpha = L._dev(rng.uniform(0.0, 1.0, n), env)
        fro, fa = env.rollout_feedback_states(acts, ro, free, alpha)
        bro, ba, flags = env.rollout_feedback_box_states(acts, ro, free, alpha, -INF, INF)
        assert torch.equal(fa, ba) and not bool(flags.any())
        for u, v in zip(fro, bro):
            assert torch.equal(u, v)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the backward pass against the restatement on the Jacobian chain
# ---------------------------------------------------------------------------------------------------------------------
CHAIN_CASES = [("lander3d", "float64", 1, 0.0), ("lander3d", "float32", 1, 0.3), ("hover3d", "float64", 1, 0.0),
               ("lander2d", "float64", 10, 0.0), ("hover1d", "float64", 1, 0.0)]
GRAD_SCALE = 0.03           # the cost gradients of section 13's model, scaled so that the band binds in part: chosen
                            # on the restatement alone (at 1, 0.1, 0.01, 0.001 the share of (k, env) pairs with a
                            # clamped control is 1.00, 1.00, 0.85, 0.16 for Lander3D and 0.90, 0.59, 0.27, 0.13 for Hover1D)
GRAD_SCALE_1D = 0.1         # ... and for the tasks with one control, whose share at 0.03 is 0.27 - 0.38


def box_nominal(ah):
    return lambda rng, shape: ah * rng.uniform(1 - 0.9 * BAND, 1 + 0.9 * BAND, shape)


def gains_against_the_chain(task, mode, substeps, mu, variant=None, n=300, K=16, seed=0):
    import model_variants
    A = L.TASK_A[task]
    rng = np.random.default_rng(2500 + seed + L.TASKS.index(task) * 10 + substeps + (mode == "float32"))
    ah = float(model_variants.hover(variant))
    lo, hi = np.float32(ah * (1 - BAND)), np.float32(ah * (1 + BAND))
    env = L._env(task, n, mode, seed=4, substeps=substeps, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        a = _chain_setup(env, task, rng, n, K, A, ah, box_nominal(ah))
        acts = L._dev(a, env)
        Q, Qf, R, q, r = L._cost_model(rng, A, K, n, diagonal_R=False)
        scale = GRAD_SCALE_1D if A == 1 else GRAD_SCALE
        q, r = scale * q, scale * r
        ro = env.rollout_states(acts)
        tape_x, tape_s = to_np(ro.x).copy(), to_np(ro.status).copy()
        state_before = env.get_state()
        got = _clone(env.rollout_lqr_box(acts, ro, Q, R, lo, hi, q=L._dev(q, env), r=L._dev(r, env), Q_final=Qf, mu=mu))
        state_after = env.get_state()
        for key in state_before:
            assert np.array_equal(state_before[key], state_after[key]), key       # get_state() is unchanged
        Ab, Bb, _ = chain_blocks(env, acts, tape_x, tape_s)
        assert (tape_s == LANDED).any() and (tape_s == CRASHED).any() and ((a < 0) | (a > 1)).any()
        name = "box %s %s substeps=%d mu=%g%s" % (task, mode, substeps, mu, " " + variant if variant else "")
        compare_box(name, got, (Ab, Bb), a, lo, hi, Q, R, q, r, Qf, mu)
    finally:
        env.close()


@pytest.mark.parametrize("task,mode,substeps,mu", CHAIN_CASES)
def test_box_gains_equal_the_restatement_on_chained_step_jacobians(task, mode, substeps, mu):
    """K = 16, 300 envs, section 13's starts (LANDED and CRASHED lanes, a stored start with the perturbation pending, a
    nominal partly outside [0, 1]); the box is hover x (1 +- BAND) with the other nominals drawn inside it; a dense R."""
    gains_against_the_chain(task, mode, substeps, mu)


def test_box_gains_with_next_step_resets_pending():
    """1 024 next_step envs (float32 storage) with resets pending: a resetting lane's first step has A = B = 0, so
    K_1 = 0, S0 = s0 = 0, and d_1 is the unconstrained -(R + mu I)^-1 r_1 clamped into the box, with no iteration."""
    from lqr_ref import chol_solve, cholesky
    n, K, A, mu = 1024, 16, 4, 0.1
    rng = np.random.default_rng(2641)
    lo, hi = np.float32(AH * (1 - BAND)), np.float32(AH * (1 + BAND))
    env = L._env("lander3d", n, "float32", autoreset="next_step", seed=13)
    try:
        env.reset()
        pend = np.zeros(n, bool)
        for _ in range(300):
            _, _, term, trunc, _ = env.step(L._dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env))
            pend = to_np(term | trunc).astype(bool)
            if pend.sum() >= 32:
                break
        a = box_nominal(AH)(rng, (K, n, 4)).astype(np.float32)
        acts = L._dev(a, env)
        Q, Qf, R, q, r = L._cost_model(rng, A, K, n, diagonal_R=False)
        q, r = GRAD_SCALE * q, GRAD_SCALE * r
        ro = env.rollout_states(acts)
        quiet = ~to_np(ro.terminated | ro.truncated).any(axis=0)
        got = _clone(env.rollout_lqr_box(acts, ro, Q, R, lo, hi, q=L._dev(q, env), r=L._dev(r, env), Q_final=Qf, mu=mu))
        assert (quiet & pend).sum() >= 8
        Ab, Bb, branch0 = chain_blocks(env, acts, None, None, stepping=True)
        assert np.all(branch0[pend] & 32)                                       # CS_JAC_RESET
        compare_box("box next_step resets", got, (Ab, Bb), a, lo, hi, Q, R, q, r, Qf, mu, resetting=pend, lanes=quiet)
        Kg, d, it = to_np(got.K), to_np(got.d), to_np(got.iters)
        assert np.all(Kg[0, pend] == 0.0) and np.any(Kg[1, quiet & pend] != 0.0)
        assert np.all(it[0, pend] == 0) and np.all(it[0, ~pend] >= 1) and np.all(it[1:] >= 1)
        Lf, ok = cholesky(np.broadcast_to(R + mu * np.eye(A), (int(pend.sum()), A, A)))
        free = -chol_solve(Lf, r[0, pend])
        l, u = np.float64(lo) - a[0, pend].astype(np.float64), np.float64(hi) - a[0, pend].astype(np.float64)
        assert ok.all() and np.array_equal(d[0, pend], np.where(free < l, l, np.where(free > u, u, free)))
        assert np.all(to_np(got.S0)[pend] == 0.0) and np.all(to_np(got.s0)[:, pend] == 0.0)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact statements
# ---------------------------------------------------------------------------------------------------------------------
def test_a_pinned_box_gives_zero_gains_and_the_open_loop_value():
    """lo = hi = the (constant) nominal: K = 0 and d = 0 exactly, dV = 0, and S0, s0 are the open-loop value recursion
    S <- A^T (S + Q) A, s <- A^T (s + q), held to section 13's bar on the chain."""
    n, K, A = 300, 16, 4
    rng = np.random.default_rng(2703)
    env = L._env("lander3d", n, "float64", seed=4)
    try:
        c = np.float32(AH * 1.05)
        a = _chain_setup(env, "lander3d", rng, n, K, A, AH, lambda rng, shape: np.full(shape, c, np.float64))
        a[:] = c
        acts = L._dev(a, env)
        Q, Qf, R, q, r = L._cost_model(rng, A, K, n, diagonal_R=False)
        ro = env.rollout_states(acts)
        tape_x, tape_s = to_np(ro.x).copy(), to_np(ro.status).copy()
        got = _clone(env.rollout_lqr_box(acts, ro, Q, R, c, c, q=L._dev(q, env), r=L._dev(r, env), Q_final=Qf))
        assert np.all(to_np(got.K) == 0.0) and np.all(to_np(got.d) == 0.0) and np.all(to_np(got.dV) == 0.0)
        assert to_np(got.ok).all() and to_np(got.iters).max() == 1
        flags = to_np(got.clamped)
        assert np.all(((flags & 15) | (flags >> 4)) == 15) and np.all((flags & 15) & (flags >> 4) == 0)
        Ab, Bb, _ = chain_blocks(env, acts, tape_x, tape_s)
        figures = {}
        for dtype in (np.float64, np.longdouble):
            S, s = np.zeros((n, 12, 12), dtype), np.zeros((n, 12), dtype)
            for k in range(K - 1, -1, -1):
                Am = Ab[k].astype(dtype)
                V, v = S + (Qf if k == K - 1 else Q).astype(dtype), s + q[k].astype(dtype)
                S = np.swapaxes(Am, 1, 2) @ V @ Am
                S = np.triu(S) + np.swapaxes(np.triu(S, 1), 1, 2)
                s = np.einsum("nji,nj->ni", Am, v)
            figures[dtype] = (S, s)
        for key, g, i in (("S0", to_np(got.S0), 0), ("s0", to_np(got.s0).T, 1)):
            ref, ext = figures[np.float64][i], figures[np.longdouble][i].astype(np.float64)
            spread, err = L._scaled(ref, ext), L._scaled(g, ref)
            print("pinned box %s: ref-spread %.2e kernel-err %.2e" % (key, spread, err))
            assert err <= max(100.0 * spread, L.FLOOR), (key, spread, err)
    finally:
        env.close()


def test_repeatability_float32_outputs_and_one_step():
    """Two calls give the same bits over NaN-filled buffers; float32 outputs are the float64 ones rounded; K = 1 and
    N = 1."""
    import torch
    A = 4
    rng = np.random.default_rng(2712)
    lo, hi = (AH * np.array([0.8, 0.9, 0.0, 0.8])).astype(np.float32), np.float32(AH * 1.2)
    for n, steps in ((257, (5, 1)), (1, (3, 1))):
        env = L._env("lander3d", n, "float32", seed=1)
        try:
            env.reset()
            for K in steps:
                state, acts, Q, Qf, R, q, r = L._small_problem(env, n, K, A, rng)
                q, r = GRAD_SCALE * q, GRAD_SCALE * r
                ro = _clone(env.rollout_states(acts, state))
                kw = dict(q=q, r=r, Q_final=Qf, mu=0.2, state=state)
                first = env.rollout_lqr_box(acts, ro, Q, R, lo, hi, **kw)
                g64 = _clone(first)
                for t in first:
                    t.fill_(float("nan") if t.dtype.is_floating_point else 1)
                again = env.rollout_lqr_box(acts, ro, Q, R, lo, hi, **kw)
                assert again.K.data_ptr() == first.K.data_ptr()
                for u, v in zip(g64, again):
                    assert torch.equal(u, v)
                g32 = env.rollout_lqr_box(acts, ro, Q, R, lo, hi, dtype=torch.float32, **kw)
                for u, v in zip(g64[:5], g32[:5]):
                    assert v.dtype == torch.float32 and torch.equal(v, u.float())
                for u, v in zip(g64[5:], g32[5:]):
                    assert torch.equal(u, v)
                assert g32.clamped.shape == (K, n) and g32.iters.dtype == torch.uint8 and g32.ok.dtype == torch.bool
                assert_exact_box_statements(g64, to_np(acts), lo, hi)
                fro, fa, flags = env.rollout_feedback_box_states(acts, ro, g64, 1.0, lo, hi, state=state)
                want, bits = ilqr_box_ref.clamp_actions(
                    feedback_actions(to_np(acts), np.ones(n), to_np(g64.d), to_np(g64.K), to_np(fro.x), to_np(ro.x)), lo, hi)
                assert np.array_equal(to_np(fa), want) and np.array_equal(to_np(flags), bits)
            if n > 1:
                assert bool(g64.clamped.any())
        finally:
            env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the clamped forward, exact
# ---------------------------------------------------------------------------------------------------------------------
FORWARD_CASES = [(t, m, 1) for t in L.TASKS for m in ("float32", "float32_rn", "float64")] + [("lander3d", "float32", 10)]


def forward_is_exact(task, mode, substeps, variant=None, n=200, K=8):
    import model_variants
    import torch
    from gym_copter_amd import LqrGains
    A = L.TASK_A[task]
    rng = np.random.default_rng(2800 + L.TASKS.index(task) * 7 + substeps + (0 if variant is None else 100))
    ah = float(model_variants.hover(variant))
    lo = np.float32(ah * 0.96)
    hi = (ah * np.array([1.04, 1.035, 1.06, 1.04])[:A]).astype(np.float32)
    env = L._env(task, n, mode, seed=2, substeps=substeps, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        x0, st = L._random_point(n, rng)
        state = {"x": x0, "status": st}
        abar = L._dev((ah * rng.uniform(0.97, 1.03, (K, n, A))).astype(np.float32), env)
        Kg = L._dev(0.002 * rng.standard_normal((K, n, A, 12)), env)
        d = L._dev(0.05 * ah * rng.standard_normal((K, n, A)), env)
        gains = LqrGains(Kg, d, None, None, None, None)
        # alpha = 0 on an in-box nominal: the nominal itself, bit for bit
        nom = _clone(env.rollout_states(abar, state))
        fro, fa, flags = env.rollout_feedback_box_states(abar, nom, gains, 0.0, lo, hi, state=state)
        assert torch.equal(fa, abar) and not bool(flags.any())
        for u, v in zip(fro, nom):
            assert torch.equal(u, v)
        # a nominal from a perturbed start, bounds narrow enough that a tenth of the actions clamp
        x1 = x0 + 0.05 * rng.standard_normal((12, n))
        off = _clone(env.rollout_states(abar, {"x": x1, "status": st}))
        alpha = rng.uniform(0.0, 1.0, n)
        fro, fa, flags = env.rollout_feedback_box_states(abar, off, gains, L._dev(alpha, env), lo, hi, state=state)
        raw = feedback_actions(to_np(abar), alpha, to_np(d), to_np(Kg), to_np(fro.x), to_np(off.x))
        want, bits = ilqr_box_ref.clamp_actions(raw, lo, hi)
        assert np.array_equal(to_np(fa), want) and np.array_equal(to_np(flags), bits)
        share = float((raw != want).mean())
        assert share >= 0.10, share
        assert ((want >= lo) & (want <= hi)).all()
        ro = env.rollout_states(fa, state)
        for u, v in zip(fro, ro):
            assert torch.equal(u, v)
        return share
    finally:
        env.close()


@pytest.mark.parametrize("task,mode,substeps", FORWARD_CASES)
def test_clamped_forward_is_exact(task, mode, substeps):
    forward_is_exact(task, mode, substeps)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the model's prediction converges to the actual change at first order, with the box binding
# ---------------------------------------------------------------------------------------------------------------------
def test_model_is_consistent_to_first_order_with_binding_bounds():
    """Section 13's test with motors 0 and 1 on their upper limit (the nominal holds them at hi exactly, the climb asks
    for more: the box binds in at least 20 % of the (k, env) pairs, asserted) and motors 2 and 3 unlimited:
    rho(alpha) = (J(alpha) - J(0)) / (alpha dV1 + alpha^2 dV2).  The error is first order in alpha, so the expected
    factor between alpha = 1e-2 and 1e-3 is 10; required: the median |rho - 1| at 1e-3 below that at 1e-2 divided by 5.

    The nominal sits ON the binding bounds because alpha dV1 + alpha^2 dV2 is the model's change for alpha < 1 only
    where the clamped controls' steps d_c are zero: the value gradient the recursion carries is that of the full step,
    s = Qx + K^T Qu + (Qux^T d + K^T Quu d), and the bracket -- zero for the unconstrained solve at mu = 0 -- is
    Qux_c^T d_c - Qux_f^T H_ff^-1 H_fc d_c under a clamp set c.  With a nominal strictly inside a box
    that binds in 99.9 % of the pairs the same quotient was 5.8e-2 at both alphas."""
    import torch
    from gym_copter_amd.ilqr import tracking_cost, tracking_gradients
    n, K = 512, 32
    rng = np.random.default_rng(2977)
    top = np.float32(AH * 1.01)
    lo, hi = -INF, np.array([top, top, INF, INF], np.float32)
    env = L._env("hover3d", n, "float64", seed=3)
    try:
        env.reset()
        x0, x_ref, Q, R = L._tracking(rng, n, K)
        state = {"x": x0, "status": np.full(n, AIRBORNE, np.uint8)}
        a = (AH * rng.uniform(0.97, 1.03, (K, n, 4))).astype(np.float32)
        a[..., :2] = top
        acts = L._dev(a, env)
        Qd, Rd, xr = L._dev(Q, env), L._dev(R, env), L._dev(x_ref, env)
        ar = torch.tensor(AH, dtype=torch.float64, device=env.device)
        nom = _clone(env.rollout_states(acts, state))
        q, r = tracking_gradients(nom.x, acts, xr, ar, Qd, Rd)
        gains = _clone(env.rollout_lqr_box(acts, nom, Q, R, lo, hi, q=q, r=r, state=state))
        assert bool(gains.ok.all())
        binding = float((gains.clamped != 0).double().mean())
        fro, fa, _ = env.rollout_feedback_box_states(acts, nom, gains, 0.0, lo, hi, state=state)
        j0 = tracking_cost(fro.x, fa, xr, ar, Qd, Rd)
        med = {}
        for alpha in (1e-2, 1e-3):
            fro, fa, _ = env.rollout_feedback_box_states(acts, nom, gains, alpha, lo, hi, state=state)
            j = tracking_cost(fro.x, fa, xr, ar, Qd, Rd)
            pred = alpha * gains.dV[:, 0] + alpha * alpha * gains.dV[:, 1]
            assert bool((pred < 0).all())
            med[alpha] = float(((j - j0) / pred - 1.0).abs().median())
        print("box model consistency: pairs with a clamped control %.1f %%; median |rho - 1| %.3e (alpha 1e-2) %.3e "
              "(alpha 1e-3)" % (100 * binding, med[1e-2], med[1e-3]))
        assert binding >= 0.20, binding
        assert med[1e-3] < med[1e-2] / 5.0, med
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. application: the driver under control limits against the clamped unconstrained driver
# ---------------------------------------------------------------------------------------------------------------------
def test_ilqr_with_bounds_beats_the_clamped_unconstrained_plan():
    """4 096 Hover3D envs, K = 64, section 13's tracking problem (a setpoint 1 m above the start) with the motors kept
    within hover +- 4 %: the unconstrained plan leaves that band.  With bounds= every accepted step lowers its env's
    cost, every returned action is in the box, at least 10 % of them lie on a bound, and the batch-mean cost is strictly
    below the baseline's: today's ilqr on the same problem, its result clamped into the box and re-rolled."""
    import torch
    import gym_copter_amd
    from gym_copter_amd.ilqr import tracking_cost
    n, K = 4096, 64
    rng = np.random.default_rng(61)
    lo, hi = np.float32(AH * 0.96), np.float32(AH * 1.04)
    env = L._env("hover3d", n, "float32", seed=1)
    try:
        env.reset()
        x0, x_ref, Q, R = L._tracking(rng, n, K)
        state = {"x": L._dev(x0, env), "status": np.full(n, AIRBORNE, np.uint8)}
        a0 = torch.full((K, n, 4), float(np.float32(AH)), dtype=torch.float32, device=env.device)
        Qd, Rd, xr = L._dev(Q, env), L._dev(R, env), L._dev(x_ref, env)
        ar = torch.tensor(AH, dtype=torch.float64, device=env.device)
        free = gym_copter_amd.ilqr(env, a0, x_ref, Q, R, a_ref=AH, iters=6, state=state)
        outside = float(((free.actions < float(lo)) | (free.actions > float(hi))).float().mean())
        assert outside > 0.10, outside                       # the unconstrained plan does leave the band
        clamped = torch.clamp(free.actions, float(lo), float(hi))
        base = float(tracking_cost(env.rollout_states(clamped, state).x, clamped, xr, ar, Qd, Rd).mean())
        res = gym_copter_amd.ilqr(env, a0, x_ref, Q, R, a_ref=AH, iters=6, state=state, bounds=(lo, hi))
        hist, alpha = to_np(res.cost), to_np(res.alpha)
        assert hist.shape == (7, n) and np.isfinite(hist).all()
        assert np.all(hist[1:][alpha > 0] < hist[:-1][alpha > 0]) and np.all(hist[1:][alpha == 0] == hist[:-1][alpha == 0])
        acts = to_np(res.actions)
        assert ((acts >= lo) & (acts <= hi)).all()
        on_bound = float(((acts == lo) | (acts == hi)).mean())
        check = env.rollout_states(res.actions, state)
        assert torch.allclose(tracking_cost(check.x, res.actions, xr, ar, Qd, Rd), res.cost[-1], rtol=1e-12, atol=0)
        box_cost = float(hist[-1].mean())
        print("hover3d tracking in hover +- 4 %%: start %.4f; unconstrained %.4f with %.1f %% of its actions outside, "
              "clamped and re-rolled %.4f; bounds= %.4f (per iteration %s), ratio %.3f; on a bound %.1f %%"
              % (hist[0].mean(), float(free.cost[-1].mean()), 100 * outside, base, box_cost,
                 " ".join("%.4f" % v for v in hist.mean(axis=1)), box_cost / base, 100 * on_bound))
        assert on_bound >= 0.10, on_bound
        assert box_cost < base, (box_cost, base)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_each_optional_output_null_leaves_the_others_alone():
    """the C ABI directly: clamped_dev and iters_dev NULL, one at a time and both, give the same bits in every other
    output (and in the one that stays)"""
    import torch
    from gym_copter_amd import _lib
    from gym_copter_amd.ilqr import _box, _feedback_blocks, _lqr_blocks
    n, K, A = 300, 3, 4
    rng = np.random.default_rng(2850)
    lo, hi = np.float32(AH * 0.9), np.float32(AH * 1.1)
    env = L._env("lander3d", n, "float64", seed=1)
    try:
        env.reset()
        state, acts, Q, Qf, R, q, r = L._small_problem(env, n, K, A, rng)
        ro = _clone(env.rollout_states(acts, state))
        full = _clone(env.rollout_lqr_box(acts, ro, Q, R, lo, hi, q=q, r=r, Q_final=Qf, state=state))
        assert bool(full.clamped.any())
        lod, hid = _box(env, lo, hi)
        for drop in (("clamped_dev",), ("iters_dev",), ("clamped_dev", "iters_dev")):
            io, lio, out, keep = _lqr_blocks(env, "lqr_box", acts, ro, Q, R, q, r, Qf, 0.0, state, None)
            flags = [torch.full((K, n), 0x11, dtype=torch.uint8, device=env.device) for _ in range(2)]
            for t in out:
                t.fill_(float("nan") if t.dtype.is_floating_point else 1)
            bio = _lib.RolloutIlqrBoxIO()
            bio.struct_size = C.sizeof(bio)
            bio.lo_dev, bio.hi_dev = lod.data_ptr(), hid.data_ptr()
            bio.clamped_dev = None if "clamped_dev" in drop else flags[0].data_ptr()
            bio.iters_dev = None if "iters_dev" in drop else flags[1].data_ptr()
            with torch.cuda.device(env.device):
                rc = env._lib.cs_ilqr_box_backward(env._ctx, C.byref(io), C.byref(lio), C.byref(bio), env._stream())
            assert rc == 0
            torch.cuda.synchronize()
            for u, v in zip(full[:6], out):
                assert torch.equal(u, v)
            for name, t, want in (("clamped_dev", flags[0], full.clamped), ("iters_dev", flags[1], full.iters)):
                assert bool((t == 0x11).all()) if name in drop else torch.equal(t, want)
        gains = full
        res = env.rollout_feedback_box_states(acts, ro, gains, 1.0, lo, hi, state=state)
        fro, fa, fl = _clone(res[0]), res[1].clone(), res[2].clone()
        io, fio, ro2, acts2, keep = _feedback_blocks(env, "feedback_box", acts, ro, gains, 1.0, state)
        acts2.fill_(float("nan"))
        bio = _lib.RolloutIlqrBoxIO()
        bio.struct_size = C.sizeof(bio)
        bio.lo_dev, bio.hi_dev = lod.data_ptr(), hid.data_ptr()
        with torch.cuda.device(env.device):
            assert env._lib.cs_ilqr_box_forward(env._ctx, C.byref(io), C.byref(fio), C.byref(bio), env._stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(acts2, fa) and bool(fl.any())
        for u, v in zip(fro, ro2):
            assert torch.equal(u, v)
    finally:
        env.close()


def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n, K, A = 4097, 6, 4
    rng = np.random.default_rng(2803)
    lo, hi = np.float32(AH * 0.8), np.float32(AH * 1.2)
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = L._env("lander3d", n, "float32", autoreset="next_step", seed=6, max_steps=1000)
    try:
        sh.reset()
        plain.reset()
        _, acts, Q, Qf, R, q, r = L._small_problem(plain, n, K, A, rng)
        r1, r2 = sh.rollout_states(acts), plain.rollout_states(acts)
        g1 = sh.rollout_lqr_box(acts, r1, Q, R, lo, hi, q=q, r=r, Q_final=Qf)
        g2 = plain.rollout_lqr_box(acts, r2, Q, R, lo, hi, q=q, r=r, Q_final=Qf)
        for u, v in zip(g1, g2):
            assert torch.equal(u, v)
        f1 = sh.rollout_feedback_box_states(acts, r1, g1, 0.5, lo, hi)
        f2 = plain.rollout_feedback_box_states(acts, r2, g2, 0.5, lo, hi)
        assert torch.equal(f1[1], f2[1]) and torch.equal(f1[2], f2[2])
        for u, v in zip(f1[0], f2[0]):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import torch
    from gym_copter_amd import CopterStepError, _lib
    n, K, A = 128, 4, 4
    rng = np.random.default_rng(2802)
    env = L._env("lander3d", n, "float64", seed=1)
    try:
        env.reset()
        state, acts, Q, Qf, R, q, r = L._small_problem(env, n, K, A, rng)
        ro = _clone(env.rollout_states(acts, state))
        gains = _clone(env.rollout_lqr_box(acts, ro, Q, R, 0.0, 1.0, q=q, r=r, state=state))
        for lo, hi, match in ((float("nan"), 1.0, "lo must not be NaN"), (0.0, float("nan"), "hi must not be NaN"),
                              (0.6, 0.5, "lo must be <= hi"), (np.zeros(3), 1.0, "lo must be a scalar or have shape"),
                              (0.0, np.ones((1, 4)), "hi must be a scalar or have shape"),
                              (np.array([0.0, 0.0, 0.9, 0.0]), np.array([1.0, 1.0, 0.8, 1.0]), "lo must be <= hi")):
            with pytest.raises(ValueError, match=match):
                env.rollout_lqr_box(acts, ro, Q, R, lo, hi, q=q, r=r, state=state)
            with pytest.raises(ValueError, match=match):
                env.rollout_feedback_box_states(acts, ro, gains, 1.0, lo, hi, state=state)
            with pytest.raises(ValueError, match=match):
                import gym_copter_amd
                gym_copter_amd.ilqr(env, acts, np.zeros(12), Q, R, state=state, bounds=(lo, hi))
        # the unconstrained calls' own errors come through
        with pytest.raises(ValueError, match="mu must be"):
            env.rollout_lqr_box(acts, ro, Q, R, 0.0, 1.0, mu=-1.0, state=state)
        with pytest.raises(ValueError, match="R must have shape"):
            env.rollout_lqr_box(acts, ro, Q, np.eye(3), 0.0, 1.0, state=state)
        with pytest.raises(ValueError, match="gains.K must"):
            env.rollout_feedback_box_states(acts, ro, gains._replace(K=gains.K.float()), 1.0, 0.0, 1.0, state=state)
        with pytest.raises(ValueError, match="alpha must"):
            env.rollout_feedback_box_states(acts, ro, gains, np.ones(n + 1), 0.0, 1.0, state=state)
        env.rollout_feedback_box_states(acts, ro, gains, 1.0, 0.0, 1.0, state=state)
        # the bounds are uploaded once while they stay the same, apart from the weights
        b1 = env._uploaded["ilqr_box"][1]
        env.rollout_lqr_box(acts, ro, Q, R, 0.0, 1.0, q=q, r=r, state=state)
        assert env._uploaded["ilqr_box"][1] is b1 and "lqr_weights" in env._uploaded
        assert {k[0] for k in env._rollout_out} >= {"lqr_box", "lqr_box_flags", "feedback_box", "feedback_box_flags"}
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), K
        io.actions_dev, io.x_dev, io.status_dev = acts.data_ptr(), ro.x.data_ptr(), ro.status.data_ptr()
        lio = _lib.RolloutLqrIO()
        lio.struct_size = C.sizeof(lio)
        lio.Q_dev, lio.R_dev = q.data_ptr(), r.data_ptr()          # (never read: the call is refused)
        bio = _lib.RolloutIlqrBoxIO()
        bio.struct_size = C.sizeof(bio) + 8
        assert env._lib.cs_ilqr_box_backward(env._ctx, C.byref(io), C.byref(lio), C.byref(bio), None) == _lib.ERR_ABI
        fio = _lib.RolloutFeedbackIO()
        fio.struct_size = C.sizeof(fio) - 8
        assert env._lib.cs_ilqr_box_forward(env._ctx, C.byref(io), C.byref(fio), C.byref(bio), None) == _lib.ERR_ABI
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_lqr_box(acts, ro, Q, R, 0.0, 1.0, q=q, r=r, state=state)
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_feedback_box_states(acts, ro, gains, 1.0, 0.0, 1.0, state=state)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_lqr_box(acts, ro, Q, R, 0.0, 1.0)
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_feedback_box_states(acts, ro, gains, 1.0, 0.0, 1.0)
