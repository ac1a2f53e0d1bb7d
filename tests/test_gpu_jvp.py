"""Forward-mode rollout tangents on the device (cs_jvp_rollout, CopterVecEnv.rollout_jvp, RolloutFunction.jvp; DESIGN.md
section 26): K = 1 against step_jacobian, central differences of the float64 oracle, the adjoint identity with
rollout_vjp_params through every branch, shapes and direction blocks, composition, the outputs' memory contract, purity,
torch.autograd.forward_ad and the sharded passthrough.

Tolerances are the project's own (_scaled(got, want) = max |got - want| / max(1, |want|)): 1e-6 against central
differences of the float64 oracle at h = 1e-6, 1e-9 between two device evaluations of the same linear map."""
import ctypes as C
import zlib

import numpy as np
import pytest

import jvp_ref
import test_gpu_rollout_param_grad as PG
from gpu_util import have_gpu, to_np
from guarded_outputs import guarded
from jacobian_fd import hover_action
from oracle.refcpu import LANDED, LEVELING

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

_env, _dev, _scaled, _random_point, _table, ROWS, MARS = (PG._env, PG._dev, PG._scaled, PG._random_point, PG._table,
                                                          PG.ROWS, PG.MARS)
TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "lander1d": 1}


def _directions(rng, D, K, n, A, table):
    """D random directions that mix actions, x0, every vehicle row (relative to the row) and the force"""
    return (0.05 * rng.standard_normal((D, K, n, A)), rng.standard_normal((D, 12, n)),
            0.1 * rng.standard_normal((D, 12, n)) * table, 10.0 * rng.standard_normal((D, 3, n)))


def _tangents(env, acts, r, dirs, state=None, vehicle=None, dtype=None, use=(True, True, True, True)):
    """rollout_jvp with the directions on the device; a copy of its buffers as NumPy (x, reward)"""
    t = [_dev(d, env) if u else None for d, u in zip(dirs, use)]
    out = env.rollout_jvp(acts, r, t_actions=t[0], t_x0=t[1], t_vehicle=t[2], t_force=t[3], state=state,
                          vehicle=vehicle, dtype=dtype)
    return to_np(out.x).copy(), to_np(out.reward).copy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. K = 1 against step_jacobian
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("task", ["lander3d", "hover3d", "lander2d", "lander1d"])
def test_one_step_equals_step_jacobian(task, substeps):
    """n = 65 (one whole and one partial tile), an explicit start with a given prev_shaping, unit directions of x0 and of
    the action (D = 12 + A): t_x is the columns of dx and du, t_reward is reward_dx and reward_du, within 1e-9."""
    n, A = 65, TASK_A[task]
    D = 12 + A
    rng = np.random.default_rng(zlib.crc32(repr((task, substeps)).encode()))
    env = _env(task, n, "float64", substeps=substeps, seed=2)
    try:
        x, st = _random_point(n, rng)
        state = {"x": _dev(x, env), "status": _dev(st, env), "force": _dev(rng.uniform(-30, 30, (3, n)), env)}
        a = (hover_action() * rng.uniform(0.6, 1.4, (1, n, A))).astype(np.float32)
        a[0, ::7] = rng.uniform(-0.3, 1.3, a[0, ::7].shape)                     # some clipped
        acts = _dev(a, env)
        jac = env.step_jacobian(acts[0], state=state)
        dx, du, rdx, rdu = (to_np(t).copy() for t in jac[:4])
        start = dict(state, prev_shaping=_dev(rng.standard_normal(n), env))
        r = env.rollout_states(acts, state=start)
        t_x0 = np.zeros((D, 12, n))
        t_x0[np.arange(12), np.arange(12)] = 1.0
        t_a = np.zeros((D, 1, n, A))
        t_a[12 + np.arange(A), 0, :, np.arange(A)] = 1.0
        out = env.rollout_jvp(acts, r, t_actions=_dev(t_a, env), t_x0=_dev(t_x0, env), state=start)
        tx, tr = to_np(out.x)[:, 0], to_np(out.reward)[:, 0]                     # [D, n, 12], [D, n]
        want_x = np.concatenate([dx.transpose(2, 0, 1), du.transpose(2, 0, 1)])  # [D, n, 12]
        want_r = np.concatenate([rdx.T, rdu.T])
        assert np.any(du != 0) and ((a < 0) | (a > 1)).any()
        assert _scaled(tx, want_x) <= 1e-9, _scaled(tx, want_x)
        assert _scaled(tr, want_r) <= 1e-9, _scaled(tr, want_r)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. central differences of the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("start", ["explicit", "stored"])
@pytest.mark.parametrize("mars", [False, True], ids=["B_law", "mars_gyro"])
def test_tangents_match_central_differences(mars, start, substeps):
    n, K, D = 256, 8, 3
    rng = np.random.default_rng(zlib.crc32(repr((mars, start, substeps)).encode()))
    env = _env("lander3d", n, "float64", substeps=substeps, seed=3, **(dict(MARS) if mars else {}))
    try:
        table = _table(rng, n, mars)
        ah = PG._mars_hover() if mars else hover_action()
        a = (ah * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32)
        if start == "explicit":
            x, st = _random_point(n, rng)
            f = rng.uniform(-30, 30, (3, n))
            state, prev = {"x": x, "status": st, "force": f}, None
        else:  # the stored start after reset: the episode's perturbation pending
            env.set_vehicle_params(table)
            env.reset()
            s = env.get_state()
            assert np.all(s["flags"] & 1)
            x, st, f, prev = s["x"], s["status"], s["force"], s["prev_shaping"]
            state = None
        acts, vt = _dev(a, env), _dev(table, env)
        dirs = _directions(rng, D, K, n, 4, table)
        if start == "stored":
            # the reset state has psi = dpsi = 0 exactly, the kink of the shaping's yaw term sqrt(psi^2 + dpsi^2): a
            # perturbation of those two slots has no derivative for central differences to find (the rule takes 0)
            dirs[1][:, 10:] = 0.0
        r = env.rollout_states(acts, state=state, vehicle=vt)
        tx, tr = _tangents(env, acts, r, dirs, state=state, vehicle=vt)
        want_x, want_r = jvp_ref.fd_tangents("lander3d", x, st, a, table, f, *dirs, prev_shaping=prev,
                                             substeps=substeps, mars=mars)
        assert _scaled(tx, want_x) <= 1e-6, ("t_x", _scaled(tx, want_x))
        assert _scaled(tr, want_r) <= 1e-6, ("t_reward", _scaled(tr, want_r))
        assert np.abs(tx).max() > 1e-2 and np.abs(tr).max() > 1e-2
        # rows that do not enter the configuration give exactly 0
        zero = ["B"] if mars else ["rho", "C_L", "Jr"]
        t_v = np.zeros((1, 12, n))
        for k in zero:
            t_v[0, ROWS.index(k)] = table[ROWS.index(k)] + 1.0
        out = env.rollout_jvp(acts, r, t_vehicle=_dev(t_v, env), state=state, vehicle=vt)
        assert not bool(out.x.any()) and not bool(out.reward.any())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the adjoint identity with rollout_vjp_params
# ---------------------------------------------------------------------------------------------------------------------
def _mixed_population(env, n, K, rng):
    """tests/test_gpu_rollout_grad.py::test_gradient_equals_chained_step_jacobians' population with per-env vehicles: a
    stored start with perturbations pending, LANDED and LEVELING envs and clipped actions"""
    table = _table(rng, n, False)
    env.set_vehicle_params(table)
    env.reset()
    x, st = _random_point(n, rng)
    q = n // 8
    x[4, :q], x[5, :q], st[:q] = 0.0, 0.0, LANDED
    x[4, q:2 * q], x[5, q:2 * q], st[q:2 * q] = 0.0, 0.0, LEVELING
    s0 = env.get_state()
    env.set_state(x=x, status=st, steps=np.ones(n, np.int32), prev_shaping=np.zeros(n), flags=s0["flags"])
    a = hover_action() * rng.uniform(0.5, 1.5, (K, n, 4))
    a[:, 2 * q:3 * q] = rng.uniform(-0.3, 1.3, (K, q, 4))
    return table, a.astype(np.float32)


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("population", ["stored", "explicit", "next_step"])
def test_adjoint_identity(population, K):
    """Per env and per direction, <gx, t_x> + <gr, t_reward> = <g_actions, t_a> + <g_x0, t_x0> + <g_vehicle, t_v> +
    <g_force, t_f>, the right-hand side from rollout_vjp_params: within 1e-9 of the sum of the absolute terms.  float32
    storage; the populations hold every branch (asserted).

    Under saturated, unbalanced motors the body rates of a few lanes grow faster than exponentially (the cross-coupling
    terms multiply two rates) and the PRIMAL overflows float64 inside K = 32 steps: the tape holds inf and NaN there (9,
    15 and 18 of 512 lanes measured in the three populations, in the mixed ones all in the clipped group; none at
    K = 8), so neither product exists.  Lanes whose tape passes
    1e30 are left out of the comparison -- at most 5 % of the lanes, asserted -- and on every other lane all of both
    kernels' outputs must be finite."""
    n, D = 512, 3
    rng = np.random.default_rng(zlib.crc32(repr((population, K)).encode()))
    env = _env("lander3d", n, "float32", autoreset="next_step" if population == "next_step" else "disabled", seed=4)
    try:
        state = None
        if population == "next_step":
            table = _table(rng, n, False)
            env.set_vehicle_params(table)
            env.reset()
            pend = np.zeros(n, bool)
            for _ in range(300):
                _, _, term, trunc, _ = env.step(_dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env))
                pend = to_np(term | trunc).astype(bool)
                if pend.sum() >= 16:
                    break
            assert pend.sum() >= 16
            a = (hover_action() * rng.uniform(0.5, 1.5, (K, n, 4))).astype(np.float32)
        else:
            table, a = _mixed_population(env, n, K, rng)
            s = env.get_state()
            assert np.all(s["flags"] & 1) and (s["status"] == LANDED).any() and (s["status"] == LEVELING).any()
            assert ((a < 0) | (a > 1)).any()
            if population == "explicit":
                state = {"x": _dev(s["x"], env), "status": _dev(s["status"], env), "force": _dev(s["force"], env)}
        acts = _dev(a, env)
        dirs = _directions(rng, D, K, n, 4, table)
        use = (True, state is not None, True, True)     # (a stored start returns no g_x0)
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        r = env.rollout_states(acts, state=state)
        status = to_np(r.status)
        if population != "next_step":
            assert (status == LANDED).any()
        with np.errstate(invalid="ignore"):
            ok = np.nan_to_num(np.abs(to_np(r.x)), nan=np.inf).max(axis=(0, 2)) < 1e30      # [n]: the primal exists
        print("adjoint identity (%s, K = %d): %d of %d lanes compared" % (population, K, ok.sum(), n))
        assert ok.mean() >= 0.95, ok.mean()
        if population != "next_step":
            q = n // 8
            assert np.all(ok[:2 * q]) and np.all(ok[3 * q:]) and ok[2 * q:3 * q].sum() > q // 2
        tx, tr = _tangents(env, acts, r, dirs, state=state, use=use)
        ga, g0, gv, gf = (None if g is None else to_np(g).copy() for g in
                          env.rollout_vjp_params(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state))
        t_a, t_x0, t_v, t_f = dirs
        lhs = [np.einsum("knj,dknj->dn", gx, tx), np.einsum("kn,dkn->dn", gr, tr)]
        labs = np.einsum("knj,dknj->dn", np.abs(gx), np.abs(tx)) + np.einsum("kn,dkn->dn", np.abs(gr), np.abs(tr))
        rhs = [np.einsum("knj,dknj->dn", ga, t_a), np.einsum("jn,djn->dn", gv, t_v), np.einsum("jn,djn->dn", gf, t_f)]
        rabs = np.einsum("knj,dknj->dn", np.abs(ga), np.abs(t_a)) + np.einsum("jn,djn->dn", np.abs(gv), np.abs(t_v)) + \
            np.einsum("jn,djn->dn", np.abs(gf), np.abs(t_f))
        if state is not None:
            rhs.append(np.einsum("jn,djn->dn", g0, t_x0))
            rabs = rabs + np.einsum("jn,djn->dn", np.abs(g0), np.abs(t_x0))
        for name, arr in (("t_x", tx), ("t_reward", tr), ("g_actions", ga), ("g_vehicle", gv), ("g_force", gf)):
            assert np.isfinite(np.compress(ok, arr, axis=-2 if name in ("t_x", "g_actions") else -1)).all(), name
        with np.errstate(invalid="ignore", over="ignore"):
            diff, scale = np.abs(sum(lhs) - sum(rhs))[:, ok], (labs + rabs)[:, ok]
        # (a LANDED lane of a stored start has no term at all: both sides are exactly 0)
        err = float(np.max(diff / np.maximum(scale, 1e-300)))
        assert err <= 1e-9, err
        assert np.abs(sum(lhs)[:, ok]).max() > 1.0
        if population == "next_step":       # the reset zeroes the x0, first-action and force tangents of its lanes
            only = (np.zeros_like(t_a), np.zeros_like(t_x0), np.zeros_like(t_v), t_f)
            only[0][:, 0] = t_a[:, 0]
            zx, zr = _tangents(env, acts, r, only, use=(True, False, False, True))
            assert np.all(zx[:, :, pend] == 0.0) and np.all(zr[:, :, pend] == 0.0)
            assert np.any(zx[:, :, ~pend] != 0.0)
            assert np.any(tx[:, 1:, pend] != 0.0)   # ... and the steps after it still carry the vehicle tangent
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. shapes: tiles, horizons and direction blocks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65])
def test_shapes_direction_blocks_zero_and_linearity(n):
    rng = np.random.default_rng(n)
    env = _env("lander3d", n, "float64", seed=5)
    try:
        table = _table(rng, n, False)
        vt = _dev(table, env)
        x, st = _random_point(n, rng)
        state = {"x": x, "status": st, "force": rng.uniform(-30, 30, (3, n))}
        for K in (1, 2, 3):
            acts = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env)
            r = env.rollout_states(acts, state=state, vehicle=vt)
            dirs = _directions(rng, 3, K, n, 4, table)
            single = [_tangents(env, acts, r, [d[j] for d in dirs], state=state, vehicle=vt) for j in range(3)]
            assert single[0][0].shape == (K, n, 12) and single[0][1].shape == (K, n)
            for D in (1, 2, 3):
                tx, tr = _tangents(env, acts, r, [d[:D] for d in dirs], state=state, vehicle=vt)
                assert tx.shape == (D, K, n, 12) and tr.shape == (D, K, n)
                for j in range(D):      # each direction of a block call equals its D = 1 call, bit for bit
                    assert np.array_equal(tx[j], single[j][0]) and np.array_equal(tr[j], single[j][1]), (K, D, j)
            zx, zr = _tangents(env, acts, r, [np.zeros_like(d) for d in dirs], state=state, vehicle=vt)
            assert not zx.any() and not zr.any()
            tx, tr = _tangents(env, acts, r, dirs, state=state, vehicle=vt)
            tx2, tr2 = _tangents(env, acts, r, [2.0 * d for d in dirs], state=state, vehicle=vt)
            assert np.array_equal(tx2, 2.0 * tx) and np.array_equal(tr2, 2.0 * tr)
            assert np.abs(tx).max() > 0
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. composition
# ---------------------------------------------------------------------------------------------------------------------
def test_tangents_compose_over_a_split_horizon():
    """float64 storage, K = 6: the tangents of steps 4 .. 6 equal a second call from the explicit start x[2], status[2]
    with t_x0 = t_x[2], within 1e-9."""
    n, K, D = 256, 6, 3
    rng = np.random.default_rng(55)
    env = _env("lander3d", n, "float64", seed=6)
    try:
        table = _table(rng, n, False)
        vt = _dev(table, env)
        x, st = _random_point(n, rng)
        state = {"x": x, "status": st, "force": rng.uniform(-30, 30, (3, n))}
        acts = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env)
        dirs = _directions(rng, D, K, n, 4, table)
        r = env.rollout_states(acts, state=state, vehicle=vt)
        x2, s2 = r.x[2].t().contiguous().clone(), r.status[2].clone()
        tx, tr = _tangents(env, acts, r, dirs, state=state, vehicle=vt)
        mid = {"x": x2, "status": s2}
        r2 = env.rollout_states(acts[3:], state=mid, vehicle=vt)
        rest = (dirs[0][:, 3:], np.ascontiguousarray(tx[:, 2].transpose(0, 2, 1)), dirs[2], dirs[3])
        tx2, tr2 = _tangents(env, acts[3:], r2, rest, state=mid, vehicle=vt, use=(True, True, True, False))
        assert _scaled(tx2, tx[:, 3:]) <= 1e-9, _scaled(tx2, tx[:, 3:])
        assert _scaled(tr2, tr[:, 3:]) <= 1e-9, _scaled(tr2, tr[:, 3:])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. outputs
# ---------------------------------------------------------------------------------------------------------------------
def _abi_call(env, acts, r, state, **fields):
    """cs_jvp_rollout called directly with the given cs_jvp_io members (tensors or None); returns its status"""
    import torch
    import gym_copter_amd._lib as L
    io, _, keep = env._rollout_io(acts, state)
    io.x_dev, io.status_dev = r.x.data_ptr(), r.status.data_ptr()
    jio = L.JvpIO()
    jio.struct_size = C.sizeof(jio)
    for k, v in fields.items():
        setattr(jio, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    with torch.cuda.device(env.device):
        rc = env._lib.cs_jvp_rollout(env._ctx, C.byref(io), C.byref(jio), env._stream())
    torch.cuda.synchronize()
    return rc


def test_float32_outputs_and_null_outputs():
    import torch
    import gym_copter_amd._lib as L
    n, K, D = 65, 3, 3
    rng = np.random.default_rng(66)
    env = _env("lander3d", n, "float32", seed=7)
    try:
        table = _table(rng, n, False)
        env.set_vehicle_params(table)
        env.reset()
        acts = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env)
        r = env.rollout_states(acts)
        dirs = _directions(rng, D, K, n, 4, table)
        tx, tr = _tangents(env, acts, r, dirs)
        tx32, tr32 = _tangents(env, acts, r, dirs, dtype=torch.float32)
        assert tx32.dtype == np.float32 and tr32.dtype == np.float32
        assert np.array_equal(tx32, tx.astype(np.float32)) and np.array_equal(tr32, tr.astype(np.float32))
        # each output NULL in turn leaves the other unchanged; a NaN-filled buffer whose pointer is NULL stays NaN
        t = [_dev(d, env) for d in dirs]
        ins = dict(num_dirs=D, t_actions_dev=t[0], t_x0_dev=t[1], t_vehicle_dev=t[2], t_force_dev=t[3])
        for code, dt in ((L.JAC_F64, torch.float64), (L.JAC_F32, torch.float32)):
            ox = torch.full((D, K, n, 12), float("nan"), dtype=dt, device=env.device)
            orr = torch.full((D, K, n), float("nan"), dtype=dt, device=env.device)
            assert _abi_call(env, acts, r, None, out_dtype=code, t_x_dev=ox, t_reward_dev=None, **ins) == 0
            assert np.array_equal(to_np(ox), tx.astype(to_np(ox).dtype)) and bool(torch.isnan(orr).all())
            ox.fill_(float("nan"))
            assert _abi_call(env, acts, r, None, out_dtype=code, t_x_dev=None, t_reward_dev=orr, **ins) == 0
            assert np.array_equal(to_np(orr), tr.astype(to_np(orr).dtype)) and bool(torch.isnan(ox).all())
        assert _abi_call(env, acts, r, None, t_x_dev=None, t_reward_dev=None, **ins) == L.ERR_ARG
    finally:
        env.close()


@pytest.mark.parametrize("dtype", [None, "float32"])
def test_outputs_are_written_exactly(dtype):
    """With the guard of tests/guarded_outputs.py at N = 65: no byte outside [D,K,N,12] and [D,K,N] is written, every
    element inside is, and no input changes."""
    import torch
    n, K, D = 65, 3, 3
    rng = np.random.default_rng(67)
    env = _env("lander3d", n, "float64", seed=7)
    try:
        table = _table(rng, n, False)
        vt = _dev(table, env)
        x, st = _random_point(n, rng)
        state = {"x": _dev(x, env), "status": _dev(st, env), "force": _dev(rng.uniform(-30, 30, (3, n)), env)}
        acts = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env)
        t = [_dev(d, env) for d in _directions(rng, D, K, n, 4, table)]
        r = env.rollout_states(acts, state=state, vehicle=vt)
        with guarded(n) as g:
            g.freeze(acts=acts, tape_x=r.x, tape_status=r.status, vehicle=vt, t_a=t[0], t_x0=t[1], t_v=t[2], t_f=t[3],
                     **{"state_" + k: v for k, v in state.items()})
            out = env.rollout_jvp(acts, r, t_actions=t[0], t_x0=t[1], t_vehicle=t[2], t_force=t[3], state=state,
                                  vehicle=vt, dtype=None if dtype is None else getattr(torch, dtype))
            torch.cuda.synchronize()
            g.assert_bands_intact()
            g.assert_fully_written(out)
            g.assert_inputs_unchanged()
        assert len(g.allocations) == 2
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. purity, refusals and the wrapper's errors
# ---------------------------------------------------------------------------------------------------------------------
def test_nothing_of_the_env_is_written():
    import torch
    n, K, D = 512, 8, 3
    rng = np.random.default_rng(70)
    env, twin = (_env("lander3d", n, "float32", autoreset="next_step", seed=8, episode_stats=True) for _ in range(2))
    try:
        table = _table(rng, n, False)
        for e in (env, twin):
            e.set_vehicle_params(table)
            e.reset()
        for _ in range(30):
            a = _dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env)
            env.step(a)
            twin.step(a)
        acts = _dev(rng.uniform(-0.1, 1.1, (K, n, 4)).astype(np.float32), env)
        before = env.get_state()
        r = env.rollout_states(acts)
        _tangents(env, acts, r, _directions(rng, D, K, n, 4, table))
        other = _dev(_table(rng, n, False), env)
        r = env.rollout_states(acts, vehicle=other)
        _tangents(env, acts, r, _directions(rng, D, K, n, 4, table), vehicle=other)
        after, s2 = env.get_state(), twin.get_state()
        assert sorted(before) == sorted(after) == sorted(s2)
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
            assert np.array_equal(after[k], s2[k], equal_nan=True), k
        for k in range(K):
            o1, o2 = env.step(acts[k]), twin.step(acts[k])
            for u, v in zip(o1[:4], o2[:4]):
                assert torch.equal(u, v)
    finally:
        env.close()
        twin.close()


def test_refusals_and_wrapper_errors():
    import torch
    from gym_copter_amd import CopterStepError
    n, K = 128, 4
    rng = np.random.default_rng(71)
    env = _env("lander3d", n, "float64", seed=2)
    try:
        env.reset()
        acts = torch.full((K, n, 4), 0.6, dtype=torch.float32, device=env.device)
        r = env.rollout_states(acts)
        t_a = torch.ones((2, K, n, 4), dtype=torch.float64, device=env.device)
        t_v = torch.ones((2, 12, n), dtype=torch.float64, device=env.device)
        assert env.rollout_jvp(acts, r, t_actions=t_a).x.shape == (2, K, n, 12)
        assert env.rollout_jvp(acts, r, t_actions=t_a[0]).reward.shape == (K, n)
        with pytest.raises(ValueError, match="at least one"):
            env.rollout_jvp(acts, r)
        with pytest.raises(ValueError, match="direction axis"):
            env.rollout_jvp(acts, r, t_actions=t_a, t_vehicle=t_v[0])
        with pytest.raises(ValueError, match="share one D"):
            env.rollout_jvp(acts, r, t_actions=t_a, t_vehicle=torch.cat([t_v, t_v]))
        with pytest.raises(ValueError, match="shape"):
            env.rollout_jvp(acts, r, t_actions=t_a[:, :, :-1])
        with pytest.raises(ValueError, match="floating"):
            env.rollout_jvp(acts, r, t_vehicle=t_v.long())
        with pytest.raises(ValueError, match="dtype"):
            env.rollout_jvp(acts, r, t_actions=t_a, dtype=torch.int32)
        with pytest.raises(ValueError, match="rollout.x"):
            env.rollout_jvp(acts[:2], r, t_actions=t_a[:, :2])
        bad = _table(rng, n, False)
        bad[ROWS.index("M"), 3] = 0.0
        with pytest.raises(ValueError, match="positive"):
            env.rollout_jvp(acts, r, t_actions=t_a, vehicle=bad)
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_jvp(acts, r, t_actions=t_a)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    env = _env("lander3d", n, "float64", seed=2, action_arith="float32")
    try:
        env.reset()
        acts = torch.full((K, n, 4), 0.6, dtype=torch.float32, device=env.device)
        r = env.rollout_states(acts)
        t_a = torch.ones((2, K, n, 4), dtype=torch.float64, device=env.device)
        assert bool(env.rollout_jvp(acts, r, t_actions=t_a).x.any())     # the plain tangents: the float64 law's
        for kw in (dict(t_vehicle=torch.ones((2, 12, n), dtype=torch.float64, device=env.device)),
                   dict(t_force=torch.ones((2, 3, n), dtype=torch.float64, device=env.device))):
            with pytest.raises(CopterStepError, match="float32 motor model"):
                env.rollout_jvp(acts, r, **kw)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. torch.autograd.forward_ad
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_ad_through_differentiable_rollout():
    import torch
    import torch.autograd.forward_ad as fwAD
    from gym_copter_amd import differentiable_rollout
    n, K = 256, 6
    rng = np.random.default_rng(80)
    env = _env("lander3d", n, "float64", seed=1)
    try:
        table = _table(rng, n, False)
        x, st = _random_point(n, rng)
        f = rng.uniform(-30, 30, (3, n))
        a = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env)
        vt, ft, xt = _dev(table, env), _dev(f, env), _dev(x, env)
        t_a = _dev((0.05 * rng.standard_normal((K, n, 4))).astype(np.float32), env)
        t_v = _dev(0.1 * rng.standard_normal((12, n)) * table, env)
        t_f, t_x0 = _dev(10.0 * rng.standard_normal((3, n)), env), _dev(rng.standard_normal((12, n)), env)
        plain = {"x": xt, "status": _dev(st, env), "force": ft}
        r = env.rollout_states(a, state=plain, vehicle=vt)
        tape = type(r)(*(t.clone() for t in r))
        # duals on the actions alone, on the vehicle alone, and on all four inputs
        for use in ((True, False, False, False), (False, False, True, False), (True, True, True, True)):
            want = env.rollout_jvp(a, tape, t_actions=t_a.double() if use[0] else None, t_x0=t_x0 if use[1] else None,
                                   t_vehicle=t_v if use[2] else None, t_force=t_f if use[3] else None, state=plain,
                                   vehicle=vt)
            want_x, want_r = want.x.clone(), want.reward.clone()
            with fwAD.dual_level():
                state = {"x": fwAD.make_dual(xt, t_x0) if use[1] else xt, "status": plain["status"],
                         "force": fwAD.make_dual(ft, t_f) if use[3] else ft}
                out = differentiable_rollout(env, fwAD.make_dual(a, t_a) if use[0] else a, state=state,
                                             vehicle=fwAD.make_dual(vt, t_v) if use[2] else vt)
                px, tx = fwAD.unpack_dual(out.x)
                pr, trw = fwAD.unpack_dual(out.reward)
                assert fwAD.unpack_dual(out.status).tangent is None
                assert torch.equal(px, tape.x) and torch.equal(pr, tape.reward)
                assert torch.equal(tx, want_x) and torch.equal(trw, want_r), use
        # backward on the same function is unchanged: rollout_vjp_params'
        ag, vg, fg = a.clone().requires_grad_(True), vt.clone().requires_grad_(True), ft.clone().requires_grad_(True)
        w = _dev(rng.standard_normal((K, n, 12)), env)
        out = differentiable_rollout(env, ag, state={"x": xt, "status": plain["status"], "force": fg}, vehicle=vg)
        ((out.x * w).sum() + out.reward.sum()).backward()
        ga, _, gv, gf = env.rollout_vjp_params(a, tape, gx=w, gr=torch.ones((K, n), dtype=torch.float64,
                                                                            device=env.device), state=plain, vehicle=vt)
        assert torch.equal(ag.grad, ga.float()) and torch.equal(vg.grad, gv) and torch.equal(fg.grad, gf)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. sharded
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_passthrough():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n, K, D = 512, 8, 3
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, state_dtype="float64")
    try:
        sh.reset()
        loc = sh.local
        rng = np.random.default_rng(1)
        tab = _table(rng, sh.n_local, False)
        table = _dev(tab, loc)
        acts = _dev((hover_action() * rng.uniform(0.7, 1.3, (K, n, 4))).astype(np.float32), loc)
        t = [_dev(d, loc) for d in _directions(rng, D, K, sh.n_local, 4, tab)]
        kw = dict(t_actions=t[0], t_x0=t[1], t_vehicle=t[2], t_force=t[3], vehicle=table)
        r = sh.rollout_states(acts, vehicle=table)
        out = sh.rollout_jvp(acts, r, **kw)
        tx, tr = out.x.clone(), out.reward.clone()
        r2 = loc.rollout_states(acts[:, sh.local_slice()], vehicle=table)
        out2 = loc.rollout_jvp(acts[:, sh.local_slice()], r2, **kw)
        assert torch.equal(tx, out2.x) and torch.equal(tr, out2.reward) and bool(tx.any())
    finally:
        sh.close()
