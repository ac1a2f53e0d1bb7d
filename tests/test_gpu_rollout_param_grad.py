"""Rollouts as functions of the vehicle and of the start's pending force (cs_rollout_states_ex / cs_rollout_vjp_ex,
CopterVecEnv.rollout_states(vehicle=) / rollout_vjp_params, differentiable_rollout(vehicle=)): the parameter gradients
against central differences of the float64 oracle, bit-identity with the plain calls and with a twin env whose vehicle
is installed, no side effects, autograd, a system-identification application, float32 outputs, shape and dtype errors
and the sharded passthrough.  DESIGN.md section 11."""
import ctypes as C
import zlib

import numpy as np
import pytest

from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, DJI_PHANTOM, G, VehicleParams
from rollout_fd import oracle_rollout

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

ROWS = ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm", "G", "rho", "C_L")
MARS = dict(thrust_model="lift", rotor_gyro=True, vehicle_params={"C_L": 0.5}, world_params={"rho": 1.0})
TASK_A = {"lander3d": 4, "hover3d": 4}


def _env(task, n, mode="float64", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _mars_hover():
    w = DJI_PHANTOM.maxrpm * np.pi / 30
    kl = 0.5 * 1.0 * (0.05 * DJI_PHANTOM.L * 4) * 0.5 * (DJI_PHANTOM.L / 2) ** 2 * w * w
    return np.sqrt(G * DJI_PHANTOM.M / (4 * kl))


def _table(rng, n, mars):
    """a per-env [12, n] vehicle table around the DJI Phantom (the Mars air when `mars`)"""
    base = dict(B=5e-3, D=2e-6, M=1.38, L=0.35, Ix=2.0, Iy=2.0, Iz=3.0, Jr=38e-4, maxrpm=15000.0, G=G,
                rho=1.0 if mars else 1.225, C_L=0.5 if mars else 0.0)
    t = np.array([np.full(n, base[k]) for k in ROWS])
    for k, lo, hi in (("M", 0.8, 1.2), ("L", 0.9, 1.1), ("Ix", 0.8, 1.2), ("Iy", 0.8, 1.2), ("Iz", 0.8, 1.2),
                      ("maxrpm", 0.9, 1.1), ("D", 0.8, 1.2), ("B", 0.9, 1.1), ("Jr", 0.8, 1.2)):
        t[ROWS.index(k)] *= rng.uniform(lo, hi, n)
    return t


def _mag(p):
    return np.where(p != 0, np.abs(p), 1.0)


def fd_params(task, x, status, actions, table, force, gx, gr, prev_shaping=None, substeps=1, mars=False, h=1e-6):
    """Central differences of L = sum(gx X) + sum(gr R) over a K-step oracle rollout with respect to every row of the
    vehicle table (relative steps h |p|, h for a row that is 0) and the pending force (steps h x 10 N).  Returns
    (g_vehicle [12,n], g_force [3,n])."""
    n = x.shape[1]
    D = 12 + 3
    reps = 2 * D
    tab = np.tile(table, (1, reps))
    F = np.tile(force, (1, reps))
    for d in range(D):
        for s, sign in ((0, 1.0), (1, -1.0)):
            sl = slice((2 * d + s) * n, (2 * d + s + 1) * n)
            if d < 12:
                tab[d, sl] += sign * h * _mag(table[d])
            else:
                F[d - 12, sl] += sign * h * 10.0
    vp = VehicleParams(**{k: tab[ROWS.index(k)] for k in ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm")})
    g = tab[ROWS.index("G")]
    mp = (tab[ROWS.index("rho")], tab[ROWS.index("C_L")]) if mars else None
    pl = None if prev_shaping is None else np.tile(prev_shaping, reps)
    xs, rs, _, _, _ = oracle_rollout(task, np.tile(x, (1, reps)), np.tile(status, reps),
                                     np.tile(np.asarray(actions, np.float64), (1, reps, 1)), force=F, prev_shaping=pl,
                                     substeps=substeps, vp=vp, g=g, mars=mp)
    L = np.einsum("knj,knj->n", xs, np.tile(gx, (1, reps, 1))) + np.einsum("kn,kn->n", rs, np.tile(gr, (1, reps)))
    L = L.reshape(D, 2, n)
    hs = np.concatenate([h * _mag(table), np.full((3, n), h * 10.0)])
    grad = (L[:, 0] - L[:, 1]) / (2 * hs)
    return grad[:12], grad[12:]


def _scaled(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _random_point(n, rng):
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    x[1], x[3], x[5] = rng.uniform(-2, 2, (3, n))
    x[4] = rng.uniform(-20, -5, n)
    x[6], x[8] = rng.uniform(-0.4, 0.4, (2, n))
    x[10] = rng.uniform(-1, 1, n)
    x[7], x[9], x[11] = rng.uniform(-1, 1, (3, n))
    return x, np.full(n, AIRBORNE, np.uint8)


def _check_grads(gv, gf, table, want_v, want_f, mars, gyro):
    gv, gf = to_np(gv), to_np(gf)
    # the vehicle rows compared as d L / d log p (the rows span 1e-6 .. 1e4)
    assert _scaled(gv * table, want_v * table) <= 1e-6, ("g_vehicle", _scaled(gv * table, want_v * table))
    assert _scaled(gf, want_f) <= 1e-6, ("g_force", _scaled(gf, want_f))
    zero = ["B"] if mars else ["rho", "C_L"]
    if not gyro:
        zero.append("Jr")
    for k in zero:
        assert np.all(gv[ROWS.index(k)] == 0.0), k


# ---------------------------------------------------------------------------------------------------------------------
# 1. the parameter gradients against central differences of the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["explicit", "stored"])
@pytest.mark.parametrize("case", [("lander3d", 1, False), ("lander3d", 10, False), ("hover3d", 1, False),
                                  ("hover3d", 10, False), ("lander3d", 1, True), ("lander3d", 10, True),
                                  ("hover3d", 10, True)])
def test_parameter_gradient_matches_central_differences(case, start):
    task, substeps, mars = case
    n, K = 256, 8
    rng = np.random.default_rng(zlib.crc32(repr((case, start)).encode()))
    env = _env(task, n, "float64", substeps=substeps, seed=3, **(dict(MARS) if mars else {}))
    try:
        table = _table(rng, n, mars)
        ah = _mars_hover() if mars else hover_action()
        a = (ah * rng.uniform(0.6, 1.4, (K, n, TASK_A[task]))).astype(np.float32)
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
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
        acts = _dev(a, env)
        vt = _dev(table, env)
        r = env.rollout_states(acts, state=state, vehicle=vt)
        ga, g0, gv, gf = env.rollout_vjp_params(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state, vehicle=vt)
        want_v, want_f = fd_params(task, x, st, a, table, f, gx, gr, prev_shaping=prev, substeps=substeps, mars=mars)
        _check_grads(gv, gf, table, want_v, want_f, mars, gyro=mars)
    finally:
        env.close()


def test_parameter_gradient_of_the_env_vehicle_and_the_uniform_vehicle():
    """Without an override the gradient is taken at the env's own vehicle: its per-env table (set_vehicle_params), or
    cs_config's uniform vehicle."""
    n, K = 256, 8
    rng = np.random.default_rng(41)
    for per_env in (True, False):
        env = _env("lander3d", n, "float64", seed=1)
        try:
            table = _table(rng, n, False) if per_env else np.array(
                [np.full(n, v) for v in (5e-3, 2e-6, 1.38, 0.35, 2.0, 2.0, 3.0, 38e-4, 15000.0, G, env.config.rho,
                                         env.config.C_L)])
            if per_env:
                env.set_vehicle_params(table)
            x, st = _random_point(n, rng)
            f = rng.uniform(-30, 30, (3, n))
            state = {"x": x, "status": st, "force": f}
            a = (hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32)
            gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
            acts = _dev(a, env)
            r = env.rollout_states(acts, state=state)
            _, _, gv, gf = env.rollout_vjp_params(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state)
            want_v, want_f = fd_params("lander3d", x, st, a, table, f, gx, gr)
            _check_grads(gv, gf, table, want_v, want_f, False, False)
        finally:
            env.close()


@pytest.mark.parametrize("start", ["stored_consumed", "explicit_no_force", "explicit_zero_force"])
def test_force_gradient_where_no_force_is_pending(start):
    """No perturbation pending -- a stored start after one step() consumed its episode's, or an explicit start without
    state["force"] -- gives a force gradient of exactly 0 (and the vehicle gradient still matches the oracle).  A zero
    state["force"] is pending: its gradient is dL / dF at F = 0, against central differences."""
    n, K = 256, 8
    rng = np.random.default_rng(zlib.crc32(start.encode()))
    env = _env("lander3d", n, "float64", seed=5)
    try:
        table = _table(rng, n, False)
        env.set_vehicle_params(table)
        a = (hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32)
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        zero = np.zeros((3, n))
        if start == "stored_consumed":
            env.reset()
            env.step(_dev(np.full((n, 4), hover_action(), np.float32), env))
            s = env.get_state()
            assert not np.any(s["flags"] & 1)
            x, st, prev, state = s["x"], s["status"], s["prev_shaping"], None
        else:
            x, st = _random_point(n, rng)
            prev = None
            state = {"x": x, "status": st}
            if start == "explicit_zero_force":
                state["force"] = zero
        acts = _dev(a, env)
        r = env.rollout_states(acts, state=state)
        _, _, gv, gf = env.rollout_vjp_params(acts, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state)
        want_v, want_f = fd_params("lander3d", x, st, a, table, zero, gx, gr, prev_shaping=prev)
        gv, gf = to_np(gv), to_np(gf)
        assert _scaled(gv * table, want_v * table) <= 1e-6, _scaled(gv * table, want_v * table)
        if start == "explicit_zero_force":
            assert _scaled(gf, want_f) <= 1e-6, _scaled(gf, want_f)
            assert np.all(np.abs(gf).sum(axis=0) > 0)
        else:
            assert np.all(gf == 0.0)
    finally:
        env.close()


def test_next_step_reset_pending_at_the_start():
    """A next_step env with resets pending: those envs' force gradient is 0 (the new episode's draw is a constant) and
    their vehicle gradient is that of the K - 1 steps after the reset, from the reset state with the new draw pending
    (2 / M multiplies it) -- what stepping the env once shows."""
    n, K = 1024, 8
    rng = np.random.default_rng(17)
    env = _env("lander3d", n, "float64", autoreset="next_step", seed=11)
    try:
        table = _table(rng, n, False)
        env.set_vehicle_params(table)
        env.reset()
        pend = np.zeros(n, bool)
        for _ in range(300):
            _, _, term, trunc, _ = env.step(_dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env))
            pend = to_np(term | trunc).astype(bool)
            if pend.sum() >= 24:
                break
        assert pend.sum() >= 24
        a = (hover_action() * rng.uniform(0.8, 1.2, (K, n, 4))).astype(np.float32)
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        acts = _dev(a, env)
        r = env.rollout_states(acts)
        _, _, gv, gf = env.rollout_vjp_params(acts, r, gx=_dev(gx, env), gr=_dev(gr, env))
        gv, gf = to_np(gv).copy(), to_np(gf).copy()
        assert np.all(gf[:, pend] == 0.0)
        assert np.all(np.abs(gv[:, pend]).sum(axis=0) > 0)
        env.step(acts[0])                           # performs the resets: the state the later steps start from
        s = env.get_state()
        lanes = np.flatnonzero(pend)
        want_v, _ = fd_params("lander3d", s["x"][:, lanes], s["status"][lanes], a[1:, lanes], table[:, lanes],
                              s["force"][:, lanes], gx[1:, lanes], gr[1:, lanes], prev_shaping=s["prev_shaping"][lanes])
        tl = table[:, lanes]
        assert _scaled(gv[:, lanes] * tl, want_v * tl) <= 1e-6, _scaled(gv[:, lanes] * tl, want_v * tl)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. bit-identity
# ---------------------------------------------------------------------------------------------------------------------
def test_ex_with_null_pio_is_the_plain_call():
    import torch
    import gym_copter_amd._lib as L
    n, K = 1000, 20
    env = _env("lander3d", n, "float32", seed=4)
    try:
        env.reset()
        rng = np.random.default_rng(3)
        acts = _dev((hover_action() * rng.uniform(0.5, 1.5, (K, n, 4))).astype(np.float32), env)
        gx = _dev(rng.standard_normal((K, n, 12)), env)
        r = [t.clone() for t in env.rollout_states(acts)]
        ga, _ = env.rollout_vjp(acts, type(env.rollout_states(acts))(*r), gx=gx)
        ga = ga.clone()
        io, _, keep = env._rollout_io(acts, None)
        out = [torch.empty_like(t) for t in r]
        io.x_dev, io.reward_dev, io.terminated_dev, io.truncated_dev, io.status_dev = (t.data_ptr() for t in out)
        with torch.cuda.device(env.device):
            L.check(env._lib.cs_rollout_states_ex(env._ctx, C.byref(io), None, env._stream()))
        for a_, b_ in zip(out, r):
            assert torch.equal(a_, b_)
        io.gx_dev = gx.data_ptr()
        g2 = torch.empty_like(ga)
        io.g_actions_dev = g2.data_ptr()
        with torch.cuda.device(env.device):
            L.check(env._lib.cs_rollout_vjp_ex(env._ctx, C.byref(io), None, env._stream()))
        torch.cuda.synchronize()
        assert torch.equal(g2, ga)
    finally:
        env.close()


@pytest.mark.parametrize("mars", [False, True])
@pytest.mark.parametrize("substeps", [1, 10])
def test_override_is_bit_identical_to_an_installed_vehicle(substeps, mars):
    """the device fold equals the host fold: a rollout with vehicle= is a twin's after set_vehicle_params, bit for bit;
    the parameter backward's g_actions / g_x0 are rollout_vjp's"""
    import torch
    n, K = 1024, 24
    rng = np.random.default_rng(substeps + 7 * mars)
    kw = dict(MARS) if mars else {}
    env, twin = _env("lander3d", n, "float32", substeps=substeps, seed=2, **kw), \
        _env("lander3d", n, "float32", substeps=substeps, seed=2, **kw)
    try:
        table = _table(rng, n, mars)
        twin.set_vehicle_params(table)
        env.reset()
        twin.reset()
        ah = _mars_hover() if mars else hover_action()
        acts = _dev((ah * rng.uniform(0.3, 1.7, (K, n, 4))).astype(np.float32), env)
        vt = _dev(table, env)
        r = [t.clone() for t in env.rollout_states(acts, vehicle=vt)]
        rt = twin.rollout_states(acts)
        for a_, b_ in zip(r, rt):
            assert torch.equal(a_, b_)
        x, st = _random_point(n, rng)
        state = {"x": x, "status": st, "force": rng.uniform(-30, 30, (3, n))}
        gx, gr = _dev(rng.standard_normal((K, n, 12)), env), _dev(rng.standard_normal((K, n)), env)
        rt = twin.rollout_states(acts, state=state)
        ga, g0 = twin.rollout_vjp(acts, rt, gx=gx, gr=gr, state=state)
        ga, g0 = ga.clone(), g0.clone()
        ga2, g02, _, _ = twin.rollout_vjp_params(acts, rt, gx=gx, gr=gr, state=state)
        assert torch.equal(ga, ga2) and torch.equal(g0, g02)
        re = env.rollout_states(acts, state=state, vehicle=vt)
        ga3, g03, gv3, gf3 = env.rollout_vjp_params(acts, re, gx=gx, gr=gr, state=state, vehicle=vt)
        assert torch.equal(ga, ga3) and torch.equal(g0, g03)
        _, _, gv4, gf4 = twin.rollout_vjp_params(acts, rt, gx=gx, gr=gr, state=state)
        assert torch.equal(gv3, gv4) and torch.equal(gf3, gf4)
    finally:
        env.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. no side effects
# ---------------------------------------------------------------------------------------------------------------------
def test_override_has_no_side_effects():
    import torch
    n, K = 1024, 16
    rng = np.random.default_rng(5)
    env, twin = _env("lander3d", n, "float32", autoreset="next_step", seed=9), \
        _env("lander3d", n, "float32", autoreset="next_step", seed=9)
    try:
        own = _table(rng, n, False)
        env.set_vehicle_params(own)
        twin.set_vehicle_params(own)
        env.reset()
        twin.reset()
        acts = _dev((hover_action() * rng.uniform(0.5, 1.5, (K, n, 4))).astype(np.float32), env)
        before = env.get_state()
        base = [t.clone() for t in env.rollout_states(acts)]
        other = _dev(_table(rng, n, False), env)
        r = env.rollout_states(acts, vehicle=other)
        env.rollout_vjp_params(acts, r, gx=_dev(rng.standard_normal((K, n, 12)), env), vehicle=other)
        after = env.get_state()
        for k in before:
            assert np.array_equal(before[k], after[k], equal_nan=True), k
        again = env.rollout_states(acts)
        for a_, b_ in zip(base, again):
            assert torch.equal(a_, b_)
        for k in range(K):                          # the RNG position: the same resets and draws as the twin
            o1 = env.step(acts[k])
            o2 = twin.step(acts[k])
            assert torch.equal(o1[0], o2[0]) and torch.equal(o1[1], o2[1])
    finally:
        env.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. autograd
# ---------------------------------------------------------------------------------------------------------------------
def test_autograd_matches_rollout_vjp_params():
    import torch
    from gym_copter_amd import differentiable_rollout
    n, K = 512, 12
    rng = np.random.default_rng(8)
    env = _env("lander3d", n, "float64", seed=1)
    try:
        table = _table(rng, n, False)
        x, st = _random_point(n, rng)
        f = rng.uniform(-30, 30, (3, n))
        a = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env).requires_grad_(True)
        vt = _dev(table, env).requires_grad_(True)
        ft = _dev(f, env).requires_grad_(True)
        state = {"x": _dev(x, env), "status": _dev(st, env), "force": ft}
        w = _dev(rng.standard_normal((K, n, 12)), env)
        out = differentiable_rollout(env, a, state=state, vehicle=vt)
        loss = (out.x * w).sum() + out.reward.sum()
        loss.backward()
        plain = {"x": x, "status": st, "force": f}
        r = env.rollout_states(a.detach(), state=plain, vehicle=vt.detach())
        ga, _, gv, gf = env.rollout_vjp_params(a.detach(), r, gx=w, gr=torch.ones((K, n), dtype=torch.float64,
                                                                                    device=env.device),
                                               state=plain, vehicle=vt.detach())
        assert torch.equal(a.grad, ga.float())
        assert torch.equal(vt.grad, gv) and torch.equal(ft.grad, gf)
        # neither a vehicle nor a force that requires grad: today's path, no parameter gradient asked for
        a.grad = None
        out = differentiable_rollout(env, a, state={"x": _dev(x, env), "status": _dev(st, env)})
        (out.x * w).sum().backward()
        assert a.grad is not None
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. application: system identification
# ---------------------------------------------------------------------------------------------------------------------
def test_system_identification_of_mass_and_inertias():
    """4 096 Lander3D envs with hidden per-env M, Ix, Iy (+-20 % around the DJI Phantom; the other rows known) fly
    K = 50 steps of exciting open-loop actions.  Gradient descent (Adam on the log parameters) on the trajectory error
    through differentiable_rollout(vehicle=) brings the median relative error of each parameter from ~10 % under 1 %."""
    import torch
    from gym_copter_amd import differentiable_rollout
    n, K = 4096, 50
    rng = np.random.default_rng(2024)
    env = _env("lander3d", n, "float64", seed=3)
    try:
        nominal = np.array([np.full(n, v) for v in (5e-3, 2e-6, 1.38, 0.35, 2.0, 2.0, 3.0, 38e-4, 15000.0, G,
                                                    env.config.rho, env.config.C_L)])
        idx = [ROWS.index("M"), ROWS.index("Ix"), ROWS.index("Iy")]
        hidden = nominal.copy()
        hidden[idx] *= rng.uniform(0.8, 1.2, (3, n))
        x0 = np.zeros((12, n))
        x0[4] = -30.0
        state = {"x": _dev(x0, env), "status": _dev(np.full(n, AIRBORNE, np.uint8), env)}
        acts = _dev((hover_action() * (1.0 + 0.15 * rng.standard_normal((K, n, 4)))).astype(np.float32), env)
        with torch.no_grad():
            obs = env.rollout_states(acts, state=state, vehicle=_dev(hidden, env)).x.clone()
        base = _dev(nominal, env)
        logp = torch.zeros((3, n), dtype=torch.float64, device=env.device, requires_grad=True)
        opt = torch.optim.Adam([logp], lr=0.02)
        iters = 300
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, iters, eta_min=2e-4)
        scale = obs.abs().amax(dim=0, keepdim=True).clamp_min(1e-3)      # per env and state slot
        err0 = np.median(np.abs(nominal[idx] / hidden[idx] - 1.0), axis=1)
        for _ in range(iters):
            opt.zero_grad()
            veh = base.clone()
            veh[idx] = base[idx] * torch.exp(logp)
            out = differentiable_rollout(env, acts, state=state, vehicle=veh)
            loss = (((out.x - obs) / scale) ** 2).sum()
            loss.backward()
            opt.step()
            sched.step()
        fit = nominal[idx] * np.exp(to_np(logp.detach()))
        err = np.median(np.abs(fit / hidden[idx] - 1.0), axis=1)
        assert np.all(err0 > 0.05), err0
        assert np.all(err < 0.01), (err0, err)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. float32 outputs, errors, sharded
# ---------------------------------------------------------------------------------------------------------------------
def test_float32_outputs_are_the_float64_values_rounded():
    import torch
    n, K = 512, 8
    rng = np.random.default_rng(12)
    env = _env("hover3d", n, "float64", seed=2)
    try:
        x, st = _random_point(n, rng)
        state = {"x": x, "status": st, "force": rng.uniform(-30, 30, (3, n))}
        acts = _dev((hover_action() * rng.uniform(0.6, 1.4, (K, n, 4))).astype(np.float32), env)
        gx = _dev(rng.standard_normal((K, n, 12)), env)
        r = env.rollout_states(acts, state=state)
        _, _, gv, gf = env.rollout_vjp_params(acts, r, gx=gx, state=state)
        gv, gf = gv.clone(), gf.clone()
        _, _, gv32, gf32 = env.rollout_vjp_params(acts, r, gx=gx, state=state, dtype=torch.float32)
        assert gv32.dtype == torch.float32 and gf32.dtype == torch.float32
        assert torch.equal(gv32, gv.float()) and torch.equal(gf32, gf.float())
    finally:
        env.close()


def test_shape_dtype_and_configuration_errors():
    import torch
    import gym_copter_amd._lib as L
    n, K = 256, 4
    env = _env("lander3d", n, "float64", seed=2)
    try:
        env.reset()
        acts = torch.full((K, n, 4), 0.6, dtype=torch.float32, device=env.device)
        good = _table(np.random.default_rng(0), n, False)
        with pytest.raises(ValueError, match="shape"):
            env.rollout_states(acts, vehicle=good[:, :-1])
        with pytest.raises(ValueError, match="shape"):
            env.rollout_states(acts, vehicle=good[:10])
        for row, v in (("M", 0.0), ("Ix", -1.0), ("G", np.nan), ("maxrpm", np.inf)):
            bad = good.copy()
            bad[ROWS.index(row), 3] = v
            with pytest.raises(ValueError, match="positive"):
                env.rollout_states(acts, vehicle=bad)
        r = env.rollout_states(acts)
        with pytest.raises(ValueError, match="dtype"):
            env.rollout_vjp_params(acts, r, dtype=torch.int32)
        io, _, keep = env._rollout_io(acts, None)
        io.x_dev, io.status_dev = r.x.data_ptr(), r.status.data_ptr()
        pio = L.RolloutParamIO()
        pio.struct_size = C.sizeof(L.RolloutParamIO) + 8
        assert env._lib.cs_rollout_vjp_ex(env._ctx, C.byref(io), C.byref(pio), env._stream()) == L.ERR_ABI
        pio.struct_size = C.sizeof(L.RolloutParamIO)
        pio.out_dtype = 7
        assert env._lib.cs_rollout_states_ex(env._ctx, C.byref(io), C.byref(pio), env._stream()) == L.ERR_ARG
        from gym_copter_amd import differentiable_rollout
        with pytest.raises(ValueError, match="float64"):
            differentiable_rollout(env, acts, vehicle=_dev(good, env, torch.float32))
    finally:
        env.close()
    env = _env("lander3d", n, "float64", seed=2, action_arith="float32")
    try:
        acts = torch.full((K, n, 4), 0.6, dtype=torch.float32, device=env.device)
        r = env.rollout_states(acts)
        with pytest.raises(Exception, match="float32 motor model"):
            env.rollout_vjp_params(acts, r)
    finally:
        env.close()


def test_sharded_passthrough():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n, K = 512, 8
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, state_dtype="float64")
    try:
        sh.reset()
        loc = sh.local
        rng = np.random.default_rng(1)
        table = _dev(_table(rng, sh.n_local, False), loc)
        acts = _dev((hover_action() * rng.uniform(0.7, 1.3, (K, n, 4))).astype(np.float32), loc)
        gx = _dev(rng.standard_normal((K, sh.n_local, 12)), loc)
        r = sh.rollout_states(acts, vehicle=table)
        _, _, gv, gf = sh.rollout_vjp_params(acts, r, gx=gx, vehicle=table)
        gv, gf = gv.clone(), gf.clone()
        r2 = loc.rollout_states(acts[:, sh.local_slice()], vehicle=table)
        _, _, gv2, gf2 = loc.rollout_vjp_params(acts[:, sh.local_slice()], r2, gx=gx, vehicle=table)
        assert torch.equal(gv, gv2) and torch.equal(gf, gf2)
    finally:
        sh.close()
