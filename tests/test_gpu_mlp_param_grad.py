"""The policy-parameter gradient on the device and the cotangent on the action tape (cs_mlp_param_grad,
cs_rollout_mlp_vjp_ex; CopterVecEnv.mlp_param_grad, rollout_mlp_vjp(g_actions_in=, reduce=),
differentiable_mlp_rollout(action_grad=, reduce=)): the device reduction against gym_copter_amd.mlp.param_grad within a
derived summation bound, bit-for-bit determinism, no cotangent = the plain backward, the cotangent against chained
step Jacobians and against central differences of the float64 oracle (tests/mlp_action_fd.py), a resetting lane,
autograd, policy training with an effort penalty, offsets past 4 GiB, the sharded passthrough and errors.  The cotangent
chain and the plain-backward identity also run under the rotor-gyro models of tests/model_variants.py."""
import zlib

import numpy as np
import pytest

import model_variants
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from mlp_action_fd import fd_mlp_action_vjp
from mlp_rollout_fd import OBS_SHAPE
from oracle.refcpu import AIRBORNE, LANDED
from rollout_fd import shaping_grad

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover1d": 1, "lander1d": 1, "hover2d": 2}
U64 = 2.0 ** -53


def _env(task, n, mode="float64", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _theta(task, hidden, seed, scale=0.1, env=None, bias=None):
    """A policy near hover: the output bias is the hover motor value (`bias`: that of a model variant), the output
    weights small."""
    import torch
    from gym_copter_amd import mlp
    p = mlp.init(OBS_SHAPE[task][1], TASK_A[task], hidden, generator=torch.Generator().manual_seed(seed),
                 out_bias=hover_action() if bias is None else bias, out_scale=scale)
    return p if env is None else p.to(env.device)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _scaled(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def _point(n, rng):
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[1], x[3], x[5] = rng.uniform(-1, 1, (3, n))
    x[4] = rng.uniform(-15, -8, n)
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    x[10] = rng.uniform(-0.5, 0.5, n)
    x[7], x[9], x[11] = rng.uniform(-0.5, 0.5, (3, n))
    return x, np.full(n, AIRBORNE, np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the device reduction equals mlp.param_grad within the bound of two float64 summations
# ---------------------------------------------------------------------------------------------------------------------
def _term_magnitudes(params, hidden, obs, ga, chunk_rows=1 << 22):
    """T [P] float64 (torch, on params' device): per parameter the sum over the rows of a bound of |term| --
    (|g_a| |W2|)_j |o_i| for the first layer, |g_a[c]| |h_j| for the second, |g_a[c]| |o_i| for hidden = 0 (|o| = 1,
    |h| = 1 for the biases)."""
    import torch
    from gym_copter_amd import mlp
    K, N, OBS = obs.shape
    A = ga.shape[2]
    p = mlp.unpack(params.detach().double(), OBS, A, hidden)
    step = max(1, chunk_rows // N)
    T = torch.zeros(params.shape[0], dtype=torch.float64, device=params.device)
    for k0 in range(0, K, step):
        o = obs[k0:k0 + step].double().reshape(-1, OBS)
        g = ga[k0:k0 + step].double().reshape(-1, A).abs()
        ao = o.abs()
        if hidden == 0:
            T += torch.cat([(g.T @ ao).reshape(-1), g.sum(0)])
            continue
        h = torch.tanh(o @ p["W1"].T + p["b1"]).abs()
        gh = g @ p["W2"].abs()
        T += torch.cat([(gh.T @ ao).reshape(-1), gh.sum(0), (g.T @ h).reshape(-1), g.sum(0)])
    return T


def _bound_ratio(dev, ref, T, R):
    """max over the parameters of |device - torch| / ((2 R + 64) 2^-53 T): any two float64 summations of R terms differ
    by at most 2 (R - 1) u sum|t|, and the per-term differences (the device's tanh against torch's, the fma chains) are
    a few u of the term's bound."""
    import torch
    bound = (2 * R + 64) * U64 * T
    diff = (dev - ref).abs()
    assert bool(torch.isfinite(dev).all())
    assert bool(((bound > 0) | (diff == 0)).all())
    return float((diff / bound.clamp_min(1e-300)).max())


# task, hidden, envs, K, dtype of g_actions: every task shape, every width with Lander3D (3 and 33 leave idle lanes),
# a ragged last tile (1 000) and whole ones (65 536), K = 1 and 24, float64 and float32 g_actions
REDUCTION_CASES = [("lander3d", 0, 1000, 24, "float64"), ("lander3d", 1, 1000, 1, "float32"),
                   ("lander3d", 3, 65536, 1, "float64"), ("lander3d", 16, 1000, 24, "float32"),
                   ("lander3d", 33, 1000, 24, "float64"), ("lander3d", 64, 65536, 24, "float64"),
                   ("hover3d", 16, 1000, 24, "float64"), ("hover3d", 0, 65536, 1, "float32"),
                   ("lander2d", 33, 1000, 24, "float32"), ("lander2d", 0, 1000, 1, "float64"),
                   ("hover1d", 64, 1000, 24, "float32"), ("hover1d", 0, 1000, 24, "float64"),
                   ("hover1d", 3, 65536, 1, "float64")]


@pytest.mark.parametrize("task,hidden,n,K,dtype", REDUCTION_CASES)
def test_device_reduction_equals_param_grad_within_the_summation_bound(task, hidden, n, K, dtype):
    """A real tape (rollout_mlp_states / rollout_mlp_vjp from airborne explicit starts -- every env's motors act --,
    random cotangents): per parameter |device - torch| <= (2 R + 64) 2^-53 T.  Measured worst ratio over the cases:
    3.6e-4."""
    import torch
    from gym_copter_amd import mlp
    env = _env(task, n, "float32", seed=3)
    try:
        env.reset()
        gen = torch.Generator(device=env.device).manual_seed(hidden * 131 + K)
        x, st = _point(n, np.random.default_rng(hidden + K))
        state = {"x": x.astype(np.float32).astype(np.float64), "status": st}
        p = _theta(task, hidden, 2 + hidden, scale=0.003 if hidden else 0.0005, env=env)   # (few actions clip)
        r = env.rollout_mlp_states(p, K, hidden, state=state)
        gx = torch.randn((K, n, 12), dtype=torch.float64, device=env.device, generator=gen)
        gr = torch.randn((K, n), dtype=torch.float64, device=env.device, generator=gen)
        _, ga, _ = env.rollout_mlp_vjp(p, r, gx=gx, gr=gr, state=state, hidden=hidden, dtype=getattr(torch, dtype),
                                       param_grad=False)
        assert float((ga != 0).double().mean()) > 0.5           # (a tape whose rows count)
        assert ga.dtype == getattr(torch, dtype)
        dev = env.mlp_param_grad(p, hidden, r.obs, ga)
        ref = mlp.param_grad(p, hidden, r.obs, ga)
        assert dev.shape == ref.shape and dev.dtype == torch.float64 and dev.device == env.device
        assert float(ref.abs().max()) > 0
        ratio = _bound_ratio(dev, ref, _term_magnitudes(p, hidden, r.obs, ga), K * n)
        print("device reduction %s H=%d N=%d K=%d %s: %.3g of the bound" % (task, hidden, n, K, dtype, ratio))
        assert ratio <= 1.0, ratio
    finally:
        env.close()


def test_device_reduction_with_saturated_units():
    """Random g_actions and a policy scaled up so that some hidden units saturate (|h| > 0.999): 1 - h^2 cancels."""
    import torch
    from gym_copter_amd import mlp
    task, hidden, n, K = "lander3d", 32, 4096, 8
    env = _env(task, n, "float32", seed=5)
    try:
        env.reset()
        gen = torch.Generator(device=env.device).manual_seed(77)
        r = env.rollout_mlp_states(_theta(task, hidden, 1, env=env), K, hidden)
        p = _theta(task, hidden, 9, scale=1.0, env=env) * 6.0
        h = torch.tanh(r.obs.double().reshape(-1, 10) @ mlp.unpack(p.double(), 10, 4, hidden)["W1"].T
                       + mlp.unpack(p.double(), 10, 4, hidden)["b1"])
        assert bool((h.abs() > 0.999).any()) and bool((h.abs() < 0.5).any())
        ga = torch.randn((K, n, 4), dtype=torch.float64, device=env.device, generator=gen)
        dev = env.mlp_param_grad(p, hidden, r.obs, ga)
        ref = mlp.param_grad(p, hidden, r.obs, ga)
        ratio = _bound_ratio(dev, ref, _term_magnitudes(p, hidden, r.obs, ga), K * n)
        print("device reduction, saturated units: %.3g of the bound" % ratio)
        assert ratio <= 1.0, ratio
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. deterministic, and written rather than accumulated
# ---------------------------------------------------------------------------------------------------------------------
def test_device_reduction_is_deterministic_and_overwrites():
    import torch
    from gym_copter_amd import mlp
    task, n = "lander3d", 5000
    env = _env(task, n, "float32", seed=8)
    try:
        env.reset()
        gen = torch.Generator(device=env.device).manual_seed(4)

        def tape(K, hidden):
            p = _theta(task, hidden, 3, scale=0.3, env=env)
            obs = env.rollout_mlp_states(p, K, hidden).obs.clone()
            return p, obs, torch.randn((K, n, 4), dtype=torch.float64, device=env.device, generator=gen)
        p, obs, ga = tape(12, 33)
        first = env.mlp_param_grad(p, 33, obs, ga)
        again = env.mlp_param_grad(p, 33, obs, ga)
        assert torch.equal(first, again)
        out = torch.full((mlp.num_params(10, 4, 33),), float("nan"), dtype=torch.float64, device=env.device)
        got = env.mlp_param_grad(p, 33, obs, ga, out=out)
        assert got is out and torch.equal(out, first)
        p2, obs2, ga2 = tape(5, 64)                             # (another K and H: the scratch is reused)
        other = env.mlp_param_grad(p2, 64, obs2, ga2)
        assert torch.equal(env.mlp_param_grad(p, 33, obs, ga), first)
        assert torch.equal(env.mlp_param_grad(p2, 64, obs2, ga2), other)
        p0, obs0, ga0 = tape(3, 0)
        lin = env.mlp_param_grad(p0, 0, obs0, ga0)
        assert torch.equal(env.mlp_param_grad(p, 33, obs, ga), first)
        assert torch.equal(env.mlp_param_grad(p0, 0, obs0, ga0), lin)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. no cotangent gives the plain backward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,hidden,variant", [
    pytest.param("lander3d", 0, None, id="lander3d-0"), pytest.param("lander3d", 32, None, id="lander3d-32"),
    pytest.param("hover3d", 16, None, id="hover3d-16"), ("lander3d", 32, "gyro_only")])
def test_no_cotangent_is_the_plain_backward(task, hidden, variant):
    """cs_rollout_mlp_vjp_ex with no block, with a block whose cotangent is NULL, and with an all-zero cotangent, all
    against cs_rollout_mlp_vjp itself.  Under gyro_only the two sides are the rotor-gyro backward kernel with and
    without the cotangent."""
    import ctypes as C
    import torch
    from gym_copter_amd import _lib
    n, K, A = 3000, 12, 4
    rng = np.random.default_rng(hidden)
    env = _env(task, n, "float32", seed=6, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        x, st = _point(n, rng)
        state = {"x": x.astype(np.float32).astype(np.float64), "status": st}
        p = _theta(task, hidden, 4, scale=0.3, env=env, bias=model_variants.hover(variant))
        gx, gr = _dev(rng.standard_normal((K, n, 12)), env), _dev(rng.standard_normal((K, n)), env)
        r = env.rollout_mlp_states(p, K, hidden, state=state)
        r = type(r)(*(t.clone() for t in r))
        if variant is not None:
            model_variants.assert_differs_from_default(variant, r.x, task, "float32", 1, state, r.actions)
        # the plain entry point, called as the parent's rollout_mlp_vjp called it
        io, _, keep = env._rollout_io(None, state, K)
        mio, _ = env._mlp_io(p, hidden, K, None, keep)
        io.out_dtype = _lib.JAC_F64
        io.x_dev, io.status_dev, mio.actions_out_dev = r.x.data_ptr(), r.status.data_ptr(), r.actions.data_ptr()
        io.gx_dev, io.gr_dev = gx.data_ptr(), gr.data_ptr()
        wa = torch.full((K, n, A), float("nan"), dtype=torch.float64, device=env.device)
        w0 = torch.full((12, n), float("nan"), dtype=torch.float64, device=env.device)
        io.g_actions_dev, io.g_x0_dev = wa.data_ptr(), w0.data_ptr()
        with torch.cuda.device(env.device):
            _lib.check(env._lib.cs_rollout_mlp_vjp(env._ctx, C.byref(io), C.byref(mio), env._stream()))
            # ... and the new one with a block whose cotangent is NULL
            xa, x0 = torch.full_like(wa, float("nan")), torch.full_like(w0, float("nan"))
            io.g_actions_dev, io.g_x0_dev = xa.data_ptr(), x0.data_ptr()
            xio = _lib.RolloutMlpExIO()
            xio.struct_size = C.sizeof(xio)
            _lib.check(env._lib.cs_rollout_mlp_vjp_ex(env._ctx, C.byref(io), C.byref(mio), C.byref(xio), env._stream()))
        assert bool(torch.isfinite(wa).all()) and float(wa.abs().max()) > 0
        assert torch.equal(xa, wa) and torch.equal(x0, w0)
        _, ga, g0 = env.rollout_mlp_vjp(p, r, gx=gx, gr=gr, state=state, hidden=hidden, g_actions_in=None)
        assert torch.equal(ga, wa) and torch.equal(g0, w0)
        zero = torch.zeros((K, n, A), dtype=torch.float64, device=env.device)
        _, ga, g0 = env.rollout_mlp_vjp(p, r, gx=gx, gr=gr, state=state, hidden=hidden, g_actions_in=zero)
        assert torch.equal(ga, wa) and torch.equal(g0, w0)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the cotangent against chained step_jacobian + a float64 policy Jacobian on the kernel's own tape
# ---------------------------------------------------------------------------------------------------------------------
def _policy_jac(theta, hidden, obs, A):
    """J_o pi at obs [n, OBS] in float64: [n, A, OBS]"""
    import torch
    from gym_copter_amd import mlp
    p = {k: v.double().numpy() for k, v in mlp.unpack(torch.as_tensor(theta).cpu(), obs.shape[-1], A, hidden).items()}
    o = obs.astype(np.float64)
    if hidden == 0:
        return np.broadcast_to(p["W"], (o.shape[0],) + p["W"].shape)
    h = np.tanh(o @ p["W1"].T + p["b1"])
    return np.einsum("ch,nh,hj->ncj", p["W2"], 1 - h * h, p["W1"])


SPREAD_INERTIA = ("vehicles", "vehicles_mars_gyro")    # motors near hover there: see tests/test_gpu_rollout_mlp.py


@pytest.mark.parametrize("task,hidden,variant", [
    pytest.param("lander3d", 0, None, id="lander3d-0"), pytest.param("lander3d", 32, None, id="lander3d-32"),
    pytest.param("hover3d", 16, None, id="hover3d-16"), ("lander3d", 32, "mars_gyro"), ("hover3d", 0, "vehicles_mars_gyro")])
def test_cotangent_equals_chained_step_jacobians_and_policy_jacobian(task, hidden, variant):
    """The construction of test_gradient_equals_chained_step_jacobians_and_policy_jacobian (test_gpu_rollout_mlp: 2 048
    envs, K = 24, LANDED lanes, clipped actions, an explicit start) with want[k] += gact[k]: g_u, g_x0 and g_theta (the
    device reduction) within 1e-9 scaled.  Under a model variant (600 envs, as there) this is the rotor-gyro backward
    kernel with a cotangent, and the x tape differs from the default model's on the same action tape."""
    import torch
    from gym_copter_amd import mlp
    n, K, A = 2048 if variant is None else 600, 24, 4
    first, od = OBS_SHAPE[task]
    rng = np.random.default_rng(31 + hidden if variant is None else zlib.crc32(repr((task, hidden, variant)).encode()))
    env = _env(task, n, "float32", seed=4, **model_variants.env_kwargs(variant))
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        x, st = _point(n, rng)
        x = x.astype(np.float32).astype(np.float64)
        q = n // 8
        x[4, :q], x[5, :q], st[:q] = 0.0, 0.0, LANDED
        u = np.zeros((K, n, A), np.float32)
        u[:, q:2 * q] = rng.uniform(-0.8, 0.8, (K, q, A))                     # some clipped
        scale = 0.3
        if variant in SPREAD_INERTIA:
            ah = model_variants.hover(variant)
            u[:, q:2 * q] = ah * rng.uniform(-2.0, 2.0, (K, q, A))            # some clipped, at 0 only
            scale = (0.003 if hidden else 0.0015) * ah / hover_action()
        state = {"x": x, "status": st}
        p = _theta(task, hidden, 5, scale=scale, env=env, bias=model_variants.hover(variant))
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        gact = rng.standard_normal((K, n, A))
        r = env.rollout_mlp_states(p, K, hidden, offsets=_dev(u, env), state=state)
        r = type(r)(*(t.clone() for t in r))
        if variant is not None:
            model_variants.assert_differs_from_default(variant, r.x, task, "float32", 1, state, r.actions)
        gp, ga, g0 = env.rollout_mlp_vjp(p, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state, hidden=hidden,
                                         g_actions_in=_dev(gact, env), reduce="device")
        gp, ga, g0 = to_np(gp).copy(), to_np(ga).copy(), to_np(g0).copy()
        tape_x, tape_s, obs = to_np(r.x).copy(), to_np(r.status).copy(), to_np(r.obs).copy()
        acts = r.actions
        assert (tape_s == LANDED).any() and (to_np(acts) < 0).any()
        lam = np.zeros((n, 12))
        want = np.zeros((K, n, A))
        max_angle = np.radians(45)
        for k in range(K - 1, -1, -1):
            lam += gx[k]
            if k == 0:
                jac = env.step_jacobian(acts[0], state={"x": x, "status": st})
            else:
                jac = env.step_jacobian(acts[k], state={"x": tape_x[k - 1].T.copy(), "status": tape_s[k - 1]})
            dx, du, rdx, rdu = (to_np(t).astype(np.float64) for t in jac[:4])
            want[k] = np.einsum("nij,ni->nj", du, lam) + gr[k][:, None] * rdu
            want[k] += gact[k]                                                 # (on a_k, before the clip: no mask)
            new = np.einsum("nij,ni->nj", dx, lam) + gr[k][:, None] * rdx
            xprev = x.T if k == 0 else tape_x[k - 1]
            xk = tape_x[k]
            tilt = ~((np.abs(xk[:, 0]) >= 10) | (np.abs(xk[:, 2]) >= 10)) & \
                ((np.abs(xk[:, 6]) >= max_angle) | (np.abs(xk[:, 8]) >= max_angle))
            if task.startswith("lander"):                                        # (the explicit start's shaping(x0))
                new -= (gr[k] * ~tilt)[:, None] * shaping_grad(xprev.T).T
            new[:, first:first + od] += np.einsum("ncj,nc->nj", _policy_jac(p.cpu(), hidden, obs[k], A), want[k])
            lam = new
        wp = mlp.param_grad(p.cpu(), hidden, torch.from_numpy(obs), torch.from_numpy(want)).numpy()
        errs = (_scaled(ga, want), _scaled(g0, lam.T), float(np.max(np.abs(gp - wp) / np.maximum(1.0, np.abs(wp)))))
        print("chained Jacobians with a cotangent %s H=%d%s: g_u %.2e g_x0 %.2e g_theta %.2e"
              % ((task, hidden, " " + variant if variant else "") + errs))
        assert max(errs) <= 1e-9, errs
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the cotangent against central differences of the float64 closed-loop oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,hidden,substeps", [("lander3d", 8, 1), ("hover3d", 0, 1), ("lander2d", 4, 10),
                                                  ("hover1d", 3, 1)])
def test_cotangent_matches_central_differences(task, hidden, substeps):
    """The set-up of test_gradient_matches_central_differences (test_gpu_rollout_mlp: float64 storage, K = 8, n = 48,
    feedback of ~10 % of hover) against tests/mlp_action_fd.py with gact standard normal: g_theta (the device
    reduction), g_u and g_x0 within that test's 1e-5 scaled."""
    n, K, A = 48, 8, TASK_A[task]
    rng = np.random.default_rng(7)
    env = _env(task, n, "float64", substeps=substeps)
    try:
        x, st = _point(n, rng)
        u = (hover_action() * rng.uniform(-0.2, 0.2, (K, n, A))).astype(np.float32)
        p = _theta(task, hidden, 9, scale=0.001 if hidden else 0.0005, env=env)   # feedback of ~10 % of hover
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        gact = rng.standard_normal((K, n, A))
        state = {"x": x, "status": st}
        r = env.rollout_mlp_states(p, K, hidden, offsets=_dev(u, env), state=state)
        gp, ga, g0 = env.rollout_mlp_vjp(p, r, gx=_dev(gx, env), gr=_dev(gr, env), state=state, hidden=hidden,
                                         g_actions_in=_dev(gact, env), reduce="device")
        wp, wu, w0 = fd_mlp_action_vjp(task, x, st, p.cpu().double().numpy(), hidden, K, offsets=u.astype(np.float64),
                                       gx=gx, gr=gr, gact=gact, substeps=substeps)
        errs = (_scaled(to_np(gp), wp), _scaled(to_np(ga), wu), _scaled(to_np(g0), w0))
        print("central differences with a cotangent %s H=%d substeps=%d: g_theta %.2e g_u %.2e g_x0 %.2e"
              % ((task, hidden, substeps) + errs))
        assert max(errs) <= 1e-5, errs
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. a lane that resets in step 1
# ---------------------------------------------------------------------------------------------------------------------
def test_resetting_lane_returns_the_cotangent_itself():
    """The set-up of test_primal_from_pending_next_step_resets (test_gpu_rollout_mlp): on the lanes with a NEXT_STEP
    reset pending at the stored start, g_actions[0] is g_actions_in[0] bit for bit, and everything is finite."""
    import torch
    n, K, hidden = 2048, 20, 32
    env = _env("lander3d", n, "float32", autoreset="next_step", seed=11)
    try:
        env.reset()
        rng = np.random.default_rng(12)
        pend = np.zeros(n, bool)
        for _ in range(200):
            _, _, term, trunc, _ = env.step(_dev(rng.uniform(0, 1, (n, 4)).astype(np.float32), env))
            pend = to_np(term | trunc).astype(bool)
            if pend.sum() >= 32:
                break
        assert pend.sum() >= 32
        p = _theta("lander3d", hidden, 3, env=env)
        r = env.rollout_mlp_states(p, K, hidden)
        gx, gr = _dev(rng.standard_normal((K, n, 12)), env), _dev(rng.standard_normal((K, n)), env)
        gact = _dev(rng.standard_normal((K, n, 4)), env)
        gp, ga, g0 = env.rollout_mlp_vjp(p, r, gx=gx, gr=gr, hidden=hidden, g_actions_in=gact, reduce="device")
        assert g0 is None
        lanes = torch.from_numpy(np.flatnonzero(pend)).to(env.device)
        assert torch.equal(ga[0, lanes], gact[0, lanes])
        assert not torch.equal(ga[0], gact[0]) and not torch.equal(ga[1, lanes], gact[1, lanes])
        assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gp).all())
        _, plain, _ = env.rollout_mlp_vjp(p, r, gx=gx, gr=gr, hidden=hidden, param_grad=False)
        assert bool((plain[0, lanes] == 0).all())                # (without a cotangent a resetting lane's g_a_1 is 0)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduce", ["torch", "device"])
def test_autograd_with_a_loss_on_the_action_tape(reduce):
    import torch
    import gym_copter_amd
    n, K, hidden = 512, 10, 16
    rng = np.random.default_rng(5)
    env = _env("lander3d", n, "float64")
    try:
        x, st = _point(n, rng)
        p = _theta("lander3d", hidden, 4, env=env).requires_grad_(True)
        u = _dev(rng.uniform(-0.1, 0.1, (K, n, 4)).astype(np.float32), env).requires_grad_(True)
        x0 = _dev(x, env).requires_grad_(True)
        state = {"x": x0, "status": st}
        gx, gr = _dev(rng.standard_normal((K, n, 12)), env), _dev(rng.standard_normal((K, n)), env)
        w = _dev(rng.uniform(0.5, 2.0, (K, n, 4)), env)
        r = gym_copter_amd.differentiable_mlp_rollout(env, p, K, hidden, offsets=u, state=state, reduce=reduce)
        assert not r.actions.requires_grad and not r.obs.requires_grad      # the default: no gradient on the tape
        r = gym_copter_amd.differentiable_mlp_rollout(env, p, K, hidden, offsets=u, state=state, action_grad=True,
                                                      reduce=reduce)
        assert r.actions.requires_grad and not r.obs.requires_grad and not r.status.requires_grad
        loss = (r.x * gx).sum() + (r.reward * gr).sum() + (r.actions.double() ** 2 * w).sum()
        loss.backward()
        r2 = env.rollout_mlp_states(p.detach(), K, hidden, offsets=u.detach(), state={"x": x, "status": st})
        gin = (2 * w * r2.actions.double()).float()             # (the cotangent autograd hands back: the tape's dtype)
        gp, ga, g0 = env.rollout_mlp_vjp(p.detach(), r2, gx=gx, gr=gr, state={"x": x, "status": st}, hidden=hidden,
                                         g_actions_in=gin, reduce=reduce)
        assert torch.equal(p.grad, gp.float()) and torch.equal(u.grad, ga.float()) and torch.equal(x0.grad, g0)
        # (the penalty is in the gradient)
        _, ga0, _ = env.rollout_mlp_vjp(p.detach(), r2, gx=gx, gr=gr, state={"x": x, "status": st}, hidden=hidden,
                                        param_grad=False)
        assert not torch.equal(ga0.float(), u.grad)
        # once differentiable: a double backward raises
        r = gym_copter_amd.differentiable_mlp_rollout(env, p, K, hidden, offsets=u, state=state, action_grad=True,
                                                      reduce=reduce)
        g, = torch.autograd.grad((r.actions.double() ** 2).sum() + r.reward.sum(), p, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
        with pytest.raises(ValueError):
            gym_copter_amd.differentiable_mlp_rollout(env, p, K, hidden, reduce="host")
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. application: analytic policy gradients on Hover3D with a control-effort penalty
# ---------------------------------------------------------------------------------------------------------------------
EFFORT_C = 1300.0


def test_policy_training_with_an_effort_penalty_holds_hover3d():
    """test_policy_training_holds_hover3d's set-up (test_gpu_rollout_mlp) with the device reduction, a gradient on the
    action tape and an added effort term c mean((a - a_hover)^2).  c = 1300 is fixed from the start point alone: the
    untrained policy's first actions have mean((a - a_hover)^2) = 1.40e-5 (float64, on the host), and
    0.1 x 0.179 (the horizon loss at the start) / 1.40e-5 = 1 276.  The horizon loss (without the
    effort term) falls below 0.7 x its start, the bar of that test, and the effort term does not grow."""
    import torch
    import gym_copter_amd
    n, K, hidden = 4096, 64, 32
    rng = np.random.default_rng(61)
    env = _env("hover3d", n, "float32", seed=1)
    try:
        x = np.zeros((12, n))
        x[0], x[2] = rng.uniform(-0.5, 0.5, (2, n))
        x[4] = -5.0 + rng.uniform(-0.5, 0.5, n)
        x[5] = rng.uniform(-1.0, 1.0, n)
        x = x.astype(np.float32).astype(np.float64)
        state = {"x": _dev(x, env), "status": np.full(n, AIRBORNE, np.uint8)}
        p = _theta("hover3d", hidden, 0, scale=0.01, env=env).requires_grad_(True)
        a_hover = float(np.float32(hover_action()))
        opt = torch.optim.Adam([p], lr=2e-4)
        horizon, effort = [], []
        for _ in range(60):
            opt.zero_grad()
            r = gym_copter_amd.differentiable_mlp_rollout(env, p, K, hidden, state=state, action_grad=True,
                                                          reduce="device")
            h = ((r.x[..., 4] + 5.0) ** 2 + 0.1 * r.x[..., 5] ** 2).mean()
            e = EFFORT_C * ((r.actions.double() - a_hover) ** 2).mean()
            (h + e).backward()
            opt.step()
            horizon.append(float(h.detach()))
            effort.append(float(e.detach()))
        print("hover3d APG with an effort penalty: horizon loss %.4f -> %.4f (min %.4f), effort term %.4f -> %.4f "
              "(max %.4f), %.2f of the loss at the start" % (horizon[0], horizon[-1], min(horizon), effort[0],
                                                           effort[-1], max(effort), effort[0] / horizon[0]))
        assert np.isfinite(horizon).all() and np.isfinite(effort).all()
        assert horizon[-1] < 0.7 * horizon[0], (horizon[0], horizon[-1])
        assert effort[-1] <= effort[0], (effort[0], effort[-1])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. 64-bit offsets
# ---------------------------------------------------------------------------------------------------------------------
def test_reduction_past_4_gib():
    """1 048 576 envs x K = 136, H = 0: g_actions in float64 is 4.6 GB, the obs tape 5.7 GB (random tapes: no rollout is
    needed).  Skips only below 32 GiB of free device memory."""
    import torch
    from gym_copter_amd import mlp
    n, K, hidden = 1 << 20, 136, 0
    assert K * n * 4 * 8 > 4 << 30 and K * n * 10 * 4 > 4 << 30
    free, _ = torch.cuda.mem_get_info(0)
    if free < 32 << 30:
        pytest.skip("needs 32 GiB of free device memory, %.1f GiB free" % (free / 2.0 ** 30))
    env = _env("lander3d", n, "float32", seed=9)
    try:
        gen = torch.Generator(device=env.device).manual_seed(13)
        p = _theta("lander3d", hidden, 3, env=env)
        obs = torch.randn((K, n, 10), dtype=torch.float32, device=env.device, generator=gen)
        ga = torch.randn((K, n, 4), dtype=torch.float64, device=env.device, generator=gen)
        dev = env.mlp_param_grad(p, hidden, obs, ga)
        ref = mlp.param_grad(p, hidden, obs, ga)
        ratio = _bound_ratio(dev, ref, _term_magnitudes(p, hidden, obs, ga), K * n)
        print("device reduction past 4 GiB: %.3g of the bound" % ratio)
        assert ratio <= 1.0, ratio
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. sharded passthrough, 11. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_single_rank_passes_the_new_keywords_through():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    n, K = 4097, 10
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = _env("lander3d", n, "float32", autoreset="next_step", seed=6, max_steps=1000)
    try:
        sh.reset()
        plain.reset()
        p = _theta("lander3d", 8, 2, env=plain)
        gr = torch.ones((K, n), dtype=torch.float64, device=plain.device)
        gact = torch.randn((K, n, 4), dtype=torch.float64, device=plain.device,
                           generator=torch.Generator(device=plain.device).manual_seed(1))
        r1, r2 = sh.rollout_mlp_states(p, K, 8), plain.rollout_mlp_states(p, K, 8)
        for red in ("device", "torch"):
            g1 = sh.rollout_mlp_vjp(p, r1, gr=gr, hidden=8, g_actions_in=gact, reduce=red)
            g2 = plain.rollout_mlp_vjp(p, r2, gr=gr, hidden=8, g_actions_in=gact, reduce=red)
            assert torch.equal(g1[0], g2[0]) and torch.equal(g1[1], g2[1])
        with_cotangent = g2[1].clone()                          # (the env's buffer: its next call overwrites it)
        g3 = plain.rollout_mlp_vjp(p, r2, gr=gr, hidden=8)
        assert not torch.equal(g3[1], with_cotangent)           # (the cotangent arrived)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import torch
    n, K = 300, 6
    rng = np.random.default_rng(2)
    env = _env("lander2d", n, "float64")
    try:
        x, st = _point(n, rng)
        state = {"x": x, "status": st}
        p = _theta("lander2d", 4, 1, env=env)
        r = env.rollout_mlp_states(p, K, 4, state=state)
        gr = _dev(rng.standard_normal((K, n)), env)
        gin = torch.zeros((K, n, 2), dtype=torch.float64, device=env.device)
        _, ga, _ = env.rollout_mlp_vjp(p, r, gr=gr, state=state, hidden=4, g_actions_in=gin)
        ga = ga.clone()
        for bad in (gin[:-1], gin[:, :-1], gin[..., :1], gin.cpu(), gin.long(), gin.cpu().numpy()):
            with pytest.raises(ValueError):
                env.rollout_mlp_vjp(p, r, gr=gr, state=state, hidden=4, g_actions_in=bad)
        with pytest.raises(ValueError):
            env.rollout_mlp_vjp(p, r, gr=gr, state=state, hidden=4, reduce="host")
        env.mlp_param_grad(p, 4, r.obs, ga)
        env.mlp_param_grad(p, 4, r.obs, ga.float())
        for obs, g in ((r.obs[:-1], ga), (r.obs[:, :-1], ga), (r.obs[..., :-1], ga), (r.obs.double(), ga),
                       (r.obs.cpu(), ga), (r.obs, ga[:-1]), (r.obs, ga[..., :1]), (r.obs, ga.half()), (r.obs, ga.cpu()),
                       (to_np(r.obs), ga), (r.obs, to_np(ga))):
            with pytest.raises(ValueError):
                env.mlp_param_grad(p, 4, obs, g)
        with pytest.raises(ValueError):
            env.mlp_param_grad(p[:-1], 4, r.obs, ga)
        with pytest.raises(ValueError):
            env.mlp_param_grad(p, 65, r.obs, ga)
        with pytest.raises(ValueError):
            env.mlp_param_grad(p, 4, r.obs, ga, out=torch.empty(3, dtype=torch.float64, device=env.device))
    finally:
        env.close()
