"""CopterVecEnv.step_jacobian on the device (cs_step_jacobian): against central differences of the float64 oracle
(tests/jacobian_fd.py), the explicit point against the stored one, the branch bits and their structure, no side
effects on the env, and an LQR about hover built from it that holds 4 096 perturbed Hover3D envs."""
import numpy as np
import pytest

from gpu_util import have_gpu, to_np
from jacobian_fd import fd_jacobian, hover_action, hover_point, lqr_gain
from oracle.refcpu import AIRBORNE, CRASHED, DJI_PHANTOM, G, LANDED, LEVELING, VehicleParams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N = 4096
BAR = 1e-6
TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover1d": 1, "lander1d": 1, "hover2d": 2}


def _env(task, n, mode="float64", **kw):
    import gym_copter_amd
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode="disabled",
                                       max_steps=100000, **kw)


def _random_point(n, rng, force=False):
    """AIRBORNE states away from every branch threshold: high above the ground, inside the bounds, tilted well
    below the angle limits, |dz| far from dz_max."""
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    x[1], x[3], x[5] = rng.uniform(-2, 2, (3, n))
    x[4] = rng.uniform(-20, -5, n)
    x[6], x[8] = rng.uniform(-0.4, 0.4, (2, n))
    x[10] = rng.uniform(-1, 1, n)
    x[7], x[9], x[11] = rng.uniform(-1, 1, (3, n))
    f = rng.uniform(-30, 30, (3, n)) if force else None
    return x, np.full(n, AIRBORNE, np.uint8), f


def _install(env, x, status, force):
    n = env.num_envs
    kw = dict(x=x, status=status, steps=np.ones(n, np.int32), prev_shaping=np.zeros(n))
    if force is not None:
        kw.update(force=force, flags=np.full(n, 5, np.uint8))         # pending + explicit
    else:
        kw.update(flags=np.zeros(n, np.uint8))
    env.set_state(**kw)


def _check(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= BAR, "%s: max scaled error %.3g at %s" % (what, err.max(), np.unravel_index(err.argmax(), err.shape))


def _against_reference(task, substeps, mode="float64", vehicles=False, mars=False, force=False, seed=0):
    import torch
    rng = np.random.default_rng(seed)
    kw = {}
    vp, g, mars_p = DJI_PHANTOM, G, None
    if mars:
        kw = dict(thrust_model="lift", rotor_gyro=True, vehicle_params={"C_L": 0.5}, world_params={"rho": 1.0})
        mars_p = (1.0, 0.5)
    env = _env(task, N, mode, substeps=substeps, **kw)
    try:
        if vehicles:
            cols = dict(M=rng.uniform(1.0, 2.0, N), L=rng.uniform(0.25, 0.45, N), Ix=rng.uniform(1.5, 2.5, N),
                        Iy=rng.uniform(1.5, 2.5, N), Iz=rng.uniform(2.5, 3.5, N), maxrpm=rng.uniform(12000, 18000, N))
            env.set_vehicle_params(**cols)
            vp = VehicleParams(B=5e-3, D=2e-6, M=cols["M"], L=cols["L"], Ix=cols["Ix"], Iy=cols["Iy"], Iz=cols["Iz"],
                               Jr=38e-4, maxrpm=cols["maxrpm"])
        x, st, f = _random_point(N, rng, force)
        _install(env, x, st, f)
        if mode != "float64":   # the point is the decoded state
            s = env.get_state()
            x, f = s["x"], (s["force"] if force else None)
        # motor values around hover (B law) / a lift that holds the vehicle, away from the clip at 0 and 1
        if mars:
            w = DJI_PHANTOM.maxrpm * np.pi / 30
            kl = 0.5 * 1.0 * (0.05 * DJI_PHANTOM.L * 4) * 0.5 * (DJI_PHANTOM.L / 2) ** 2 * w * w
            ah = np.sqrt(G * DJI_PHANTOM.M / (4 * kl))
        else:
            ah = hover_action()
        A = TASK_A[task]
        a = (ah * rng.uniform(0.5, 1.5, (N, A))).astype(np.float32)
        jac = env.step_jacobian(torch.from_numpy(a).to(env.device))
        want = fd_jacobian(task, x, st, a.astype(np.float64), force=f, substeps=substeps, vp=vp, g=g, mars=mars_p)
        for name, got, w_ in zip(("dx", "du", "reward_dx", "reward_du"), jac[:4], want):
            _check(to_np(got), w_, "%s %s substeps=%d" % (task, name, substeps))
        assert np.all(to_np(jac.branch) == 1)          # integrated, nothing else
    finally:
        env.close()


@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("task", ["lander3d", "hover3d", "lander2d", "hover1d", "lander1d", "hover2d"])
def test_jacobian_matches_central_differences_of_the_reference(task, substeps):
    _against_reference(task, substeps, force=(substeps == 10))


@pytest.mark.parametrize("substeps", [1, 10])
def test_jacobian_per_env_vehicles(substeps):
    _against_reference("lander3d", substeps, vehicles=True, seed=1)


@pytest.mark.parametrize("substeps", [1, 10])
def test_jacobian_mars_model_with_rotor_gyro(substeps):
    _against_reference("lander3d", substeps, mars=True, seed=2)


@pytest.mark.parametrize("mode", ["float32", "float32_rn"])
def test_jacobian_float32_storage_at_the_decoded_state(mode):
    import gym_copter_amd.vecenv as V
    if mode not in V._STATE_MODES:
        pytest.skip("storage mode %r not offered" % mode)
    _against_reference("lander3d", 10, mode=mode, force=True, seed=3)


@pytest.mark.parametrize("force", [False, True])
def test_explicit_point_equals_stored_point_bit_for_bit(force):
    import torch
    rng = np.random.default_rng(4)
    env = _env("lander3d", N, "float32", substeps=10)
    try:
        x, st, f = _random_point(N, rng, force)
        _install(env, x, st, f)
        s = env.get_state()
        a = torch.from_numpy((hover_action() * rng.uniform(0.5, 1.5, (N, 4))).astype(np.float32)).to(env.device)
        stored = [to_np(t).copy() for t in env.step_jacobian(a)]
        pt = {"x": s["x"], "status": s["status"]}
        if force:
            pt["force"] = s["force"]
        explicit = [to_np(t).copy() for t in env.step_jacobian(a, state=pt)]
        for g_, w_ in zip(explicit, stored):
            assert g_.tobytes() == w_.tobytes()
    finally:
        env.close()


def test_branch_bits_and_structure():
    import torch
    from gym_copter_amd import _lib
    import gym_copter_amd
    n = 8
    env = gym_copter_amd.CopterVecEnv(task="lander3d", num_envs=n, state_dtype="float64", autoreset_mode="next_step")
    try:
        x, st, _ = _random_point(n, np.random.default_rng(5))
        x[:, 0] = 0.0                                       # 0: LANDED on the ground
        st[0] = LANDED
        x[4, 1], x[5, 1], x[3, 1], x[6, 1] = 0.01, 0.5, 0.1, 0.1   # 1: ground contact, soft (-> LEVELING)
        st[2] = LEVELING                                    # 2: levelling the wings
        st[3] = CRASHED                                     # 3: crashed
        flags = np.zeros(n, np.uint8)
        flags[4] = 2                                        # 4: a NEXT_STEP reset pending
        env.set_state(x=x, status=st, steps=np.ones(n, np.int32), prev_shaping=np.zeros(n), flags=flags)
        a = np.full((n, 4), hover_action(), np.float32)
        a[5] = [1.5, hover_action(), -0.3, hover_action()]  # 5: motors 0 and 2 clipped; 6, 7: free flight
        j = env.step_jacobian(torch.from_numpy(a).to(env.device))
        dx, du, b = to_np(j.dx), to_np(j.du), to_np(j.branch)
        I = np.eye(12)
        assert b[0] == _lib.JAC_LANDED and np.array_equal(dx[0], I) and not du[0].any()
        assert b[1] == _lib.JAC_CONTACT and np.array_equal(dx[1], I) and not du[1].any()
        lev = I.copy()
        lev[6, 6] = lev[8, 8] = 0.0
        assert b[2] == _lib.JAC_LEVELING and np.array_equal(dx[2], lev) and not du[2].any()
        assert b[3] == _lib.JAC_CRASHED and np.array_equal(dx[3], I) and not du[3].any()
        assert b[4] == _lib.JAC_RESET and not dx[4].any() and not du[4].any()
        assert not to_np(j.reward_dx)[4].any() and not to_np(j.reward_du)[4].any()
        assert b[5] == _lib.JAC_INTEGRATED | _lib.JAC_CLIPPED
        assert not du[5][:, [0, 2]].any() and du[5][:, [1, 3]].any()
        assert np.all(b[6:] == _lib.JAC_INTEGRATED)
    finally:
        env.close()


def test_no_side_effects_on_the_env():
    """A twin with the same seed that never calls step_jacobian: every output and the whole state stay bit-identical."""
    import torch
    import gym_copter_amd
    envs = [gym_copter_amd.make("Lander-v0", num_envs=N, seed=11, autoreset_mode="next_step", device=0) for _ in range(2)]
    try:
        rng = np.random.default_rng(6)
        for e in envs:
            e.reset()
        for t in range(30):
            a = torch.from_numpy(rng.uniform(-1, 1, (N, 4)).astype(np.float32)).to(envs[0].device)
            envs[0].step_jacobian(a)
            envs[0].step_jacobian(a, dtype=torch.float32)
            outs = [[to_np(v).copy() for v in e.step(a)[:4]] for e in envs]
            for u, v in zip(*outs):
                assert u.tobytes() == v.tobytes(), t
        ak = torch.from_numpy(rng.uniform(-1, 1, (5, N, 4)).astype(np.float32)).to(envs[0].device)
        envs[0].step_jacobian(ak[0])
        outs = [[to_np(v).copy() for v in e.step_many(ak)[:4]] for e in envs]
        for u, v in zip(*outs):
            assert u.tobytes() == v.tobytes()
        s0, s1 = envs[0].get_state(), envs[1].get_state()
        for k in s0:
            assert np.asarray(s0[k]).tobytes() == np.asarray(s1[k]).tobytes(), k
    finally:
        for e in envs:
            e.close()


def test_lqr_about_hover_holds_perturbed_envs():
    """A discrete LQR gain from dx / du at the hover point closes the loop through step(): 4 096 Hover3D envs started
    with the reference's random perturbation stay within 0.5 m of their start for 1 000 steps, none terminates.
    Control case: under the constant hover action at least 90 % of the same envs leave that box."""
    import torch

    def fly(controlled):
        env = _env("hover3d", N, "float32", seed=3)
        try:
            env.reset()
            dev = env.device
            a_star = np.float32(hover_action())
            xh, sh = hover_point(N)
            j = env.step_jacobian(np.full((N, 4), a_star, np.float32), state={"x": xh, "status": sh})
            A, B = to_np(j.dx)[0], to_np(j.du)[0]
            K = torch.from_numpy(lqr_gain(A, B, np.ones(12), np.full(4, 1e4))).to(dev)
            xs = torch.from_numpy(xh[:, :1]).to(dev)
            x0 = env.state_tensors()["x"].double().clone()
            worst = torch.zeros(N, dtype=torch.float64, device=dev)
            done = torch.zeros(N, dtype=torch.bool, device=dev)
            for _ in range(1000):
                xnow = env.state_tensors()["x"].double()
                if controlled:
                    u = (float(a_star) - (K @ (xnow - xs)).T).float().contiguous()
                else:
                    u = torch.full((N, 4), float(a_star), dtype=torch.float32, device=dev)
                _, _, term, trunc, _ = env.step(u)
                done |= term | trunc
                dev_now = (env.state_tensors()["x"].double()[[0, 2, 4]] - x0[[0, 2, 4]]).abs().amax(0)
                worst = torch.maximum(worst, dev_now)
            return worst.cpu().numpy(), done.cpu().numpy()
        finally:
            env.close()

    worst, done = fly(True)
    assert not done.any() and worst.max() < 0.5, (done.sum(), worst.max())
    worst_c, _ = fly(False)
    assert np.mean(worst_c > 0.5) >= 0.9, np.mean(worst_c > 0.5)


@pytest.mark.parametrize("task", sorted(TASK_A))
def test_shapes_dtypes_and_float32_rounding(task):
    import torch
    n = 100     # a ragged last tile
    env = _env(task, n, "float32", substeps=2)
    try:
        env.reset()
        A = TASK_A[task]
        a = torch.from_numpy(np.random.default_rng(7).uniform(-0.2, 1.2, (n, A)).astype(np.float32)).to(env.device)
        j64 = [t.clone() for t in env.step_jacobian(a)]
        j32 = env.step_jacobian(a, dtype=torch.float32)
        shapes = [(n, 12, 12), (n, 12, A), (n, 12), (n, A), (n,)]
        for t64, t32, shp in zip(j64, j32, shapes):
            assert tuple(t64.shape) == shp and tuple(t32.shape) == shp
        for t64, t32 in zip(j64[:4], j32[:4]):
            assert t64.dtype == torch.float64 and t32.dtype == torch.float32
            assert torch.equal(t64.float(), t32)
        assert j64[4].dtype == torch.uint8 and torch.equal(j64[4], j32[4])
        # the buffers are reused across calls of the same dtype
        again = env.step_jacobian(a)
        assert again.dx.data_ptr() == env.step_jacobian(a).dx.data_ptr()
    finally:
        env.close()


def test_closed_env_raises():
    env = _env("lander3d", 64)
    env.close()
    with pytest.raises(RuntimeError):
        env.step_jacobian(np.zeros((64, 4), np.float32))
