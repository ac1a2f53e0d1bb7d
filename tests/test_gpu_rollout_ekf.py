"""The extended Kalman filter on the device (cs_rollout_ekf, CopterVecEnv.rollout_ekf, gym_copter_amd.ekf): every step
of the kernel's recursion against the NumPy restatement (tests/ekf_ref.py) on the kernel's OWN tapes -- the Jacobian
depends on the filter's own mean, so a reference chained over K steps could take another branch than the device at a
touchdown; one step at a time it cannot, and by induction over k the whole recursion is verified.  For step k the
reference takes the device's posterior of step k - 1, the device's x_pred[k] (pinned, bit for bit, to rollout_states; in
float32 storage, where rollout_states rounds its stored words once and the filter's mean is not rounded, within 2^-23
max(1, |value|): measured 0.015 of that in the guarded mode, 0.49 in float32_rn) and
A = step_jacobian(actions[k], state = that posterior's mean and status).dx.

The bar per output is 100 x the float64 reference's own distance from the same step in numpy.longdouble, floored at
1e-12 scaled (ekf_ref.FLOOR).  Worst measured ratio to the bar on an MI355X over all cases: x 0.017, P_tape and var below
0.0005, nis 0.033, loglik 0.004."""
import zlib

import numpy as np
import pytest

import ekf_ref
import model_variants
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover2d": 2, "lander1d": 1, "hover1d": 1}
AH = hover_action()
N, K = 300, 16          # four whole wavefronts and one of 44 lanes


def _env(task, n, mode="float64", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode="disabled", **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


GROUPS = ("hover", "soft0", "hard0", "soft_mid", "hard_mid", "landed", "crashed", "clip")


def _points(n, steps, A, rng, ah):
    """Start means, one group of envs per branch: high hover; descents in ground contact at the first call (z > 0), soft
    and hard; low descents that touch down inside the horizon, soft and hard; LANDED and CRASHED starts; motors outside
    [0, 1] on both sides.  A motor above 1 is a motor at 1, 900 times the hover thrust of the default vehicle (the hover
    motor value is 0.0166 and the thrust goes with its square): the step's Jacobian then has entries of 180 to 700 per
    radian, so those lanes ("clip_hi": every third of the clip group, in step 1 only) are given a small P0 by _problem,
    or P- would be so large that Q's share of its entries is no longer far above the floor.  Returns (x [12,n], status
    [n], actions [steps,n,A] float32, group names [n])."""
    grp = np.array([GROUPS[i % len(GROUPS)] for i in range(n)])
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[1], x[3] = rng.uniform(-0.3, 0.3, (2, n))
    x[4] = rng.uniform(-8, -4, n)
    x[5] = rng.uniform(-0.5, 0.5, n)
    x[6], x[8] = rng.uniform(-0.05, 0.05, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-0.3, 0.3, (4, n))
    st = np.full(n, AIRBORNE, np.uint8)
    a = ah * rng.uniform(0.8, 1.2, (steps, n, A))
    for name, dz in (("soft0", (0.1, 0.6)), ("hard0", (1.5, 3.0)), ("soft_mid", (0.2, 0.6)), ("hard_mid", (1.5, 3.0))):
        m = grp == name
        k = int(m.sum())
        x[5, m] = rng.uniform(*dz, k)
        if name.endswith("0"):
            x[4, m] = rng.uniform(1e-3, 0.05, k)
        else:                                    # z passes 0 after 6 .. 18 steps of 0.01 s at this descent rate: most of
            #                                      these lanes touch down inside 16 steps, the lowest third inside 10
            x[4, m] = -x[5, m] * rng.uniform(3, 9, k) / 50.0
    m = grp == "landed"
    x[4, m], x[5, m], st[m] = 0.0, 0.0, LANDED
    st[grp == "crashed"] = CRASHED
    m = grp == "clip"
    k = int(m.sum())
    a[:, m] = np.where(rng.uniform(size=(steps, k, A)) < 0.5, rng.uniform(-0.4, -0.01, (steps, k, A)), a[:, m])
    hi = np.flatnonzero(m)[::3]
    a[0, hi, A - 1] = rng.uniform(1.01, 1.4, hi.size)
    grp[hi] = "clip_hi"
    return x, st, a.astype(np.float32), grp


def _spd(rng, n, scale=0.1):
    m = rng.standard_normal((n, 12, 12))
    P = scale * (m @ np.swapaxes(m, 1, 2) / 12 + 0.2 * np.eye(12))
    return (P + np.swapaxes(P, 1, 2)) / 2          # symmetric to the bit: the kernel reads the upper triangle only


def _model(rng, M, dense):
    if dense:
        H = rng.standard_normal((M, 12)) / np.sqrt(12)
    else:
        H = np.zeros((M, 12))
        H[np.arange(M), rng.permutation(12)[:M]] = 1.0
    return H, rng.uniform(0.01, 0.1, M)


def _problem(env, task, rng, M=6, dense=True, missing=0.0, steps=K, seed=5, ah=AH):
    """the filter's inputs on env: starts of every branch, a random SPD P0 per env, and measurements synthesised from the
    rollout_states tape of the same starts"""
    from gym_copter_amd import measure
    n, A = env.num_envs, TASK_A[task]
    x0, st0, acts, grp = _points(n, steps, A, rng, ah)
    H, r = _model(rng, M, dense)
    P0 = _spd(rng, n)
    P0[grp == "clip_hi"] *= 1e-4
    acts_d = _dev(acts, env)
    truth = env.rollout_states(acts_d, state={"x": x0, "status": st0}).x.clone()
    z = measure(truth, H, r, seed, missing=missing)
    return dict(acts=acts_d, z=z, H=H, r=r, Q=ekf_ref.test_Q(), x0=_dev(x0, env), P0=_dev(P0, env),
                st0=_dev(st0, env), grp=grp)


def _run(env, p, **kw):
    return env.rollout_ekf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], status0=p["st0"], **kw)


def _clone(res):
    return type(res)(*[None if t is None else t.clone() for t in res])


WORST = {}


def _check_steps(name, env, p, res, lanes=None, exact_pred=True):
    """every step of res (a tape=True result, cloned) against one reference step from the device's own tapes; returns the
    branch bits step_jacobian reports at the filter's own points [K,n] and the reference's predicted covariances"""
    import torch
    steps, n = res.x.shape[:2]
    lanes = slice(None) if lanes is None else lanes
    acts, Q = p["acts"], p["Q"]
    xprev, Pprev, sprev = p["x0"], to_np(p["P0"][lanes]), p["st0"]
    bits, ppred = [], []
    ok = np.ones(n, bool)[lanes]
    ll64, llbar = 0.0, 0.0
    worst = {}
    assert torch.equal(res.P, res.P_tape[-1])
    assert torch.equal(res.var, torch.diagonal(res.P_tape, dim1=2, dim2=3))
    assert torch.equal(res.P_tape, res.P_tape.transpose(2, 3))
    for k in range(steps):
        state = {"x": xprev, "status": sprev}
        jac = env.step_jacobian(acts[k], state=state)
        A, br = to_np(jac.dx[lanes]).astype(np.float64), jac.branch.clone()
        one = env.rollout_states(acts[k:k + 1], state=state)
        if exact_pred:
            assert torch.equal(one.x[0], res.x_pred[k]), (name, k)
        else:   # float32 storage: rollout_states rounds the stored words to 24 bits, the filter's mean is not rounded
            want = to_np(one.x[0]).astype(np.float64)
            err = np.abs(to_np(res.x_pred[k]) - want) / np.maximum(1.0, np.abs(want))
            worst["x_pred / 2^-23"] = max(worst.get("x_pred / 2^-23", 0.0), float(err.max()) * 2.0 ** 23)
            assert np.all(err <= 2.0 ** -23), (name, k, float(err.max()) * 2.0 ** 23)
        assert torch.equal(one.status[0], res.status[k]), (name, k)
        assert torch.equal(br, res.branch[k]), (name, k)
        bits.append(to_np(br))
        xp = to_np(res.x_pred[k][lanes])
        zk = to_np(p["z"][k][lanes])
        r64 = ekf_ref.one_step(A, Pprev, xp, Q, p["H"], p["r"], zk)
        rld = ekf_ref.one_step(A, Pprev, xp, Q, p["H"], p["r"], zk, dtype=np.longdouble)
        ok &= r64["ok"]
        bar = ekf_ref.bars(r64, rld)
        # Q's share of every entry of P- is far above the bar: a dropped Q cannot pass
        share = np.abs(Q)[None] / np.maximum(1.0, np.abs(r64["P_pred"]))
        assert share.min() >= 1e3 * bar["P"], (name, k, share.min(), bar["P"])
        got = dict(x=to_np(res.x[k][lanes]), P=to_np(res.P_tape[k][lanes]), var=to_np(res.var[k][lanes]),
                   nis=to_np(res.nis[k][lanes]))
        for key, g in got.items():
            e = ekf_ref.scaled(g, r64[key])
            worst[key] = max(worst.get(key, 0.0), e / bar[key])
            assert e <= bar[key], (name, key, k, e, bar[key])
        ll64 = ll64 + r64["loglik"]
        llbar += bar["loglik"]
        ppred.append(r64["P_pred"])
        xprev, Pprev, sprev = res.x[k].T.contiguous(), got["P"], res.status[k]
    e = ekf_ref.scaled(to_np(res.loglik[lanes]), ll64)
    worst["loglik"] = e / llbar
    assert e <= llbar, (name, "loglik", e, llbar)
    assert np.array_equal(to_np(res.ok[lanes]), ok)
    WORST[name] = worst
    print("%s: worst ratio to the bar " % name + " ".join("%s %.3f" % kv for kv in worst.items()))
    return np.array(bits), np.array(ppred)


# ---------------------------------------------------------------------------------------------------------------------
# 1. through every branch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps", [1, 10])
def test_every_step_through_every_branch(substeps):
    import torch
    from gym_copter_amd import _lib
    rng = np.random.default_rng(700 + substeps)
    env = _env("lander3d", N, substeps=substeps, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        res = _clone(_run(env, p, tape=True))
        bits, _ = _check_steps("lander3d substeps=%d" % substeps, env, p, res)
        frac = {nm: float(((bits & b) != 0).mean()) for nm, b in (
            ("INTEGRATED", _lib.JAC_INTEGRATED), ("LANDED", _lib.JAC_LANDED), ("CONTACT", _lib.JAC_CONTACT),
            ("CRASHED", _lib.JAC_CRASHED), ("CLIPPED", _lib.JAC_CLIPPED), ("LEVELING", _lib.JAC_LEVELING))}
        print("branch shares of the (k, env) pairs: " + " ".join("%s %.3f" % kv for kv in frac.items()))
        for nm in ("INTEGRATED", "LANDED", "CONTACT", "CRASHED", "CLIPPED"):
            assert frac[nm] >= 0.01, (nm, frac[nm])
        assert not (bits & _lib.JAC_RESET).any()
        # the same bits in every other output without the tape
        plain = _run(env, p)
        assert plain.P_tape is None
        for a, b in zip(plain[:9], res[:9]):
            assert torch.equal(a, b)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes and models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,mode,M", [("hover3d", "float32", 6), ("lander2d", "float64", 1), ("hover1d", "float64", 12)])
def test_every_step_for_other_tasks_storage_modes_and_measurement_counts(task, mode, M):
    rng = np.random.default_rng(zlib.crc32(repr((task, mode, M)).encode()))
    env = _env(task, N, mode, seed=3)
    try:
        env.reset()
        p = _problem(env, task, rng, M=M)
        res = _clone(_run(env, p, tape=True))
        # (float32 storage: rollout_states rounds the stored words, the filter's mean is not rounded)
        _check_steps("%s %s M=%d" % (task, mode, M), env, p, res, exact_pred=mode == "float64")
    finally:
        env.close()


@pytest.mark.parametrize("variant", ["vehicles", "mars_gyro"])
def test_every_step_under_model_variants(variant):
    rng = np.random.default_rng(zlib.crc32(variant.encode()))
    env = _env("lander3d", N, seed=3, **model_variants.env_kwargs(variant))
    ref = _env("lander3d", N, seed=3)
    try:
        model_variants.install(variant, env, rng)
        env.reset()
        ref.reset()
        p = _problem(env, "lander3d", rng, ah=model_variants.hover(variant))
        res = _clone(_run(env, p, tape=True))
        _check_steps("lander3d %s" % variant, env, p, res)
        # the default model gives another x_pred in every lane that flies
        other = to_np(_run(ref, p).x_pred)
        same = np.all(to_np(res.x_pred).view(np.uint64) == other.view(np.uint64), axis=(0, 2))
        flies = np.isin(p["grp"], ("hover", "clip", "clip_hi", "soft_mid", "hard_mid"))
        assert flies.sum() >= N // 3 and not np.any(same & flies), np.flatnonzero(same & flies)[:8]
    finally:
        env.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. missing measurements
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_measurements_are_skipped():
    import torch
    rng = np.random.default_rng(31)
    env = _env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, M=6, dense=False, missing=0.3)
        p["z"][3] = float("nan")                       # steps without a measurement for any env
        p["z"][K - 1] = float("nan")
        gone = torch.isnan(p["z"])
        assert 0.25 < float(gone[[0, 1, 2, 4]].double().mean()) < 0.35
        blind = gone.all(dim=2).all(dim=1)
        assert blind.tolist() == [k in (3, K - 1) for k in range(K)]
        res = _clone(_run(env, p, tape=True))
        # (on a step without measurements the reference's posterior IS its predicted covariance: the comparison inside
        # pins P_tape[k] to P- there)
        _check_steps("lander3d 30% missing", env, p, res)
        for k in (3, K - 1):
            assert torch.equal(res.x[k], res.x_pred[k])
            assert bool((res.nis[k] == 0).all())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. exact statements
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("status", [LANDED, CRASHED])
def test_grounded_filter_without_measurements_adds_q_exactly(status):
    import torch
    rng = np.random.default_rng(41 + status)
    env = _env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        p["st0"] = torch.full((N,), int(status), dtype=torch.uint8, device=env.device)
        p["z"] = torch.full_like(p["z"], float("nan"))
        res = _run(env, p, tape=True)
        want = to_np(p["P0"]).copy()
        for k in range(K):
            want = want + p["Q"]                       # (((P0 + Q) + Q) + ...), in this order
            assert torch.equal(res.x[k], p["x0"].T), k
            assert np.array_equal(to_np(res.P_tape[k]), want), k
        assert bool((res.status == int(status)).all()) and bool(res.ok.all())
        assert bool((res.nis == 0).all()) and bool((res.loglik == 0).all())
    finally:
        env.close()


def test_a_nonpositive_innovation_variance_clears_ok_for_that_env_only():
    import torch
    rng = np.random.default_rng(43)
    env = _env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, dense=False)
        good = _clone(_run(env, p, tape=True))
        assert bool(good.ok.all())
        bad_env = 77
        p["P0"] = p["P0"].clone()
        p["P0"][bad_env] = -torch.eye(12, dtype=torch.float64, device=env.device)
        res = _run(env, p, tape=True)
        ok = to_np(res.ok)
        assert not ok[bad_env] and ok.sum() == N - 1
        others = torch.arange(N, device=env.device) != bad_env
        for a, b in zip(res, good):
            sel = (lambda t: t[others]) if a.shape[0] == N else (lambda t: t[:, others])
            assert torch.equal(sel(a), sel(b))
            assert bool(torch.isfinite(sel(a).double()).all())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. chunking
# ---------------------------------------------------------------------------------------------------------------------
def test_chunked_filter_is_the_single_call_bit_for_bit():
    import torch
    from gym_copter_amd import ekf
    rng = np.random.default_rng(51)
    env = _env("lander3d", N, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, missing=0.1)
        one = _clone(_run(env, p, tape=True))
        args = (env, p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"])
        for chunk in (5, None, 1):
            got = ekf(*args, status0=p["st0"], chunk=chunk)
            for name in ("x", "x_pred", "P", "var", "nis", "status", "branch", "ok", "P_tape"):
                assert torch.equal(getattr(got, name), getattr(one, name)), (chunk, name)
            assert torch.allclose(got.loglik, one.loglik, rtol=1e-13, atol=1e-12)
    finally:
        env.close()
    # K = 1 and N = 1 also run
    env = _env("lander3d", 1, seed=3)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, steps=1)
        res = _clone(_run(env, p, tape=True))
        assert res.x.shape == (1, 1, 12) and res.P_tape.shape == (1, 1, 12, 12)
        _check_steps("N=1 K=1", env, p, res)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. application
# ---------------------------------------------------------------------------------------------------------------------
def test_hover_tracking_is_consistent():
    """Hover3D, 300 envs, 48 steps, positions and angles measured: the inputs of
    test_rollout_ekf_cpu.py::test_application_conditions_hold_on_the_oracle_restatement (which satisfy the same four
    conditions on the float64 oracle: mean NIS 6.02; final RMSE 0.027 m, 0.10 m/s, 0.0028 rad, 0.010 rad/s)."""
    from gym_copter_amd import measure
    a, x0, xhat0, H, r = ekf_ref.app_inputs(AH, seed=1)
    n = ekf_ref.APP_N
    env = _env("hover3d", n, seed=3)
    try:
        env.reset()
        acts = _dev(a, env)
        ro = env.rollout_states(acts, state={"x": x0, "status": np.full(n, AIRBORNE, np.uint8)})
        truth = ro.x.clone()
        assert bool((ro.status == AIRBORNE).all())
        z = measure(truth, H, r, seed=1)
        P0 = np.repeat(ekf_ref.APP_P0[None], n, axis=0)
        res = env.rollout_ekf(acts, z, H, r, ekf_ref.APP_Q, _dev(xhat0, env), _dev(P0, env))
        assert bool(res.ok.all())
        rmse0 = np.sqrt(np.mean((xhat0 - x0)[[1, 3, 5]] ** 2, axis=1))
        fig = ekf_ref.app_conditions(to_np(res.x), to_np(torch_diag(res.P)), to_np(res.nis), to_np(truth), rmse0)
        print("mean NIS %.3f rmse %s sd %s" % (fig["mean_nis"], np.round(fig["rmse"], 4), np.round(fig["sd"], 4)))
    finally:
        env.close()


def torch_diag(P):
    import torch
    return torch.diagonal(P, dim1=1, dim2=2)


# ---------------------------------------------------------------------------------------------------------------------
# 7. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_float32_outputs_repeatability_overwrite_and_no_state_change():
    import torch
    rng = np.random.default_rng(71)
    env = _env("lander3d", 257, "float32", seed=3)
    try:
        env.reset()
        before = env.get_state()
        p = _problem(env, "lander3d", rng, missing=0.2)
        r64 = _clone(_run(env, p, tape=True))
        for t in _run(env, p, tape=True):                # the env's buffers: poison them, then run again
            t.fill_(float("nan") if t.dtype.is_floating_point else 1)
        again = _run(env, p, tape=True)
        for a, b in zip(again, r64):
            assert torch.equal(a, b)                     # NaN-filled outputs are overwritten, the same bits on every call
        r32 = _run(env, p, tape=True, dtype=torch.float32)
        for name in ("P", "var", "nis", "loglik", "P_tape"):
            assert getattr(r32, name).dtype == torch.float32
            assert torch.equal(getattr(r32, name), getattr(r64, name).float()), name
        for name in ("x", "x_pred", "status", "branch", "ok"):
            assert torch.equal(getattr(r32, name), getattr(r64, name)), name
        assert r32.ok.dtype == torch.bool and not any(t.requires_grad for t in r32)
        # status0 defaults to AIRBORNE
        p2 = dict(p, st0=None)
        air = dict(p, st0=torch.full((257,), AIRBORNE, dtype=torch.uint8, device=env.device))
        for a, b in zip(_clone(_run(env, p2)), _run(env, air)):
            assert a is None or torch.equal(a, b)
        after = env.get_state()
        assert sorted(before) == sorted(after)
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]), equal_nan=True), key
    finally:
        env.close()


def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    rng = np.random.default_rng(72)
    n = 4097
    sh = ShardedCopterVecEnv("lander3d", n, device=0, seed=6, autoreset_mode="next_step")
    plain = _env("lander3d", n, "float32", seed=6)
    try:
        sh.reset()
        plain.reset()
        p = _problem(plain, "lander3d", rng, steps=6)
        a = sh.rollout_ekf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], status0=p["st0"], tape=True)
        b = _run(plain, p, tape=True)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_offsets_past_4_gib():
    """P_tape [K,N,12,12] float64 is 4.8 GB at K = 4 with 2^20 envs; the last 1 000 envs pass the one-step bar."""
    import torch
    from gym_copter_amd import measure
    n, steps, M = 1 << 20, 4, 6
    assert steps * n * 144 * 8 > 4 << 30 > (steps - 1) * n * 144 * 8
    rng = np.random.default_rng(73)
    env = _env("lander3d", n, seed=9)
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        acts = torch.rand((steps, n, 4), generator=g, device=env.device, dtype=torch.float32) * 0.2 * float(AH) + 0.9 * float(AH)
        x0 = torch.randn((12, n), generator=g, device=env.device, dtype=torch.float64) * 0.2
        x0[4] -= 6.0
        st0 = torch.full((n,), AIRBORNE, dtype=torch.uint8, device=env.device)
        H, r = _model(rng, M, True)
        P0 = (torch.eye(12, dtype=torch.float64, device=env.device) * 0.05).expand(n, 12, 12).contiguous()
        P0 = P0 * (1.0 + torch.rand((n, 1, 1), generator=g, device=env.device, dtype=torch.float64))
        truth = env.rollout_states(acts, state={"x": x0, "status": st0}).x
        z = measure(truth, H, r, 7)
        del truth
        p = dict(acts=acts, z=z, H=H, r=r, Q=ekf_ref.test_Q(), x0=x0, P0=P0, st0=st0)
        res = _run(env, p, tape=True)
        assert bool(res.ok.all())
        _check_steps("2^20 envs, last 1000", env, p, res, lanes=slice(n - 1000, n))
    finally:
        env.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib
    rng = np.random.default_rng(74)
    n = 128
    env = _env("lander3d", n, seed=1)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, steps=4)
        base = dict(actions=p["acts"], z=p["z"], H=p["H"], r=p["r"], Q=p["Q"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        env.rollout_ekf(**base)
        badQ = p["Q"].copy()
        badQ[0, 1] += 1e-9
        nanr = p["r"].copy()
        nanr[0] = np.nan
        for kw, match in ((dict(actions=p["acts"][:, :n - 1]), "actions must have shape"),
                          (dict(z=p["z"][:2]), "z must have shape"), (dict(z=p["z"].cpu()), "z must be on"),
                          (dict(z=p["z"].long()), "z must be a floating-point"),
                          (dict(H=np.zeros((13, 12))), "H must have shape"), (dict(H=np.zeros((0, 12))), "H must have shape"),
                          (dict(H=p["H"][:, :11]), "H must have shape"), (dict(H=p["H"] * np.inf), "H must be finite"),
                          (dict(r=p["r"][:3]), "r must have shape"), (dict(r=-p["r"]), "r must be positive"),
                          (dict(r=p["r"] * 0), "r must be positive"), (dict(r=nanr), "r must be finite"),
                          (dict(Q=badQ), "Q must be symmetric"), (dict(Q=p["Q"][:6]), "Q must have shape"),
                          (dict(Q=p["Q"] * np.nan), "Q must be finite"),
                          (dict(x0=p["x0"][:6]), "x0 must have shape"), (dict(x0=p["x0"].cpu()), "x0 must be on"),
                          (dict(P0=p["P0"][:, :6]), "P0 must have shape"), (dict(P0=p["P0"].cpu()), "P0 must be on"),
                          (dict(P0=p["P0"].long()), "P0 must be a floating-point"),
                          (dict(status0=p["st0"][:5]), "status0"), (dict(dtype=torch.float16), "dtype must be")):
            args = dict(base)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_ekf(**args)
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), 4
        io.actions_dev, io.start_x_dev, io.start_status_dev = p["acts"].data_ptr(), p["x0"].data_ptr(), p["st0"].data_ptr()
        eio = _lib.RolloutEkfIO()
        eio.struct_size = C.sizeof(eio) + 8
        assert env._lib.cs_rollout_ekf(env._ctx, C.byref(io), C.byref(eio), None) == _lib.ERR_ABI
        # refused while a serve session is open
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_ekf(**base)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_ekf(**base)
    f32 = _env("lander3d", n, seed=1, action_arith="float32")
    try:
        f32.reset()
        with pytest.raises(CopterStepError, match="float32 motor model"):
            f32.rollout_ekf(**base)
    finally:
        f32.close()
