"""The bootstrap particle filter on the device (cs_rollout_pf, CopterVecEnv.rollout_pf, gym_copter_amd.pf): every step
of the kernel against the NumPy restatement (tests/pf_ref.py) on the kernel's OWN tapes -- a chained reference could
resample where the device does not after a one-ulp difference in exp.  The start of step k is part_tape[k-1] gathered
through anc_tape[k-1] (the Gaussian start for the first step).  Exact: the prior particles (a K = 1 rollout_states from
those N P explicit points plus the reference's noise), everything downstream of the integer weights, the carried state.
Within section 19's bar (100 x the float64 reference's distance from its numpy.longdouble twin, floored at 1e-12
scaled): lw, x, var, P and loglik."""
import zlib

import numpy as np
import pytest

import ekf_ref
import model_variants
import pf_ref
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover2d": 2, "lander1d": 1, "hover1d": 1}
AH = hover_action()
N, K = pf_ref.TEST_N, pf_ref.TEST_K
SEED = 3


def _env(task, n, mode="float64", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    kw.setdefault("seed", SEED)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode="disabled", **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _problem(env, task, rng, M=6, dense=True, missing=0.0, ah=AH):
    """pf_ref.test_problem on env: measurements synthesised in NumPy from the rollout_states tape of the same starts"""
    x0, st0, P0, acts, H, r = pf_ref.test_problem(rng, TASK_A[task], ah, M=M, dense=dense)
    acts_d = _dev(acts, env)
    truth = to_np(env.rollout_states(acts_d, state={"x": x0, "status": st0}).x).astype(np.float64)
    z = truth @ H.T + np.sqrt(r) * rng.standard_normal((K, N, M))
    if missing:
        z[rng.uniform(size=z.shape) < missing] = np.nan
    return dict(acts=acts_d, z=_dev(z, env), H=H, r=r, Q=ekf_ref.test_Q(), x0=_dev(x0, env), P0=_dev(P0, env),
                st0=_dev(st0, env), nonce=7, ess_frac=0.5)


def _run(env, p, P, **kw):
    kw.setdefault("tape", True)
    return env.rollout_pf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], particles=P, nonce=p["nonce"],
                          ess_frac=p["ess_frac"], status0=p["st0"], **kw)


def _clone(res):
    return type(res)(*[None if t is None else t.clone() for t in res])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _particle_env(task, P, substeps, variant=None, installed=None, mode="float64"):
    """an env of N P lanes for the K = 1 rollout_states of every particle: lane e P + p is particle p of env e, under env
    e's vehicle"""
    kw = model_variants.env_kwargs(variant) if variant else {}
    env = _env(task, N * P, mode, substeps=substeps, **kw)
    if isinstance(installed, dict):
        env.set_vehicle_params(**{k: np.repeat(np.asarray(v), P) for k, v in installed.items()})
    env.reset()
    return env


WORST = {}


def _check_steps(name, env, penv, p, res, P, exact=True, first_step=1, start=None, g=None):
    """every step of res (a tape=True result, cloned) against the reference from the device's own tapes; g: the global
    ids of env's lanes (env_id_base + lane; default base 0); returns the status tape [K,N,P] and the resampled flags"""
    import torch
    steps = res.x.shape[0]
    g = np.arange(N) if g is None else np.asarray(g, np.int64)
    H, r, nonce = p["H"], p["r"], p["nonce"]
    Lq = pf_ref.factor_q(p["Q"])
    if start is None:
        L0 = to_np(torch.linalg.cholesky(p["P0"]))
        Xs = pf_ref.gaussian_start(SEED, g, nonce, to_np(p["x0"]), L0, P)
        Ss = np.repeat(to_np(p["st0"])[:, None], P, axis=1)
        lw = np.full((N, P), pf_ref.neg_ln(P))
    else:
        Xs, Ss, lw = (to_np(t) for t in start)
    z = to_np(p["z"])
    part, pst, lwt = to_np(res.part_tape), to_np(res.pstatus_tape), to_np(res.lw_tape)
    wqt, anct = to_np(res.wq_tape).astype(np.int64), to_np(res.anc_tape).astype(np.int64)
    ll64, llbar = np.zeros(N), 0.0
    ok = np.ones(N, bool)
    worst = {}

    def hold(key, got, r64, rld):
        b = pf_ref.bar(r64, rld)
        e = pf_ref.scaled(got, r64)
        worst[key] = max(worst.get(key, 0.0), e / b)
        assert e <= b, (name, key, k, e, b)
    rows = np.arange(N)
    for k in range(steps):
        kg = first_step + k
        # -- the prior particles: a K = 1 rollout_states from the N P explicit points, plus the reference's noise
        one = penv.rollout_states(p["acts"][k:k + 1].repeat_interleave(P, dim=1),
                                  state={"x": Xs.reshape(N * P, 12).T, "status": Ss.reshape(N * P)})
        want = to_np(one.x[0]).astype(np.float64).reshape(N, P, 12) + \
            pf_ref.colour(Lq, pf_ref.eps_block(SEED, g, nonce, kg, P))
        if exact:
            assert np.array_equal(_bits(part[k]), _bits(want)), (name, k)
        else:   # float32 storage: rollout_states rounds the stored words to 24 bits, the particles are not rounded
            assert np.all(np.abs(part[k] - want) <= 2.0 ** -23 * np.maximum(1.0, np.abs(want))), (name, k)
        assert np.array_equal(pst[k], to_np(one.status[0]).reshape(N, P)), (name, k)
        # -- the weights, from the previous lw and the device's prior particles
        w64 = pf_ref.weight_step(lw, part[k], H, r, z[k])
        wld = pf_ref.weight_step(lw, part[k], H, r, z[k], dtype=np.longdouble)
        hold("lw", lwt[k], w64["lw"], wld["lw"])
        assert np.array_equal(np.isneginf(lwt[k]), np.isneginf(w64["lw"])), (name, k)
        ll64 = ll64 + w64["loglik"]
        llbar += pf_ref.bar(w64["loglik"], wld["loglik"])
        ok &= ~w64["dead"]
        with np.errstate(invalid="ignore"):
            e = np.where(w64["dead"][:, None], 1.0, np.exp(lwt[k] - lwt[k].max(axis=1, keepdims=True)))
        assert np.all(np.abs(wqt[k] - pf_ref.quantise(e)) <= 1), (name, k)
        assert np.all(wqt[k].max(axis=1) == pf_ref.WQ_ONE), (name, k)
        # -- exact from the integer weights on
        it = pf_ref.integer_step(wqt[k], pf_ref.resample_u(SEED, g, nonce, kg), p["ess_frac"])
        assert np.array_equal(_bits(to_np(res.ess[k])), _bits(it["ess"])), (name, k)
        assert np.array_equal(to_np(res.resampled[k]), it["resampled"]), (name, k)
        assert np.array_equal(anct[k], it["anc"]), (name, k)
        assert np.array_equal(to_np(res.best[k]), it["best"]), (name, k)
        assert np.array_equal(to_np(res.status[k]), pst[k][rows, it["best"]]), (name, k)
        # -- the estimates
        e64 = pf_ref.estimate(part[k], wqt[k])
        eld = pf_ref.estimate(part[k], wqt[k], dtype=np.longdouble)
        hold("x", to_np(res.x[k]), e64[0], eld[0])
        hold("var", to_np(res.var[k]), e64[1], eld[1])
        if k == steps - 1:
            Pd = to_np(res.P)
            hold("P", Pd, e64[2], eld[2])
            assert np.array_equal(_bits(Pd), _bits(np.swapaxes(Pd, 1, 2)))
            assert np.array_equal(_bits(np.diagonal(Pd, axis1=1, axis2=2)), _bits(to_np(res.var[k])))
        # -- the next start
        Xs = np.take_along_axis(part[k], anct[k][:, :, None], axis=1)
        Ss = np.take_along_axis(pst[k], anct[k], axis=1)
        lw = np.where(it["resampled"][:, None], pf_ref.neg_ln(P), lwt[k])
    assert np.array_equal(_bits(to_np(res.part)), _bits(Xs)), name
    assert np.array_equal(to_np(res.pstatus), Ss) and np.array_equal(_bits(to_np(res.lw)), _bits(lw)), name
    e = pf_ref.scaled(to_np(res.loglik), ll64)
    worst["loglik"] = e / llbar
    assert e <= llbar, (name, "loglik", e, llbar)
    assert np.array_equal(to_np(res.ok), ok)
    WORST[name] = worst
    print("%s: worst ratio to the bar " % name + " ".join("%s %.3f" % kv for kv in worst.items()))
    return pst, to_np(res.resampled), wqt


# ---------------------------------------------------------------------------------------------------------------------
# 1. every step, through a touchdown that splits the particles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,substeps", [(64, 1), (128, 1), (256, 10), (512, 10), (1024, 1), (1024, 10)])
def test_every_step_on_the_devices_own_tapes(P, substeps):
    import torch
    rng = np.random.default_rng(900 + P + substeps)
    env = _env("lander3d", N, substeps=substeps)
    penv = _particle_env("lander3d", P, substeps)
    try:
        env.reset()
        before = env.get_state()
        p = _problem(env, "lander3d", rng)
        res = _clone(_run(env, p, P))
        pst, resampled, wq = _check_steps("lander3d P=%d substeps=%d" % (P, substeps), env, penv, p, res, P)
        # both outcomes of the resampling test, a weight of 0, and the straddle of env 1
        assert resampled.any() and not resampled.all()
        assert (wq == 0).any()
        if P >= 256:
            split = [all((pst[k, 1] == s).any() for s in (LANDED, CRASHED, AIRBORNE)) for k in range(K)]
            assert any(split), [[int((pst[k, 1] == s).sum()) for s in (CRASHED, LANDED, 2, AIRBORNE)] for k in range(K)]
        # motors outside [0, 1] were in the tape
        a4 = to_np(p["acts"][:, 4])
        assert (a4 < 0).any() and (a4 > 1).any()
        # a call without tapes gives the same bits elsewhere, and two calls give the same bits
        plain = _run(env, p, P, tape=False)
        assert plain.part_tape is None and plain.anc_tape is None
        for a, b in zip(plain[:12], res[:12]):
            assert torch.equal(a, b)
        for t in _run(env, p, P):                        # the env's buffers: poison them, then run again
            t.fill_(float("nan") if t.dtype.is_floating_point else 1)
        for a, b in zip(_run(env, p, P), res):
            assert torch.equal(a, b)
        # float32 outputs are the float64 ones rounded
        r32 = _run(env, p, P, dtype=torch.float32)
        for nm in ("var", "ess", "P", "loglik"):
            assert getattr(r32, nm).dtype == torch.float32 and torch.equal(getattr(r32, nm), getattr(res, nm).float()), nm
        for nm in ("x", "status", "best", "resampled", "ok", "part", "pstatus", "lw", "wq_tape", "anc_tape"):
            assert torch.equal(getattr(r32, nm), getattr(res, nm)), nm
        after = env.get_state()
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]), equal_nan=True), key
    finally:
        env.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1b. the draws away from global id 0 and from small steps; ess_frac at both ends
# ---------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_global_env_id_up_to_the_last_one():
    """env_id_base = 2^32 - N, the largest cs_create admits: the last lane's id is 2^32 - 1, where pf_ref.words is pinned
    to the host build of pf_noise.h (test_rollout_pf_cpu.py).  Then a shard of two lanes with base + 3: what lanes 3 and
    4 of the whole batch give, bit for bit, whatever the batch size."""
    import torch
    P = 128
    base = 2 ** 32 - N
    rng = np.random.default_rng(941)
    env = _env("lander3d", N, env_id_base=base)
    shard = _env("lander3d", 2, env_id_base=base + 3)
    penv = _particle_env("lander3d", P, 1)
    try:
        env.reset()
        shard.reset()
        p = _problem(env, "lander3d", rng)
        res = _clone(_run(env, p, P))
        _check_steps("lander3d ids from 2^32 - %d" % N, env, penv, p, res, P, g=base + np.arange(N))
        cut = lambda t, lanes_first: (t[3:5] if lanes_first else t[:, 3:5]).contiguous()      # noqa: E731
        p2 = dict(p, acts=cut(p["acts"], False), z=cut(p["z"], False), x0=cut(p["x0"], False), P0=cut(p["P0"], True),
                  st0=cut(p["st0"], True))
        part = _run(shard, p2, P)
        for nm, a, b in zip(res._fields, part, res):
            assert a.shape[0] in (2, K) and b.shape[0] in (N, K), nm
            assert torch.equal(a, cut(b, b.shape[0] == N)), nm
    finally:
        env.close()
        shard.close()
        penv.close()


def test_draws_follow_the_global_step_up_to_the_last_one():
    """first_step = 2^32 - K: the last step's index is 2^32 - 1, the largest cs_rollout_pf admits (the key's (k << 10)
    wraps in 32 bits there, as pf_ref.words restates and the host build of pf_noise.h confirms on the CPU)."""
    import torch
    P = 128
    first = 2 ** 32 - K
    rng = np.random.default_rng(942)
    env = _env("lander3d", N)
    penv = _particle_env("lander3d", P, 1)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        early = _run(env, p, P).part_tape[0].clone()
        res = _clone(_run(env, p, P, first_step=first))
        _check_steps("lander3d steps from 2^32 - %d" % K, env, penv, p, res, P, first_step=first)
        differs = (res.part_tape[0] != early).flatten(1).any(dim=1)
        assert bool(differs.all()), differs.tolist()
    finally:
        env.close()
        penv.close()


def test_ess_frac_zero_never_resamples_and_one_resamples_whenever_the_weights_differ():
    import torch
    P = 64
    rng = np.random.default_rng(943)
    env = _env("lander3d", N)
    penv = _particle_env("lander3d", P, 1)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        at_half = int(_run(env, p, P).resampled.sum())
        p0 = dict(p, ess_frac=0.0)
        res = _clone(_run(env, p0, P))
        _, resampled, _ = _check_steps("lander3d ess_frac=0", env, penv, p0, res, P)
        assert not resampled.any()
        ident = torch.arange(P, dtype=res.anc_tape.dtype, device=env.device).expand(K, N, P)
        assert torch.equal(res.anc_tape, ident)
        p1 = dict(p, ess_frac=1.0)
        res = _clone(_run(env, p1, P))
        _, resampled, _ = _check_steps("lander3d ess_frac=1", env, penv, p1, res, P)
        print("resampled (step, env) pairs of %d: %d at ess_frac 0.5, %d at 1.0" % (K * N, at_half, int(resampled.sum())))
        assert int(resampled.sum()) > at_half
    finally:
        env.close()
        penv.close()


def test_gaussian_start_is_xhat0_plus_l0_eps():
    """a LANDED start under zero process noise and no measurement: the first prior particles ARE the start particles"""
    import torch
    rng = np.random.default_rng(17)
    P = 256
    env = _env("lander3d", N)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        st = torch.full((N,), int(LANDED), dtype=torch.uint8, device=env.device)
        z = torch.full_like(p["z"][:1], float("nan"))
        res = env.rollout_pf(p["acts"][:1], z, p["H"], p["r"], np.zeros(12), p["x0"], p["P0"], particles=P, nonce=5,
                             status0=st, tape=True)
        L0 = to_np(torch.linalg.cholesky(p["P0"]))
        want = pf_ref.gaussian_start(SEED, np.arange(N), 5, to_np(p["x0"]), L0, P)
        want = want + 0.0                                 # (the zero noise is still added: -0.0 becomes +0.0)
        assert np.array_equal(_bits(to_np(res.part_tape[0])), _bits(want))
        assert np.array_equal(_bits(to_np(res.part)), _bits(want))
        assert bool((res.lw_tape[0] == pf_ref.neg_ln(P)).all()) and bool((res.loglik == 0).all())
        assert bool((res.wq_tape == pf_ref.WQ_ONE).all()) and not bool(res.resampled.any())
        # P0 = None: every particle is xhat_0
        res = env.rollout_pf(p["acts"][:1], z, p["H"], p["r"], np.zeros(12), p["x0"], None, particles=P, status0=st,
                             tape=True)
        assert np.array_equal(_bits(to_np(res.part)), _bits(np.repeat(to_np(p["x0"]).T[:, None] + 0.0, P, axis=1)))
        assert bool((res.var == 0).all())
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. shapes and models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,M,P", [("hover3d", 6, 256), ("lander2d", 1, 64), ("hover1d", 12, 1024)])
def test_every_step_for_other_tasks_in_float32_storage(task, M, P):
    rng = np.random.default_rng(zlib.crc32(repr((task, M, P)).encode()))
    env = _env(task, N, "float32")
    penv = _particle_env(task, P, 1, mode="float32")
    try:
        env.reset()
        p = _problem(env, task, rng, M=M)
        res = _clone(_run(env, p, P))
        _check_steps("%s float32 M=%d P=%d" % (task, M, P), env, penv, p, res, P, exact=False)
    finally:
        env.close()
        penv.close()


@pytest.mark.parametrize("variant", ["vehicles", "mars_gyro"])
def test_every_step_under_model_variants(variant):
    rng = np.random.default_rng(zlib.crc32(variant.encode()))
    P = 256
    env = _env("lander3d", N, **model_variants.env_kwargs(variant))
    ref = _env("lander3d", N)
    try:
        installed = model_variants.install(variant, env, rng)
        penv = _particle_env("lander3d", P, 1, variant=variant, installed=installed)
        try:
            env.reset()
            ref.reset()
            p = _problem(env, "lander3d", rng, ah=model_variants.hover(variant))
            res = _clone(_run(env, p, P))
            _check_steps("lander3d %s" % variant, env, penv, p, res, P)
            # the default model gives other particles in every env that flies (0, 1 and 4)
            other = to_np(_run(ref, p, P).part_tape[0])
            same = np.all(_bits(to_np(res.part_tape[0])) == _bits(other), axis=(1, 2))
            assert not same[[0, 1, 4]].any(), same
        finally:
            penv.close()
    finally:
        env.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. missing measurements, a measurement at infinity
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_measurements_are_skipped_and_an_infinite_one_clears_ok():
    import torch
    rng = np.random.default_rng(31)
    P = 256
    env = _env("lander3d", N)
    penv = _particle_env("lander3d", P, 1)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, dense=False, missing=0.3)
        p["z"][3] = float("nan")                         # steps without a measurement for any env
        p["z"][K - 1] = float("nan")
        gone = torch.isnan(p["z"])
        assert 0.15 < float(gone[[0, 1, 2, 4, 5, 6, 7, 8, 9, 10]].double().mean()) < 0.45
        res = _clone(_run(env, p, P))
        _check_steps("lander3d 30% missing", env, penv, p, res, P)
        for k in (3, K - 1):
            prev = torch.where(res.resampled[k - 1][:, None], torch.full_like(res.lw_tape[k], pf_ref.neg_ln(P)),
                               torch.gather(res.lw_tape[k - 1], 1, res.anc_tape[k - 1].long()))
            assert torch.equal(res.lw_tape[k], prev), k
        # ... and those steps add exactly 0: the filter over the first K - 1 steps has the same loglik, bit for bit
        short = env.rollout_pf(p["acts"][:K - 1], p["z"][:K - 1], p["H"], p["r"], p["Q"], p["x0"], p["P0"], particles=P,
                               nonce=p["nonce"], status0=p["st0"])
        assert torch.equal(short.loglik, res.loglik)
        # z = +inf on env 2 at step 5: that env's ok clears, every other env keeps its bits
        p2 = dict(p, z=p["z"].clone())
        p2["z"][5, 2, :] = float("inf")
        bad = _run(env, p2, P)
        assert to_np(bad.ok).tolist() == [True, True, False, True, True] and bool(res.ok.all())
        others = torch.tensor([0, 1, 3, 4], device=env.device)
        for a, b in zip(bad, res):
            sel = (lambda t: t[others]) if a.shape[0] == N else (lambda t: t[:, others])
            assert torch.equal(sel(a), sel(b))
    finally:
        env.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. chunking, N = 1 with K = 1
# ---------------------------------------------------------------------------------------------------------------------
def test_chunked_filter_is_the_single_call_bit_for_bit():
    import torch
    from gym_copter_amd import pf
    rng = np.random.default_rng(51)
    P = 1024
    env = _env("lander3d", N)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, missing=0.1)
        one = _clone(_run(env, p, P))
        for chunk in (5, 1, None):
            got = pf(env, p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], P, nonce=p["nonce"],
                     ess_frac=p["ess_frac"], status0=p["st0"], chunk=chunk)
            for name in one._fields:
                if name != "loglik":
                    assert torch.equal(getattr(got, name), getattr(one, name)), (chunk, name)
            assert torch.allclose(got.loglik, one.loglik, rtol=1e-13, atol=1e-12)
    finally:
        env.close()
    env = _env("lander3d", 1)
    try:
        env.reset()
        z = torch.zeros((1, 1, 2), dtype=torch.float64, device=env.device)
        H = np.zeros((2, 12))
        H[0, 4], H[1, 5] = 1.0, 1.0
        x0 = np.zeros((12, 1))
        x0[4] = -5.0
        res = env.rollout_pf(np.full((1, 1, 4), AH, np.float32), z, H, [0.1, 0.1], np.full(12, 1e-4), x0,
                             0.01 * np.eye(12)[None], particles=64, tape=True)
        assert res.x.shape == (1, 1, 12) and res.part_tape.shape == (1, 1, 64, 12) and bool(res.ok.all())
        assert bool(torch.isfinite(res.x).all()) and int(res.wq_tape.max()) == pf_ref.WQ_ONE
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    rng = np.random.default_rng(72)
    sh = ShardedCopterVecEnv("lander3d", N, device=0, seed=SEED, autoreset_mode="next_step")
    plain = _env("lander3d", N, "float32")
    try:
        sh.reset()
        plain.reset()
        p = _problem(plain, "lander3d", rng)
        a = sh.rollout_pf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], particles=256, nonce=7,
                          status0=p["st0"], tape=True)
        b = _run(plain, p, 256)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib
    rng = np.random.default_rng(74)
    env = _env("lander3d", N)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng)
        base = dict(actions=p["acts"], z=p["z"], H=p["H"], r=p["r"], Q=p["Q"], x0=p["x0"], P0=p["P0"], particles=64,
                    status0=p["st0"])
        first = env.rollout_pf(**base)
        badQ = p["Q"].copy()
        badQ[0, 1] += 1e-9
        nanr = p["r"].copy()
        nanr[0] = np.nan
        for kw, match in ((dict(actions=p["acts"][:, :N - 1]), "actions must have shape"),
                          (dict(z=p["z"][:2]), "z must have shape"), (dict(z=p["z"].cpu()), "z must be on"),
                          (dict(z=p["z"].long()), "z must be a floating-point"),
                          (dict(H=np.zeros((13, 12))), "H must have shape"), (dict(H=p["H"] * np.inf), "H must be finite"),
                          (dict(r=p["r"][:3]), "r must have shape"), (dict(r=-p["r"]), "r must be positive"),
                          (dict(r=nanr), "r must be finite"), (dict(Q=badQ), "Q must be symmetric"),
                          (dict(Q=p["Q"][:6]), "Q must have shape"), (dict(Q=-np.eye(12)), "Q must be positive definite"),
                          (dict(Q=-np.ones(12)), "Q must be >= 0"),
                          (dict(x0=p["x0"][:6]), "x0 must have shape"), (dict(P0=p["P0"][:, :6]), "P0 must have shape"),
                          (dict(P0=-p["P0"]), "P0 must be symmetric positive definite"),
                          (dict(status0=p["st0"][:3]), "status0"), (dict(dtype=torch.float16), "dtype must be"),
                          (dict(particles=96), "particles must be"), (dict(particles=32), "particles must be"),
                          (dict(particles=2048), "particles must be"), (dict(nonce=-1), "nonce must be"),
                          (dict(nonce=1 << 32), "nonce must be"), (dict(first_step=0), "first_step must be"),
                          (dict(ess_frac=1.5), "ess_frac must be"), (dict(start=first), "exactly one start"),
                          (dict(x0=None), "exactly one start"),
                          (dict(x0=None, P0=None, status0=None, start=(first.part, first.pstatus)), "start must be"),
                          (dict(x0=None, P0=None, status0=None, start=first, particles=256), "start part must have shape")):
            args = dict(base)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_pf(**args)
        # the C ABI: a wrong struct_size is CS_ERR_ABI with a live context too
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps = C.sizeof(io), 4
        io.actions_dev, io.start_x_dev, io.start_status_dev = p["acts"].data_ptr(), p["x0"].data_ptr(), p["st0"].data_ptr()
        pio = _lib.RolloutPfIO()
        pio.struct_size = C.sizeof(pio) + 8
        assert env._lib.cs_rollout_pf(env._ctx, C.byref(io), C.byref(pio), None) == _lib.ERR_ABI
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_pf(**base)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_pf(**base)
    f32 = _env("lander3d", N, action_arith="float32")
    try:
        f32.reset()
        with pytest.raises(CopterStepError, match="float32 motor model"):
            f32.rollout_pf(**base)
    finally:
        f32.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the memory contract of tests/test_gpu_output_bounds.py: nothing outside the outputs, every element written, the
#    inputs unchanged
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,dtype", [(64, None), (256, "float32"), (1024, None)])
def test_outputs_are_written_fully_and_nothing_else(P, dtype):
    import torch
    from guarded_outputs import guarded
    rng = np.random.default_rng(95 + P)
    env = _env("lander3d", N)
    try:
        env.reset()
        p = _problem(env, "lander3d", rng, missing=0.2)
        dt = None if dtype is None else getattr(torch, dtype)
        ins = dict(actions=p["acts"], z=p["z"], x0=p["x0"], P0=p["P0"], status0=p["st0"])

        def run(g, call, **inputs):
            g.release()
            g.freeze(**inputs)
            res = call()
            torch.cuda.synchronize()
            g.assert_bands_intact()
            g.assert_fully_written(res)
            g.assert_inputs_unchanged()
            return res
        with guarded(N) as g:
            a = run(g, lambda: _run(env, p, P, tape=False, dtype=dt), **ins)
            assert a.part_tape is None
            b = run(g, lambda: _run(env, p, P, dtype=dt), **ins)
            assert tuple(b.part_tape.shape) == (K, N, P, 12)
            # a carried start from tensors of the caller's own
            start = tuple(t.clone() for t in (b.part, b.pstatus, b.lw))
            run(g, lambda: env.rollout_pf(p["acts"], p["z"], p["H"], p["r"], p["Q"], particles=P, nonce=p["nonce"],
                                          start=start, first_step=K + 1, tape=True, dtype=dt),
                actions=p["acts"], z=p["z"], part=start[0], pstatus=start[1], lw=start[2])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. application
# ---------------------------------------------------------------------------------------------------------------------
def test_hover_tracking_is_calibrated():
    """Hover3D, section 19's sensors and P0, 32 envs, 32 steps, 1 024 particles: the inputs of
    test_rollout_pf_cpu.py::test_application_conditions_hold_on_the_oracle_restatement, which satisfy both conditions on
    the float64 oracle at this seed and nonce (position RMSE 0.055 / 0.053 / 0.062 m against a sensor of 0.1 m; ratios
    0.74 .. 1.22).  The device differs from that run at resampling ties only.  rollout_ekf on the same data: on the CPU
    0.039 / 0.031 / 0.040 m, the particle filter's position RMSE 1.53 x the EKF's; the device may exceed the EKF's by
    that margin plus 25 %."""
    a, x0, xhat0, H, r = pf_ref.app_inputs(AH, seed=1)
    n, P = pf_ref.APP_N, pf_ref.APP_P
    env = _env("hover3d", n, seed=pf_ref.APP_SEED)
    try:
        env.reset()
        acts = _dev(a, env)
        ro = env.rollout_states(acts, state={"x": x0, "status": np.full(n, AIRBORNE, np.uint8)})
        truth = to_np(ro.x).astype(np.float64)
        assert bool((ro.status == AIRBORNE).all())
        z = _dev(pf_ref.app_measurements(truth, H, r), env)
        P0 = _dev(np.repeat(ekf_ref.APP_P0[None], n, axis=0), env)
        res = env.rollout_pf(acts, z, H, r, pf_ref.APP_Q, _dev(xhat0, env), P0, particles=P, nonce=pf_ref.APP_NONCE)
        assert bool(res.ok.all())
        rmse, ratio = pf_ref.app_conditions(to_np(res.x[-1]), to_np(res.var[-1]), truth[-1])
        filt = env.rollout_ekf(acts, z, H, r, ekf_ref.APP_Q, _dev(xhat0, env), P0)
        ekf_rmse = np.sqrt(np.mean((to_np(filt.x[-1]) - truth[-1]) ** 2, axis=0))
        margin = pf_ref.position_rmse(rmse) / pf_ref.position_rmse(ekf_rmse)
        print("pf rmse %s ratio %s\nekf rmse %s\nposition rmse pf / ekf %.3f" % (np.round(rmse, 4), np.round(ratio, 2),
                                                                              np.round(ekf_rmse, 4), margin))
        assert margin <= pf_ref.APP_CPU_MARGIN * 1.25, margin
    finally:
        env.close()
