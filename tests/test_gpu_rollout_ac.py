"""cs_rollout_actor_critic / cs_gae on the GPU: the transitions against a twin env stepped with
the returned action tape (step_many), the live mask against the rule stated from the twin's flags; the deterministic
policy against the unchanged rollout_mlp_states, the means and values against the float64 policy; the noise, the
log-probabilities and the advantages against tests/ppo_ref.py; the ppo driver; plumbing.  The code under test is never
its own reference."""
import zlib

import numpy as np
import pytest

import model_variants
import ppo_ref
from gpu_util import have_gpu, to_np
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

TASK_SHAPE = {"lander3d": (10, 4), "hover3d": (12, 4), "lander2d": (6, 2), "hover1d": (2, 1), "lander1d": (2, 1),
              "hover2d": (6, 2)}
AH = hover_action()
U32 = 2.0 ** -24


def _env(task, n, mode="float32", autoreset="next_step", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _low_starts(n, rng):
    """Low starts after tests/test_gpu_rollout_es.py's recipe: 0.05-0.9 m up and descending at up to 4 m/s.  Chosen on the
    CPU oracle (oracle.refvec.VecOracle under hover thrust with 0.003 of noise): within K = 24 steps (0.24 s, up to
    0.96 m of descent) 40-50 % of the lanes touch down or crash and end their episode, the others stay up -- on every task
    used here; with 1.2 m the share was 29-34 %, too near the 25 % asserted on the twin's tapes where this is used."""
    x = np.empty((12, n))
    x[0], x[2] = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    x[1], x[3] = rng.uniform(-2, 2, (2, n))
    x[4] = rng.uniform(-0.9, -0.05, n)
    x[5] = rng.uniform(0.0, 4.0, n)
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    x[10] = rng.uniform(-1, 1, n)
    x[7], x[9], x[11] = rng.uniform(-1, 1, (3, n))
    return x


def _policy(task, H, Hv, seed, env, bias=AH, sigma=0.003, scale=0.005):
    """An actor near hover (the hover motor value, 0.0166 for the default vehicle, as its output bias; output weights and
    a default sigma that are small against it: the env clips the motors at 0, so noise of the hover value's own size
    raises the mean thrust and nobody comes down), a critic of nn.Linear-sized draws, and log_std = ln(sigma) spread
    +-10 % over the components."""
    import torch
    from gym_copter_amd import mlp
    od, A = TASK_SHAPE[task]
    gen = torch.Generator().manual_seed(seed)
    actor = mlp.init(od, A, H, generator=gen, out_bias=float(bias), out_scale=scale).to(env.device)
    critic = mlp.init(od, 1, Hv, generator=gen).to(env.device)
    log_std = torch.log(torch.tensor([sigma * (0.9 + 0.2 * c / max(A - 1, 1)) for c in range(A)], dtype=torch.float64))
    return actor, critic, log_std.to(torch.float32).to(env.device)


def _clone(roll):
    return type(roll)(*(None if t is None else t.clone() for t in roll))


def _install_low_starts(envs, rng, pending_share=0.0):
    """reset(), then the same low starts in every env of `envs` through set_state (the perturbation of reset() stays
    pending); with pending_share, that share of the lanes gets a NEXT_STEP reset pending (flags bit 1)."""
    n = envs[0].num_envs
    x = _low_starts(n, rng)
    pend = rng.uniform(size=n) < pending_share
    for e in envs:
        e.reset()
        s = e.get_state()
        flags = (s["flags"] | np.where(pend, 2, 0)).astype(np.uint8)
        e.set_state(x=x, status=np.full(n, AIRBORNE, np.uint8), flags=flags)
    return pend


def _states_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _check_against_twin(name, env, twin, roll, pending0, next_step, rng, expect_events):
    """The twin, fed the returned action tape through step_many, gives torch.equal observations (rows 1..K), reward and
    both flags; the live mask is ppo_ref.live of the TWIN's flags; the stored states are equal afterwards and three
    further step()s agree."""
    import torch
    K, n = roll.reward.shape
    obs0 = to_np(twin.state_tensors()["x"]).T.copy()
    first, od = {10: (0, 10), 12: (0, 12), 6: (2, 6), 2: (4, 2)}[roll.obs.shape[2]]
    tobs, trew, tterm, ttrunc = (t.clone() for t in twin.step_many(roll.actions))
    assert torch.equal(roll.obs[1:], tobs), name
    assert torch.equal(roll.reward, trew), name
    assert torch.equal(roll.terminated, tterm) and torch.equal(roll.truncated, ttrunc), name
    # row 0: the stored state's observation (the state tensors carry the stored value rounded to float32)
    assert np.array_equal(to_np(roll.obs[0]), obs0[:, first:first + od]), name
    done = to_np(tterm | ttrunc)
    want_live = ppo_ref.live(to_np(tterm), to_np(ttrunc), pending0, next_step)
    assert np.array_equal(to_np(roll.live), want_live), name
    ended = done.any(0)
    print("%s: %.0f %% of the lanes end an episode within K = %d, %.0f %% do not; terminated %d, truncated %d; reset "
          "steps %d" % (name, 100 * ended.mean(), K, 100 * (~ended).mean(), int(to_np(tterm).sum()),
                        int(to_np(ttrunc).sum()), int((~want_live).sum())))
    if expect_events and K > 1:
        assert ended.mean() >= 0.25 and (~ended).mean() >= 0.25, (name, float(ended.mean()))
        if next_step:
            assert (~want_live[1:]).any(), name
    _states_equal(env.get_state(), twin.get_state())
    A = roll.actions.shape[2]
    for _ in range(3):
        a = _dev(rng.uniform(0, 1, (n, A)).astype(np.float32), env)
        for u, v in zip(env.step(a)[:4], twin.step(a)[:4]):
            assert torch.equal(u, v), name


# ---------------------------------------------------------------------------------------------------------------------
# 1. transitions: the env advances exactly as under step_many with the same actions
# ---------------------------------------------------------------------------------------------------------------------
TRANSITIONS = [
    # task, mode, autoreset, substeps, variant, n, H, Hv
    ("lander3d", "float32", "next_step", 1, None, 256, 32, 16),
    ("lander3d", "float32", "same_step", 1, None, 200, 64, 0),
    ("lander3d", "float32_rn", "next_step", 1, None, 200, 0, 16),
    ("lander3d", "float32_rn", "same_step", 1, None, 256, 1, 0),
    ("lander3d", "float64", "next_step", 1, None, 256, 64, 16),
    ("lander3d", "float64", "same_step", 1, None, 200, 32, 0),
    ("hover3d", "float32", "next_step", 1, None, 256, 32, 16),
    ("lander2d", "float32", "next_step", 10, None, 200, 1, 0),
    ("hover1d", "float32", "same_step", 1, None, 256, 0, 16),
    ("lander3d", "float32", "next_step", 1, "mars_gyro", 256, 32, 16),
    ("lander3d", "float64", "same_step", 1, "vehicles", 200, 64, 0),
]


@pytest.mark.parametrize("case", TRANSITIONS, ids=lambda c: "-".join(str(v) for v in c))
def test_transitions_equal_a_twin_fed_the_action_tape(case):
    """Low stored starts (a share of the lanes with a NEXT_STEP reset pending at the call's start), K = 24 and then
    K = 1 on the same env, sampled actions at sigma = 0.003 (small against the hover motor value)."""
    task, mode, autoreset, substeps, variant, n, H, Hv = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    kw = dict(model_variants.env_kwargs(variant), seed=5, substeps=substeps)
    env, twin = _env(task, n, mode, autoreset, **kw), _env(task, n, mode, autoreset, **kw)
    try:
        installed = model_variants.draw(variant, rng, n)
        for e in (env, twin):
            model_variants.install_same(e, installed)
        next_step = autoreset == "next_step"
        pend = _install_low_starts((env, twin), rng, pending_share=0.125 if next_step else 0.0)
        assert not next_step or pend.sum() >= n // 16
        actor, critic, log_std = _policy(task, H, Hv, 3, env, bias=model_variants.hover(variant))
        for K, nonce in ((24, 1), (1, 2)):
            pending0 = (env.get_state()["flags"] & 2) != 0
            roll = _clone(env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=nonce))
            assert tuple(roll.obs.shape) == (K + 1, n, TASK_SHAPE[task][0]) and tuple(roll.values.shape) == (K + 1, n)
            assert roll.means is None and tuple(roll.logp.shape) == tuple(roll.live.shape) == (K, n)
            _check_against_twin("%s K %d" % ("-".join(str(v) for v in case), K), env, twin, roll, pending0, next_step,
                                rng, expect_events=True)
    finally:
        env.close()
        twin.close()


@pytest.mark.parametrize("truncates", [True, False])
def test_transitions_with_a_time_limit_inside_the_horizon(truncates):
    """A step limit of 10 inside K = 24: every lane still flying then is truncated (or, without time_limit_truncates,
    terminated), resets in the next step and flies on."""
    n, K, H, Hv = 200, 24, 32, 16
    rng = np.random.default_rng(78 + truncates)
    kw = dict(seed=8, max_steps=10, time_limit_truncates=truncates)
    env, twin = _env("lander3d", n, "float32", "next_step", **kw), _env("lander3d", n, "float32", "next_step", **kw)
    try:
        _install_low_starts((env, twin), rng)
        actor, critic, log_std = _policy("lander3d", H, Hv, 4, env)
        pending0 = (env.get_state()["flags"] & 2) != 0
        roll = _clone(env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=3))
        _check_against_twin("time limit, truncates %s" % truncates, env, twin, roll, pending0, True, rng,
                            expect_events=False)
        flag = to_np(roll.truncated if truncates else roll.terminated)
        assert flag.any(0).mean() >= 0.25                                      # the limit is met inside the horizon
        assert truncates or not to_np(roll.truncated).any()
        assert (to_np(roll.terminated) | to_np(roll.truncated)).any(0).all()   # nobody flies K steps without an end
    finally:
        env.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the policy: the deterministic form against rollout_mlp_states, means and values against the float64 policy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,H,Hv,n", [("lander3d", 0, 0, 256), ("lander3d", 1, 16, 200), ("lander3d", 32, 16, 256),
                                         ("lander3d", 64, 0, 200), ("lander2d", 32, 16, 256)])
def test_deterministic_policy_equals_rollout_mlp_states_and_the_float64_policy(task, H, Hv, n):
    import torch
    from gym_copter_amd import mlp
    from test_gpu_rollout_mlp import _action_bound
    K = 24
    od, A = TASK_SHAPE[task]
    rng = np.random.default_rng(zlib.crc32(repr((task, H, Hv, n)).encode()))
    env = _env(task, n, "float32", "disabled", seed=6)
    try:
        _install_low_starts((env,), rng)
        actor, critic, log_std = _policy(task, H, Hv, 5, env)
        ref = env.rollout_mlp_states(actor, K, H)                       # (unchanged by this feature; writes no state)
        ref = type(ref)(*(t.clone() for t in ref))
        roll = _clone(env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, deterministic=True, means=True))
        done = to_np(ref.terminated | ref.truncated)
        d = np.where(done.any(0), done.argmax(0) + 1, K)                # the first done step, 1-based
        upto = torch.from_numpy(np.arange(K)[:, None] < d[None, :]).to(env.device)
        assert (d < K).mean() >= 0.25 and (d == K).mean() >= 0.25
        assert torch.equal(roll.actions[upto], ref.actions[upto]) and torch.equal(roll.obs[:-1][upto], ref.obs[upto])
        assert torch.equal(roll.actions, roll.means) and roll.live.all()
        # logp of a = mu: -sum log_std - (A/2) ln 2 pi, the float64 value rounded once
        ls = to_np(log_std).astype(np.float64)
        want = np.float32((-0.0 - ls.sum()) - A * 0.5 * np.log(2 * np.pi))
        assert np.all(np.abs(to_np(roll.logp).astype(np.float64) - float(want)) <= 2 * U32 * max(1.0, abs(float(want))))
        # means and values (row K too) against the float64 policy on the returned observations
        obs = to_np(roll.obs)
        for params, hidden, act_dim, got in ((actor, H, A, to_np(roll.means)), (critic, Hv, 1, to_np(roll.values)[..., None])):
            o = obs[:got.shape[0]]
            want = mlp.forward64(params.cpu(), torch.from_numpy(o), hidden, act_dim).numpy()
            bound = _action_bound(params.cpu().numpy(), hidden, o, act_dim) + U32 * np.abs(want)
            err = np.abs(got.astype(np.float64) - want)
            assert got.shape == want.shape and np.all(err <= bound), (hidden, float(np.max(err - bound)))
        assert to_np(roll.values).shape == (K + 1, n)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. sampling: the noise reconstructed from the tapes, the log-probabilities
# ---------------------------------------------------------------------------------------------------------------------
# |eps32 - eps64| per unit of max(R, 1): 4 x the worst measured -- the host build's 4.2e-7 (tests/test_rollout_ac_cpu.py,
# 2^20 draws) and the device run's 3.8e-7 beyond the reconstruction's own error (_check_noise prints it; DESIGN.md
# section 17): the larger of the two
EPS_BAR = 4 * 4.2e-7


def _check_noise(name, roll, log_std, seed, nonce, g0):
    """(a - mu) / sigma from the tapes against ppo_ref.noise.  Reconstructing eps from float32 tapes has an error of its
    own, allowed for beside EPS_BAR: a = fl32(mu + fl32(sigma eps)) rounds the product (u |eps|) and the sum (u |a| /
    sigma), and sigma = expf(log_std) is a few ulp off exp (3 u |eps| taken)."""
    a, mu = to_np(roll.actions).astype(np.float64), to_np(roll.means).astype(np.float64)
    K, n, A = a.shape
    sigma = np.exp(to_np(log_std).astype(np.float64))
    got = (a - mu) / sigma
    g = (g0 + np.arange(n))[None, :, None]
    k = np.arange(1, K + 1)[:, None, None]
    c = np.arange(A)[None, None, :]
    want = ppo_ref.noise(seed, g, nonce, k, c)
    r = ppo_ref.noise_radius(seed, g, nonce, k, c)
    recon = U32 * (np.abs(a) + np.abs(mu)) / sigma + 4 * U32 * np.abs(want)
    err = np.abs(got - want)
    unit = (err - recon).clip(min=0) / np.maximum(r, 1.0)
    print("%s: eps error beyond the reconstruction's %.3e of max(R, 1) (bar %.3e); raw worst %.3e"
          % (name, unit.max(), EPS_BAR, err.max()))
    assert np.all(err <= EPS_BAR * np.maximum(r, 1.0) + recon), (name, float(unit.max()))
    return got


@pytest.mark.parametrize("sigma", [0.05, 1.5])
def test_noise_and_logp_match_the_reference(sigma):
    import torch
    seed, nonce, K, H, Hv = 17, (1 << 32) - 1, 24, 32, 16
    rng = np.random.default_rng(int(sigma * 100))
    env = _env("lander3d", 256, "float32", "next_step", seed=seed, env_id_base=256)
    big = _env("lander3d", 512, "float32", "next_step", seed=seed)
    try:
        _install_low_starts((env,), rng)
        big.reset()
        actor, critic, log_std = _policy("lander3d", H, Hv, 6, env, sigma=sigma)
        s0 = env.get_state()
        roll = _clone(env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=nonce, means=True))
        eps = _check_noise("sigma %g, N 256 at id base 256" % sigma, roll, log_std, seed, nonce, 256)
        assert abs(eps.mean()) < 0.05 and abs(eps.std() - 1) < 0.05
        # the second half of N = 512, addressed by global id: the same draws
        rb = big.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=nonce, means=True)
        half = type(rb)(*(None if t is None else t[:, 256:] for t in rb))
        _check_noise("sigma %g, second half of N 512" % sigma, half, log_std, seed, nonce, 256)
        # logp against the float64 formula on the float32 tapes: 100 x float64's own distance from longdouble, floored
        # at 4 float32 ulp of the value's scale (it is stored as float32)
        a, mu, ls = to_np(roll.actions), to_np(roll.means), to_np(log_std)
        want = ppo_ref.logp(a, mu, ls)
        own = np.abs(want - ppo_ref.logp(a, mu, ls, np.longdouble)).astype(np.float64)
        bar = np.maximum(100 * own, 4 * U32 * np.maximum(np.abs(want), 1.0))
        err = np.abs(to_np(roll.logp).astype(np.float64) - want)
        print("sigma %g: logp error worst %.3e, worst bar %.3e, float64's own distance %.3e" % (sigma, err.max(), bar.max(), own.max()))
        assert np.all(err <= bar), float((err - bar).max())
        # the same state and nonce again: every output bit for bit; another K: the same first steps
        env.set_state(**s0)
        again = _clone(env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=nonce, means=True))
        for u, v in zip(roll, again):
            assert torch.equal(u.view(torch.uint8), v.view(torch.uint8))
        env.set_state(**s0)
        short = env.rollout_actor_critic(actor, critic, log_std, 7, H, Hv, nonce=nonce, means=True)
        assert torch.equal(short.actions, roll.actions[:7]) and torch.equal(short.obs, roll.obs[:8])
        assert torch.equal(short.logp, roll.logp[:7]) and torch.equal(short.values, roll.values[:8])
        # another nonce, another seed: other noise
        env.set_state(**s0)
        other = env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=nonce - 1, means=True)
        assert torch.equal(other.means[0], roll.means[0]) and (other.actions[0] == roll.actions[0]).float().mean() < 0.01
        env.seed(seed + 1)
        env.set_state(**s0)
        other = env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=nonce, means=True)
        assert torch.equal(other.means[0], roll.means[0]) and (other.actions[0] == roll.actions[0]).float().mean() < 0.01
    finally:
        env.close()
        big.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the advantages
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n", [(1, 200), (1, 256), (24, 200), (24, 256)])
def test_gae_equals_the_reference_bit_for_bit(K, n):
    import torch
    rng = np.random.default_rng(K * 1000 + n)
    env = _env("lander3d", n, "float32", "next_step", seed=1)
    try:
        r = (rng.standard_normal((K, n)) * 10).astype(np.float32)
        v = (rng.standard_normal((K + 1, n)) * 20).astype(np.float32)
        term, trunc = rng.uniform(size=(K, n)) < 0.2, rng.uniform(size=(K, n)) < 0.15
        assert (term | trunc).mean() >= 0.25 and (term | trunc).any(1).all()
        flags = _dev(np.stack([term, trunc], axis=2).astype(np.uint8), env)
        forms = ((flags[:, :, 0].view(torch.bool), flags[:, :, 1].view(torch.bool)),      # interleaved, read in place
                 (_dev(term, env), _dev(trunc.astype(np.uint8), env)))                      # two plain arrays
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
            want = ppo_ref.gae(r, v, term, trunc, gamma, lam)
            for t, u in forms:
                adv, ret = env.gae(_dev(r, env), _dev(v, env), t, u, gamma, lam)
                first = (adv.clone(), ret.clone())
                for got, w in zip(first, want):
                    assert got.dtype == torch.float32 and tuple(got.shape) == (K, n)
                    assert np.array_equal(to_np(got).view(np.uint32), w.view(np.uint32)), (K, n, gamma, lam)
                adv.fill_(float("nan"))
                ret.fill_(float("nan"))                                           # written, not accumulated
                again = env.gae(_dev(r, env), _dev(v, env), t, u, gamma, lam)
                assert again[0].data_ptr() == adv.data_ptr()
                assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    finally:
        env.close()


def test_gae_on_the_collection_tapes():
    """gae on what rollout_actor_critic returned (the interleaved flags read in place) against ppo_ref.gae."""
    n, K, H, Hv = 200, 24, 32, 16
    rng = np.random.default_rng(9)
    env = _env("lander3d", n, "float32", "next_step", seed=4)
    try:
        _install_low_starts((env,), rng)
        actor, critic, log_std = _policy("lander3d", H, Hv, 8, env)
        roll = env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=5)
        adv, ret = env.gae(roll.reward, roll.values, roll.terminated, roll.truncated)
        want = ppo_ref.gae(to_np(roll.reward), to_np(roll.values), to_np(roll.terminated), to_np(roll.truncated), 0.99,
                           0.95)
        assert to_np(roll.terminated | roll.truncated).any()
        assert np.array_equal(to_np(adv).view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(to_np(ret).view(np.uint32), want[1].view(np.uint32))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the driver
# ---------------------------------------------------------------------------------------------------------------------
DRIVER = dict(task="lander3d", n=8192, K=64, H=16, Hv=16, iterations=30, sigma0=0.1, lr=3e-4)


def driver_problem():
    """Lander3D from reset() under next_step auto-reset.  The initial policy: mlp.init with the hover motor value as its
    output bias and an output layer scaled by 0.01, as tests/test_gpu_rollout_es.py's; an untrained critic."""
    import torch
    from gym_copter_amd import mlp
    gen = torch.Generator().manual_seed(11)
    actor0 = mlp.init(10, 4, DRIVER["H"], generator=gen, out_bias=float(AH), out_scale=0.01)
    critic0 = mlp.init(10, 1, DRIVER["Hv"], generator=gen, out_scale=0.01)
    log_std0 = torch.full((4,), float(np.log(DRIVER["sigma0"])), dtype=torch.float32)
    return actor0, critic0, log_std0


def evaluate(actor, critic, log_std, calls=16):
    """Mean reward per live step of a policy on a FRESH env of the driver's size and seed: `calls` collections of K
    steps from reset(), sampled actions, nonces apart from the driver's."""
    d = DRIVER
    env = _env(d["task"], d["n"], "float32", "next_step", seed=2, max_steps=1000)
    try:
        env.reset()
        total, count = 0.0, 0.0
        for j in range(calls):
            roll = env.rollout_actor_critic(actor.to(env.device), critic.to(env.device), log_std.to(env.device), d["K"],
                                            d["H"], d["Hv"], nonce=100000 + j)
            live = roll.live.float()
            total += float((roll.reward * live).sum())
            count += float(live.sum())
        return total / count
    finally:
        env.close()


# The improvement of the mean reward per live step of the final policy over the initial one, both on a fresh env, measured
# on an MI355X with these settings (profiles/ppo_driver_path.txt): -55.02 -> -1.74.  The bar is half
# of it: the minibatch permutations and Adam's path make the endpoint vary.
DRIVER_MEASURED = -1.7406 - (-55.0222)


def test_ppo_driver():
    """gym_copter_amd.ppo on Lander3D: 8 192 envs, K = 64, H = Hv = 16, 30 iterations.  Mechanics: every loss finite,
    the ratio 1 within float32 at the first minibatch of every iteration, the live-masked sample count what the flags
    say; and the mean reward per live step of the final policy on a fresh env against the INITIAL policy's there.

    The ratio's bar is reasoned: torch recomputes mu in float32 in another summation order, |d mu| <= (OBS + H + 2) u x
    the sum of the terms' magnitudes (about 2) = 3.4e-6; logp moves by |z| |d mu| / sigma <= 5.9 x 3.4e-6 / 0.05 = 4e-4
    for sigma >= 0.05, plus the float32 rounding of logp itself (|logp| <= 40: 2.4e-6): 1e-3 taken."""
    import gym_copter_amd
    from gym_copter_amd.ppo import STATS
    d = DRIVER
    actor0, critic0, log_std0 = driver_problem()
    before = evaluate(actor0, critic0, log_std0)
    env = _env(d["task"], d["n"], "float32", "next_step", seed=2, max_steps=1000)
    try:
        env.reset()
        res = gym_copter_amd.ppo(env, actor0, critic0, log_std0, d["H"], d["Hv"], d["K"], d["iterations"], lr=d["lr"])
    finally:
        env.close()
    stats = to_np(res.stats).astype(np.float64)
    col = {k: stats[:, i] for i, k in enumerate(STATS)}
    after = evaluate(res.actor, res.critic, res.log_std)
    print("ppo driver: mean reward per live step on a fresh env, initial policy %.4f, after %d iterations %.4f; sigma %s"
          % (before, d["iterations"], after, np.exp(to_np(res.log_std)).round(4).tolist()))
    print("iteration: mean reward per live step | live samples | first-minibatch |ratio - 1| | policy loss | value loss"
          " | done rate")
    for t in range(stats.shape[0]):
        print("%3d %10.4f %8d %.3e %+.4e %.4e %.5f" % (t, col["mean_reward_per_live_step"][t], col["live_samples"][t],
                                                      col["first_ratio_error"][t], col["policy_loss"][t],
                                                      col["value_loss"][t], col["done_rate"][t]))
    assert stats.shape == (d["iterations"], len(STATS)) and np.isfinite(stats).all()
    assert np.array_equal(to_np(res.history), to_np(res.stats)[:, 0])
    assert col["first_ratio_error"].max() <= 1e-3, float(col["first_ratio_error"].max())
    # live = 1 - (the step before ended an episode): K N minus the ends, up to the ends of a call's last step and the
    # resets pending at its start (at most N each)
    total = d["K"] * d["n"]
    assert np.all(col["live_samples"] <= total)
    assert np.all(np.abs(total - col["live_samples"] - col["done_rate"] * total) <= d["n"])
    for got, start in ((res.actor, actor0), (res.critic, critic0), (res.log_std, log_std0)):
        assert tuple(got.shape) == tuple(start.shape) and not np.array_equal(to_np(got), to_np(start))
    assert after - before >= 0.5 * DRIVER_MEASURED, (before, after)


# ---------------------------------------------------------------------------------------------------------------------
# 6. plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    from gym_copter_amd import CopterStepError
    n, K, H, Hv = 128, 4, 8, 16
    env = _env("lander3d", n, "float64", "next_step", seed=1)
    try:
        env.reset()
        before = env.get_state()
        actor, critic, log_std = _policy("lander3d", H, Hv, 2, env)
        good = dict(actor=actor, critic=critic, log_std=log_std, K=K, hidden=H, critic_hidden=Hv)
        for kw, match in ((dict(K=0), "K must be"), (dict(K=2.0), "K must be"), (dict(hidden=65), "hidden must be"),
                          (dict(hidden=9), "actor must be"), (dict(critic_hidden=8), "critic must be"),
                          (dict(critic_hidden=-1), "hidden must be"), (dict(actor=actor.double()), "actor must be"),
                          (dict(actor=to_np(actor)), "actor must be"), (dict(log_std=log_std[:3]), "log_std must be"),
                          (dict(nonce=-1), "nonce must be"), (dict(nonce=1 << 32), "nonce must be")):
            args = dict(good)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_actor_critic(**args)
        _states_equal(before, env.get_state())                                 # refused before any launch
        roll = env.rollout_actor_critic(actor, None, log_std, 1, H)           # K = 1, no critic
        assert roll.values is None and roll.means is None and tuple(roll.obs.shape) == (2, n, 10)
        r = torch.zeros((K, n), device=env.device)
        v = torch.zeros((K + 1, n), device=env.device)
        f = torch.zeros((K, n), dtype=torch.bool, device=env.device)
        for args, match in (((r, v[:K], f, f), "values must have shape"), ((r.double(), v, f, f), "reward must be"),
                            ((r, v, f[:1], f), "terminated must be"), ((r, v, f, f.float()), "truncated must be"),
                            ((r.cpu(), v, f, f), "reward must be")):
            with pytest.raises(ValueError, match=match):
                env.gae(*args)
        for kw in (dict(gamma=float("nan")), dict(lam=1e39), dict(gamma=1e30, lam=1e30)):
            with pytest.raises(ValueError, match="gamma and lam"):
                env.gae(r, v, f, f, **kw)
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_actor_critic(**good)
            with pytest.raises(CopterStepError, match="serv"):
                env.gae(r, v, f, f)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_actor_critic(**good)
    with pytest.raises(RuntimeError, match="closed"):
        env.gae(r, v, f, f)
