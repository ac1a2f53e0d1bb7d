"""cs_rollout_actor_critic's bookkeeping around advance() on the GPU: the running episode return,
the tick counter and the episode counter through several collections on the SAME env, so that what one launch stores the
next one loads; the lean and the full-featured form of the kernel on the same inputs; the whole-episode register across
2^E, 2^(E+1) and 2^32; the lander1d and hover2d instantiations.

Every case has two references, never the code under test itself: (a) a twin env of the same configuration fed the
returned action tape through step_many (tests/test_gpu_rollout_ac.py: _check_against_twin), and (b) where the oracle has
the model, oracle.refvec.VecOracle in the same storage mode, mirrored field by field from get_state() before the first
launch and stepped with the returned action tape.  The running return is also restated exactly from the device's own
reward and flag tapes.

Lanes leave the oracle comparisons only by a rule that uses the reference alone: a second VecOracle in float64 storage
runs on the same starts and tape, and a lane whose flag tapes differ between the two oracle runs straddles a threshold.
At most 2 % of the lanes (asserted); the twin comparison never leaves a lane out."""
import collections
import zlib

import numpy as np
import pytest

import model_variants
import ppo_ref
from gpu_util import (AUTORESET, MODE_TOL, assert_state_close, assert_step_close, device_episode_bits, have_gpu,
                      make_pair, reward_limit, to_np)
from oracle import refvec
from oracle.refcpu import TaskParams
from oracle.refvec import VecOracle
from test_gpu_rollout_ac import _check_against_twin, _clone, _env, _install_low_starts, _policy, _states_equal

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

U32 = 2.0 ** -24
SEED = 5
LAUNCHES = ((7, 1), (24, 2), (1, 3), (12, 4))          # (K, nonce) of the four collections on the same env
X_TOL, R_ABS = 2e-6, "auto"                            # test_episode_counter_crosses_its_boundaries_...'s tolerances
TAPES = ("obs", "actions", "logp", "values", "reward", "terminated", "truncated", "live")

Case = collections.namedtuple("Case", "task mode autoreset substeps variant stats ticks extra oracle n H Hv start_seed")
TRUNC = (("max_steps", 10), ("time_limit_truncates", True))
CASES = [
    # task, mode, autoreset, substeps, variant, episode_stats, track_time, further keywords, oracle, n, H, Hv, start seed
    Case("lander3d", "float32", "next_step", 1, None, True, False, (), True, 256, 32, 16, 0),
    Case("lander3d", "float32", "next_step", 1, None, False, True, (), True, 256, 32, 16, 20),
    Case("lander3d", "float32", "same_step", 1, None, True, True, (), True, 200, 64, 0, 13),
    Case("lander3d", "float64", "next_step", 4, None, True, True, (), True, 256, 32, 16, 2),
    Case("lander3d", "float32_rn", "next_step", 1, None, True, True, TRUNC, True, 200, 0, 16, 0),
    Case("hover3d", "float32", "next_step", 1, None, True, True, (), True, 256, 32, 16, 0),
    Case("lander1d", "float32", "same_step", 1, None, False, False, (), True, 200, 1, 0, 0),
    Case("lander1d", "float32", "next_step", 1, None, False, False, (), True, 256, 32, 16, 0),   # the lean instantiation
    Case("lander1d", "float32", "next_step", 1, None, True, True, (), True, 256, 32, 16, 1),
    Case("hover2d", "float32_rn", "next_step", 1, None, False, False, (), True, 200, 32, 16, 0),  # lean too
    Case("hover2d", "float64", "same_step", 1, None, True, True, (), True, 256, 64, 0, 2),
    Case("lander3d", "float32", "next_step", 1, "vehicles_mars_gyro", True, True, (), True, 256, 32, 16, 1),
    Case("lander3d", "float32", "next_step", 1, "act_f32", True, True, (), False, 200, 32, 16, 13),
    Case("lander3d", "float32", "next_step", 1, "gyro_only", True, True, (), False, 256, 1, 16, 0),
]


def _name(case):
    return "-".join(str(v) for v in case[:5]) + ("-stats" if case.stats else "") + ("-ticks" if case.ticks else "") + \
        "".join("-%s=%s" % kv for kv in case.extra) + "-n%d" % case.n


def _env_kwargs(case):
    kw = dict(model_variants.env_kwargs(case.variant), seed=SEED, substeps=case.substeps, **dict(case.extra))
    if case.stats:
        kw["episode_stats"] = True
    if case.ticks:
        kw["track_time"] = True
    return kw


def _prepare(case, envs):
    """The per-env model of the variant, then the low starts (under next_step an eighth of the lanes with a reset
    pending), the same in every env of `envs`.  The starts' generator is seeded by the case's name and its start seed."""
    rng = np.random.default_rng([zlib.crc32(_name(case).encode()), case.start_seed])
    installed = model_variants.draw(case.variant, rng, case.n)
    for e in envs:
        model_variants.install_same(e, installed)
    next_step = case.autoreset == "next_step"
    pend = _install_low_starts(envs, rng, pending_share=0.125 if next_step else 0.0)
    assert not next_step or pend.sum() >= case.n // 16
    return rng, installed


def _oracle(case, mode, installed):
    extra = dict(case.extra)
    tp = TaskParams(max_steps=extra.get("max_steps", 100000))             # (_env's default step limit)
    return VecOracle(case.task, case.n, tp, substeps=case.substeps, store_mode=mode, autoreset=AUTORESET[case.autoreset],
                     seed=SEED, time_limit_truncates=bool(extra.get("time_limit_truncates", False)),
                     **model_variants.oracle_model(case.variant, installed))


def _mirror(orc, st):
    """The env's stored state into the oracle, field by field, as test_single_step_random_states mirrors one."""
    orc.x[:] = orc._round(st["x"])
    orc.status[:] = st["status"]
    orc.steps[:] = st["steps"]
    orc.prev_shaping[:] = st["prev_shaping"].astype(orc.T)
    orc.force[:] = st["force"].astype(orc.T)
    orc.pending[:] = (st["flags"] & 1) != 0
    orc.done_pending[:] = (st["flags"] & 2) != 0
    orc.episode[:] = st["episode"]
    orc.ticks[:] = st.get("ticks", 0)
    orc.ep_return[:] = st.get("episode_return", 0.0)


def _reset_masks(term, trunc, pending0, next_step):
    """(before, after) [K,N]: the lanes whose episode restarts in step k before the step's reward is taken (next_step:
    the reset step replaces the step, oracle/refvec.py: step -- `resetting` lanes are not live -- and _reset_lanes zeroes
    ep_return) and after it (same_step: `fin` lanes are reset at the end of the step that finished them)."""
    done = term | trunc
    if next_step:
        return ~ppo_ref.live(term, trunc, pending0, True), np.zeros_like(done)
    return np.zeros_like(done), done


class _Running:
    """Per lane, of the running episode: the float32 return restated from the device's tapes, the number m of rewards in
    it, sum |r_k| and the sum of the per-step reward tolerances against the oracle."""

    def __init__(self, n):
        self.ret = np.zeros(n, np.float32)
        self.m = np.zeros(n, np.int64)
        self.abs_sum = np.zeros(n)
        self.tol_sum = np.zeros(n)

    def replay(self, ret0, reward, before, after, limits):
        self.ret = np.asarray(ret0).astype(np.float32)
        for k in range(reward.shape[0]):
            acc = ~before[k]
            self.ret = np.where(acc, (self.ret + reward[k]).astype(np.float32), self.ret)     # ep_ret += (float)reward
            self.m += acc
            self.abs_sum += np.where(acc, np.abs(reward[k].astype(np.float64)), 0.0)
            self.tol_sum += np.where(acc, limits[k], 0.0)
            z = before[k] | after[k]
            self.ret[z] = 0.0
            self.m[z] = 0
            self.abs_sum[z] = 0.0
            self.tol_sum[z] = 0.0


def _np_roll(roll):
    return {k: to_np(getattr(roll, k)) for k in TAPES if getattr(roll, k) is not None}


@pytest.mark.parametrize("case", CASES, ids=_name)
def test_return_ticks_and_episode_through_four_collections_on_one_env(case):
    """Four launches on the same env, K = 7, 24, 1, 12, sampled actions at sigma = 0.003 around hover from low starts;
    after every launch the tapes and get_state() against the twin and the oracle, get_time(), state_tensors() and
    batch_stats() against get_state().

    The running return: the kernel does ep_ret += (float)reward in float32 (dev_task.h: advance; contraction is off in
    the kernel's file and there is nothing to contract) and zeroes it in the reset; the reward tape holds the same
    (float)reward.  So get_state()["episode_return"] is the sequential np.float32 sum of the tape's rewards since the
    lane's last reset, started from the value get_state() gave before the launch: BIT EQUALITY is asserted.  Against the
    oracle's float64 ep_return the bound is derived: (m + 1) 2^-24 sum |r_k| over the m rewards of the running episode
    (one rounding per float32 conversion and per addition, each at most 2^-24 of a partial sum that sum |r_k| bounds)
    plus the sum of the per-step reward tolerances assert_step_close allows the rewards themselves.

    Non-vacuity, on the oracle (the twin where there is no oracle, at the checkpoints before its last launch): 25 % of
    the lanes start a new episode, 25 % do not end their first episode in the first launch, with episode_stats half of
    the lanes hold a non-zero return at some checkpoint, with track_time 5 % of the lanes have ticks != substeps x
    (steps - 1) at some checkpoint.  Seed rule of the starts: the first start seed, counted from 0, for which these
    conditions hold for the case on the CPU oracle under the same policy and noise (tests/ppo_ref.py)."""
    import torch
    name, n, next_step = _name(case), case.n, case.autoreset == "next_step"
    kw = _env_kwargs(case)
    env, twin = _env(case.task, n, case.mode, case.autoreset, **kw), _env(case.task, n, case.mode, case.autoreset, **kw)
    try:
        rng, installed = _prepare(case, (env, twin))
        actor, critic, log_std = _policy(case.task, case.H, case.Hv, 3, env, bias=model_variants.hover(case.variant))
        st0 = env.get_state()
        assert ("episode_return" in st0) == case.stats and ("ticks" in st0) == case.ticks
        orc = o64 = None
        if case.oracle:
            orc, o64 = _oracle(case, case.mode, installed), _oracle(case, "float64", installed)
            _mirror(orc, st0)
            _mirror(o64, st0)
        dt = 1.0 / (float(env.config.frames_per_second) * case.substeps)
        assert orc is None or dt == orc.dt
        run = _Running(n)
        keep = np.ones(n, bool)
        held_return, tick_share, first_not_ended, worst_ratio = np.zeros(n, bool), [], None, 0.0
        witness = None                                           # the state the non-vacuity conditions are read from
        for li, (K, nonce) in enumerate(LAUNCHES):
            ctx = "%s launch %d (K %d)" % (name, li, K)
            last = li == len(LAUNCHES) - 1
            before = env.get_state()
            pending0 = (before["flags"] & 2) != 0
            roll = _clone(env.rollout_actor_critic(actor, critic, log_std, K, case.H, case.Hv, nonce=nonce))
            t = _np_roll(roll)
            after = env.get_state()
            limits = np.zeros((K, n))
            # ---- (b) the oracle, stepped with the returned action tape; the float64 oracle decides who straddles ----
            if orc is not None:
                o_pending0 = orc.done_pending.copy()
                wants = []
                for k in range(K):
                    a = t["actions"][k].astype(np.float64)
                    want, w64 = orc.step(a), o64.step(a)
                    keep &= (want[2] == w64[2]) & (want[3] == w64[3])
                    wants.append(want)
                    limits[k] = reward_limit(want[0], want[1])
                assert (~keep).mean() <= 0.02, (ctx, int((~keep).sum()))
                oterm, otrunc = np.stack([w[2] for w in wants]), np.stack([w[3] for w in wants])
                if li == 0:
                    first_not_ended = ~(oterm | otrunc).any(0)
                witness = dict(episode=orc.episode.copy(), steps=orc.steps.copy(), ticks=orc.ticks.copy(),
                               episode_return=orc.ep_return.copy())
                for k in range(K):
                    got = (t["obs"][k + 1][keep], t["reward"][k][keep], t["terminated"][k][keep], t["truncated"][k][keep])
                    assert_step_close(got, tuple(w[keep] for w in wants[k]), X_TOL, r_abs=R_ABS, ctx="%s step %d" % (ctx, k))
                assert np.array_equal(t["live"][:, keep], ppo_ref.live(oterm, otrunc, o_pending0, next_step)[:, keep]), ctx
                for key, want in (("status", orc.status), ("steps", orc.steps), ("episode", orc.episode)) + \
                        ((("ticks", orc.ticks),) if case.ticks else ()):
                    assert np.array_equal(after[key][keep], want[keep]), (ctx, key)
                assert np.array_equal(after["force"].astype(np.float32)[:, keep], orc.force.astype(np.float32)[:, keep]), ctx
                assert np.array_equal(((after["flags"] & 1) != 0)[keep], orc.pending[keep]), ctx
                if next_step:
                    assert np.array_equal(((after["flags"] & 2) != 0)[keep], orc.done_pending[keep]), ctx
            # ---- (a) the twin under step_many with the same actions (the last launch: _check_against_twin below) ----
            if not last:
                tw = [x.clone() for x in twin.step_many(roll.actions)]
                assert torch.equal(roll.obs[1:], tw[0]) and torch.equal(roll.reward, tw[1]), ctx
                assert torch.equal(roll.terminated, tw[2]) and torch.equal(roll.truncated, tw[3]), ctx
                tst = twin.get_state()
                if orc is None:
                    witness = tst
                    if li == 0:
                        first_not_ended = ~to_np(tw[2] | tw[3]).any(0)
                _states_equal(after, tst)
            # ---- the running return, restated from the device's own tapes ----
            resets = _reset_masks(t["terminated"], t["truncated"], pending0, next_step)
            assert np.array_equal(t["live"], ~resets[0]), ctx
            run.replay(before.get("episode_return", np.zeros(n)), t["reward"], resets[0], resets[1], limits)
            if case.stats:
                got = after["episode_return"]
                assert np.array_equal(got.astype(np.float32).view(np.uint32), run.ret.view(np.uint32)), \
                    (ctx, np.flatnonzero(got.astype(np.float32) != run.ret)[:8])
                if orc is not None:
                    bound = (run.m + 1) * U32 * run.abs_sum + run.tol_sum
                    err = np.abs(got - orc.ep_return)
                    ratio = float(np.max(np.where(keep & (bound > 0), err / np.maximum(bound, 1e-300), 0.0)))
                    worst_ratio = max(worst_ratio, ratio)
                    assert np.all(err[keep] <= bound[keep]), (ctx, ratio)
            # ---- the counters' other outlets ----
            tens = {k: to_np(v).copy() for k, v in env.state_tensors().items()}
            assert np.array_equal(tens["steps"], after["steps"]) and np.array_equal(tens["status"], after["status"]), ctx
            if case.ticks:
                assert np.array_equal(tens["ticks"], after["ticks"]), ctx
                gt = to_np(env.get_time())
                assert gt.dtype == np.float64 and np.array_equal(gt, after["ticks"].astype(np.float64) * dt), ctx
            else:
                assert (tens["ticks"] == -1).all(), ctx
            s = to_np(env.batch_stats()).copy()
            assert s[0] == n and s[1] == np.sum(after["status"] == 3), ctx
            assert s[2] == after["steps"].sum() and s[3] == after["steps"].max(), ctx
            assert s[4] == after["episode"].astype(np.int64).sum(), ctx
            if case.stats:
                assert abs(s[5] - after["episode_return"].sum()) <= 1e-6 * max(1.0, abs(s[5])), ctx
            if orc is not None:       # (the lanes left out contribute the device's own figures)
                assert s[4] - after["episode"][~keep].astype(np.int64).sum() == orc.episode[keep].astype(np.int64).sum(), ctx
                assert s[2] - after["steps"][~keep].sum() == orc.steps[keep].sum(), ctx
            # ---- what the non-vacuity conditions need of this checkpoint ----
            if orc is not None or not last:
                if case.stats:
                    held_return |= witness["episode_return"] != 0
                if case.ticks:
                    tick_share.append(float((witness["ticks"] != case.substeps * (witness["steps"] - 1)).mean()))
            if last:
                started = float((witness["episode"] != st0["episode"]).mean())
                print("%s: %.0f %% of the lanes started a new episode, %.0f %% did not end their first episode in the "
                      "first launch, %.0f %% held a non-zero return at a checkpoint, ticks != substeps x (steps - 1) in "
                      "%s %% of the lanes at the checkpoints; %d lanes left out of the oracle comparison; return against "
                      "the oracle: worst error / bound %.3f"
                      % (name, 100 * started, 100 * first_not_ended.mean(), 100 * held_return.mean(),
                         [round(100 * v, 1) for v in tick_share], int((~keep).sum()), worst_ratio))
                assert started >= 0.25 and first_not_ended.mean() >= 0.25, name
                assert not case.stats or held_return.mean() >= 0.5, name
                assert not case.ticks or max(tick_share) >= 0.05, (name, tick_share)
                _check_against_twin(ctx, env, twin, roll, pending0, next_step, rng, expect_events=False)
    finally:
        env.close()
        twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the lean and the full-featured form on the same inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [200, 256])
@pytest.mark.parametrize("task,mode", [("lander3d", "float32"), ("hover3d", "float32"), ("lander2d", "float64")])
def test_lean_and_full_featured_forms_give_the_same_bits(task, mode, n):
    """A default env (the kernel's lean form), one with episode_stats and track_time and one with track_time alone (the
    full-featured form through either switch): same task, seed, id base, starts, policy and nonce.  Every tape as bytes
    and every get_state() array the three share are equal, over two launches on the same envs (K = 24, then 7); the two
    tick counters agree as well."""
    import torch
    rng = np.random.default_rng(zlib.crc32(repr((task, mode, n)).encode()))
    base = dict(seed=SEED, env_id_base=512, substeps=1)
    envs = [_env(task, n, mode, "next_step", **dict(base, **kw))
            for kw in ({}, dict(episode_stats=True, track_time=True), dict(track_time=True))]
    try:
        _install_low_starts(envs, rng, pending_share=0.125)
        actor, critic, log_std = _policy(task, 32, 16, 3, envs[0])
        ended = np.zeros(n, bool)
        for K, nonce in ((24, 9), (7, 10)):
            rolls = [_clone(e.rollout_actor_critic(actor, critic, log_std, K, 32, 16, nonce=nonce, means=True)) for e in envs]
            for other in rolls[1:]:
                for u, v in zip(rolls[0], other):
                    assert u.dtype == v.dtype and torch.equal(u.contiguous().view(torch.uint8), v.contiguous().view(torch.uint8))
            states = [e.get_state() for e in envs]
            assert set(states[1]) - set(states[0]) == {"episode_return", "ticks"} and "ticks" in states[2]
            for st in states[1:]:
                for key in states[0]:
                    assert np.array_equal(states[0][key], st[key], equal_nan=True), (task, mode, n, K, key)
            assert np.array_equal(states[1]["ticks"], states[2]["ticks"])
            ended |= to_np(rolls[0].terminated | rolls[0].truncated).any(0)
            assert not to_np(rolls[0].live).all()                              # reset steps inside the launch
        assert ended.mean() >= 0.25 and (~ended).mean() >= 0.25, float(ended.mean())
        assert (states[1]["ticks"] != states[1]["steps"] - 1).any() and (states[1]["episode_return"] != 0).any()
    finally:
        for e in envs:
            e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the episode counter across its boundaries inside this kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lean", "full"])
def test_episode_counter_crosses_its_boundaries_inside_the_collection_kernel(form):
    """The actor-critic twin of test_episode_counter_crosses_its_boundaries_inside_k_step_and_served_kernels: this
    kernel keeps the WHOLE episode number in a register over its own loop (resolve_episode / split_episode) and keys the
    Philox reset draws inside the loop with it.  The same parking (just below 2^E, below 2^(E+1), below 2^32, an
    arbitrary large number, small numbers), then four launches of K = 12 whose reset churn comes from the policy (zero
    output bias, log_std = ln 0.5: actions about N(0, 0.5), envs tilt, crash and hit the 40-step limit): outputs, episode
    numbers and the forces drawn for them against the oracle stepped with the returned tape, then the one-launch step on
    what the kernel left in the EPH row.  `full`: the same with episode_stats and track_time (the full-featured form)."""
    import torch
    n, K, max_steps, H, Hv = 320, 12, 40, 32, 16
    extra = dict(episode_stats=True, track_time=True) if form == "full" else {}
    env, orc = make_pair("lander3d", n, "float32", "next_step", seed=33, max_steps=max_steps, **extra)
    try:
        ebits = device_episode_bits(max_steps)
        ep_mask = (1 << ebits) - 1
        env.reset()
        orc.reset()
        ep = np.full(n, ep_mask - 1, np.uint32)
        ep[::7] = ep_mask
        ep[1::7] = 3
        ep[2::7] = 2 * (ep_mask + 1) - 2
        ep[3::7] = 0xFFFFFFFE
        ep[4::7] = 0x9E3779B9
        env.set_state(episode=ep)
        orc.episode[:] = ep
        orc.force[:] = refvec.draw_forces(orc.seed, orc.env_ids, ep - np.uint32(1), orc.tp.initial_random_force).astype(orc.T)
        actor, critic, _ = _policy("lander3d", H, Hv, 7, env, bias=0.0)
        log_std = torch.full((4,), float(np.log(0.5)), dtype=torch.float32, device=env.device)
        for launch in range(4):
            pending0 = orc.done_pending.copy()
            roll = env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=20 + launch)
            t = _np_roll(roll)
            terms, truncs = [], []
            for k in range(K):
                want = orc.step(t["actions"][k].astype(np.float64))
                assert_step_close((t["obs"][k + 1], t["reward"][k], t["terminated"][k], t["truncated"][k]), want, X_TOL,
                                  r_abs=R_ABS, ctx="%s launch %d step %d" % (form, launch, k))
                terms.append(want[2])
                truncs.append(want[3])
            assert np.array_equal(t["live"], ppo_ref.live(np.stack(terms), np.stack(truncs), pending0, True)), (form, launch)
            st = env.get_state()
            assert np.array_equal(st["episode"], orc.episode), (form, launch)
            assert np.array_equal(st["force"].astype(np.float32), orc.force.astype(np.float32)), (form, launch)
            if form == "full":
                assert np.array_equal(st["ticks"], orc.ticks) and np.array_equal(st["steps"], orc.steps), (form, launch)
        e0, e1 = ep.astype(np.int64), orc.episode.astype(np.int64)
        print("%s: %d lanes passed 2^E, %d wrapped past 2^32; %d resets in all"
              % (form, int(np.sum((e0 <= ep_mask) & (e1 > ep_mask))), int(np.sum((e0 > 0xFFFFFF00) & (e1 < 100) & (e1 >= 1))),
                 int(((e1 - e0) % (1 << 32)).sum())))
        assert np.any((e0 <= ep_mask) & (e1 > ep_mask)) and np.any((e0 > 0xFFFFFF00) & (e1 < 100) & (e1 >= 1))
        # ... and the one-launch step picks up what the collection kernel left in the EPH row
        rng = np.random.default_rng(8)
        a = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        for j in range(6):
            o, r, te, tr, _ = env.step(torch.from_numpy(a).to(env.device))
            want = orc.step(a.astype(np.float64))
            assert_step_close(tuple(to_np(v) for v in (o, r, te, tr)), want, X_TOL, r_abs=R_ABS, ctx="%s tail %d" % (form, j))
        assert np.array_equal(env.get_state(only=("episode",))["episode"], orc.episode)
        assert_state_close(env, orc, MODE_TOL["float32"])
    finally:
        env.close()
