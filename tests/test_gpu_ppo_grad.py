"""cs_ppo_grad on the GPU (CopterVecEnv.ppo_grad, gym_copter_amd.ppo_loss, ppo(update="device")):
the gradient and the statistics against the float64 autograd reference of tests/ppo_update_ref.py within a derived bar
and nearer to it than the float32 autograd they replace; determinism; the index's semantics; an all-dead minibatch; the
collection's own tapes; autograd; the driver; offsets past 4 GiB; errors.  The code under test is never its own
reference.

The gradient bar.  Per parameter |device - reference| <= c (2 B + 64) 2^-53 T, T the sum over the rows of |term|
(ppo_update_ref.reference).  Section 12's bar is the case c = 1: two float64 summations of B terms differ by at most
2 (B - 1) u sum|t|, and a term there is a product of numbers read from memory, a few u more.  Here a term is
dL/dlogp x z e^-ls x (a factor of the network), dL/dlogp = -w Ahat rho / W, and carries in addition, in units of u = 2^-53:
  * rho = exp(logp - logp_old): exp is within an ulp, but its ARGUMENT differs between two evaluations by
    sum_c |z_c| d z_c + 2 (A + 4) (z^2 / 2 + sum|ls| + A ln(2 pi) / 2 + |logp_old|), with d z_c = e^-ls_c d mu_c + 6 |z_c| and
    d mu_c the difference of two summation orders of the network's output, 2 (H + 2) (|W2| |h| + |b2|) + |W2| d h, d h =
    2 ((OBS + 2) (|W1| |o| + |b1|) + 2 |h|): with sigma = 0.05 the factor e^-ls = 20 turns d mu ~ 100 into d logp of
    thousands -- this is the largest part, and it does not shrink with B;
  * Ahat = (adv - m) / (sd + 1e-8): m and sd are sums of B terms of their own, each within (B + 2) u of its terms'
    magnitudes on either side, and m's error enters EVERY Ahat absolutely: 3 (B + 8) (mean|adv| / sd + |Ahat|);
  * z itself (d z above), the products and the division by W: a few.
reference() adds these up per row and per parameter from the reference's own numbers (no device output enters) and returns
the least c that covers them, c_needed: 3.0 to 9.4 for the cases with B >= 200 and 54.3 at B = 37, where 2 B + 64 = 138 is
least.  c = 64 (ppo_update_ref.BAR_C), the next power of two, is taken for every case, and every test asserts c_needed <= c
on its reference before it looks at the device.  The same c bounds the summed statistics on their own terms' magnitudes S.
Measured worst ratios: see test_gradient_and_statistics_equal_the_reference."""
import numpy as np
import pytest

import ppo_update_ref as pur
from gpu_util import have_gpu, to_np

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

U64 = 2.0 ** -53
C = pur.BAR_C
KW = dict(vf_coef=0.5, ent_coef=0.01)


def _env(task, n=64, autoreset="next_step", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype="float32", autoreset_mode=autoreset, **kw)


def _call(env, s, index=None, **kw):
    """env.ppo_grad on the tapes of the dict s (ppo_update_ref.synthetic's keys)."""
    return env.ppo_grad(s["actor"], s["critic"], s["log_std"], s["hidden"], s["critic_hidden"], s["obs"], s["actions"],
                        s["logp"], s["advantages"], s["returns"], live=kw.pop("live", s["live"]), index=index, **kw)


def _check(name, got, ref, B, s=None, idx=None, kw=None):
    """The gradient within the bar, the statistics within theirs; with s: nearer than the float32 autograd.  Returns the
    worst ratio to the gradient's bar."""
    import torch
    assert ref["c_needed"] <= C and ref["c_stats"] <= C, (ref["c_needed"], ref["c_stats"])
    ratio = pur.bound_ratio(got.grad, ref["grad"], ref["T"], B, C)
    st, want, S = got.stats, ref["stats"], ref["S"]
    assert bool(torch.isfinite(st).all())
    sums = [float((st[k] - want[k]).abs() / (C * (2 * B + 64) * U64 * S[k]).clamp_min(1e-300)) for k in (1, 2, 3, 4, 5)
            if float(S[k]) > 0 or float((st[k] - want[k]).abs()) > 0]
    r7 = float((st[7] - want[7]).abs()) / (ref["ratio_err"] * U64)
    dist = pur.scaled(got.grad, ref["grad"])
    line = "%s: gradient %.3g of its bar (c_needed %.1f), statistics %.3g of theirs, max|rho - 1| %.3g of its; scaled " \
           "distance %.2e" % (name, ratio, ref["c_needed"], max(sums), r7, dist)
    d32 = None
    if s is not None:
        d32 = pur.float32_distance(s, idx, ref["grad"], **kw)
        line += ", float32 autograd %.2e" % d32
    print(line)
    assert ratio <= 1.0, ratio
    assert float(st[0]) == ref["count"] and float(st[6]) == float(want[6])          # exact: a count, and a count / W
    assert max(sums) <= 1.0, sums
    # exp at the largest |logp - logp_old| of the case: rho (d logp + 2) u, rho up to exp(max_dlogp)
    assert r7 <= 1.0, (r7, ref["max_dlogp"])
    if d32 is not None:
        assert dist < d32, (dist, d32)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------
# 1. the gradient and the statistics against the reference
# ---------------------------------------------------------------------------------------------------------------------
_TAPES = {}


def _tapes(env, task, H, Hv, R, seed):
    """The synthetic tapes of a case on the device, made once and shared (never changed)."""
    key = (task, H, Hv, R, seed)
    if key not in _TAPES:
        _TAPES.clear()                                            # (one case's tapes at a time: the large one is 5 MB)
        _TAPES[key] = pur.to_device(pur.synthetic(task, H, Hv, R, seed), env.device)
    return _TAPES[key]


@pytest.mark.parametrize("clip", [0.2, 0.1])
@pytest.mark.parametrize("task,H,Hv,R,B,seed,opt", pur.CASES)
def test_gradient_and_statistics_equal_the_reference(task, H, Hv, R, B, seed, opt, clip):
    """The cases of ppo_update_ref.CASES at clip 0.2 and 0.1, ent_coef 0.01, vf_coef 0.5.  The reference's own conditions
    first (clipped share in [1 %, 50 %], no ratio within 1e-8 of an edge, a dead row, the bar's constant covering the
    budget), then the device: the gradient within c (2 B + 64) 2^-53 T per parameter, sum w and the clipped share exact,
    the summed statistics within the same kind of bar on their terms, max|rho - 1| within exp's error, and the scaled
    distance from the reference smaller than the float32 autograd's (what ppo.py computes today).
    Measured on an MI355X: the worst ratio to the gradient's bar over the twenty cases is recorded in DESIGN section 18."""
    import torch
    env = _env(task)
    try:
        s = _tapes(env, task, H, Hv, R, seed)
        rng = opt.get("range", False)
        kw = dict(KW, clip=clip, normalize=opt.get("normalize", True))
        idx = torch.arange(B, device=env.device) if rng else s["perm"][:B].contiguous()
        ref = pur.reference(s, idx, live=not rng, **kw)
        pur.check_conditions(ref, need_dead=not rng)
        if rng:
            got = _call(env, s, index=None, live=None, row_base=0, num_samples=B, **kw)
        else:
            got = _call(env, s, index=idx, **kw)
        assert got.grad.dtype == torch.float64 and got.grad.shape == ref["grad"].shape and got.stats.shape == (8,)
        _check("ppo_grad %s H=%s/%s R=%d B=%d clip=%.1f%s" % (task, H, Hv, R, B, clip, " " + str(opt) if opt else ""),
               got, ref, B, s, idx, dict(kw, live=not rng))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. deterministic, written rather than accumulated, a scratch of its own
# ---------------------------------------------------------------------------------------------------------------------
def test_deterministic_and_overwrites():
    import torch
    n, K = 64, 4
    env = _env("lander3d", n)
    try:
        env.reset()
        s = pur.to_device(pur.synthetic("lander3d", 33, 16, 4096, 2), env.device)
        idx = s["perm"][:1000].contiguous()
        kw = dict(KW, clip=0.2)
        first = _call(env, s, index=idx, **kw)
        first = type(first)(first.grad.clone(), first.stats.clone())
        again = _call(env, s, index=idx, **kw)
        assert torch.equal(first.grad, again.grad) and torch.equal(first.stats, again.stats)
        out = torch.full_like(first.grad, float("nan"))
        st = torch.full_like(first.stats, float("nan"))
        got = _call(env, s, index=idx, out=out, stats_out=st, **kw)
        assert got.grad is out and got.stats is st
        assert torch.equal(out, first.grad) and torch.equal(st, first.stats)
        # other widths and another B in between (the scratch is reused), and the parameter gradient's own scratch
        s2 = pur.to_device(pur.synthetic("lander3d", 64, 0, 300, 3), env.device)
        other = _call(env, s2, index=s2["perm"][:77].contiguous(), **kw)
        other = type(other)(other.grad.clone(), other.stats.clone())
        p = s2["actor"]
        obs = torch.randn((K, n, 10), device=env.device)
        ga = torch.randn((K, n, 4), dtype=torch.float64, device=env.device)
        pg = env.mlp_param_grad(p, 64, obs, ga).clone()
        got = _call(env, s, index=idx, **kw)
        assert torch.equal(got.grad, first.grad) and torch.equal(got.stats, first.stats)
        assert torch.equal(env.mlp_param_grad(p, 64, obs, ga), pg)
        got2 = _call(env, s2, index=s2["perm"][:77].contiguous(), **kw)
        assert torch.equal(got2.grad, other.grad) and torch.equal(got2.stats, other.stats)
        # index = 0 .. B-1 is the row range from 0, bit for bit (and row_base moves the range)
        a = _call(env, s, index=torch.arange(1000, device=env.device), **kw)
        a = type(a)(a.grad.clone(), a.stats.clone())
        b = _call(env, s, index=None, row_base=0, num_samples=1000, **kw)
        assert torch.equal(a.grad, b.grad) and torch.equal(a.stats, b.stats)
        c = _call(env, s, index=torch.arange(100, 1100, device=env.device), **kw)
        c = type(c)(c.grad.clone(), c.stats.clone())
        d = _call(env, s, index=None, row_base=100, num_samples=1000, **kw)
        assert torch.equal(c.grad, d.grad) and torch.equal(c.stats, d.stats) and not torch.equal(a.grad, c.grad)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the index: duplicates count as often as they occur, entries outside [0, R) are skipped by the kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_index_semantics():
    """The tapes are allocated with 64 rows of finite garbage past num_rows (and the kernel is given the first R): a
    missing range check shows as a wrong value, and cannot touch memory the test does not own.  The skipped samples
    shift the others' places in the tiles, so the result equals the call on the in-range samples alone within the bar
    (both against the reference on those), not bit for bit."""
    import torch
    R, B, slack = 1000, 600, 64
    env = _env("lander3d")
    try:
        full = pur.to_device(pur.synthetic("lander3d", 16, 16, R + slack, 4), env.device)
        s = dict(full)
        for k in ("obs", "actions", "logp", "advantages", "returns", "live"):
            if k != "live":
                full[k][R:] = 1e3                                   # finite garbage: a read of it moves every sum
            s[k] = full[k][:R]
        full["live"][R:] = True
        perm = s["perm"][s["perm"] < R]
        kw = dict(KW, clip=0.2)
        # duplicates
        idx = torch.cat([perm[:B], perm[:B // 3], perm[:7]]).contiguous()
        ref = pur.reference(s, idx, **kw)
        _check("duplicated indices", _call(env, s, index=idx, **kw), ref, idx.shape[0])
        # out of range: -1 and R (and far outside) interleaved with the in-range samples
        good = perm[:B].contiguous()
        bad = torch.tensor([-1, R, R + 1, R + slack - 1, -(1 << 40), 1 << 40, R, -1], device=env.device)
        mixed = torch.cat([good[:100], bad[:3], good[100:433], bad[3:], good[433:], bad[:2]]).contiguous()
        ref = pur.reference(s, good, **kw)
        assert ref["dead"] >= 1
        got = _call(env, s, index=mixed, **kw)
        _check("out-of-range indices", got, ref, B)
        alone = _call(env, s, index=good, **kw)
        assert float(got.stats[0]) == float(alone.stats[0]) == ref["count"]
        assert float(got.stats[6]) == float(alone.stats[6])
        # only out-of-range samples: nothing counts
        none = _call(env, s, index=bad.contiguous(), **kw)
        P, Pv = s["actor"].shape[0], s["critic"].shape[0]
        assert float(none.stats[0]) == 0 and bool((none.grad[:P + Pv] == 0).all())
        assert torch.equal(none.grad[P + Pv:], torch.full((4,), -0.01, dtype=torch.float64, device=env.device))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. an all-dead minibatch
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hv", [(16, 16), (0, 0)])
def test_all_dead_minibatch(H, Hv):
    import torch
    env = _env("lander3d")
    try:
        s = pur.to_device(pur.synthetic("lander3d", H, Hv, 500, 5), env.device)
        s["live"] = torch.zeros_like(s["live"])
        got = _call(env, s, index=s["perm"][:300].contiguous(), clip=0.2, **KW)
        P, Pv = s["actor"].shape[0], s["critic"].shape[0]
        assert bool(torch.isfinite(got.grad).all()) and bool(torch.isfinite(got.stats).all())
        assert bool((got.grad[:P + Pv] == 0).all())
        assert torch.equal(got.grad[P + Pv:], torch.full((4,), -0.01, dtype=torch.float64, device=env.device))
        st = to_np(got.stats)
        assert st[0] == 0 and st[1] == 0 and st[2] == 0 and st[5] == 0 and st[6] == 0 and st[7] == 0
        want_h = float(s["log_std"].double().sum()) + 2.0 * (1.0 + np.log(2.0 * np.pi))
        assert abs(st[3] - want_h) <= 1e-14 * abs(want_h) and abs(st[4] + 0.01 * want_h) <= 1e-15
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. on the collection's own tapes
# ---------------------------------------------------------------------------------------------------------------------
def test_on_the_collections_own_tapes():
    """Lander3D, 256 envs, K = 24, next_step, the low stored starts of tests/test_gpu_rollout_ac.py (40-50 % of the lanes
    end an episode, so some rows are reset steps with live = 0) and that file's policy near hover, the parameters the
    tapes were collected with: the ratio is 1 up to the precision and order in which mu is recomputed -- the bar
    reasoned in test_ppo_driver, 1e-3, holds here for the same reason: the collection's float32 mu is within (OBS + H +
    2) 2^-24 x the sum of its terms' magnitudes (0.03 for this policy) = 5e-8 of another evaluation, logp moves by |z|
    |d mu| / sigma <= 5.9 x 5e-8 / 0.0027 = 1.1e-4, plus the float32 rounding of the stored logp (2.4e-6) --, no sample is
    clipped, the approximate KL is within the same bar, and the gradient is within test 1's bar of the reference on
    the same tapes.  The [K+1,N,OBS] obs tape and the [K,N] tapes are passed as they are."""
    import torch
    from test_gpu_rollout_ac import _install_low_starts, _policy
    n, K, H, Hv = 256, 24, 16, 16
    env = _env("lander3d", n, seed=3, max_steps=1000)
    try:
        _install_low_starts([env], np.random.default_rng(7))
        actor, critic, log_std = _policy("lander3d", H, Hv, 4, env)
        roll = env.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=1)
        adv, ret = env.gae(roll.reward, roll.values, roll.terminated, roll.truncated)
        dead = int((~roll.live).sum())
        assert 0 < dead < K * n // 2
        idx = torch.randperm(K * n, device=env.device, generator=torch.Generator(device=env.device).manual_seed(1))
        idx = idx[:K * n // 2].contiguous()
        kw = dict(KW, clip=0.2)
        got = env.ppo_grad(actor, critic, log_std, H, Hv, roll.obs, roll.actions, roll.logp, adv, ret, live=roll.live,
                           index=idx, **kw)
        st = to_np(got.stats)
        print("collection's tapes: %d dead rows of %d; max|rho - 1| %.3e, approximate KL %.3e, clipped share %g"
              % (dead, K * n, st[7], st[5], st[6]))
        assert st[7] <= 1e-3 and st[6] == 0 and abs(st[5]) <= 1e-3
        s = dict(hidden=H, critic_hidden=Hv, actor=actor, critic=critic, log_std=log_std,
                 obs=roll.obs[:K].reshape(K * n, 10), actions=roll.actions.reshape(K * n, 4),
                 logp=roll.logp.reshape(K * n), advantages=adv.reshape(K * n), returns=ret.reshape(K * n),
                 live=roll.live.reshape(K * n))
        ref = pur.reference(s, idx, **kw)
        assert ref["edge"] >= 1e-8 and ref["dead"] >= 1
        _check("collection's tapes", got, ref, idx.shape[0])
        flat = env.ppo_grad(actor, critic, log_std, H, Hv, s["obs"], s["actions"], s["logp"], s["advantages"],
                            s["returns"], live=s["live"], index=idx, **kw)
        assert torch.equal(flat.grad, got.grad) and torch.equal(flat.stats, got.stats)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. autograd
# ---------------------------------------------------------------------------------------------------------------------
def test_ppo_loss_autograd():
    import torch
    import gym_copter_amd
    env = _env("hover3d")
    try:
        s = pur.to_device(pur.synthetic("hover3d", 16, 8, 2000, 6), env.device)
        idx = s["perm"][:700].contiguous()
        kw = dict(KW, clip=0.2, live=s["live"], index=idx)
        tapes = (s["obs"], s["actions"], s["logp"], s["advantages"], s["returns"])
        want = env.ppo_grad(s["actor"], s["critic"], s["log_std"], 16, 8, *tapes, **kw)
        want = type(want)(want.grad.clone(), want.stats.clone())
        P, Pv = s["actor"].shape[0], s["critic"].shape[0]
        for scale in (1.0, 2.0):
            leaves = [s[k].clone().requires_grad_(True) for k in ("actor", "critic", "log_std")]
            loss, stats = gym_copter_amd.ppo_loss(env, leaves[0], leaves[1], leaves[2], 16, 8, *tapes, **kw)
            assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.requires_grad and not stats.requires_grad
            assert torch.equal(loss.detach(), want.stats[4]) and torch.equal(stats, want.stats)
            (scale * loss).backward()
            g = scale * want.grad
            assert leaves[0].grad.dtype == torch.float32
            assert torch.equal(leaves[0].grad, g[:P].float()) and torch.equal(leaves[1].grad, g[P:P + Pv].float())
            assert torch.equal(leaves[2].grad, g[P + Pv:].float())
        # no critic: two leaves
        a, ls = s["actor"].clone().requires_grad_(True), s["log_std"].clone().requires_grad_(True)
        loss, _ = gym_copter_amd.ppo_loss(env, a, None, ls, 16, None, *tapes[:4], None, **kw)
        loss.backward()
        assert a.grad is not None and ls.grad is not None and float(a.grad.abs().max()) > 0
        # once differentiable
        a = s["actor"].clone().requires_grad_(True)
        loss, _ = gym_copter_amd.ppo_loss(env, a, s["critic"], s["log_std"], 16, 8, *tapes, **kw)
        g, = torch.autograd.grad(loss, a, create_graph=True)
        with pytest.raises(RuntimeError):
            g.sum().backward()
        with pytest.raises(ValueError):
            gym_copter_amd.ppo_loss(env, a, s["critic"], s["log_std"], 16, 8, *tapes, out=want.grad, **kw)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. the driver with update="device"
# ---------------------------------------------------------------------------------------------------------------------
def test_ppo_driver_with_the_device_update():
    """test_ppo_driver's set-up (tests/test_gpu_rollout_ac.py: Lander3D, 8 192 envs, K = 64, H = Hv = 16, 30 iterations)
    with update="device": the mechanics as there (finite statistics, the first minibatch's |ratio - 1| <= 1e-3, the
    live-count identity), and the final policy on a fresh env beats the initial one by at least 0.5 x DRIVER_MEASURED,
    the project's bar for the same algorithm -- the device path differs from the torch path by rounding only.  Both
    paths' endpoints are printed."""
    import gym_copter_amd
    from gym_copter_amd.ppo import STATS
    from test_gpu_rollout_ac import DRIVER, DRIVER_MEASURED, driver_problem, evaluate
    d = DRIVER
    actor0, critic0, log_std0 = driver_problem()
    before = evaluate(actor0, critic0, log_std0)
    results = {}
    for update in ("device", "torch"):
        env = _env(d["task"], d["n"], seed=2, max_steps=1000)
        try:
            env.reset()
            results[update] = gym_copter_amd.ppo(env, actor0, critic0, log_std0, d["H"], d["Hv"], d["K"], d["iterations"],
                                                 lr=d["lr"], update=update)
        finally:
            env.close()
    res = results["device"]
    after = {k: evaluate(r.actor, r.critic, r.log_std) for k, r in results.items()}
    print("ppo driver: mean reward per live step on a fresh env, initial policy %.4f; after %d iterations: "
          "update='device' %.4f, update='torch' %.4f" % (before, d["iterations"], after["device"], after["torch"]))
    stats = to_np(res.stats).astype(np.float64)
    col = {k: stats[:, i] for i, k in enumerate(STATS)}
    tcol = to_np(results["torch"].stats).astype(np.float64)
    print("iteration: mean reward per live step (device | torch) | live samples | first-minibatch |ratio - 1| | policy "
          "loss | value loss")
    for t in range(stats.shape[0]):
        print("%3d %10.4f %10.4f %8d %.3e %+.4e %.4e" % (t, col["mean_reward_per_live_step"][t], tcol[t, 0],
                                                        col["live_samples"][t], col["first_ratio_error"][t],
                                                        col["policy_loss"][t], col["value_loss"][t]))
    assert stats.shape == (d["iterations"], len(STATS)) and np.isfinite(stats).all()
    assert np.array_equal(to_np(res.history), to_np(res.stats)[:, 0])
    assert col["first_ratio_error"].max() <= 1e-3, float(col["first_ratio_error"].max())
    total = d["K"] * d["n"]
    assert np.all(col["live_samples"] <= total)
    assert np.all(np.abs(total - col["live_samples"] - col["done_rate"] * total) <= d["n"])
    # the two paths see the same first collection (the same seed, nonce and initial parameters)
    assert stats[0, 0] == tcol[0, 0] and stats[0, 1] == tcol[0, 1]
    for got, start in ((res.actor, actor0), (res.critic, critic0), (res.log_std, log_std0)):
        assert tuple(got.shape) == tuple(start.shape) and not np.array_equal(to_np(got), to_np(start))
    assert after["device"] - before >= 0.5 * DRIVER_MEASURED, (before, after)


# ---------------------------------------------------------------------------------------------------------------------
# 8. 64-bit offsets
# ---------------------------------------------------------------------------------------------------------------------
def test_offsets_past_4_gib():
    """R = 2^27 rows of random Lander3D observations (5.4 GB: R x OBS x 4 passes 4 GiB), B = 1 000 samples in the last 2^20
    rows, H = Hv = 0, against the reference on those rows.  The rows the minibatch names carry a synthetic case's values;
    the others are never read.  Skips only below 32 GiB of free device memory."""
    import torch
    R, B = 1 << 27, 1000
    assert R * 10 * 4 > 4 << 30
    free, _ = torch.cuda.mem_get_info(0)
    if free < 32 << 30:
        pytest.skip("needs 32 GiB of free device memory, %.1f GiB free" % (free / 2.0 ** 30))
    env = _env("lander3d")
    try:
        dev = env.device
        small = pur.to_device(pur.synthetic("lander3d", 0, 0, B, 7), dev)
        gen = torch.Generator(device=dev).manual_seed(2)
        idx = (R - (1 << 20) + torch.randperm(1 << 20, device=dev, generator=gen)[:B]).contiguous()
        assert int(idx.min()) * 10 * 4 > 4 << 30
        s = dict(small)
        s["obs"] = torch.randn((R, 10), dtype=torch.float32, device=dev, generator=gen)
        s["obs"][idx] = small["obs"]
        for k, shape, dt in (("actions", (R, 4), torch.float32), ("logp", (R,), torch.float32),
                             ("advantages", (R,), torch.float32), ("returns", (R,), torch.float32),
                             ("live", (R,), torch.bool)):
            s[k] = torch.zeros(shape, dtype=dt, device=dev)
            s[k][idx] = small[k]
        kw = dict(KW, clip=0.2)
        ref = pur.reference(small, torch.arange(B, device=dev), **kw)
        pur.check_conditions(ref)
        got = _call(env, s, index=idx, **kw)
        _check("offsets past 4 GiB", got, ref, B)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    import gym_copter_amd
    from gym_copter_amd import CopterStepError
    R, H, Hv = 300, 8, 4
    env = _env("lander2d", 32, seed=1)
    try:
        env.reset()
        before = env.get_state()
        s = pur.to_device(pur.synthetic("lander2d", H, Hv, R, 1), env.device)
        idx = s["perm"][:100].contiguous()
        good = dict(actor=s["actor"], critic=s["critic"], log_std=s["log_std"], hidden=H, critic_hidden=Hv,
                    obs=s["obs"], actions=s["actions"], logp=s["logp"], advantages=s["advantages"],
                    returns=s["returns"], live=s["live"], index=idx)
        env.ppo_grad(**good)
        cases = [(dict(hidden=65), "hidden must be"), (dict(critic_hidden=-1), "hidden must be"),
                 (dict(hidden=9), "actor must be"), (dict(critic_hidden=5), "critic must be"),
                 (dict(actor=s["actor"].double()), "actor must be"), (dict(actor=s["actor"].cpu()), "actor must be"),
                 (dict(actor=to_np(s["actor"])), "actor must be"), (dict(log_std=s["log_std"][:1]), "log_std must be"),
                 (dict(obs=s["obs"][:-1]), "obs must have shape"), (dict(obs=s["obs"][:, :-1]), "obs must have shape"),
                 (dict(obs=s["obs"].double()), "obs must be"), (dict(obs=s["obs"].cpu()), "obs must be"),
                 (dict(obs=to_np(s["obs"])), "obs must be"), (dict(actions=s["actions"][:, :1]), "actions must have shape"),
                 (dict(actions=s["actions"].reshape(-1)), "actions must be"),
                 (dict(logp=s["logp"][:-1]), "logp must have shape"), (dict(logp=s["logp"].double()), "logp must be"),
                 (dict(advantages=s["advantages"][::2]), "advantages must"),
                 (dict(returns=None), "returns must be"), (dict(returns=s["returns"].cpu()), "returns must be"),
                 (dict(live=s["live"][:-1]), "live must have shape"), (dict(live=s["live"].float()), "live must be"),
                 (dict(index=idx.int()), "index must be"), (dict(index=s["perm"][:200:2]), "index must be"),
                 (dict(index=idx.cpu()), "index must be"), (dict(index=idx.reshape(10, 10)), "index must be"),
                 (dict(index=idx[:0]), "index must be"), (dict(index=to_np(idx)), "index must be"),
                 (dict(index=idx, num_samples=99), "num_samples"),
                 (dict(index=None, row_base=-1), "row_base"), (dict(index=None, row_base=250, num_samples=51), "row_base"),
                 (dict(index=None, num_samples=0), "row_base"), (dict(index=None, row_base=1.5), "row_base"),
                 (dict(clip=0.0), "clip must be"), (dict(clip=float("nan")), "clip must be"),
                 (dict(vf_coef=float("inf")), "vf_coef and ent_coef"), (dict(ent_coef=float("nan")), "vf_coef and ent_coef"),
                 (dict(out=torch.empty(3, dtype=torch.float64, device=env.device)), "out must have shape"),
                 (dict(stats_out=torch.empty(8, dtype=torch.float32, device=env.device)), "stats_out must be")]
        for kw, match in cases:
            args = dict(good)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.ppo_grad(**args)
        with pytest.raises(ValueError, match="update must be"):
            gym_copter_amd.ppo(env, s["actor"], s["critic"], s["log_std"], H, Hv, 4, 1, update="host")
        state = env.get_state()
        assert set(state) == set(before)
        for k in before:                                                     # no refusal (and no call) moved the env
            assert np.array_equal(np.asarray(before[k]), np.asarray(state[k]), equal_nan=True), k
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.ppo_grad(**good)
        finally:
            env.serve_end(wait=False)
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.ppo_grad(**good)
