"""cs_ppo_grad on the GPU, what tests/test_gpu_ppo_grad.py leaves open: every one of the 40
instantiations of the template <OBS, A, HP, head>, each width class at its full width and at a ragged one; minibatches
large enough that all four wavefronts of a workgroup take tiles and the last workgroup holds fewer; rows that must never
be read, poisoned with NaN and +inf; degenerate normalisations; `live` bytes other than 0 and 1; tapes that are views
into larger buffers and the refusal of a misaligned obs; and the driver's plumbing against the documented loop run by
hand.

The bar, its constant and the reference are those of tests/test_gpu_ppo_grad.py (its docstring derives them): |device -
reference| <= c (2 B + 64) 2^-53 T per parameter with c = ppo_update_ref.BAR_C, the reference float64 autograd
(ppo_update_ref.reference), and every case asserts the reference's own conditions before it looks at the device.  No
other tolerance appears here: everything else is bit-equality or an exact value."""
import numpy as np
import pytest

import ppo_update_ref as pur
from gpu_util import have_gpu, to_np
from test_gpu_ppo_grad import C, KW, _call, _check, _env

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

KW2 = dict(KW, clip=0.2)
TAPES = ("obs", "actions", "logp", "advantages", "returns")


def _keep(r):
    return type(r)(r.grad.clone(), r.stats.clone())


def _same(a, b):
    import torch
    return torch.equal(a.grad, b.grad) and torch.equal(a.stats, b.stats)


def _conditions(ref, need_conditions=True):
    """What is asserted of the reference alone before the device is looked at."""
    if need_conditions:
        pur.check_conditions(ref)
    assert ref["c_needed"] <= C and ref["c_stats"] <= C, (ref["c_needed"], ref["c_stats"])


# ---------------------------------------------------------------------------------------------------------------------
# 1. every instantiation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,H,Hv,R,B,seed", pur.MATRIX)
def test_every_instantiation_equals_the_reference(task, H, Hv, R, B, seed):
    """ppo_update_ref.MATRIX: 4 shapes x 5 width pairs, which reach every (shape, width class, head) and each class both
    full and ragged (tests/test_ppo_grad_cpu.py asserts that of the list), and lander1d / hover2d by name.  R = 512,
    B = 300 (four full tiles and one of 44), clip 0.2, vf_coef 0.5, ent_coef 0.01, the index a prefix of perm.
    Measured on an MI355X: the worst ratio to the gradient's bar over the matrix is recorded in DESIGN section 18."""
    env = _env(task)
    try:
        assert (env.obs_dim, env.action_dim) == pur.TASK_SHAPE[task]
        s = pur.to_device(pur.synthetic(task, H, Hv, R, seed), env.device)
        idx = s["perm"][:B].contiguous()
        ref = pur.reference(s, idx, **KW2)
        _conditions(ref)
        got = _call(env, s, index=idx, **KW2)
        assert got.grad.shape == ref["grad"].shape and got.stats.shape == (8,)
        _check("matrix %s H=%d/%d (HP %d/%d)" % (task, H, Hv, pur.width_class(H), pur.width_class(Hv)), got, ref, B, s,
               idx, dict(KW2, live=True))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. all four wavefronts of a workgroup, and a last workgroup that holds fewer tiles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,H,Hv,R,B,seed", pur.LARGE)
def test_all_four_wavefronts_and_an_uneven_last_workgroup(task, H, Hv, R, B, seed):
    """B = 200 000.  The launch's geometry, restated from ppo_launch (copterstep_ppo_grad.hip): tiles = ceil(B / 64),
    tiles_per_group = ceil(tiles / 1024), groups = ceil(tiles / tiles_per_group); a workgroup hands its tiles to its four
    wavefronts in turn (tile = first + wave; tile += 4).  Here 3 125 tiles, 4 per workgroup -- every wavefront stages a tile
    in its own part of the LDS, which the epilogue then reuses for the reduction -- on 782 workgroups, the last with one
    tile.  Against the reference as everywhere, and index = arange(B) against the row range from 0 bit for bit (both
    walk the same tile schedule).  Measured worst ratios: DESIGN section 18."""
    import torch
    tiles = -(-B // 64)
    per_group = -(-tiles // 1024)
    groups = -(-tiles // per_group)
    assert per_group == 4 and tiles % 4 != 0                      # all four wavefronts; an uneven last workgroup
    assert 0 < tiles - (groups - 1) * per_group < per_group and groups <= 1024
    env = _env(task)
    try:
        s = pur.to_device(pur.synthetic(task, H, Hv, R, seed), env.device)
        idx = s["perm"][:B].contiguous()
        ref = pur.reference(s, idx, **KW2)
        _conditions(ref)
        got = _call(env, s, index=idx, **KW2)
        _check("large %s H=%d/%d B=%d" % (task, H, Hv, B), got, ref, B, s, idx, dict(KW2, live=True))
        del ref
        a = _keep(_call(env, s, index=torch.arange(B, device=env.device), **KW2))
        b = _call(env, s, index=None, row_base=0, num_samples=B, **KW2)
        assert _same(a, b)
        assert not torch.equal(a.grad, got.grad)                   # (another minibatch than the permuted one)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. rows that must never be read
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,H,Hv", [("lander3d", 16, 16), ("hover1d", 5, 0)])
def test_dead_unnamed_and_out_of_range_rows_are_never_read(task, H, Hv):
    """The tapes are allocated with 64 slack rows past num_rows and the kernel is given the first R.  The index mixes live
    rows, dead rows, values in [R, R + 64) (whose offsets land in the slack rows: memory the test owns) and the far ones of
    test_index_semantics (-1, R, +-2^40).  After a call on clean tapes, every dead row, every row the index does not name
    and every slack row is filled with NaN, then with +inf, in obs, actions, logp, advantages and returns, and the slack
    rows are marked live: the results keep their bits -- a skipped sample is staged as zeros either way, so the others'
    places in the tiles do not move.  A kernel that loaded such a row and multiplied by w = 0 would return NaN."""
    import torch
    R, slack, named_n = 1000, 64, 600
    env = _env(task)
    try:
        dev = env.device
        full = pur.to_device(pur.synthetic(task, H, Hv, R + slack, 1), dev)
        perm = full["perm"][full["perm"] < R]
        named = perm[:named_n]
        live = full["live"][:R]
        assert int((~live[named]).sum()) >= 10 and int(live[named].sum()) >= 100
        in_slack = torch.arange(R, R + slack, 3, device=dev)
        far = torch.tensor([-1, R, -(1 << 40), 1 << 40], device=dev)
        index = torch.cat([named[:100], in_slack[:7], named[100:433], far, named[433:], in_slack[7:], far[:2]])
        index = index.contiguous()
        near = index[(index.abs() < (1 << 39)) & (index != -1)]
        assert int(near.max()) < R + slack and int(near.min()) >= 0   # nothing but the far four points outside the tapes
        keep = torch.zeros(R + slack, dtype=torch.bool, device=dev)  # the rows a call may read: named and live
        keep[named] = True
        keep[:R] &= live
        assert not bool(keep[R:].any())
        variants = ("as it is", "normalize=False", "critic=None")

        def run(tapes):
            s = dict(full)
            for k in TAPES + ("live",):
                s[k] = tapes[k][:R]
            return [_keep(_call(env, s, index=index, **KW2)),
                    _keep(_call(env, s, index=index, normalize=False, **KW2)),
                    _keep(_call(env, dict(s, critic=None), index=index, **KW2))]
        clean = run(full)
        for r in clean:
            assert bool(torch.isfinite(r.grad).all()) and bool(torch.isfinite(r.stats).all())
            assert float(r.stats[0]) == float(live[named].sum())
        for poison in (float("nan"), float("inf")):
            bad = {k: full[k].clone() for k in TAPES + ("live",)}
            for k in TAPES:
                bad[k][~keep] = poison
            bad["live"][R:] = True
            for v, a, b in zip(variants, clean, run(bad)):
                assert _same(a, b), (poison, v)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. degenerate minibatches
# ---------------------------------------------------------------------------------------------------------------------
def _assert_zero_advantage(got, plain, P, Pv, A, count):
    """The exact values of a minibatch whose normalised advantage is 0 on every live sample: both sides of the clip test
    are false, dL/dlogp = -(0 rho) / W is a zero, every actor column is a sum of zeros, log_std's are 0 - ent_coef, the
    surrogate and the clipped share are 0, and the critic's columns, which the advantage does not enter, have the bits
    of the call without normalisation."""
    import torch
    assert bool((got.grad[:P] == 0).all())
    assert torch.equal(got.grad[P + Pv:], torch.full((A,), -KW["ent_coef"], dtype=torch.float64, device=got.grad.device))
    assert float(got.stats[0]) == count and float(got.stats[1]) == 0.0 and float(got.stats[6]) == 0.0
    assert torch.equal(got.grad[P:P + Pv], plain.grad[P:P + Pv])
    assert bool(torch.isfinite(got.grad).all()) and bool(torch.isfinite(got.stats).all())


@pytest.mark.parametrize("task,H,Hv,seed", pur.ONE_LIVE)
def test_one_live_sample(task, H, Hv, seed):
    """65 samples, 64 of them dead (the live one in the first tile, the second tile a single dead sample).  Without
    normalisation: within the bar of the reference on the same samples.  With it: m = adv, sd = 0, Ahat = 0 exactly."""
    env = _env(task)
    try:
        s, idx = pur.one_live(task, H, Hv, seed)
        s, idx = pur.to_device(s, env.device), idx.to(env.device)
        B, A = idx.shape[0], s["actions"].shape[1]
        assert B == 65 and int(s["live"][idx].sum()) == 1
        kw = dict(KW2, normalize=False)
        ref = pur.reference(s, idx, **kw)
        _conditions(ref, need_conditions=False)                       # (one live row: its clipped share is 0 or 1)
        plain = _keep(_call(env, s, index=idx, **kw))
        _check("one live sample %s H=%d/%d, not normalised" % (task, H, Hv), plain, ref, B)
        got = _call(env, s, index=idx, **KW2)
        _assert_zero_advantage(got, plain, s["actor"].shape[0], s["critic"].shape[0], A, 1.0)
    finally:
        env.close()


@pytest.mark.parametrize("task,H,Hv,seed", pur.EQUAL_ADV)
def test_equal_advantages(task, H, Hv, seed):
    """256 samples, every advantage 0.5: sums of 0.5 are exact in any order, so m = 0.5 and Ahat = 0 exactly.  Without
    normalisation the same tapes are an ordinary case, with the conditions."""
    env = _env(task)
    try:
        s, idx = pur.equal_advantages(task, H, Hv, seed)
        s, idx = pur.to_device(s, env.device), idx.to(env.device)
        B, A = idx.shape[0], s["actions"].shape[1]
        kw = dict(KW2, normalize=False)
        ref = pur.reference(s, idx, **kw)
        _conditions(ref)
        assert 1 < ref["count"] < B
        plain = _keep(_call(env, s, index=idx, **kw))
        _check("equal advantages %s H=%d/%d, not normalised" % (task, H, Hv), plain, ref, B, s, idx, dict(kw, live=True))
        got = _call(env, s, index=idx, **KW2)
        _assert_zero_advantage(got, plain, s["actor"].shape[0], s["critic"].shape[0], A, ref["count"])
    finally:
        env.close()


def test_live_bytes_nonzero_is_live():
    """A uint8 `live` tape of 0 / 1 gives the bits of the bool tape, and so do the bytes 2 and 255 in place of 1: nonzero is
    live (include/copterstep.h, live_dev)."""
    import torch
    env = _env("lander3d")
    try:
        s = pur.to_device(pur.synthetic("lander3d", 16, 16, 512, 1), env.device)
        idx = s["perm"][:300].contiguous()
        assert s["live"].dtype == torch.bool and 0 < int((~s["live"][idx]).sum()) < 300
        want = _keep(_call(env, s, index=idx, **KW2))
        ranged = _keep(_call(env, s, index=None, row_base=100, num_samples=300, **KW2))
        one = s["live"].to(torch.uint8)
        assert int(one.max()) == 1
        for byte in (1, 2, 255):
            s8 = dict(s, live=one * byte)
            assert s8["live"].dtype == torch.uint8 and int(s8["live"].max()) == byte
            assert _same(_call(env, s8, index=idx, **KW2), want), byte
            assert _same(_call(env, s8, index=None, row_base=100, num_samples=300, **KW2), ranged), byte
        every = _call(env, s, index=idx, live=None, **KW2)
        assert float(every.stats[0]) == 300 and not torch.equal(every.grad, want.grad)
    finally:
        env.close()


def test_row_range_with_a_live_mask():
    """index=None, row_base=100 WITH the live mask equals the reference on arange(100, 100 + B) with that mask."""
    import torch
    task, H, Hv, seed = pur.RANGE_LIVE
    env = _env(task)
    try:
        s = pur.to_device(pur.synthetic(task, H, Hv, pur.DEGENERATE_R, seed), env.device)
        B = pur.RANGE_B
        idx = torch.arange(pur.RANGE_BASE, pur.RANGE_BASE + B, device=env.device)
        ref = pur.reference(s, idx, **KW2)
        _conditions(ref)
        got = _call(env, s, index=None, row_base=pur.RANGE_BASE, num_samples=B, **KW2)
        _check("row range with a live mask", got, ref, B, s, idx, dict(KW2, live=True))
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. views into larger buffers, and a misaligned obs
# ---------------------------------------------------------------------------------------------------------------------
def _views(s, idx, k):
    """The tapes of s as contiguous views that start at row k of larger buffers, the index at element 1 of its own."""
    import torch
    v = dict(s)
    for key in TAPES + ("live",):
        t = s[key]
        pad = torch.ones((k,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        v[key] = torch.cat([pad * 1000 if t.dtype != torch.bool else pad, t])[k:]
        assert v[key].is_contiguous() and v[key].storage_offset() == k * int(np.prod(t.shape[1:], dtype=np.int64))
    index = torch.cat([idx[:1], idx])[1:]
    assert index.is_contiguous() and index.storage_offset() == 1
    return v, index


@pytest.mark.parametrize("task,H,Hv,ks", [("hover3d", 17, 5, (1, 2)), ("lander3d", 16, 16, (2,)), ("lander2d", 5, 64, (2,)),
                                          ("hover1d", 9, 0, (2,))])
def test_views_into_larger_buffers(task, H, Hv, ks):
    import torch
    env = _env(task)
    try:
        s = pur.to_device(pur.synthetic(task, H, Hv, 512, 1), env.device)
        idx = s["perm"][:300].contiguous()
        want = _keep(_call(env, s, index=idx, **KW2))
        for k in ks:
            v, index = _views(s, idx, k)
            assert v["obs"].data_ptr() % 16 == 0
            assert _same(_call(env, v, index=index, **KW2), want), k
    finally:
        env.close()


@pytest.mark.parametrize("task,H,Hv", [("lander3d", 16, 16), ("lander2d", 5, 64), ("hover1d", 9, 0)])
def test_a_misaligned_obs_is_refused_before_any_launch(task, H, Hv):
    """A view from row 1 puts obs on an 8-byte boundary for OBS in {10, 6, 2}; the contract wants obs_dev 16-byte aligned
    (include/copterstep.h).  The call is refused with an error that names the alignment, NaN-filled outputs stay NaN (no
    kernel ran), and the next good call is unaffected."""
    import torch
    from gym_copter_amd import CopterStepError
    env = _env(task)
    try:
        s = pur.to_device(pur.synthetic(task, H, Hv, 512, 1), env.device)
        idx = s["perm"][:300].contiguous()
        want = _keep(_call(env, s, index=idx, **KW2))
        v, index = _views(s, idx, 1)
        assert v["obs"].data_ptr() % 16 == 8
        out = torch.full_like(want.grad, float("nan"))
        st = torch.full_like(want.stats, float("nan"))
        with pytest.raises(CopterStepError, match="obs_dev must be 16-byte aligned"):
            _call(env, v, index=index, out=out, stats_out=st, **KW2)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(st).all())
        v["obs"] = s["obs"]                                             # the same call with an aligned obs
        got = _call(env, v, index=index, out=out, stats_out=st, **KW2)
        assert got.grad is out and _same(got, want)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the driver's plumbing
# ---------------------------------------------------------------------------------------------------------------------
def test_the_driver_runs_the_documented_loop():
    """ppo(update="device") against the loop its docstring documents, run by hand on a twin env with the same seed and
    starts: Lander3D, 64 envs, next_step, low stored starts (some rows are reset steps: dead), K = 7, 2 iterations x 2
    epochs x 3 minibatches of 448 samples (ragged thirds: 149, 149, 150), seed 5.  Both sides run the same kernels on the
    same inputs in the same order, so the returned parameters are torch.equal, and first_ratio_error / policy_loss /
    value_loss of an iteration are the hand loop's first and last minibatch statistics as float32.  This checks ppo.py --
    the slices of the permutation, one permutation per epoch, live=, the statistics' places --, not the kernel, which is on
    both sides on purpose."""
    import torch
    import gym_copter_amd
    from gym_copter_amd.ppo import STATS
    from test_gpu_rollout_ac import _install_low_starts, _policy
    n, K, H, Hv, iterations, epochs, minibatches, seed, lr = 64, 7, 16, 16, 2, 2, 3, 5, 3e-4
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)
    env, twin = (_env("lander3d", n, seed=3, max_steps=1000) for _ in range(2))
    try:
        _install_low_starts([env, twin], np.random.default_rng(7))
        actor0, critic0, log_std0 = _policy("lander3d", H, Hv, 4, env)
        res = gym_copter_amd.ppo(env, actor0, critic0, log_std0, H, Hv, K, iterations, epochs=epochs,
                                 minibatches=minibatches, lr=lr, seed=seed, update="device", **kw)
        dev, B = twin.device, K * n
        assert B % minibatches != 0
        actor, critic, log_std = (t.detach().clone().requires_grad_(True) for t in (actor0, critic0, log_std0))
        P, Pv = actor.shape[0], critic.shape[0]
        opt = torch.optim.Adam([actor, critic, log_std], lr=lr, eps=1e-5)
        gen = torch.Generator(device=dev).manual_seed(seed)
        dead, rows = 0, []
        for t in range(iterations):
            with torch.no_grad():
                roll = twin.rollout_actor_critic(actor, critic, log_std, K, H, Hv, nonce=t)
                adv, ret = twin.gae(roll.reward, roll.values, roll.terminated, roll.truncated)
            dead += int((~roll.live).sum())
            first = last = None
            for ep in range(epochs):
                perm = torch.randperm(B, device=dev, generator=gen)
                for mb in range(minibatches):
                    idx = perm[mb * B // minibatches:(mb + 1) * B // minibatches]
                    with torch.no_grad():
                        got = twin.ppo_grad(actor, critic, log_std, H, Hv, roll.obs, roll.actions, roll.logp, adv, ret,
                                            live=roll.live, index=idx, **kw)
                    g = got.grad.to(torch.float32)
                    actor.grad, critic.grad, log_std.grad = g[:P].clone(), g[P:P + Pv].clone(), g[P + Pv:].clone()
                    opt.step()
                    last = got.stats.clone()
                    first = last if first is None else first
            rows.append((first[7].to(torch.float32), last[1].to(torch.float32), last[2].to(torch.float32),
                         float(roll.live.sum())))
        assert 0 < dead < iterations * B
        for name, got, want, start in (("actor", res.actor, actor, actor0), ("critic", res.critic, critic, critic0),
                                       ("log_std", res.log_std, log_std, log_std0)):
            assert torch.equal(got, want.detach()), name
            assert not torch.equal(got, start.to(got.device)), name
        col = {k: res.stats[:, i] for i, k in enumerate(STATS)}
        for t, (first_err, pol, val, count) in enumerate(rows):
            assert torch.equal(col["first_ratio_error"][t], first_err), t
            assert torch.equal(col["policy_loss"][t], pol) and torch.equal(col["value_loss"][t], val), t
            assert float(col["live_samples"][t]) == count, t
        print("driver against the hand loop: %d dead rows of %d, first-minibatch |rho - 1| %s"
              % (dead, iterations * B, to_np(col["first_ratio_error"])))
    finally:
        env.close()
        twin.close()
