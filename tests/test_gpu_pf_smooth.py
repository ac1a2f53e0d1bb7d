"""The backward-simulation particle smoother on the device (cs_pf_smooth, CopterVecEnv.rollout_pf_smooth,
gym_copter_amd.pf_smooth): every row of the kernel against the NumPy restatement (tests/pf_smooth_ref.py) on the device's
OWN tapes -- the filter's, and the smoother's logb_tape and bwq_tape: a chained reference could draw another particle
after a one-ulp difference in exp.  Exact: log beta (mu is a K = 1 rollout_states from the N P taped particles; then only
+, - and x in a fixed order) with its -inf pattern, and the indices from the device's integer weights.  The integer
weights within 1 of the restatement's; x and var within section 19's bar (100 x the float64 reference's distance from
its numpy.longdouble twin, floored at 1e-12 scaled)."""
import zlib

import numpy as np
import pytest

import model_variants
import pf_ref
import pf_smooth_ref as R
import test_gpu_rollout_pf as F
from gpu_util import have_gpu, to_np
from oracle.refcpu import AIRBORNE

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K = pf_ref.TEST_N, pf_ref.TEST_K
SEED = F.SEED
NONCE = 11           # the backward draws' stream (the filter's is 7)
_bits = F._bits


def _smooth(env, p, filt, S, **kw):
    kw.setdefault("nonce", NONCE)
    kw.setdefault("tapes", True)
    return env.rollout_pf_smooth(p["acts"], filt, p["Q"], paths=S, **kw)


def _take(a, idx):
    return np.take_along_axis(a, idx[..., None] if a.ndim == idx.ndim + 1 else idx, axis=1)


def _propagate(penv, acts_row, X, s, P):
    """(mu [N,P,12], sigma [N,P]): a K = 1 rollout_states of the N P particles X [N,P,12], s [N,P] under acts_row [1,N,A]"""
    n = X.shape[0]
    one = penv.rollout_states(acts_row.repeat_interleave(P, dim=1),
                              state={"x": X.reshape(n * P, 12).T, "status": s.reshape(n * P)})
    return to_np(one.x[0]).astype(np.float64).reshape(n, P, 12), to_np(one.status[0]).reshape(n, P)


def _check_rows(name, penv, p, filt, res, P, S, exact=True, first_step=1, g=None, end=None, nonce=NONCE):
    """every row of res (a tapes=True result, cloned) against the restatement from the device's own tapes; returns
    (the statuses of the paths [K,N,S], the mask of log beta entries that are -inf by the status indicator alone)"""
    g = np.arange(N) if g is None else np.asarray(g, np.int64)
    part, pst, lwt = to_np(filt.part_tape), to_np(filt.pstatus_tape), to_np(filt.lw_tape)
    wqt = to_np(filt.wq_tape).astype(np.int64)
    idx, logb, bwq = to_np(res.idx).astype(np.int64), to_np(res.logb_tape), to_np(res.bwq_tape).astype(np.int64)
    steps = idx.shape[0]
    assert idx.shape == (steps, N, S) and logb.shape == bwq.shape == (steps, N, S, P)
    assert idx.min() >= 0 and idx.max() < P
    Linv = R.noise_inverse(p["Q"])
    paths = np.arange(S)[None, :]
    ok = np.ones(N, bool)
    by_status = np.zeros(logb.shape, bool)
    worst = {}

    def hold(key, k, got, r64, rld):
        b = pf_ref.bar(r64, rld)
        e = pf_ref.scaled(got, r64)
        worst[key] = max(worst.get(key, 0.0), e / b)
        assert e <= b, (name, key, k, e, b)
    # -- row K-1: the caller's, or drawn from the filter's integer weights
    last = steps - 1
    if end is None:
        u = R.draw_u(SEED, g[:, None], nonce, first_step + last, paths)
        assert np.array_equal(idx[last], R.draw_index(np.repeat(wqt[last][:, None, :], S, axis=1), u)), name
        assert np.array_equal(_bits(logb[last]), _bits(np.repeat(lwt[last][:, None, :], S, axis=1))), name
        assert np.array_equal(bwq[last], np.repeat(wqt[last][:, None, :], S, axis=1)), name
    else:
        assert np.array_equal(idx[last], to_np(end)), name
    for k in range(steps - 2, -1, -1):
        mu, sigma = _propagate(penv, p["acts"][k + 1:k + 2], part[k], pst[k], P)
        Xt, st = _take(part[k + 1], idx[k + 1]), _take(pst[k + 1], idx[k + 1])
        Y, Yt = R.whiten(Linv, mu), R.whiten(Linv, Xt)
        want = R.log_beta(lwt[k], Y, sigma, Yt, st)
        assert np.array_equal(np.isneginf(logb[k]), np.isneginf(want)), (name, k)
        if exact:
            assert np.array_equal(_bits(logb[k]), _bits(want)), (name, k)
        else:
            # float32 storage: rollout_states rounds the stored words to 24 bits, the kernel's mu is not rounded.  With
            # |dmu_j| <= 2^-23 max(1, |mu_j|): |dy_r| <= sum_j |Linv[r][j]| |dmu_j|, |d(d2)| <= sum_r (2 |t_r| |dy_r| + dy_r^2),
            # and log beta moves by half of that (plus the float64 rounding of the sums, 1e-12 scaled)
            dmu = 2.0 ** -23 * np.maximum(1.0, np.abs(mu))
            dy = dmu @ np.abs(Linv).T
            t = np.abs(Yt[:, :, None, :] - Y[:, None, :, :])
            room = 0.5 * np.sum(2.0 * t * dy[:, None, :, :] + dy[:, None, :, :] ** 2, axis=-1)
            fin = np.isfinite(want)
            assert np.all(np.abs(logb[k][fin] - want[fin]) <= (room + 1e-12 * np.maximum(1.0, np.abs(want)))[fin]), (name, k)
        by_status[k] = np.isneginf(logb[k]) & (sigma[:, None, :] != st[:, :, None]) & np.isfinite(lwt[k])[:, None, :]
        # -- the integer weights from the device's own log beta
        e, dead = R.weights(logb[k])
        assert np.all(np.abs(bwq[k] - R.quantise(e)) <= 1), (name, k)
        assert np.all(bwq[k].max(axis=-1) == pf_ref.WQ_ONE), (name, k)
        ok &= ~dead.any(axis=1)
        # -- exact from the integer weights on
        u = R.draw_u(SEED, g[:, None], nonce, first_step + k, paths)
        assert np.array_equal(idx[k], R.draw_index(bwq[k], u)), (name, k)
    for k in range(steps):
        e64, eld = R.estimate(part[k], idx[k]), R.estimate(part[k], idx[k], dtype=np.longdouble)
        hold("x", k, to_np(res.x[k]), e64[0], eld[0])
        hold("var", k, to_np(res.var[k]), e64[1], eld[1])
    assert np.array_equal(to_np(res.ok), ok), name
    print("%s: worst ratio to the bar " % name + " ".join("%s %.3f" % kv for kv in worst.items()))
    return np.stack([_take(pst[k], idx[k]) for k in range(steps)]), by_status


# ---------------------------------------------------------------------------------------------------------------------
# 1. every row, every workgroup width (P = 64, 128, 256 and up), run length (P / 64 = 1 .. 16) and path count per wavefront
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 1), (64, 5), (128, 64), (256, 7), (512, 64), (1024, 64), (64, 1024)]


@pytest.mark.parametrize("substeps", [1, 10])
@pytest.mark.parametrize("P,S", SHAPES)
def test_every_row_on_the_devices_own_tapes(P, S, substeps):
    import torch
    rng = np.random.default_rng(2100 + P + substeps)
    env = F._env("lander3d", N, substeps=substeps)
    penv = F._particle_env("lander3d", P, substeps)
    try:
        env.reset()
        before = env.get_state()
        p = F._problem(env, "lander3d", rng)
        filt = F._clone(F._run(env, p, P))
        res = F._clone(_smooth(env, p, filt, S))
        assert res.idx0 is None
        path_status, by_status = _check_rows("lander3d P=%d S=%d substeps=%d" % (P, S, substeps), penv, p, filt, res, P, S)
        # the branch of the status indicator ran: in env 1 (the touchdown) some particle is excluded by its status alone,
        # and with enough paths some row holds paths of two statuses.  (The seeds were checked on the CPU restatement over
        # the oracle step: at every shape with S >= 64 the paths of env 1 hold 2 to 4 statuses in every row, and at least
        # 189 entries of its log beta are -inf.)
        mixed = [len(np.unique(path_status[k, 1])) for k in range(K)]
        print("env 1: statuses among the paths per row %s, entries excluded by status %d" % (mixed, int(by_status[:, 1].sum())))
        assert by_status[:, 1].any()
        if S >= 64:
            assert max(mixed) >= 2, mixed
        # a call without the tapes gives the same bits elsewhere, and two calls give the same bits
        plain = _smooth(env, p, filt, S, tapes=False)
        assert plain.logb_tape is None and plain.bwq_tape is None
        for name in ("x", "var", "idx", "ok"):
            assert torch.equal(getattr(plain, name), getattr(res, name)), name
        for t in _smooth(env, p, filt, S):                    # the env's buffers: poison them, then run again
            if t is not None:
                t.fill_(float("nan") if t.dtype.is_floating_point else 1)
        for a, b in zip(_smooth(env, p, filt, S), res):
            assert (a is None and b is None) or torch.equal(a, b)
        # a float32 var is the float64 one rounded
        r32 = _smooth(env, p, filt, S, dtype=torch.float32)
        assert r32.var.dtype == torch.float32 and torch.equal(r32.var, res.var.float())
        assert torch.equal(r32.x, res.x) and torch.equal(r32.idx, res.idx)
        # another nonce draws other paths from the same weights
        if S >= 5:
            assert not torch.equal(_smooth(env, p, filt, S, nonce=NONCE + 1).idx, res.idx)
        after = env.get_state()
        for key in before:
            assert np.array_equal(np.asarray(before[key]), np.asarray(after[key]), equal_nan=True), key
    finally:
        env.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the draws away from global id 0 and from small rows
# ---------------------------------------------------------------------------------------------------------------------
def test_draws_follow_the_global_env_id_and_the_global_step_up_to_the_last_ones():
    """env_id_base = 2^32 - N and first_step = 2^32 - K: the last lane's id and the last row's index are 2^32 - 1, where
    the restatement's words are pinned to the host build of the kernel's header (test_pf_smooth_cpu.py).  Then a shard of
    two lanes with base + 3: what lanes 3 and 4 of the whole batch give, bit for bit, whatever the batch size."""
    import torch
    P, S = 128, 16
    base, first = 2 ** 32 - N, 2 ** 32 - K
    rng = np.random.default_rng(2201)
    env = F._env("lander3d", N, env_id_base=base)
    shard = F._env("lander3d", 2, env_id_base=base + 3)
    penv = F._particle_env("lander3d", P, 1)
    try:
        env.reset()
        shard.reset()
        p = F._problem(env, "lander3d", rng)
        filt = F._clone(F._run(env, p, P, first_step=first))
        early = _smooth(env, p, filt, S).idx.clone()
        res = F._clone(_smooth(env, p, filt, S, first_step=first))
        _check_rows("lander3d ids from 2^32 - %d, rows from 2^32 - %d" % (N, K), penv, p, filt, res, P, S, first_step=first,
                    g=base + np.arange(N))
        assert not torch.equal(early, res.idx)
        cut = lambda t, lanes_first: (t[3:5] if lanes_first else t[:, 3:5]).contiguous()      # noqa: E731
        sub = type(filt)(*[None] * 12, *(cut(t, False) for t in (filt.part_tape, filt.pstatus_tape, filt.lw_tape,
                                                                  filt.wq_tape)), None)
        part = _smooth(shard, dict(p, acts=cut(p["acts"], False)), sub, S, first_step=first)
        for nm in ("x", "var", "idx", "logb_tape", "bwq_tape"):
            assert torch.equal(getattr(part, nm), cut(getattr(res, nm), False)), nm
        assert torch.equal(part.ok, res.ok[3:5])
    finally:
        env.close()
        shard.close()
        penv.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. chunking, the caller's last row, the start set
# ---------------------------------------------------------------------------------------------------------------------
def test_chunked_smoother_is_the_single_call_bit_for_bit():
    import torch
    import gym_copter_amd
    rng = np.random.default_rng(2301)
    P, S = 256, 64
    env = F._env("lander3d", N)
    try:
        env.reset()
        p = F._problem(env, "lander3d", rng)
        filt = F._clone(F._run(env, p, P))
        one = F._clone(_smooth(env, p, filt, S, tapes=False))
        for chunk in (5, 1, None):
            got = gym_copter_amd.pf_smooth(env, p["acts"], filt, p["Q"], paths=S, nonce=NONCE, chunk=chunk)
            for name in ("idx", "x", "var", "ok"):
                assert torch.equal(getattr(got, name), getattr(one, name)), (chunk, name)
            at = one.idx.long().unsqueeze(-1).expand(-1, -1, -1, 12)
            assert tuple(got.paths_x.shape) == (K, N, S, 12)
            assert torch.equal(got.paths_x, torch.gather(filt.part_tape, 2, at)), chunk
            assert torch.allclose(got.paths_x.mean(dim=2), one.x, rtol=1e-12, atol=1e-12)
        # smooth() forwards a PfResult, and keeps the Kalman results' argument order
        via = gym_copter_amd.smooth(env, p["acts"], filt, p["Q"], paths=S, nonce=NONCE, chunk=5)
        assert torch.equal(via.idx, one.idx) and torch.equal(via.x, one.x)
        with pytest.raises(ValueError, match="x0 and P0"):
            gym_copter_amd.smooth(env, p["acts"], env.rollout_ekf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"],
                                                                  p["P0"], status0=p["st0"], tape=True), p["Q"])
        # the rows k0 .. K-1 alone, ending in the single call's last row and starting from the filter's row k0 - 1:
        # end is honoured verbatim, the rows are the single call's, and idx0 is its row k0 - 1
        k0 = 7
        sub = type(filt)(*[None] * 12, *(t[k0:] for t in (filt.part_tape, filt.pstatus_tape, filt.lw_tape, filt.wq_tape)),
                         None)
        start = (filt.part_tape[k0 - 1], filt.pstatus_tape[k0 - 1], filt.lw_tape[k0 - 1])
        tail = env.rollout_pf_smooth(p["acts"][k0:], sub, p["Q"], paths=S, nonce=NONCE, first_step=k0 + 1, start=start,
                                     end=one.idx[K - 1].clone(), tapes=True)
        assert torch.equal(tail.idx, one.idx[k0:]) and torch.equal(tail.idx0, one.idx[k0 - 1])
        assert torch.equal(tail.x, one.x[k0:]) and torch.equal(tail.var, one.var[k0:])
        # another last row is taken as it is, and the rows below follow from it
        end = torch.randint(0, P, (N, S), dtype=torch.int32, device=env.device,
                            generator=torch.Generator(device=env.device).manual_seed(5))
        other = env.rollout_pf_smooth(p["acts"], filt, p["Q"], paths=S, nonce=NONCE, end=end, tapes=True)
        assert torch.equal(other.idx[K - 1], end) and not torch.equal(other.idx[K - 2], one.idx[K - 2])
    finally:
        env.close()
    # N = 1 with K = 1: the last row alone; with a start, one backward step
    env = F._env("lander3d", 1)
    try:
        env.reset()
        z = torch.zeros((1, 1, 2), dtype=torch.float64, device=env.device)
        H = np.zeros((2, 12))
        H[0, 4], H[1, 5] = 1.0, 1.0
        x0 = np.zeros((12, 1))
        x0[4] = -5.0
        acts = np.full((1, 1, 4), F.AH, np.float32)
        q = np.full(12, 1e-4)
        filt = F._clone(env.rollout_pf(acts, z, H, [0.1, 0.1], q, x0, 0.01 * np.eye(12)[None], particles=64, tape=True))
        res = env.rollout_pf_smooth(acts, filt, q, paths=3)
        assert res.idx.shape == (1, 1, 3) and res.idx0 is None and bool(res.ok.all())
        u = R.draw_u(SEED, 0, 0, 1, np.arange(3))
        assert np.array_equal(to_np(res.idx[0, 0]), R.draw_index(np.repeat(to_np(filt.wq_tape)[0].astype(np.int64), 3, 0), u))
        res = env.rollout_pf_smooth(acts, filt, q, paths=3, start=(filt.part_tape[0], filt.pstatus_tape[0], filt.lw_tape[0]))
        assert res.idx0.shape == (1, 3) and int(res.idx0.min()) >= 0 and int(res.idx0.max()) < 64
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. another task in float32 storage, a model variant, the sharded env
# ---------------------------------------------------------------------------------------------------------------------
def test_every_row_for_another_task_in_float32_storage():
    task, M, P, S = "hover3d", 6, 256, 64
    rng = np.random.default_rng(zlib.crc32(repr((task, M, P, S)).encode()))
    env = F._env(task, N, "float32")
    penv = F._particle_env(task, P, 1, mode="float32")
    try:
        env.reset()
        p = F._problem(env, task, rng, M=M)
        filt = F._clone(F._run(env, p, P))
        res = F._clone(_smooth(env, p, filt, S))
        _check_rows("%s float32 P=%d S=%d" % (task, P, S), penv, p, filt, res, P, S, exact=False)
    finally:
        env.close()
        penv.close()


def test_every_row_under_a_model_variant():
    variant, P, S = "mars_gyro", 256, 64
    rng = np.random.default_rng(zlib.crc32(variant.encode()) + 1)
    env = F._env("lander3d", N, **model_variants.env_kwargs(variant))
    ref = F._env("lander3d", N)
    try:
        installed = model_variants.install(variant, env, rng)
        penv = F._particle_env("lander3d", P, 1, variant=variant, installed=installed)
        try:
            env.reset()
            ref.reset()
            p = F._problem(env, "lander3d", rng, ah=model_variants.hover(variant))
            filt = F._clone(F._run(env, p, P))
            res = F._clone(_smooth(env, p, filt, S))
            _check_rows("lander3d %s" % variant, penv, p, filt, res, P, S)
            # the default model weighs the same tapes otherwise in every env that flies (0, 1 and 4)
            other = to_np(_smooth(ref, p, filt, S).logb_tape[:K - 1])
            same = np.all(_bits(to_np(res.logb_tape[:K - 1])) == _bits(other), axis=(0, 2, 3))
            assert not same[[0, 1, 4]].any(), same
        finally:
            penv.close()
    finally:
        env.close()
        ref.close()


def test_sharded_single_rank_matches_plain_env():
    import torch
    from gym_copter_amd.sharded import ShardedCopterVecEnv
    rng = np.random.default_rng(2401)
    sh = ShardedCopterVecEnv("lander3d", N, device=0, seed=SEED, autoreset_mode="next_step")
    plain = F._env("lander3d", N, "float32")
    try:
        sh.reset()
        plain.reset()
        p = F._problem(plain, "lander3d", rng)
        filt = F._clone(F._run(plain, p, 256))
        a = sh.rollout_pf_smooth(p["acts"], filt, p["Q"], paths=64, nonce=NONCE, tapes=True)
        b = _smooth(plain, p, filt, 64)
        for u, v in zip(a, b):
            assert (u is None and v is None) or torch.equal(u, v)
    finally:
        sh.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import ctypes as C
    import torch
    from gym_copter_amd import CopterStepError, _lib
    rng = np.random.default_rng(2501)
    P, S = 64, 8
    env = F._env("lander3d", N)
    try:
        env.reset()
        p = F._problem(env, "lander3d", rng)
        filt = F._clone(F._run(env, p, P))
        bare = env.rollout_pf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"], particles=P, status0=p["st0"])
        base = dict(actions=p["acts"], filt=filt, Q=p["Q"], paths=S)
        good = F._clone(env.rollout_pf_smooth(**base))
        start = (filt.part_tape[0], filt.pstatus_tape[0], filt.lw_tape[0])
        zero_q = np.diag(p["Q"]).copy()
        zero_q[3] = 0.0
        odd = filt._replace(part_tape=filt.part_tape[:, :, :48].contiguous())
        for kw, match in ((dict(filt=bare), "filt has no tapes"), (dict(filt=filt[:4]), "filt must be the PfResult"),
                          (dict(filt=filt._replace(lw_tape=filt.lw_tape.float())), "filt.lw_tape must be a contiguous"),
                          (dict(filt=filt._replace(wq_tape=filt.wq_tape.long())), "filt.wq_tape must be a contiguous"),
                          (dict(filt=filt._replace(pstatus_tape=filt.pstatus_tape[:, :, :32])), "filt.pstatus_tape must have"),
                          (dict(filt=filt._replace(lw_tape=filt.lw_tape.cpu())), "filt.lw_tape must be a contiguous"),
                          (dict(filt=odd), "P a power of two"),
                          (dict(actions=p["acts"][:5]), "filt.part_tape must have shape"),
                          (dict(actions=p["acts"][:, :N - 1]), "actions must have shape"),
                          (dict(paths=0), "paths must be"), (dict(paths=1025), "paths must be"),
                          (dict(paths=2.0), "paths must be"), (dict(nonce=-1), "nonce must be"),
                          (dict(first_step=0), "first_step must be"), (dict(first_step=2 ** 32 - 3), "below 2\\*\\*32"),
                          (dict(Q=zero_q), "slot 3 has zero variance"), (dict(Q=np.ones((12, 12))), "positive definite"),
                          (dict(Q=p["Q"][:6]), "Q must have shape"), (dict(dtype=torch.float16), "dtype must be"),
                          (dict(start=start[:2]), "start must be the triple"),
                          (dict(start=(start[0], None, start[2])), "start must be the triple"),
                          (dict(start=(start[0], start[1], start[2].float())), "start lw must be a contiguous"),
                          (dict(end=torch.zeros((N, S), dtype=torch.int64, device=env.device)), "end must be a contiguous"),
                          (dict(end=torch.zeros((N, S + 1), dtype=torch.int32, device=env.device)), "end must have shape")):
            args = dict(base)
            args.update(kw)
            with pytest.raises(ValueError, match=match):
                env.rollout_pf_smooth(**args)
        # the C ABI with a live context: a wrong struct_size is CS_ERR_ABI, idx0 without a start CS_ERR_ARG
        io = _lib.RolloutIO()
        io.struct_size, io.num_steps, io.actions_dev = C.sizeof(io), K, p["acts"].data_ptr()
        sio = _lib.PfSmoothIO()
        sio.struct_size, sio.num_particles, sio.num_paths, sio.first_step = C.sizeof(sio), P, S, 1
        sio.part_tape_dev, sio.pstatus_tape_dev = filt.part_tape.data_ptr(), filt.pstatus_tape.data_ptr()
        sio.lw_tape_dev, sio.wq_tape_dev = filt.lw_tape.data_ptr(), filt.wq_tape.data_ptr()
        Linv = torch.from_numpy(R.noise_inverse(p["Q"])).to(env.device)
        idx0 = torch.zeros((N, S), dtype=torch.int32, device=env.device)
        sio.Linv_dev, sio.idx0_dev = Linv.data_ptr(), idx0.data_ptr()
        call = lambda e: e._lib.cs_pf_smooth(e._ctx, C.byref(io), C.byref(sio), None)      # noqa: E731
        assert call(env) == _lib.ERR_ARG and b"idx0_dev needs" in env._lib.cs_last_error()
        sio.part_in_dev, sio.pstatus_in_dev = start[0].data_ptr(), start[1].data_ptr()
        assert call(env) == _lib.ERR_ARG and b"all three or none" in env._lib.cs_last_error()
        sio.idx0_dev, sio.part_in_dev, sio.pstatus_in_dev = None, None, None
        sio.struct_size = C.sizeof(sio) + 8
        assert call(env) == _lib.ERR_ABI
        sio.struct_size = C.sizeof(sio)
        assert call(env) == 0                                  # every output NULL: nothing to write, no error
        torch.cuda.synchronize()
        env.serve_begin(2)
        try:
            with pytest.raises(CopterStepError, match="serv"):
                env.rollout_pf_smooth(**base)
        finally:
            env.serve_end(wait=False)
        # ... and the refusals left nothing behind
        for a, b in zip(env.rollout_pf_smooth(**base), good):
            assert (a is None and b is None) or torch.equal(a, b)
        f32 = F._env("lander3d", N, action_arith="float32")
        try:
            f32.reset()
            with pytest.raises(ValueError, match='not available under action_arith="float32"'):
                f32.rollout_pf_smooth(**base)
            assert call(f32) == _lib.ERR_ARG and b"float32 motor model" in f32._lib.cs_last_error()
        finally:
            f32.close()
    finally:
        env.close()
    with pytest.raises(RuntimeError, match="closed"):
        env.rollout_pf_smooth(**base)


# ---------------------------------------------------------------------------------------------------------------------
# 6. application
# ---------------------------------------------------------------------------------------------------------------------
def test_smoothing_improves_the_unmeasured_velocities():
    """Hover3D, section 19's sensors and P0, 32 envs, 32 steps, 1 024 particles, 256 paths: the inputs of
    test_pf_smooth_cpu.py::test_application_improves_the_velocities_on_the_oracle.  On the float64 oracle the smoothed
    RMSE of dX, dY, dZ over the interior rows is 0.949 / 1.044 / 1.236 m/s against the filter's 1.020 / 1.167 / 1.377 --
    better in every one of the three slots, pooled ratio 0.905 (pf_smooth_ref.APP_CPU_RATIO).  The device filters and
    draws with other ties than that chain, so it is another sample of the same estimator: its pooled ratio may be 25 %
    worse, and the smoothed RMSE must be below the filter's."""
    a, x0, xhat0, H, r = pf_ref.app_inputs(F.AH, seed=1)
    n, P = pf_ref.APP_N, pf_ref.APP_P
    env = F._env("hover3d", n, seed=pf_ref.APP_SEED)
    try:
        import ekf_ref
        env.reset()
        acts = F._dev(a, env)
        ro = env.rollout_states(acts, state={"x": x0, "status": np.full(n, AIRBORNE, np.uint8)})
        truth = to_np(ro.x).astype(np.float64)
        z = F._dev(pf_ref.app_measurements(truth, H, r), env)
        P0 = F._dev(np.repeat(ekf_ref.APP_P0[None], n, axis=0), env)
        filt = env.rollout_pf(acts, z, H, r, pf_ref.APP_Q, F._dev(xhat0, env), P0, particles=P, nonce=pf_ref.APP_NONCE,
                              tape=True)
        res = env.rollout_pf_smooth(acts, filt, pf_ref.APP_Q, paths=R.APP_S, nonce=R.APP_SMOOTH_NONCE)
        assert bool(res.ok.all())
        for slot in R.APP_VEL_SLOTS:
            s, fl = R.app_ratio(to_np(res.x), to_np(filt.x), truth, slots=(slot,))
            print("slot %d: smoothed rmse %.4f, filtered %.4f, ratio %.3f" % (slot, s, fl, s / fl))
            assert s < fl, slot
        s, fl = R.app_ratio(to_np(res.x), to_np(filt.x), truth)
        print("pooled: smoothed rmse %.4f, filtered %.4f, ratio %.4f (cpu %.3f)" % (s, fl, s / fl, R.APP_CPU_RATIO))
        assert s < fl
        assert s / fl <= R.APP_CPU_RATIO * 1.25, s / fl
    finally:
        env.close()
