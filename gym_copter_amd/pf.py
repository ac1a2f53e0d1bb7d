"""The bootstrap particle filter's host side: CopterVecEnv.rollout_pf -- one call of
cs_rollout_pf on the env's cached buffers; vecenv.py binds it to the class -- and pf(), a small streaming driver on it
for a filter whose measurements arrive a chunk of steps at a time.

    x_p <- step(x_p, a) + Lq eps;     lw_p <- lw_p - 1/2 sum (z_i - H[i] x_p)^2 / r_i;     systematic resampling

The particles, their statuses and their log-weights are carried from call to call on the device; nothing is read by the
host.  Synthetic measurements to try it on: gym_copter_amd.measure.

And the filter's smoother: CopterVecEnv.rollout_pf_smooth -- one call of cs_pf_smooth, backward
simulation over the filter's tapes; CopterVecEnv inherits it from ParticleSmoother -- and pf_smooth(), its chunked driver,
which also gathers the drawn trajectories."""
import collections

import numpy as np

from . import _lib, _wire
from . import ekf as _ekf
from . import rollout as _rollout
from ._wire import _torch


# CopterVecEnv.rollout_pf's result: the weighted means x [K,N,12] and variances var [K,N,12] before
# each step's resampling, ess [K,N], resampled [K,N] bool, best [K,N] int32 (the heaviest particle) and its status
# [K,N], the weighted covariance after step K P [N,12,12], loglik [N], ok [N] bool; the carried state after step K,
# post-resample: part [N,P,12], pstatus [N,P], lw [N,P]; and with tape=True (else None) part_tape [K,N,P,12] (the prior
# particles), pstatus_tape [K,N,P], lw_tape [K,N,P], wq_tape [K,N,P] int32 (the integer weights, <= 2^24) and anc_tape
# [K,N,P] int32
PfResult = collections.namedtuple("PfResult", "x var ess resampled best status P loglik ok part pstatus lw part_tape "
                                              "pstatus_tape lw_tape wq_tape anc_tape")


def _noise_factor(q):
    """Lq of the process noise q, a finite float64 host array: Q [12,12] symmetric positive definite is factored
    (numpy.linalg.cholesky), Q [12] of variances >= 0 gives diag sqrt(Q)."""
    if q.shape == (12,):
        if not (q >= 0).all():
            raise ValueError("Q must be >= 0: the process noise variances")
        return np.diag(np.sqrt(q))
    if q.shape != (12, 12):
        raise ValueError("Q must have shape (12, 12) or (12,), got %s" % (q.shape,))
    if not np.array_equal(q, q.T):
        raise ValueError("Q must be symmetric")
    try:
        return np.linalg.cholesky(q)
    except np.linalg.LinAlgError:
        raise ValueError("Q must be positive definite (a Q with zero variances: pass the 12 variances)") from None


def rollout_pf(self, actions, z, H, r, Q, x0=None, P0=None, particles=256, nonce=0, ess_frac=0.5, status0=None,
               start=None, first_step=1, tape=False, dtype=None):
    """A bootstrap particle filter over the env step, K steps of propagate / weight / estimate / resample per env in
    one kernel, `particles` particles per env that stay on the compute unit: the sampling twin of rollout_ekf, for a
    belief that straddles a branch of the step (touchdown, crash, the motor clip).  The filter's state is the
    caller's: NO env state is read but the configuration and the vehicle, and none changes.

    actions [K,N,A], z [K,N,M] (NaN = no measurement), H [M,12] and r [M] > 0 are rollout_ekf's.  Q is the process
    noise added to every particle each step whatever its status: [12,12] symmetric positive definite, or [12]
    variances (zeros allowed).  The start is either Gaussian -- x0 [12,N], P0 [N,12,12] symmetric positive definite
    (factored by torch.linalg.cholesky; None: every particle starts at x0), status0 [N] uint8 (default AIRBORNE) --
    or start=, a previous PfResult (or its (part, pstatus, lw)): the particles carried after its last step.
    first_step is the global index of this call's first step, so that a run in chunks draws the noise of a single
    call; nonce selects another noise stream.  particles is a power of two in 64 .. 1024.  The step resamples
    (systematically, on integer weights) when its effective sample size is below ess_frac * particles.

    Returns PfResult (see its comment).  dtype: torch.float64 (default) or torch.float32 (var, ess, P, loglik: the
    float64 values rounded).  Not available under action_arith="float32".  Asynchronous on the current stream; the
    tensors are buffers of this env, overwritten by its next call with the same K, particles, dtype and tape (a
    `start` that is such a buffer is read before it is overwritten)."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    Hd, rd, Lqd = _wire.uploaded(self, "pf", lambda: (
        *_ekf._measurement_model(H, r), _noise_factor(_ekf._host_array(Q, "Q"))), given=(H, r, Q))
    M = int(Hd.shape[0])
    P = _wire.int_in(particles, "particles", _lib.PF_MIN_PARTICLES, _lib.PF_MAX_PARTICLES + 1,
                     "a power of two in %d .. %d" % (_lib.PF_MIN_PARTICLES, _lib.PF_MAX_PARTICLES),
                     ok=lambda p: not p & (p - 1))
    nonce = _wire.int_in(nonce, "nonce", 0, _wire.U32, _wire.IN_U32)
    first_step = _wire.int_in(first_step, "first_step", 1, None, "an int >= 1")
    if not 0.0 <= float(ess_frac) <= 1.0:
        raise ValueError("ess_frac must be in [0, 1], got %r" % (ess_frac,))
    io, K, keep = _rollout._rollout_io(self, actions, None)
    if first_step + K - 1 >= _wire.U32:
        raise ValueError("first_step + K - 1 must be below 2**32")
    n = self.num_envs
    zt = _ekf._input(self, z, (K, n, M), "z", keep)
    pio = _wire.block(_lib.RolloutPfIO, out_dtype=_wire.dtype_code(dtype), num_meas=M, num_particles=P, nonce=nonce,
                      first_step=first_step, ess_frac=float(ess_frac))
    if (x0 is None) == (start is None):
        raise ValueError("give exactly one start: x0 (with P0, status0) or start (a previous PfResult)")
    if start is not None:
        if P0 is not None or status0 is not None:
            raise ValueError("P0 and status0 belong to the Gaussian start: leave them out with start=")
        if isinstance(start, PfResult):
            start = (start.part, start.pstatus, start.lw)
        if not isinstance(start, (tuple, list)) or len(start) != 3:
            raise ValueError("start must be a PfResult or its (part, pstatus, lw)")
        _wire.check_tape(self, "rollout_pf", (start[0], "start part", (n, P, 12), torch.float64),
                         (start[1], "start pstatus", (n, P), torch.uint8),
                         (start[2], "start lw", (n, P), torch.float64))
        keep.extend(start)
        pio.part_in_dev, pio.pstatus_in_dev, pio.lw_in_dev = (t.data_ptr() for t in start)
    else:
        xt = _ekf._input(self, x0, (12, n), "x0", keep)
        io.start_x_dev = xt.data_ptr()
        io.start_status_dev = _ekf._start_status(self, status0, keep)
        if P0 is not None:
            Pt = _ekf._input(self, P0, (n, 12, 12), "P0", keep)
            try:
                L0 = torch.linalg.cholesky(Pt).contiguous()
            except RuntimeError as e:          # torch.linalg.LinAlgError
                raise ValueError("P0 must be symmetric positive definite: %s" % e) from None
            keep.append(L0)
            pio.L0_dev = L0.data_ptr()
    tape = bool(tape)
    e = lambda shape, dt: _wire.empty(self, shape, dt)      # noqa: E731
    out = _wire.rollout_cache(self, ("pf", K, P, dtype, tape), lambda: PfResult(
        e((K, n, 12), torch.float64), e((K, n, 12), dtype), e((K, n), dtype), e((K, n), torch.bool),
        e((K, n), torch.int32), e((K, n), torch.uint8), e((n, 12, 12), dtype), e(n, dtype), e(n, torch.bool),
        e((n, P, 12), torch.float64), e((n, P), torch.uint8), e((n, P), torch.float64),
        e((K, n, P, 12), torch.float64) if tape else None, e((K, n, P), torch.uint8) if tape else None,
        e((K, n, P), torch.float64) if tape else None, e((K, n, P), torch.int32) if tape else None,
        e((K, n, P), torch.int32) if tape else None))
    io.x_dev, io.status_dev = out.x.data_ptr(), out.status.data_ptr()
    pio.H_dev, pio.r_dev, pio.Lq_dev, pio.z_dev = Hd.data_ptr(), rd.data_ptr(), Lqd.data_ptr(), zt.data_ptr()
    pio.var_dev, pio.ess_dev, pio.resampled_dev = out.var.data_ptr(), out.ess.data_ptr(), out.resampled.data_ptr()
    pio.best_dev, pio.P_dev, pio.loglik_dev, pio.ok_dev = (out.best.data_ptr(), out.P.data_ptr(),
                                                           out.loglik.data_ptr(), out.ok.data_ptr())
    pio.part_out_dev, pio.pstatus_out_dev, pio.lw_out_dev = (out.part.data_ptr(), out.pstatus.data_ptr(),
                                                             out.lw.data_ptr())
    if tape:
        pio.part_tape_dev, pio.pstatus_tape_dev = out.part_tape.data_ptr(), out.pstatus_tape.data_ptr()
        pio.lw_tape_dev, pio.wq_tape_dev = out.lw_tape.data_ptr(), out.wq_tape.data_ptr()
        pio.anc_tape_dev = out.anc_tape.data_ptr()
    _wire.launch(self, "cs_rollout_pf", io, pio, keep=keep + [Hd, rd, Lqd])
    return out


# -- the backward-simulation smoother over the filter's tapes ------------------------------------------
# CopterVecEnv.rollout_pf_smooth's result: the means x [K,N,12] and variances var [K,N,12] of the S drawn particles of
# every row, idx [K,N,S] int32 (the particle of row k on path m: trajectory m is part_tape[k, env, idx[k, env, m]]),
# idx0 [N,S] int32 (the particles of the start set, with start=; else None), ok [N] bool, and with tapes=True (else None)
# logb_tape [K,N,S,P] float64 and bwq_tape [K,N,S,P] int32
PfSmoothResult = collections.namedtuple("PfSmoothResult", "x var idx idx0 ok logb_tape bwq_tape")

# pf_smooth's result: PfSmoothResult's x, var, idx and ok, and paths_x [K,N,S,12], the S trajectories themselves
PfPaths = collections.namedtuple("PfPaths", "x var idx ok paths_x")


def noise_inverse(Q):
    """Linv = Lq^-1 of the process noise Q ([12,12] or [12], as rollout_pf takes it), lower triangular, by forward
    substitution in float64 on the host (one column at a time, sums in ascending order): what rollout_pf_smooth
    uploads.  A singular factor -- a zero variance among the 12, or a zero pivot -- raises ValueError: the transition
    density the smoother weighs with does not exist."""
    L = _noise_factor(_ekf._host_array(Q, "Q"))
    d = np.diag(L)
    if not (d > 0).all():
        raise ValueError("Q must be nonsingular for the smoother: slot %d has zero variance, so the transition has no "
                         "density there" % int(np.flatnonzero(~(d > 0))[0]))
    X = np.zeros((12, 12))
    for c in range(12):
        X[c, c] = 1.0 / L[c, c]
        for r in range(c + 1, 12):
            acc = 0.0
            for j in range(c, r):
                acc = acc + L[r, j] * X[j, c]
            X[r, c] = -acc / L[r, r]
    if not np.isfinite(X).all():
        raise ValueError("Q must be nonsingular for the smoother: the inverse of its factor is not finite")
    return X


def rollout_pf_smooth(self, actions, filt, Q, paths=256, nonce=0, first_step=1, start=None, end=None, tapes=False,
                      dtype=None):
    """A backward-simulation particle smoother (forward filtering, backward simulation) over the tapes of rollout_pf,
    K backward steps per env in one kernel: `paths` trajectories per env drawn backwards through the taped particle
    sets, each earlier particle reweighted by its filter weight times the transition density N(x_next; step(x), Q) --
    and by whether the step takes it to the next point's flight status.  The particle filter's counterpart of
    rollout_rts; NO env state is read but the configuration and the vehicle, and none changes.

    actions [K,N,A] and Q are the filter's; filt is its PfResult with the tapes (rollout_pf(..., tape=True) or pf());
    nonce selects the stream of the backward draws (it need not be the filter's) and first_step is the filter's, so
    that a run in chunks draws what a single call draws.  Q must be nonsingular ([12]: every variance > 0).  paths is
    1 .. 1024.  end [N,paths] int32: the particles of the last row, indices in [0, P) (the device takes them mod P;
    None: drawn from the filter's last weights).
    start: the prior particles of the step before this call's first -- (part [N,P,12], pstatus [N,P], lw [N,P]), rows of
    the filter's tapes -- for one more backward step, whose indices come back as idx0.

    Returns PfSmoothResult (see its comment); ok [N] is False where some path found no particle that reaches its next
    point (the draw was then uniform).  dtype: torch.float64 (default) or torch.float32 (var: the float64 values
    rounded).  Not available under action_arith="float32".  Asynchronous on the current stream; the tensors are buffers
    of this env, overwritten by its next call with the same K, particles, paths, dtype, tapes and start."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    if self.config.action_arith != _lib.ARITH_F64:
        raise ValueError('rollout_pf_smooth is not available under action_arith="float32"')
    Linv, = _wire.uploaded(self, "pf_smooth", lambda: (noise_inverse(Q),), given=(Q,))
    S = _wire.int_in(paths, "paths", 1, _lib.PFS_MAX_PATHS + 1, "an int in 1 .. %d" % _lib.PFS_MAX_PATHS)
    nonce = _wire.int_in(nonce, "nonce", 0, _wire.U32, _wire.IN_U32)
    first_step = _wire.int_in(first_step, "first_step", 1, None, "an int >= 1")
    io, K, keep = _rollout._rollout_io(self, actions, None)
    if first_step + K - 1 >= _wire.U32:
        raise ValueError("first_step + K - 1 must be below 2**32")
    n = self.num_envs
    if not isinstance(filt, PfResult):
        raise ValueError("filt must be the PfResult of rollout_pf(..., tape=True)")
    if any(t is None for t in (filt.part_tape, filt.pstatus_tape, filt.lw_tape, filt.wq_tape)):
        raise ValueError("filt has no tapes: filter with rollout_pf(..., tape=True)")
    shape = tuple(filt.part_tape.shape) if isinstance(filt.part_tape, torch.Tensor) else ()
    P = shape[2] if len(shape) == 4 else 0
    if P < _lib.PF_MIN_PARTICLES or P > _lib.PF_MAX_PARTICLES or P & (P - 1):
        raise ValueError("filt.part_tape must have shape (K, N, P, 12) with P a power of two in %d .. %d, got %s"
                         % (_lib.PF_MIN_PARTICLES, _lib.PF_MAX_PARTICLES, shape))
    _wire.check_tape(self, "rollout_pf", (filt.part_tape, "filt.part_tape", (K, n, P, 12), torch.float64),
                     (filt.pstatus_tape, "filt.pstatus_tape", (K, n, P), torch.uint8),
                     (filt.lw_tape, "filt.lw_tape", (K, n, P), torch.float64),
                     (filt.wq_tape, "filt.wq_tape", (K, n, P), torch.int32))
    sio = _wire.block(_lib.PfSmoothIO, out_dtype=_wire.dtype_code(dtype), num_particles=P, num_paths=S, nonce=nonce,
                      first_step=first_step)
    if end is not None:
        _wire.check_tape(self, "rollout_pf_smooth", (end, "end", (n, S), torch.int32))
        keep.append(end)
    if start is not None:
        if not isinstance(start, (tuple, list)) or len(start) != 3 or any(t is None for t in start):
            raise ValueError("start must be the triple (part [N,P,12], pstatus [N,P], lw [N,P]): all three or none")
        _wire.check_tape(self, "rollout_pf", (start[0], "start part", (n, P, 12), torch.float64),
                         (start[1], "start pstatus", (n, P), torch.uint8),
                         (start[2], "start lw", (n, P), torch.float64))
        keep.extend(start)
        sio.part_in_dev, sio.pstatus_in_dev, sio.lw_in_dev = (t.data_ptr() for t in start)
    tapes = bool(tapes)
    e = lambda shape, dt: _wire.empty(self, shape, dt)      # noqa: E731
    out = _wire.rollout_cache(self, ("pf_smooth", K, P, S, dtype, tapes, start is not None), lambda: PfSmoothResult(
        e((K, n, 12), torch.float64), e((K, n, 12), dtype), e((K, n, S), torch.int32),
        e((n, S), torch.int32) if start is not None else None, e(n, torch.bool),
        e((K, n, S, P), torch.float64) if tapes else None, e((K, n, S, P), torch.int32) if tapes else None))
    if end is not None:
        # (no output may overlap an input: a caller's end that is this call's own idx0 buffer is copied first)
        if out.idx0 is not None and end.data_ptr() == out.idx0.data_ptr():
            end = end.clone()
            keep.append(end)
        sio.end_idx_dev = end.data_ptr()
    io.x_dev = out.x.data_ptr()
    sio.part_tape_dev, sio.pstatus_tape_dev = filt.part_tape.data_ptr(), filt.pstatus_tape.data_ptr()
    sio.lw_tape_dev, sio.wq_tape_dev, sio.Linv_dev = filt.lw_tape.data_ptr(), filt.wq_tape.data_ptr(), Linv.data_ptr()
    sio.var_dev, sio.idx_dev, sio.ok_dev = out.var.data_ptr(), out.idx.data_ptr(), out.ok.data_ptr()
    if out.idx0 is not None:
        sio.idx0_dev = out.idx0.data_ptr()
    if tapes:
        sio.logb_tape_dev, sio.bwq_tape_dev = out.logb_tape.data_ptr(), out.bwq_tape.data_ptr()
    _wire.launch(self, "cs_pf_smooth", io, sio,
                 keep=keep + [Linv, filt.part_tape, filt.pstatus_tape, filt.lw_tape, filt.wq_tape])
    return out


class ParticleSmoother:
    """CopterVecEnv's particle smoother, a base class of it, like ukf.UnscentedSmoother: the class
    body's rollout_* methods are the closed list that tests/test_gpu_output_bounds.py covers one by one, and this one is
    held to the same memory contract in a file of its own, tests/test_gpu_pf_smooth_memory.py."""
    rollout_pf_smooth = rollout_pf_smooth


def pf_smooth(env, actions, filt, Q, paths=256, nonce=0, chunk=None):
    """Run env.rollout_pf_smooth over the K steps of a particle filter's tapes in chunks of `chunk` steps (None: one
    call), last chunk first: a chunk that starts at row k0 > 0 takes the filter's tapes at row k0 - 1 as its start set,
    and the chunk before it ends in the indices (idx0) that chunk returned.  filt is the PfResult of the whole filter
    with its tapes (its first step is step 1: rollout_pf's default, and pf()'s).  Returns PfPaths: x, var [K,N,12], idx
    [K,N,S] and ok [N] -- bit-identical to the single call's, tensors of their own -- and paths_x [K,N,S,12], the S
    trajectories gathered from filt.part_tape by idx."""
    torch = _torch()
    K = int(actions.shape[0])
    chunk = K if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %r" % (chunk,))
    if not isinstance(filt, PfResult) or any(t is None for t in (filt.part_tape, filt.pstatus_tape, filt.lw_tape,
                                                                  filt.wq_tape)):
        raise ValueError("filt must be a PfResult with its tapes (rollout_pf(..., tape=True) or pf())")
    taped = (filt.part_tape, filt.pstatus_tape, filt.lw_tape, filt.wq_tape)
    for t in taped:
        if not isinstance(t, torch.Tensor) or t.shape[0] != K:
            raise ValueError("filt's tapes must be tensors of K = %d rows" % K)
    parts, end, ok = [], None, None
    for k0 in reversed(range(0, K, chunk)):
        k1 = min(k0 + chunk, K)
        sub = PfResult(*([None] * 12), *(t[k0:k1] for t in taped), None)
        start = None if k0 == 0 else tuple(t[k0 - 1] for t in taped[:3])
        res = env.rollout_pf_smooth(actions[k0:k1], sub, Q, paths=paths, nonce=nonce, first_step=k0 + 1, start=start,
                                    end=end)
        parts.append([t.clone() for t in (res.x, res.var, res.idx)])
        end = None if res.idx0 is None else res.idx0.clone()
        ok = res.ok.clone() if ok is None else ok & res.ok
    x, var, idx = (torch.cat([p[j] for p in reversed(parts)]) for j in range(3))
    at = idx.long().unsqueeze(-1).expand(-1, -1, -1, 12)
    return PfPaths(x, var, idx, ok, torch.gather(filt.part_tape, 2, at))


def pf(env, actions, z, H, r, Q, x0, P0, particles, nonce=0, ess_frac=0.5, status0=None, chunk=None, tape=True):
    """Run env.rollout_pf over actions [K,N,A] and z [K,N,M] in chunks of `chunk` steps (None: one call), as a filter
    whose measurements arrive `chunk` at a time: the particles after each chunk start the next, and first_step tells
    every chunk where it stands, so that it draws the noise a single call draws.  Returns PfResult with the tapes of all K
    steps concatenated (the particle tapes with tape=True), P the weighted covariance after the last step, loglik the sum
    of the chunks' and ok their conjunction -- tensors of their own, not the env's buffers.  Every tape, the carried
    state, P and ok are bit-identical to the single call's: a chunk boundary rounds nothing (float64 throughout).  loglik
    equals the single call's to rounding only: it is the sum of the chunks' sums.  The other arguments are rollout_pf's."""
    taped = ("x", "var", "ess", "resampled", "best", "status") + \
        (("part_tape", "pstatus_tape", "lw_tape", "wq_tape", "anc_tape") if tape else ())

    def call(a, zc, k0, prev):      # the carried state is the chunk before's result itself (None: the Gaussian start)
        kw = dict(particles=particles, nonce=nonce, ess_frac=ess_frac, first_step=k0 + 1, tape=tape)
        if prev is None:
            return env.rollout_pf(a, zc, H, r, Q, x0, P0, status0=status0, **kw)
        return env.rollout_pf(a, zc, H, r, Q, start=prev, **kw)
    cat, res, loglik, ok = _ekf._chunked(actions, z, chunk, taped, None, call, lambda res: res)
    return PfResult(cat["x"], cat["var"], cat["ess"], cat["resampled"], cat["best"], cat["status"], res.P.clone(), loglik,
                    ok, res.part.clone(), res.pstatus.clone(), res.lw.clone(), cat.get("part_tape"),
                    cat.get("pstatus_tape"), cat.get("lw_tape"), cat.get("wq_tape"), cat.get("anc_tape"))
