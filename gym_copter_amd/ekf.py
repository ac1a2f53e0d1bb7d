"""The extended Kalman filter's host side: CopterVecEnv.rollout_ekf and the smoother over its
tapes, CopterVecEnv.rollout_rts -- one library call each on the env's cached buffers; vecenv.py
binds them to the class -- the kit the other filters (pf.py, lqg.py, ukf.py) share with them, a small streaming driver
for a filter whose measurements arrive a chunk of steps at a time, the synthetic measurements to try it on, and the
chunked driver of the smoothers (this one's and ukf.py's rollout_urts).

    z = H x + e,  e ~ N(0, diag(r));     x- = step(xhat, a),  P- = A P A^T + Q;     sequential scalar updates

The filter's state (mean, covariance, flight status) is carried from call to call on the device; nothing is read by the
host."""
import collections

import numpy as np

from . import _lib, _wire
from . import rollout as _rollout
from ._wire import _torch

# CopterVecEnv.rollout_ekf's result: the filtered means x [K,N,12] and the priors x_pred [K,N,12], the
# last posterior covariance P [N,12,12], its diagonal per step var [K,N,12], nis [K,N], loglik [N], the status [K,N] and
# step_jacobian branch bits [K,N] of the filter's own mean, ok [N] bool, and P_tape [K,N,12,12] (None without tape=True)
EkfResult = collections.namedtuple("EkfResult", "x x_pred P var nis loglik status branch ok P_tape")
# CopterVecEnv.rollout_rts' result: the smoothed means x [K,N,12], their covariances P_tape
# [K,N,12,12] (None with tape=False) and diagonals var [K,N,12], the smoothed starting point x0 [12,N], P0 [N,12,12], and
# ok [N] bool (every Cholesky pivot positive and finite)
RtsResult = collections.namedtuple("RtsResult", "x P_tape var x0 P0 ok")


# -- the filter family (DESIGN sections 19 to 23): the model every env and step shares, and the start's status.  pf.py,
#    lqg.py and ukf.py use this kit too --------
def _kalman_model(env, slot, H, r, Q):
    """(Hd, rd, Qd, M): the checked model of rollout_ekf, rollout_lqg and rollout_ukf on the device, from the
    entry point's cache `slot` (_wire.uploaded: host arrays by value, the same device tensors by identity)."""
    Hd, rd, Qd = _wire.uploaded(env, slot, lambda: (*_measurement_model(H, r), _process_noise(Q)), given=(H, r, Q))
    return Hd, rd, Qd, int(Hd.shape[0])


def _kalman_tensors(env, K, n, dtype, tape):
    """The ten result tensors those three have in common, in EkfResult's order: x, x_pred, P, var, nis, loglik,
    status, the step's byte (branch or spread), ok, P_tape (None without tape)."""
    torch = _torch()
    e = lambda shape, dt: _wire.empty(env, shape, dt)      # noqa: E731
    return (e((K, n, 12), torch.float64), e((K, n, 12), torch.float64), e((n, 12, 12), dtype), e((K, n, 12), dtype),
            e((K, n), dtype), e(n, dtype), e((K, n), torch.uint8), e((K, n), torch.uint8), e(n, torch.bool),
            e((K, n, 12, 12), dtype) if tape else None)


def _kalman_wire(struct_cls, dtype, model, P0, res):
    """A cs_rollout_ekf_io, cs_rollout_lqg_io or cs_rollout_ukf_io with the fields the three share by name: its size,
    dtype, the model (_kalman_model's), P0 and the outputs of `res` (an EkfResult or a UkfResult)."""
    Hd, rd, Qd, M = model
    fio = _wire.block(struct_cls)          # (filled member by member: three filters call this every chunk)
    fio.out_dtype, fio.num_meas = _wire.dtype_code(dtype), M
    fio.H_dev, fio.r_dev, fio.Q_dev, fio.P0_dev = Hd.data_ptr(), rd.data_ptr(), Qd.data_ptr(), P0.data_ptr()
    fio.x_pred_dev, fio.P_dev, fio.var_dev = res.x_pred.data_ptr(), res.P.data_ptr(), res.var.data_ptr()
    fio.nis_dev, fio.loglik_dev, fio.ok_dev = res.nis.data_ptr(), res.loglik.data_ptr(), res.ok.data_ptr()
    if res.P_tape is not None:
        fio.P_tape_dev = res.P_tape.data_ptr()
    return fio


def _host_array(m, name):
    """m, a tensor or an array of real numbers, as a finite float64 host array."""
    a = np.asarray(m.detach().cpu() if isinstance(m, _torch().Tensor) else m)
    if a.dtype.kind not in "fiu":
        raise ValueError("%s must be a real floating-point array, got dtype %s" % (name, a.dtype))
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    return a


def _measurement_model(H, r):
    """H [M,12] (1 <= M <= 12) and r [M] > 0 of rollout_ekf and rollout_pf, on the host."""
    h = _host_array(H, "H")
    if h.ndim != 2 or h.shape[1] != 12 or not 1 <= h.shape[0] <= _lib.EKF_MAX_MEAS:
        raise ValueError("H must have shape (M, 12) with 1 <= M <= %d, got %s" % (_lib.EKF_MAX_MEAS, h.shape))
    rv = _host_array(r, "r")
    if rv.shape != (h.shape[0],):
        raise ValueError("r must have shape (%d,) (one variance per row of H), got %s" % (h.shape[0], rv.shape))
    if not (rv > 0).all():
        raise ValueError("r must be positive: the measurement variances")
    return h, rv


def _process_noise(Q):
    """Q [12,12] symmetric of rollout_ekf and rollout_rts, on the host."""
    q = _host_array(Q, "Q")
    if q.shape != (12, 12):
        raise ValueError("Q must have shape (12, 12), got %s" % (q.shape,))
    if not (q == q.T).all():
        raise ValueError("Q must be symmetric")
    return q


def _start_status(env, status0, keep):
    """The start_status_dev of a filter's start: the caller's status0 [N] uint8, AIRBORNE by default."""
    torch = _torch()
    if status0 is None:
        st = torch.full((env.num_envs,), _lib.STATUS_AIRBORNE, dtype=torch.uint8, device=env.device)
        keep.append(st)
        return st.data_ptr()
    return _rollout._state(env, status0, (env.num_envs,), torch.uint8, "status0", keep)


def _input(env, v, shape, name, keep):
    """A per-env input of a filter as a contiguous float64 device tensor, kept alive in `keep`: a floating-point
    tensor on this env's device, or a host array."""
    return _wire.tensor(env, v, shape, _torch().float64, name, keep, floating=True, strict=True, foreign=False)


# -- the extended Kalman filter over the env step: CopterVecEnv.rollout_ekf, bound in vecenv.py ------
def rollout_ekf(self, actions, z, H, r, Q, x0, P0, status0=None, tape=False, dtype=None):
    """An extended Kalman filter over the env step, K predict / update steps per env in one kernel: the mean goes
    through the step's own physics, the covariance through the step Jacobian of step_jacobian (every branch rule of
    DESIGN section 9), applied on the fly and never stored.  The filter's state is the caller's: NO env state is read
    but the configuration and the vehicle, and none changes.

    actions [K,N,A]: step k takes actions[k-1].  z [K,N,M] float64: the measurements z = H x + e, e ~ N(0, diag(r));
    a NaN entry means "no measurement" and its update is skipped.  H [M,12] (1 <= M <= 12), r [M] > 0 and Q [12,12]
    symmetric PSD (the process noise added per step) are shared by every env and step.  x0 [12,N] float64 and
    P0 [N,12,12] (symmetric: its upper triangle is read) are the mean and covariance before step 1; status0 [N] uint8
    the flight status of that mean (default AIRBORNE).

    Per step: x- = the physics from (xhat, status), P- = A P A^T + Q; then for each row i of H in order, skipping NaN
    z: p = P h, s = h^T p + r_i, nu = z_i - h^T x, x += (p / s) nu, P -= (p / s) p^T.

    Returns EkfResult(x [K,N,12] the filtered means, x_pred [K,N,12] the priors, P [N,12,12] the last posterior, var
    [K,N,12] the posteriors' diagonals, nis [K,N] the steps' sums of nu^2 / s, loglik [N] the sum of
    -1/2 (nu^2 / s + ln(2 pi s)), status [K,N] and branch [K,N] (step_jacobian's bits) of the filter's own mean, ok
    [N] bool (False where some s was not finite or <= 0), P_tape [K,N,12,12] with tape=True, else None).  dtype:
    torch.float64 (default) or torch.float32 (P, var, nis, loglik, P_tape: the float64 values rounded).  Not available
    under action_arith="float32".  Asynchronous on the current stream; the tensors are buffers of this env,
    overwritten by its next call with the same K, dtype and tape."""
    self._check_open()
    dtype = _wire.out_dtype(dtype)
    model = _kalman_model(self, "ekf", H, r, Q)
    M = model[3]
    io, K, keep = _rollout._rollout_io(self, actions, None)
    n = self.num_envs
    zt = _input(self, z, (K, n, M), "z", keep)
    xt = _input(self, x0, (12, n), "x0", keep)
    Pt = _input(self, P0, (n, 12, 12), "P0", keep)
    io.start_status_dev = _start_status(self, status0, keep)
    io.start_x_dev = xt.data_ptr()
    tape = bool(tape)
    out = _wire.rollout_cache(self, ("ekf", K, dtype, tape), lambda: EkfResult(*_kalman_tensors(self, K, n, dtype, tape)))
    eio = _kalman_wire(_lib.RolloutEkfIO, dtype, model, Pt, out)
    eio.z_dev, eio.branch_dev = zt.data_ptr(), out.branch.data_ptr()
    io.x_dev, io.status_dev = out.x.data_ptr(), out.status.data_ptr()
    _wire.launch(self, "cs_rollout_ekf", io, eio, keep=keep + list(model[:3]))
    return out


# -- the Rauch-Tung-Striebel smoother over the filter's tapes: CopterVecEnv.rollout_rts --------
def rollout_rts(self, actions, filt, Q, x0, P0, status0=None, end=None, tape=True, dtype=None):
    """A Rauch-Tung-Striebel fixed-interval smoother over the tapes of rollout_ekf, K backward steps per env in one
    kernel: the estimate of every step given the measurements of all K steps, and that of the starting point.  The
    step Jacobian is applied on the fly at the filter's own points and never stored.  NO env state is read but the
    configuration and the vehicle, and none changes.

    actions [K,N,A], Q, x0 [12,N], P0 [N,12,12] and status0 are what the filter was given; filt is its EkfResult
    from rollout_ekf(..., tape=True) in float64 (x, x_pred, status and P_tape are read).  Q should be positive
    definite: a merely PSD Q can make a prior singular, which clears ok.  end = (x_end [12,N], P_end [N,12,12])
    gives the smoothed last row (default: the filter's own last row) -- the smoothed starting point of the chunk that
    follows, for a tape smoothed in chunks (gym_copter_amd.smooth).

    Row K-1 is the given one; then for j = K-2 down to -1 (row -1 is the starting point), with A the step Jacobian at
    (x_f[j], status_f[j]) under actions[j+1]:  P- = A P_f[j] A^T + Q (the filter's prior, bit for bit),
    G = P-^-1 A P_f[j] by Cholesky,  x_s[j] = x_f[j] + G^T (x_s[j+1] - x_pred[j+1]),
    P_s[j] = P_f[j] + G^T (P_s[j+1] - P-) G.

    Returns RtsResult(x [K,N,12] the smoothed means, P_tape [K,N,12,12] their covariances (None with tape=False),
    var [K,N,12] the covariances' diagonals, x0 [12,N] and P0 [N,12,12] the smoothed starting point, ok [N] bool
    (False where a Cholesky pivot was <= 0 or not finite; the outputs are written regardless)).  dtype: torch.float64
    (default) or torch.float32 (P_tape, var, P0: the float64 values rounded).  Not available under
    action_arith="float32".  Asynchronous on the current stream; the tensors are buffers of this env, overwritten by
    its next call with the same K, dtype and tape."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    if self.config.action_arith != _lib.ARITH_F64:
        raise ValueError('rollout_rts is not available under action_arith="float32"')
    Qd, = _wire.uploaded(self, "rts", lambda: (_process_noise(Q),), given=(Q,))
    io, K, keep = _rollout._rollout_io(self, actions, None)
    n = self.num_envs
    if not isinstance(filt, EkfResult):
        raise ValueError("filt must be the EkfResult of rollout_ekf(..., tape=True)")
    if filt.P_tape is None:
        raise ValueError("filt has no P_tape: filter with rollout_ekf(..., tape=True)")
    if isinstance(filt.P_tape, torch.Tensor) and filt.P_tape.dtype != torch.float64:
        raise ValueError("filt.P_tape must be float64 (rollout_ekf's default dtype), got %s" % filt.P_tape.dtype)
    _wire.check_tape(self, "rollout_ekf", (filt.x, "filt.x", (K, n, 12), torch.float64),
                     (filt.x_pred, "filt.x_pred", (K, n, 12), torch.float64),
                     (filt.status, "filt.status", (K, n), torch.uint8),
                     (filt.P_tape, "filt.P_tape", (K, n, 12, 12), torch.float64))
    xt = _input(self, x0, (12, n), "x0", keep)
    Pt = _input(self, P0, (n, 12, 12), "P0", keep)
    io.start_status_dev = _start_status(self, status0, keep)
    io.start_x_dev = xt.data_ptr()
    rio = _wire.block(_lib.RolloutRtsIO, out_dtype=_wire.dtype_code(dtype))
    if end is not None:
        if not isinstance(end, (tuple, list)) or len(end) != 2 or end[0] is None or end[1] is None:
            raise ValueError("end must be the pair (x_end [12,N], P_end [N,12,12]): both or neither")
        rio.end_x_dev = _input(self, end[0], (12, n), "end[0]", keep).data_ptr()
        rio.end_P_dev = _input(self, end[1], (n, 12, 12), "end[1]", keep).data_ptr()
    rio.x_f_dev, rio.x_pred_dev = filt.x.data_ptr(), filt.x_pred.data_ptr()
    rio.status_f_dev, rio.P_f_dev = filt.status.data_ptr(), filt.P_tape.data_ptr()
    rio.Q_dev, rio.P0_dev = Qd.data_ptr(), Pt.data_ptr()
    tape = bool(tape)
    out = _wire.rollout_cache(self, ("rts", K, dtype, tape), lambda: RtsResult(
        _wire.empty(self, (K, n, 12), torch.float64), _wire.empty(self, (K, n, 12, 12), dtype) if tape else None,
        _wire.empty(self, (K, n, 12), dtype), _wire.empty(self, (12, n), torch.float64),
        _wire.empty(self, (n, 12, 12), dtype), _wire.empty(self, n, torch.bool)))
    # (no output may overlap an input: the caller's tensors that are this call's own buffers are copied first)
    mine = {t.data_ptr() for t in out if t is not None}
    for name in ("end_x_dev", "end_P_dev", "P0_dev"):
        if getattr(rio, name) in mine:
            src = next(t for t in keep if t.data_ptr() == getattr(rio, name))
            cp = src.clone()
            keep.append(cp)
            setattr(rio, name, cp.data_ptr())
    if io.start_x_dev in mine:
        cp = xt.clone()
        keep.append(cp)
        io.start_x_dev = cp.data_ptr()
    io.x_dev = out.x.data_ptr()
    rio.var_dev, rio.x0_dev, rio.P0_s_dev = out.var.data_ptr(), out.x0.data_ptr(), out.P0.data_ptr()
    rio.ok_dev = out.ok.data_ptr()
    if tape:
        rio.P_tape_dev = out.P_tape.data_ptr()
    _wire.launch(self, "cs_rollout_rts", io, rio, keep=keep + [Qd, filt.x, filt.x_pred, filt.status, filt.P_tape])
    return out


def measure(x_tape, H, r, seed, missing=0.0):
    """Synthetic measurements of a rollout_states tape: z [K,N,M] float64 = H x + sqrt(r) N(0, 1) on x_tape's device, from
    a torch generator seeded with `seed` on that device; where a Bernoulli(missing) draw says so the entry is NaN ("no
    measurement", which rollout_ekf skips).  x_tape [K,N,12]; H [M,12]; r [M] > 0 the variances."""
    torch = _torch()
    if not isinstance(x_tape, torch.Tensor) or x_tape.dim() != 3 or x_tape.shape[2] != 12:
        raise ValueError("x_tape must be a tensor of shape (K, N, 12) (rollout_states' x)")
    if not 0.0 <= float(missing) <= 1.0:
        raise ValueError("missing must be a probability, got %r" % (missing,))
    dev = x_tape.device
    Hd = torch.as_tensor(H, dtype=torch.float64).to(dev)
    rd = torch.as_tensor(r, dtype=torch.float64).to(dev)
    if Hd.dim() != 2 or Hd.shape[1] != 12 or tuple(rd.shape) != (Hd.shape[0],):
        raise ValueError("H must have shape (M, 12) and r shape (M,), got %s and %s" % (tuple(Hd.shape), tuple(rd.shape)))
    if not bool((rd > 0).all()):
        raise ValueError("r must be positive: the measurement variances")
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    K, n, M = x_tape.shape[0], x_tape.shape[1], Hd.shape[0]
    noise = torch.randn((K, n, M), generator=gen, dtype=torch.float64, device=dev)
    z = x_tape.to(torch.float64) @ Hd.T + noise * torch.sqrt(rd)
    if missing > 0.0:
        gone = torch.rand((K, n, M), generator=gen, dtype=torch.float64, device=dev) < float(missing)
        z = torch.where(gone, torch.full_like(z, float("nan")), z)
    return z


def _chunked(actions, z, chunk, taped, state, call, carry):
    """The chunk loop of ekf(), ukf() and pf(): call(actions' chunk, z's chunk, k0, state) runs the chunk that starts at
    step k0 from the carried `state` and returns its result (buffers of the env); its fields `taped` are cloned, and
    carry(result) is the state that starts the next chunk.  Returns (the taped fields concatenated over the chunks, by
    name; the state after the last chunk; loglik, the sum of the chunks'; ok, their conjunction)."""
    torch = _torch()
    K = int(actions.shape[0])
    chunk = K if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %r" % (chunk,))
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] != K:
        raise ValueError("z must be a tensor of shape (K, N, M) with K = %d steps" % K)
    parts = {name: [] for name in taped}
    loglik, ok = None, None
    for k0 in range(0, K, chunk):
        res = call(actions[k0:k0 + chunk], z[k0:k0 + chunk], k0, state)
        for name in taped:
            parts[name].append(getattr(res, name).clone())
        state = carry(res)
        loglik = res.loglik.clone() if loglik is None else loglik + res.loglik
        ok = res.ok.clone() if ok is None else ok & res.ok
    return {name: torch.cat(parts[name]) for name in taped}, state, loglik, ok


def _carry_gaussian(res):
    """What a Kalman filter carries from chunk to chunk: the last mean as [12,N], the last covariance and the status."""
    return res.x[-1].T.contiguous(), res.P.clone(), res.status[-1].clone()


def ekf(env, actions, z, H, r, Q, x0, P0, status0=None, chunk=None):
    """Run env.rollout_ekf over actions [K,N,A] and z [K,N,M] in chunks of `chunk` steps (None: one call), as a filter
    whose measurements arrive `chunk` at a time: the mean, the covariance and the status after each chunk start the next.
    Returns EkfResult with the tapes of all K steps concatenated (P_tape included), P the last posterior, loglik the sum
    of the chunks' and ok their conjunction -- tensors of their own, not the env's buffers.  Every tape, P and ok are
    bit-identical to the single call's: a chunk boundary rounds nothing (float64 throughout).  loglik equals the single
    call's to rounding only: it is the sum of the chunks' sums.  The arguments are rollout_ekf's."""
    cat, (_, P, _), loglik, ok = _chunked(
        actions, z, chunk, ("x", "x_pred", "var", "nis", "status", "branch", "P_tape"), (x0, P0, status0),
        lambda a, zc, k0, s: env.rollout_ekf(a, zc, H, r, Q, s[0], s[1], status0=s[2], tape=True), _carry_gaussian)
    return EkfResult(cat["x"], cat["x_pred"], P, cat["var"], cat["nis"], loglik, cat["status"], cat["branch"], ok,
                     cat["P_tape"])


def smooth(env, actions, filt, Q, x0=None, P0=None, status0=None, chunk=None, alpha=1.0, beta=0.0, kappa=1.0, paths=256,
           nonce=0):
    """Run a fixed-interval smoother over the K steps of a filter's tapes in chunks of `chunk` steps (None: one call),
    last chunk first: env.rollout_rts for an EkfResult, env.rollout_urts for a UkfResult (alpha, beta and kappa are
    the filter's; an EkfResult ignores them).  A chunk starts from the filter's row before it (the caller's x0, P0,
    status0 for the first chunk) and ends in the smoothed starting point the chunk after it returned.  Returns RtsResult
    with the tapes of all K steps concatenated (P_tape included), x0 and P0 the smoothed starting point and ok the
    chunks' conjunction -- tensors of their own, not the env's buffers.  Every tape, x0, P0 and ok are bit-identical to
    the single call's: a chunk boundary rounds nothing (float64 throughout).  filt is the result of the whole filter with
    its float64 P_tape (rollout_ekf(..., tape=True) or ekf(); rollout_ukf(..., tape=True) or ukf()); the other arguments
    are rollout_rts'.

    A PfResult (rollout_pf(..., tape=True) or pf()) goes to pf.pf_smooth, the backward-simulation smoother, with `paths`
    trajectories per env and the draws' `nonce`; it returns PfPaths.  The particle set before step 1 is not on a tape,
    so x0, P0 and status0 are not used there (and are required for the other two)."""
    torch = _torch()
    from .pf import PfResult, pf_smooth    # (pf.py imports this module: looked up when a call needs it)
    if isinstance(filt, PfResult):
        return pf_smooth(env, actions, filt, Q, paths=paths, nonce=nonce, chunk=chunk)
    if x0 is None or P0 is None:
        raise ValueError("x0 and P0 (the filter's starting point) are required to smooth an EkfResult or a UkfResult")
    K = int(actions.shape[0])
    chunk = K if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %r" % (chunk,))
    if isinstance(filt, EkfResult):
        def sub(k0, k1):
            return EkfResult(filt.x[k0:k1], filt.x_pred[k0:k1], None, None, None, None, filt.status[k0:k1], None, None,
                             filt.P_tape[k0:k1])
        call = env.rollout_rts
    else:
        from .ukf import UkfResult         # (ukf.py imports this module: looked up when a call needs it)
        if not isinstance(filt, UkfResult):
            raise ValueError("filt must be an EkfResult or a UkfResult with its P_tape (rollout_ekf / rollout_ukf(..., "
                             "tape=True)), or a PfResult with its tapes")

        def sub(k0, k1):
            return UkfResult(filt.x[k0:k1], filt.x_pred[k0:k1], None, None, None, None, filt.status[k0:k1], None, None,
                             filt.P_tape[k0:k1], None, None, None)

        def call(*args, **kwargs):
            return env.rollout_urts(*args, alpha=alpha, beta=beta, kappa=kappa, **kwargs)
    if filt.P_tape is None:
        raise ValueError("filt must be an EkfResult or a UkfResult with its P_tape (rollout_ekf / rollout_ukf(..., "
                         "tape=True))")
    for t, name in ((filt.x, "x"), (filt.x_pred, "x_pred"), (filt.status, "status"), (filt.P_tape, "P_tape")):
        if not isinstance(t, torch.Tensor) or t.shape[0] != K:
            raise ValueError("filt.%s must be a tensor of K = %d rows" % (name, K))
    parts, end, ok, res = [], None, None, None
    for k0 in reversed(range(0, K, chunk)):
        k1 = min(k0 + chunk, K)
        if k0 == 0:
            start = (x0, P0, status0)
        else:
            start = (filt.x[k0 - 1].T.contiguous(), filt.P_tape[k0 - 1], filt.status[k0 - 1])
        res = call(actions[k0:k1], sub(k0, k1), Q, start[0], start[1], status0=start[2], end=end, tape=True)
        parts.append([t.clone() for t in (res.x, res.P_tape, res.var)])
        end = (res.x0.clone(), res.P0.clone())
        ok = res.ok.clone() if ok is None else ok & res.ok
    xs, pt, var = (torch.cat([p[j] for p in reversed(parts)]) for j in range(3))
    return RtsResult(xs, pt, var, end[0], end[1], ok)
