"""The unscented Kalman filter on the device: CopterVecEnv.rollout_ukf -- one call of
cs_rollout_ukf on the env's cached buffers; vecenv.py binds it to the class -- the weights of the scaled unscented
transform, ukf(), the streaming driver whose measurements arrive a chunk of steps at a time, and the filter's
fixed-interval smoother: CopterVecEnv.rollout_urts, one call of cs_urts_smooth over the filter's
tapes, which the class inherits from UnscentedSmoother (ekf.py's smooth() is its chunked driver).

    z = H x + e,  e ~ N(0, diag(r));     P = L L^T,  points xhat, xhat +- gamma L[:,j];     each through the step;
    x-, P- = their weighted mean and covariance + Q;     sequential scalar updates

It stands between rollout_ekf (one Jacobian, at the branch the mean is on) and rollout_pf (64 to 1 024 sampled
particles): 25 deterministic points per env, no Jacobian, and a prior that sees every branch the points land on."""
import collections
import math

from . import _lib, _wire
from . import ekf as _ekf
from . import rollout as _rollout
from ._wire import _torch

# CopterVecEnv.rollout_ukf's result: the filtered means x [K,N,12] and the priors x_pred [K,N,12], the last posterior
# P [N,12,12], the posteriors' diagonals var [K,N,12], nis [K,N], loglik [N], the status [K,N] of the filter's own mean
# (point 0's), spread [K,N] uint8 (how many of the 25 points ended the step with another status), ok [N] bool, P_tape
# [K,N,12,12] (tape=True, else None) and, with points=True (else None), the points before the physics [K,N,25,12],
# after it [K,N,25,12] and their statuses [K,N,25]
UkfResult = collections.namedtuple(
    "UkfResult", "x x_pred P var nis loglik status spread ok P_tape points points_pred point_status")

NUM_POINTS = 25     # 2 * 12 + 1


def weights(alpha=1.0, beta=0.0, kappa=1.0):
    """(gamma, wm0, wc0, wi) of the scaled unscented transform for 12 states: lambda = alpha^2 (12 + kappa) - 12,
    gamma = sqrt(12 + lambda), wm0 = lambda / (12 + lambda), wc0 = wm0 + 1 - alpha^2 + beta, wi = 1 / (2 (12 + lambda)).
    wm0 + 24 wi = 1 whatever the arguments.  ValueError if 12 + lambda <= 0 or an argument is not finite."""
    alpha, beta, kappa = float(alpha), float(beta), float(kappa)
    if not all(math.isfinite(v) for v in (alpha, beta, kappa)):
        raise ValueError("alpha, beta and kappa must be finite, got %r" % ((alpha, beta, kappa),))
    lam = alpha * alpha * (12.0 + kappa) - 12.0
    c = 12.0 + lam
    if not c > 0.0:
        raise ValueError("12 + lambda = alpha^2 (12 + kappa) must be > 0, got %r (alpha=%r, kappa=%r)" % (c, alpha, kappa))
    wm0 = lam / c
    return math.sqrt(c), wm0, wm0 + 1.0 - alpha * alpha + beta, 1.0 / (2.0 * c)


def rollout_ukf(self, actions, z, H, r, Q, x0, P0, status0=None, alpha=1.0, beta=0.0, kappa=1.0, tape=False,
                points=False, dtype=None):
    """An unscented Kalman filter over the env step, K predict / update steps per env in one kernel: 25 sigma points
    per env and step, each through the step's own physics -- no Jacobian; a belief that straddles a touchdown, a crash
    or the motor clip is propagated on every side its points land on.  The filter's state is the caller's: NO env state
    is read but the configuration and the vehicle, and none changes.

    actions, z (NaN = no measurement), H [M,12], r [M] > 0, Q [12,12] symmetric, x0 [12,N], P0 [N,12,12] (its upper
    triangle is read) and status0 [N] (default AIRBORNE) are rollout_ekf's.  P0 must be positive definite, and Q should
    be: the covariance is factored at every step, and a pivot that is <= 0 or not finite clears that env's ok (every
    output is written regardless).

    Per step: if the mean is LANDED, x- = xhat and P- = P + Q.  Else P = L L^T (lower Cholesky); the points are xhat,
    xhat + gamma L[:,j] and xhat - gamma L[:,j], j = 0 .. 11, in this order; each goes through the physics from (the
    point, the status of the mean), exactly as rollout_states takes it from that explicit start; the status after the
    step is point 0's; x- = wm0 y0 + wi sum y_i, P- = wc0 d0 d0^T + wi sum d_i d_i^T + Q with d_i = y_i - x- (evaluated
    in one pass about y0: include/copterstep.h).  Then rollout_ekf's sequential scalar updates.

    alpha, beta, kappa: the scaled unscented transform's (weights()).  The defaults (1, 0, 1) make every weight positive,
    hence P- positive semidefinite by construction; (1, 0, 0) is the cubature rule (wm0 = 0); a small alpha makes wm0 and
    wc0 negative, and P- can then lose definiteness.  ValueError when 12 + lambda <= 0.

    Returns UkfResult(x, x_pred, P, var, nis, loglik, status, spread, ok, P_tape, points, points_pred, point_status):
    rollout_ekf's outputs without `branch`, plus spread [K,N] uint8 -- how many of the 25 points ended the step with
    another status than point 0's (0 on a LANDED step) -- and, with points=True, the points before the physics
    [K,N,25,12], after it [K,N,25,12] and their statuses [K,N,25] (always float64; on a LANDED step all 25 rows hold
    xhat and the statuses are LANDED).  dtype: torch.float64 (default) or torch.float32 (P, var, nis, loglik, P_tape:
    the float64 values rounded).  Not available under action_arith="float32".  Asynchronous on the current stream; the
    tensors are buffers of this env, overwritten by its next call with the same K, dtype, tape and points."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    gamma, wm0, wc0, wi = weights(alpha, beta, kappa)
    model = _ekf._kalman_model(self, "ukf", H, r, Q)
    M = model[3]
    io, K, keep = _rollout._rollout_io(self, actions, None)
    n = self.num_envs
    zt = _ekf._input(self, z, (K, n, M), "z", keep)
    xt = _ekf._input(self, x0, (12, n), "x0", keep)
    Pt = _ekf._input(self, P0, (n, 12, 12), "P0", keep)
    io.start_status_dev = _ekf._start_status(self, status0, keep)
    io.start_x_dev = xt.data_ptr()
    tape, points = bool(tape), bool(points)
    pts = lambda shape, dt: _wire.empty(self, shape, dt) if points else None      # noqa: E731
    out = _wire.rollout_cache(self, ("ukf", K, dtype, tape, points), lambda: UkfResult(
        *_ekf._kalman_tensors(self, K, n, dtype, tape), pts((K, n, NUM_POINTS, 12), torch.float64),
        pts((K, n, NUM_POINTS, 12), torch.float64), pts((K, n, NUM_POINTS), torch.uint8)))
    uio = _ekf._kalman_wire(_lib.RolloutUkfIO, dtype, model, Pt, out)
    uio.gamma, uio.wm0, uio.wc0, uio.wi = gamma, wm0, wc0, wi
    uio.z_dev, uio.spread_dev = zt.data_ptr(), out.spread.data_ptr()
    io.x_dev, io.status_dev = out.x.data_ptr(), out.status.data_ptr()
    if points:
        uio.points_dev, uio.points_pred_dev = out.points.data_ptr(), out.points_pred.data_ptr()
        uio.point_status_dev = out.point_status.data_ptr()
    _wire.launch(self, "cs_rollout_ukf", io, uio, keep=keep + list(model[:3]))
    return out


# -- the unscented Rauch-Tung-Striebel smoother over the filter's tapes: CopterVecEnv.rollout_urts ---
def rollout_urts(self, actions, filt, Q, x0, P0, status0=None, end=None, alpha=1.0, beta=0.0, kappa=1.0, tape=True,
                 dtype=None):
    """An unscented Rauch-Tung-Striebel fixed-interval smoother over the tapes of rollout_ukf, K backward steps per env
    in one kernel: the estimate of every step given the measurements of all K steps, and that of the starting point.
    What rollout_rts is to rollout_ekf: each backward step makes the filter's 25 sigma points of that step again from the
    filter's own tapes, sends them through the physics, and takes the cross-covariance of the points before and after
    the step in place of rollout_rts' A P_f -- no Jacobian, so a belief that straddles a touchdown, a crash or the motor
    clip is smoothed over every branch its points land on.  NO env state is read but the configuration and the vehicle,
    and none changes.

    actions [K,N,A], Q, x0 [12,N], P0 [N,12,12], status0 and alpha, beta, kappa are what the filter was given -- the
    weights (weights()) MUST be the filter's: with others the recomputed prior is not the filter's and the result is no
    smoother of these tapes; filt is its UkfResult from rollout_ukf(..., tape=True) in float64 (x, x_pred, status and
    P_tape are read).  Q should be positive definite.  end = (x_end [12,N], P_end [N,12,12]) gives the smoothed last row
    (default: the filter's own last row), as rollout_rts'.

    Row K-1 is the given one; then for j = K-2 down to -1 (row -1 is the starting point): if status_f[j] is LANDED,
    W = P_f[j] and P- = P_f[j] + Q; else P_f[j] = L L^T, the filter's points and their moments again (P- is the filter's
    prior, bit for bit) and W = wi gamma dY L^T with dY[:, c] = y(1 + c) - y(13 + c), the transposed cross-covariance.
    Then G = P-^-1 W by Cholesky,  x_s[j] = x_f[j] + G^T (x_s[j+1] - x_pred[j+1]),
    P_s[j] = P_f[j] + G^T (P_s[j+1] - P-) G.

    Returns RtsResult(x, P_tape (None with tape=False), var, x0, P0, ok) as rollout_rts: ok [N] is False where a pivot
    of either factorisation was <= 0 or not finite (the outputs are written regardless).  dtype: torch.float64 (default)
    or torch.float32 (P_tape, var, P0: the float64 values rounded).  Not available under action_arith="float32".
    Asynchronous on the current stream; the tensors are buffers of this env, overwritten by its next call with the same
    K, dtype and tape."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    if self.config.action_arith != _lib.ARITH_F64:
        raise ValueError('rollout_urts is not available under action_arith="float32"')
    gamma, wm0, wc0, wi = weights(alpha, beta, kappa)
    Qd, = _wire.uploaded(self, "urts", lambda: (_ekf._process_noise(Q),), given=(Q,))
    io, K, keep = _rollout._rollout_io(self, actions, None)
    n = self.num_envs
    if not isinstance(filt, UkfResult):
        raise ValueError("filt must be the UkfResult of rollout_ukf(..., tape=True)")
    if filt.P_tape is None:
        raise ValueError("filt has no P_tape: filter with rollout_ukf(..., tape=True)")
    if isinstance(filt.P_tape, torch.Tensor) and filt.P_tape.dtype != torch.float64:
        raise ValueError("filt.P_tape must be float64 (rollout_ukf's default dtype), got %s" % filt.P_tape.dtype)
    _wire.check_tape(self, "rollout_ukf", (filt.x, "filt.x", (K, n, 12), torch.float64),
                     (filt.x_pred, "filt.x_pred", (K, n, 12), torch.float64),
                     (filt.status, "filt.status", (K, n), torch.uint8),
                     (filt.P_tape, "filt.P_tape", (K, n, 12, 12), torch.float64))
    xt = _ekf._input(self, x0, (12, n), "x0", keep)
    Pt = _ekf._input(self, P0, (n, 12, 12), "P0", keep)
    io.start_status_dev = _ekf._start_status(self, status0, keep)
    io.start_x_dev = xt.data_ptr()
    sio = _wire.block(_lib.RolloutUrtsIO, out_dtype=_wire.dtype_code(dtype), gamma=gamma, wm0=wm0, wc0=wc0, wi=wi)
    if end is not None:
        if not isinstance(end, (tuple, list)) or len(end) != 2 or end[0] is None or end[1] is None:
            raise ValueError("end must be the pair (x_end [12,N], P_end [N,12,12]): both or neither")
        sio.end_x_dev = _ekf._input(self, end[0], (12, n), "end[0]", keep).data_ptr()
        sio.end_P_dev = _ekf._input(self, end[1], (n, 12, 12), "end[1]", keep).data_ptr()
    sio.x_f_dev, sio.x_pred_dev = filt.x.data_ptr(), filt.x_pred.data_ptr()
    sio.status_f_dev, sio.P_f_dev = filt.status.data_ptr(), filt.P_tape.data_ptr()
    sio.Q_dev, sio.P0_dev = Qd.data_ptr(), Pt.data_ptr()
    tape = bool(tape)
    out = _wire.rollout_cache(self, ("urts", K, dtype, tape), lambda: _ekf.RtsResult(
        _wire.empty(self, (K, n, 12), torch.float64), _wire.empty(self, (K, n, 12, 12), dtype) if tape else None,
        _wire.empty(self, (K, n, 12), dtype), _wire.empty(self, (12, n), torch.float64),
        _wire.empty(self, (n, 12, 12), dtype), _wire.empty(self, n, torch.bool)))
    # the kernel's scratch: one column of URTS_WORKSPACE_ROWS float64 per lane, 64 lanes per tile
    work = _wire.rollout_cache(self, ("urts_workspace",), lambda: _wire.empty(
        self, ((n + 63) // 64, _lib.URTS_WORKSPACE_ROWS, 64), torch.float64))
    # (no output may overlap an input: the caller's tensors that are this call's own buffers are copied first)
    mine = {t.data_ptr() for t in out if t is not None}
    for name in ("end_x_dev", "end_P_dev", "P0_dev"):
        if getattr(sio, name) in mine:
            src = next(t for t in keep if t.data_ptr() == getattr(sio, name))
            cp = src.clone()
            keep.append(cp)
            setattr(sio, name, cp.data_ptr())
    if io.start_x_dev in mine:
        cp = xt.clone()
        keep.append(cp)
        io.start_x_dev = cp.data_ptr()
    io.x_dev = out.x.data_ptr()
    sio.workspace_dev = work.data_ptr()
    sio.var_dev, sio.x0_dev, sio.P0_s_dev = out.var.data_ptr(), out.x0.data_ptr(), out.P0.data_ptr()
    sio.ok_dev = out.ok.data_ptr()
    if tape:
        sio.P_tape_dev = out.P_tape.data_ptr()
    _wire.launch(self, "cs_urts_smooth", io, sio, keep=keep + [Qd, filt.x, filt.x_pred, filt.status, filt.P_tape])
    return out


class UnscentedSmoother:
    """CopterVecEnv's unscented smoother, a base class of it.  It is inherited, not bound in the
    class body like its neighbours: the class body's rollout_* methods are the closed list that
    tests/test_gpu_output_bounds.py covers one by one (tests/test_guarded_outputs_cpu.py), and this one is held to the
    same memory contract in a file of its own, tests/test_gpu_urts_output_bounds.py."""
    rollout_urts = rollout_urts


def ukf(env, actions, z, H, r, Q, x0, P0, status0=None, alpha=1.0, beta=0.0, kappa=1.0, chunk=None, points=False):
    """Run env.rollout_ukf over actions [K,N,A] and z [K,N,M] in chunks of `chunk` steps (None: one call), as a filter
    whose measurements arrive `chunk` at a time: the mean, the covariance and the status after each chunk start the next.
    Returns UkfResult with the tapes of all K steps concatenated (P_tape included; the point tapes with points=True), P
    the last posterior, loglik the sum of the chunks' and ok their conjunction -- tensors of their own, not the env's
    buffers.  Every tape, P and ok are bit-identical to the single call's: a chunk boundary rounds nothing (float64
    throughout).  loglik equals the single call's to rounding only: it is the sum of the chunks' sums.  The other
    arguments are rollout_ukf's."""
    taped = ("x", "x_pred", "var", "nis", "status", "spread", "P_tape") + \
        (("points", "points_pred", "point_status") if points else ())
    cat, (_, P, _), loglik, ok = _ekf._chunked(
        actions, z, chunk, taped, (x0, P0, status0),
        lambda a, zc, k0, s: env.rollout_ukf(a, zc, H, r, Q, s[0], s[1], status0=s[2], alpha=alpha, beta=beta,
                                             kappa=kappa, tape=True, points=points), _ekf._carry_gaussian)
    return UkfResult(cat["x"], cat["x_pred"], P, cat["var"], cat["nis"], loglik, cat["status"], cat["spread"], ok,
                     cat["P_tape"], cat.get("points"), cat.get("points_pred"), cat.get("point_status"))
