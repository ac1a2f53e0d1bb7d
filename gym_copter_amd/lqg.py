"""Output-feedback (LQG) control on the device: CopterVecEnv.rollout_lqg -- one call of
cs_rollout_lqg on the env's cached buffers; vecenv.py binds it to the class -- the measurement noise to feed it, and
lqg(), the small driver that designs the gains at a nominal rollout and flies them on the filter's estimate.

    a_k = abar_k + K_k (xhat_{k-1} - xbar_{k-1});   x_k = step(x_{k-1}, a_k);   z_k = H x_k + e_k;
    xhat_k = the extended Kalman filter's update on z_k after its predict under a_k

The controller never sees the true state: only the filter's estimate, which in turn is told every action."""
import collections

import numpy as np

from . import _lib, _wire
from . import ekf as _ekf
from . import rollout as _rollout
from ._wire import _torch
from .ekf import EkfResult
from .ilqr import tracking_gradients

# CopterVecEnv.rollout_lqg's result: rollout, the Rollout of the truth (x [K,N,12], reward, terminated, truncated,
# status); actions [K,N,A] float32, what the law chose (unclipped); z [K,N,M] float64, the measurements (NaN = none);
# filter, an EkfResult of the filter's own tapes (its status is that of its estimate, not the truth's)
LqgResult = collections.namedtuple("LqgResult", "rollout actions z filter")


def rollout_lqg(self, actions, gains, xbar, noise, H, r, Q, xhat0, P0, status0=None, state=None, tape=False, dtype=None):
    """K steps of output-feedback control per env in one kernel: the affine law of rollout_feedback_states evaluated
    at the estimate of rollout_ekf's filter, the true env step under that action, its measurement, and the filter's
    predict (under the same action) and update.  NO env state changes.

    Per step k = 1..K:  a_k = float32(actions[k-1] + gains[k-1] (xhat_{k-1} - xbar[k-1])), float64 in a fixed order
    (per state slot a subtraction, a multiply and an add), xhat_0 = xhat0;  x_k = rollout_states' step under a_k from
    `state` (None: the stored state, with its pending perturbation or NEXT_STEP reset; else rollout_states' dict);
    z_k = H x_k + noise[k-1] (NaN noise = no measurement);  then rollout_ekf's step under a_k on z_k.

    actions [K,N,A]: the nominal actions.  gains: a float64 tensor [K,N,A,12], or rollout_lqr's result (its .K).  xbar
    [K,N,12] float64: row k-1 is the reference point BEFORE step k (for a nominal rollout: its start, then its rows 0 ..
    K-2).  noise [K,N,M] float64: the measurement noise, already scaled by sqrt(r) (measurement_noise()).  H [M,12],
    r [M] > 0, Q [12,12], xhat0 [12,N], P0 [N,12,12], status0 [N] (of the estimate; default AIRBORNE), tape and dtype
    are rollout_ekf's.

    Returns LqgResult(rollout, actions, z, filter): the truth's Rollout, bit-identical to rollout_states(actions_out,
    state); actions_out [K,N,A] float32 (unclipped; the step clips); z [K,N,M]; and an EkfResult bit-identical to
    rollout_ekf(actions_out, z, ...).  Not available under action_arith="float32".  Asynchronous on the current stream;
    the tensors are buffers of this env, overwritten by its next call with the same K, M, dtype and tape."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    model = _ekf._kalman_model(self, "lqg", H, r, Q)
    M = model[3]
    io, K, keep = _rollout._rollout_io(self, actions, state)
    n, ad = self.num_envs, self.action_dim
    Kg = getattr(gains, "K", gains)
    _wire.check_tape(self, "rollout_lqr", (Kg, "gains", (K, n, ad, 12), torch.float64))
    _wire.check_tape(self, "rollout_states", (xbar, "xbar", (K, n, 12), torch.float64))
    et = _ekf._input(self, noise, (K, n, M), "noise", keep)
    xt = _ekf._input(self, xhat0, (12, n), "xhat0", keep)
    Pt = _ekf._input(self, P0, (n, 12, 12), "P0", keep)
    status0_dev = _ekf._start_status(self, status0, keep)
    tape = bool(tape)
    out = _wire.rollout_cache(self, ("lqg", K, M, dtype, tape), lambda: LqgResult(
        _rollout._rollout_tensors(self, K), _wire.empty(self, (K, n, ad), torch.float32),
        _wire.empty(self, (K, n, M), torch.float64), EkfResult(*_ekf._kalman_tensors(self, K, n, dtype, tape))))
    ro, f = out.rollout, out.filter
    _rollout._wire_rollout(io, ro)
    lio = _ekf._kalman_wire(_lib.RolloutLqgIO, dtype, model, Pt, f)
    lio.K_dev, lio.xbar_dev, lio.e_dev = Kg.data_ptr(), xbar.data_ptr(), et.data_ptr()
    lio.xhat0_dev, lio.status0_dev = xt.data_ptr(), status0_dev
    lio.actions_out_dev, lio.z_dev = out.actions.data_ptr(), out.z.data_ptr()
    lio.xhat_dev, lio.fstatus_dev, lio.branch_dev = f.x.data_ptr(), f.status.data_ptr(), f.branch.data_ptr()
    _wire.launch(self, "cs_rollout_lqg", io, lio, keep=keep + list(model[:3]) + [Kg, xbar])
    return out


def measurement_noise(K, N, r, seed, missing=0.0, device=None):
    """The noise tape of rollout_lqg: e [K,N,M] float64 = sqrt(r) N(0, 1) on `device`, from a torch generator seeded with
    `seed` on that device; where a Bernoulli(missing) draw says so the entry is NaN ("no measurement").  r [M] > 0 are
    the measurement variances."""
    torch = _torch()
    if not 0.0 <= float(missing) <= 1.0:
        raise ValueError("missing must be a probability, got %r" % (missing,))
    dev = torch.device("cuda" if device is None else device)
    rd = torch.as_tensor(r, dtype=torch.float64).to(dev)
    if rd.dim() != 1 or rd.shape[0] < 1:
        raise ValueError("r must have shape (M,), got %s" % (tuple(rd.shape),))
    if not bool((rd > 0).all()):
        raise ValueError("r must be positive: the measurement variances")
    if int(K) < 1 or int(N) < 1:
        raise ValueError("K and N must be >= 1, got %r and %r" % (K, N))
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    shape = (int(K), int(N), int(rd.shape[0]))
    e = torch.randn(shape, generator=gen, dtype=torch.float64, device=dev) * torch.sqrt(rd)
    if missing > 0.0:
        gone = torch.rand(shape, generator=gen, dtype=torch.float64, device=dev) < float(missing)
        e = torch.where(gone, torch.full_like(e, float("nan")), e)
    return e


def lqg(env, actions, x_ref, Qc, Rc, H, r, Qn, xhat0, P0, seed, missing=0.0, state=None, Q_final=None, a_ref=None):
    """Design and fly an output-feedback controller in five device calls: the nominal rollout_states(actions, state);
    rollout_lqr at it for the tracking cost of ilqr (x_ref, Qc, Rc, Q_final, a_ref; gradients by
    ilqr.tracking_gradients); xbar = the start's x followed by the nominal's rows 0 .. K-2; the measurement noise
    measurement_noise(K, N, r, seed, missing); and rollout_lqg with those gains, H, r and the filter's process noise Qn
    from the estimate (xhat0, P0).  x_ref and a_ref broadcast against [K,N,12] and [K,N,A] (a_ref=None: zero).  Returns
    rollout_lqg's LqgResult (buffers of the env)."""
    torch = _torch()
    dev = env.device
    f64 = dict(dtype=torch.float64, device=dev)

    def dev64(v):
        return (v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float64))).to(**f64)
    Qd, Rd = dev64(Qc), dev64(Rc)
    Qfd = None if Q_final is None else dev64(Q_final)
    xr = dev64(x_ref)
    ar = torch.zeros((), **f64) if a_ref is None else dev64(a_ref)
    acts = (actions.detach() if isinstance(actions, torch.Tensor) else torch.from_numpy(np.asarray(actions)))
    acts = acts.to(device=dev, dtype=torch.float32).contiguous()
    K, n = int(acts.shape[0]), int(acts.shape[1])
    nominal = env.rollout_states(acts, state=state)
    q, rr = tracking_gradients(nominal.x, acts, xr, ar, Qd, Rd, Qfd)
    gains = env.rollout_lqr(acts, nominal, Qd.cpu().numpy(), Rd.cpu().numpy(), q=q, r=rr,
                            Q_final=None if Qfd is None else Qfd.cpu().numpy(), state=state)
    x0 = state["x"] if state is not None else env.get_state(only=("x",))["x"]
    x0 = dev64(x0)
    xbar = torch.cat([x0.T[None], nominal.x[:-1]]).contiguous()
    noise = measurement_noise(K, n, r, seed, missing=missing, device=dev)
    return env.rollout_lqg(acts, gains, xbar, noise, H, r, Qn, xhat0, P0, state=state)
