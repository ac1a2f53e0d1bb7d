"""A small iLQR driver on CopterVecEnv.rollout_lqr / rollout_feedback_states and, under control
limits, rollout_lqr_box / rollout_feedback_box_states (section 24): batched trajectory optimisation of open-loop
actions for a quadratic tracking cost, one independent problem per env.

    J = sum_{k=1..K} 1/2 (x_k - x_ref)^T Q_k (x_k - x_ref) + 1/2 (a_k - a_ref)^T R (a_k - a_ref),   Q_K = Q_final

Every iteration is one backward kernel (the Riccati sweep over the nominal tape) and one forward kernel per line-search
candidate; the cost and its gradients at the tape are a few torch expressions on the device."""
import collections
import functools

import numpy as np

from . import _lib, _wire
from . import rollout as _rollout
from ._wire import _torch
from .rollout import Rollout

IlqrResult = collections.namedtuple("IlqrResult", "actions cost alpha rollout mu")
# CopterVecEnv.rollout_lqr's result: the time-varying gains K [K,N,A,12] and d [K,N,A], the model's predicted cost change
# dV [N,2], the value model at the start S0 [N,12,12], s0 [12,N], and ok [N] bool (every Cholesky pivot positive)
LqrGains = collections.namedtuple("LqrGains", "K d dV S0 s0 ok")
# CopterVecEnv.rollout_lqr_box's: the same, then clamped [K,N] uint8 (bit a: control a held at its lower bound, bit 4+a:
# at its upper) and iters [K,N] uint8 (iterations of the step's box-constrained programme)
BoxGains = collections.namedtuple("BoxGains", "K d dV S0 s0 ok clamped iters")


# -- the iLQR backward pass and its line-search forward: CopterVecEnv's methods, bound in vecenv.py --
def _weight(m, shape, name):
    """A cost matrix on the host: float64, of `shape`, finite and symmetric."""
    a = np.asarray(m.detach().cpu() if isinstance(m, _torch().Tensor) else m, dtype=np.float64)
    if a.shape != shape:
        raise ValueError("%s must have shape %s, got %s" % (name, shape, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    if not (a == a.T).all():
        raise ValueError("%s must be symmetric" % name)
    return a


def _lqr_weights(env, Q, R, Q_final, definite=True):
    """Q [12,12], R [A,A], Q_final [12,12] or None, checked on the host (symmetric, finite; R's diagonal > 0, or
    >= 0 with definite=False: MPPI inverts nothing) and kept on the device: the same values are uploaded once (the
    iLQR and MPPI drivers pass them every iteration)."""
    ad = env.action_dim
    q = _weight(Q, (12, 12), "Q")
    r = _weight(R, (ad, ad), "R")
    d = r.diagonal()
    if definite and not (d > 0).all():
        raise ValueError("R must be positive definite: its diagonal must be > 0")
    if not (d >= 0).all():
        raise ValueError("R must be positive semidefinite: its diagonal must be >= 0")
    qf = None if Q_final is None else _weight(Q_final, (12, 12), "Q_final")
    return _wire.uploaded(env, "lqr_weights", lambda: (q, r, qf))


def rollout_lqr(self, actions, rollout, Q, R, q=None, r=None, Q_final=None, mu=0.0, state=None, dtype=None):
    """The iLQR backward pass over a rollout's tape, one kernel: the Riccati recursion of the quadratic model of a
    cost J = sum_k [l_k(x_k) + m_k(a_k)] around the rollout, with the step Jacobians of step_jacobian (every branch
    rule of DESIGN section 9) applied on the fly and never stored.  `rollout` is what rollout_states(actions, state)
    returned for the same actions and start (as rollout_vjp takes it).  q [K,N,12] = grad l_k at rollout.x[k-1],
    r [K,N,A] = grad m_k at actions[k-1] (None: zero); Q [12,12] symmetric PSD, R [A,A] symmetric PD and Q_final
    (replaces Q at the last step) are the Hessians, shared by every env and step; mu >= 0 is the Levenberg term
    added to Quu's diagonal before it is inverted.

    Returns LqrGains(K [K,N,A,12], d [K,N,A], dV [N,2], S0 [N,12,12], s0 [12,N], ok [N] bool): the action
    a_k + alpha d_k + K_k (x_{k-1} - xbar_{k-1}) (rollout_feedback_states) changes the model's cost by
    alpha dV[:,0] + alpha^2 dV[:,1]; S0, s0 are the value model at the start; ok is False where a Cholesky pivot was
    not positive (raise mu).  dtype: torch.float64 (default) or torch.float32 (the float64 values rounded).
    Asynchronous on the current stream; the tensors are buffers of this env, overwritten by its next call with the
    same K and dtype.  No env state changes."""
    self._check_open()
    io, lio, out, keep = _lqr_blocks(self, "lqr", actions, rollout, Q, R, q, r, Q_final, mu, state, dtype)
    _wire.launch(self, "cs_rollout_lqr", io, lio, keep=keep)
    return LqrGains(*out)


def _lqr_blocks(self, slot, actions, rollout, Q, R, q, r, Q_final, mu, state, dtype):
    """(io, lio, the six output buffers of cache slot `slot`, what the call reads): the blocks of a backward pass."""
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    mu = _wire.finite(float(mu), "mu", 0)
    Qd, Rd, Qfd = _lqr_weights(self, Q, R, Q_final)
    io, K, keep = _rollout._rollout_io(self, actions, state)
    n, ad = self.num_envs, self.action_dim
    _rollout._tape(self, io, rollout, K)
    lio = _wire.block(_lib.RolloutLqrIO, out_dtype=_wire.dtype_code(dtype), mu=mu, Q_dev=Qd.data_ptr(),
                      R_dev=Rd.data_ptr(), Q_final_dev=None if Qfd is None else Qfd.data_ptr())
    if q is not None:
        lio.q_dev = _wire.tensor(self, q, (K, n, 12), torch.float64, "q", keep, host=False, floating=True,
                                 foreign=False).data_ptr()
    if r is not None:
        lio.r_dev = _wire.tensor(self, r, (K, n, ad), torch.float64, "r", keep, host=False, floating=True,
                                 foreign=False).data_ptr()
    out = _wire.rollout_cache(self, (slot, K, dtype), lambda: (
        _wire.empty(self, (K, n, ad, 12), dtype), _wire.empty(self, (K, n, ad), dtype), _wire.empty(self, (n, 2), dtype),
        _wire.empty(self, (n, 12, 12), dtype), _wire.empty(self, (12, n), dtype), _wire.empty(self, n, torch.bool)))
    lio.K_dev, lio.d_dev, lio.dV_dev, lio.S0_dev, lio.s0_dev, lio.ok_dev = (t.data_ptr() for t in out)
    return io, lio, out, keep + [Qd, Rd, Qfd]


def _box(env, lo, hi):
    """The box lo <= a <= hi on the host: each a scalar or [A], float32, no NaN, lo <= hi (infinite bounds are allowed);
    the device copies (lo [A], hi [A]), uploaded once while the values stay the same."""
    ad = env.action_dim

    def check():
        out = []
        for v, name in ((lo, "lo"), (hi, "hi")):
            a = np.asarray(v.detach().cpu() if isinstance(v, _torch().Tensor) else v, dtype=np.float32)
            if a.shape not in ((), (ad,)):
                raise ValueError("%s must be a scalar or have shape (%d,), got %s" % (name, ad, a.shape))
            if np.isnan(a).any():
                raise ValueError("%s must not be NaN" % name)
            out.append(np.ascontiguousarray(np.broadcast_to(a, (ad,))))
        if not (out[0] <= out[1]).all():
            raise ValueError("lo must be <= hi in every component, got lo %s, hi %s" % (out[0], out[1]))
        return out
    return _wire.uploaded(env, "ilqr_box", check)


def rollout_lqr_box(self, actions, rollout, Q, R, lo, hi, q=None, r=None, Q_final=None, mu=0.0, state=None, dtype=None):
    """rollout_lqr with the control limits lo <= a <= hi handled inside the backward pass (control-limited DDP; DESIGN
    section 24): at every step d_k minimises the step's quadratic model 1/2 d^T (Quu + mu I) d + Qu^T d over
    lo - a_k <= d <= hi - a_k (a projected-Newton box QP, at most 16 iterations, in registers), the gain rows of the
    controls it holds at a bound are zero, and the free rows are -(Quu + mu I)_ff^-1 Qux_f.  Everything else is
    rollout_lqr's: its arguments, its value recursion, dV and the outputs.  lo, hi: a scalar or [A] (float32; -inf /
    +inf allowed; ValueError on NaN, on lo > hi or on another shape).  With lo = -inf, hi = +inf the result is
    rollout_lqr's bit for bit.

    Returns BoxGains(K, d, dV, S0, s0, ok, clamped [K,N] uint8, iters [K,N] uint8): clamped has bit a set where control
    a is held at its lower bound and bit 4+a at its upper; iters is the QP's iteration count (0 on the first step of a
    lane with a NEXT_STEP reset pending, which takes the clamped unconstrained step); ok is also False where the QP
    exhausted its 16 iterations or a free block's Cholesky pivot was not positive.  The tensors are buffers of this
    env, overwritten by its next call with the same K and dtype (they are not rollout_lqr's).  No env state changes."""
    self._check_open()
    torch = _torch()
    lod, hid = _box(self, lo, hi)
    io, lio, out, keep = _lqr_blocks(self, "lqr_box", actions, rollout, Q, R, q, r, Q_final, mu, state, dtype)
    K, n = io.num_steps, self.num_envs
    clamped, iters = _wire.rollout_cache(self, ("lqr_box_flags", K), lambda: (
        _wire.empty(self, (K, n), torch.uint8), _wire.empty(self, (K, n), torch.uint8)))
    bio = _wire.block(_lib.RolloutIlqrBoxIO, lo_dev=lod.data_ptr(), hi_dev=hid.data_ptr(),
                      clamped_dev=clamped.data_ptr(), iters_dev=iters.data_ptr())
    _wire.launch(self, "cs_ilqr_box_backward", io, lio, bio, keep=keep + [lod, hid])
    return BoxGains(*out, clamped, iters)


def rollout_feedback_states(self, actions, rollout, gains, alpha, state=None):
    """rollout_states under the feedback of rollout_lqr, the line search's forward pass: step k takes
    a_k = float32(actions[k-1] + alpha d_k + K_k (x_{k-1} - rollout.x[k-2])), x_{k-1} the state of THIS rollout
    before the step (step 1 has no deviation: both rollouts share the start).  The arithmetic is float64 and fixed:
    one multiply and one add for alpha d, then per state slot in order a subtraction, a multiply and an add, one
    rounding to float32.  `rollout` is the nominal rollout_states(actions, state) result, `gains` rollout_lqr's
    (float64), alpha a float or [N] float64 (per env).  Returns (Rollout, actions_out [K,N,A] float32): the Rollout
    is bit-identical to rollout_states(actions_out, state).  Asynchronous on the current stream; the tensors are
    buffers of this env, overwritten by its next call with the same K (they are not rollout_states' buffers).  No
    env state changes."""
    self._check_open()
    io, fio, ro, acts, keep = _feedback_blocks(self, "feedback", actions, rollout, gains, alpha, state)
    _wire.launch(self, "cs_rollout_feedback_states", io, fio, keep=keep)
    return ro, acts


def _feedback_blocks(self, slot, actions, rollout, gains, alpha, state):
    """(io, fio, the Rollout and action buffers of cache slot `slot`, what the call reads): a forward pass's blocks."""
    torch = _torch()
    io, K, keep = _rollout._rollout_io(self, actions, state)
    n, ad, dev = self.num_envs, self.action_dim, self.device
    xbar = getattr(rollout, "x", None)
    Kg, d = getattr(gains, "K", None), getattr(gains, "d", None)
    _wire.check_tape(self, "rollout_states", (xbar, "rollout.x", (K, n, 12), torch.float64))
    _wire.check_tape(self, "rollout_lqr", (Kg, "gains.K", (K, n, ad, 12), torch.float64),
                     (d, "gains.d", (K, n, ad), torch.float64))
    if isinstance(alpha, torch.Tensor):
        if tuple(alpha.shape) not in ((), (n,)) or not alpha.dtype.is_floating_point:
            raise ValueError("alpha must be a float or a floating-point tensor of shape (%d,)" % n)
        if alpha.device != dev and alpha.dim() == 1:
            raise ValueError("alpha must be on %s, got %s" % (dev, alpha.device))
        al = alpha.detach().to(device=dev, dtype=torch.float64).expand(n).contiguous()
    else:
        a = np.asarray(alpha, dtype=np.float64)
        if a.shape not in ((), (n,)):
            raise ValueError("alpha must be a float or have shape (%d,), got %s" % (n, a.shape))
        al = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (n,)))).to(dev)
    keep.append(al)
    ro, acts = _wire.rollout_cache(self, (slot, K), lambda: (
        _rollout._rollout_tensors(self, K), _wire.empty(self, (K, n, ad), torch.float32)))
    _rollout._wire_rollout(io, ro)
    fio = _wire.block(_lib.RolloutFeedbackIO, xbar_dev=xbar.data_ptr(), K_dev=Kg.data_ptr(), d_dev=d.data_ptr(),
                      alpha_dev=al.data_ptr(), actions_out_dev=acts.data_ptr())
    return io, fio, ro, acts, keep + [xbar, Kg, d]


def rollout_feedback_box_states(self, actions, rollout, gains, alpha, lo, hi, state=None):
    """rollout_feedback_states with the action clamped into the box after its rounding to float32:
    a_k = clamp(float32(actions[k-1] + alpha d_k + K_k (x_{k-1} - rollout.x[k-2])), lo, hi), a NaN left as it is.  The
    clamped value is what the step takes and what actions_out holds.  gains: rollout_lqr_box's (or rollout_lqr's);
    lo, hi as in rollout_lqr_box.  Returns (Rollout, actions_out [K,N,A] float32, clamped [K,N] uint8: bit a where
    the clamp raised action a to lo, bit 4+a where it lowered it to hi); the Rollout is bit-identical to
    rollout_states(actions_out, state).  The tensors are buffers of this env, overwritten by its next call with the
    same K (they are not rollout_feedback_states').  No env state changes."""
    self._check_open()
    torch = _torch()
    lod, hid = _box(self, lo, hi)
    io, fio, ro, acts, keep = _feedback_blocks(self, "feedback_box", actions, rollout, gains, alpha, state)
    clamped = _wire.rollout_cache(self, ("feedback_box_flags", io.num_steps), lambda: _wire.empty(
        self, (io.num_steps, self.num_envs), torch.uint8))
    bio = _wire.block(_lib.RolloutIlqrBoxIO, lo_dev=lod.data_ptr(), hi_dev=hid.data_ptr(),
                      clamped_dev=clamped.data_ptr())
    _wire.launch(self, "cs_ilqr_box_forward", io, fio, bio, keep=keep + [lod, hid])
    return ro, acts, clamped


class ControlLimited:
    """CopterVecEnv's control-limited iLQR methods, a base class of it.  They are inherited, not
    bound in the class body like their neighbours: the class body's rollout_* methods are the closed list that
    tests/test_gpu_output_bounds.py covers one by one (tests/test_guarded_outputs_cpu.py), and these two are held to the
    same memory contract in a file of their own, tests/test_gpu_ilqr_box_output_bounds.py."""
    rollout_lqr_box = rollout_lqr_box
    rollout_feedback_box_states = rollout_feedback_box_states


def tracking_cost(x, a, x_ref, a_ref, Q, R, Q_final=None):
    """J per env [N] (float64) of a tape x [K,N,12] and actions a [K,N,A]."""
    torch = _torch()
    dx = x - x_ref
    da = a.to(torch.float64) - a_ref
    lx = 0.5 * ((dx @ Q) * dx).sum(-1)
    if Q_final is not None:
        lx = torch.cat([lx[:-1], 0.5 * ((dx[-1:] @ Q_final) * dx[-1:]).sum(-1)])
    return lx.sum(0) + 0.5 * ((da @ R) * da).sum(-1).sum(0)


def tracking_gradients(x, a, x_ref, a_ref, Q, R, Q_final=None):
    """(q [K,N,12], r [K,N,A]): the gradients of tracking_cost's terms at the tape (Q, R symmetric)."""
    torch = _torch()
    dx = x - x_ref
    q = dx @ Q
    if Q_final is not None:
        q = torch.cat([q[:-1], dx[-1:] @ Q_final])
    return q, (a.to(torch.float64) - a_ref) @ R


def ilqr(env, actions0, x_ref, Q, R, Q_final=None, a_ref=None, iters=10,
         alphas=(1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125), mu0=0.0, state=None, bounds=None):
    """Minimise the tracking cost above over the actions [K,N,A] of env's rollout from `state` (None: its stored
    state), starting from actions0.  x_ref and a_ref broadcast against [K,N,12] and [K,N,A] (a_ref=None: zero).

    Per iteration: q, r at the nominal tape (torch), rollout_lqr, then a per-env backtracking line search with
    rollout_feedback_states: each env keeps the first alpha of `alphas` whose ACTUAL cost is below its current one,
    else its nominal (alpha 0).  The Levenberg term mu starts at mu0 and is raised tenfold (from at least 1e-6) for the
    next call whenever rollout_lqr reported a failed factorisation anywhere; those envs' candidates are not finite and
    are never accepted.  The host reads one small tensor per line-search candidate (have all envs accepted?) and
    nothing else.

    bounds=(lo, hi), each a scalar or [A]: control limits.  actions0 is clamped into the box first,
    the backward pass is rollout_lqr_box and the forward rollout_feedback_box_states, so every candidate and every
    returned action lies in the box and the model behind the line search knows which controls are held.  None: no
    limits, the calls and the bits of the unconstrained driver.

    Returns IlqrResult(actions [K,N,A] float32, cost [iters+1,N] float64: per env, before the first iteration and
    after each, alpha [iters,N]: the accepted step (0 = none), rollout: the Rollout-like tape of the result (x,
    status), mu: the last Levenberg term)."""
    torch = _torch()
    dev = env.device
    f64 = dict(dtype=torch.float64, device=dev)

    def dev64(v):
        return (v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float64))).to(**f64)
    Qd, Rd = dev64(Q), dev64(R)
    Qfd = None if Q_final is None else dev64(Q_final)
    Qh, Rh = Qd.cpu().numpy(), Rd.cpu().numpy()
    Qfh = None if Qfd is None else Qfd.cpu().numpy()
    xr = dev64(x_ref)
    ar = torch.zeros((), **f64) if a_ref is None else dev64(a_ref)
    acts = (actions0.detach() if isinstance(actions0, torch.Tensor) else torch.from_numpy(np.asarray(actions0)))
    acts = acts.to(device=dev, dtype=torch.float32).clone().contiguous()
    if bounds is not None:
        lo, hi = bounds
        lod, hid = _box(env, lo, hi)
        acts = torch.minimum(torch.maximum(acts, lod), hid)
        backward = functools.partial(env.rollout_lqr_box, lo=lo, hi=hi)

        def forward(*a, **kw):
            return env.rollout_feedback_box_states(*a, lo, hi, **kw)[:2]
    else:
        backward, forward = env.rollout_lqr, env.rollout_feedback_states
    n = acts.shape[1]
    ro = env.rollout_states(acts, state=state)
    x, status = ro.x.clone(), ro.status.clone()      # (the env's buffers are overwritten by its next call)
    cost = tracking_cost(x, acts, xr, ar, Qd, Rd, Qfd)
    history, taken = [cost], []
    mu = float(mu0)
    zero = torch.zeros(n, **f64)
    for _ in range(iters):
        q, r = tracking_gradients(x, acts, xr, ar, Qd, Rd, Qfd)
        nominal = Rollout(x, None, None, None, status)
        gains = backward(acts, nominal, Qh, Rh, q=q, r=r, Q_final=Qfh, mu=mu, state=state)
        accepted = torch.zeros(n, dtype=torch.bool, device=dev)
        step = zero.clone()
        new_x, new_status, new_acts, new_cost = x, status, acts, cost
        all_ok = True
        for al in alphas:
            alpha = torch.where(accepted, zero, torch.full_like(zero, float(al)))
            fro, fa = forward(acts, nominal, gains, alpha, state=state)
            c = tracking_cost(fro.x, fa, xr, ar, Qd, Rd, Qfd)
            better = ~accepted & (c < cost)           # (a non-finite candidate compares False)
            new_x = torch.where(better[None, :, None], fro.x, new_x)
            new_status = torch.where(better[None, :], fro.status, new_status)
            new_acts = torch.where(better[None, :, None], fa, new_acts)
            new_cost = torch.where(better, c, new_cost)
            step = torch.where(better, alpha, step)
            accepted = accepted | better
            flags = torch.stack([accepted.all(), gains.ok.all()]).cpu()   # the iteration's one kind of host read
            all_ok = bool(flags[1])
            if bool(flags[0]):
                break
        x, status, acts, cost = new_x, new_status, new_acts.contiguous(), new_cost
        history.append(cost)
        taken.append(step)
        if not all_ok:
            mu = max(mu, 1e-7) * 10.0
    return IlqrResult(acts, torch.stack(history), torch.stack(taken) if taken else torch.zeros((0, n), **f64),
                      Rollout(x, None, None, None, status), mu)
