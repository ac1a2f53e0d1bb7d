"""MPPI on the device (DESIGN.md sections 14 and 15): CopterVecEnv.rollout_mppi_costs / rollout_mppi_update /
rollout_mppi_temperature -- bound to the class by vecenv.py -- the knot table of the smooth noise, and mppi(), a small
driver on them: batched sampling-based trajectory optimisation of open-loop actions, one independent problem per env.

    S = sum_{k=1..K} 1/2 (x_k - x_ref)^T Q_k (x_k - x_ref) + 1/2 (a_k - a_ref)^T R (a_k - a_ref) - reward_weight reward_k

with Q_K = Q_final.  Every iteration is three kernels -- the costs of `samples` noisy copies of the plan, their weighted
average, the cost of that candidate -- and a few torch selections on the device; nothing is read by the host.  With
hold > 1 the noise is smooth (piecewise linear between knots `hold` steps apart); with ess_target a fourth kernel solves a
temperature per env between the costs and the update."""
import collections
import ctypes as C

import numpy as np

from . import _lib, _wire
from . import rollout as _rollout
from ._wire import _torch
from .ilqr import _lqr_weights

MppiResult = collections.namedtuple("MppiResult", "actions cost ess")
# CopterVecEnv.rollout_mppi_costs' and rollout_mppi_update's results
MppiCosts = collections.namedtuple("MppiCosts", "costs best")
MppiUpdate = collections.namedtuple("MppiUpdate", "actions ess cost_min")
# CopterVecEnv.rollout_mppi_temperature's result
MppiTemperature = collections.namedtuple("MppiTemperature", "lam ess")
MPPI_MAX_KNOT = 16384                                        # knot + 1 <= 16 384: the noise keys stay distinct
_SAMPLES = "an int in [1, %d]" % _lib.MPPI_MAX_SAMPLES


def mppi_knots(K, hold):
    """The knot table of K steps for normalised linear interpolation over holds of `hold` steps, as rollout_mppi_costs /
    rollout_mppi_update take it (knots=): (knot [K] uint32, w [K,2] float32) with, for step k = 1..K,

        knot[k] = (k - 1) // hold + 1,   t = ((k - 1) % hold) / hold,   w[k] = (1 - t, t) / sqrt((1 - t)^2 + t^2)

    computed in float64 and rounded once: the noise of step k is w[k][0] eps(knot[k]) + w[k][1] eps(knot[k] + 1), of unit
    variance at every step, and steps inside a hold are correlated.  hold = 1 is the white table (k, 1, 0)."""
    _wire.int_in(K, "K", 1, None, "an int >= 1")
    _wire.int_in(hold, "hold", 1, None, "an int >= 1")
    k0 = np.arange(int(K), dtype=np.int64)
    t = (k0 % int(hold)).astype(np.float64) / float(hold)
    w = np.stack([1.0 - t, t], axis=1) / np.sqrt((1.0 - t) ** 2 + t ** 2)[:, None]
    knot = k0 // int(hold) + 1
    if int(knot[-1]) + 1 > MPPI_MAX_KNOT:
        raise ValueError("K / hold is too large: knot + 1 must be <= %d" % MPPI_MAX_KNOT)
    return knot.astype(np.uint32), w.astype(np.float32)


# -- MPPI: sampled rollouts, their costs and the weighted update: CopterVecEnv's methods ------------
def _mppi_small(env, v, name, dtype, nonneg):
    """sigma / a_ref: a scalar or [A] values, checked on the host and kept on the device: the same values are
    uploaded once (the MPPI driver passes them every iteration)."""
    ad = env.action_dim
    a = np.asarray(v.detach().cpu() if isinstance(v, _torch().Tensor) else v, dtype=np.float64)
    if a.shape not in ((), (ad,)):
        raise ValueError("%s must be a scalar or have shape (%d,), got %s" % (name, ad, a.shape))
    a = np.ascontiguousarray(np.broadcast_to(a, (ad,))).astype(dtype)
    if not np.isfinite(a).all() or (nonneg and not (a >= 0).all()):
        raise ValueError("%s must be finite%s" % (name, " and >= 0" if nonneg else ""))
    return _wire.uploaded(env, name, lambda: (a,))[0]


def _mppi_knots(env, knots, K):
    """knots=(knot [K], w [K,2]) (mppi_knots' layout), checked on the host and kept on the device: the same table is
    uploaded once.  Returns the two device tensors."""
    def check():
        torch = _torch()
        try:
            knot, w = knots
            knot = np.asarray(knot.detach().cpu() if isinstance(knot, torch.Tensor) else knot)
            w = np.asarray(w.detach().cpu() if isinstance(w, torch.Tensor) else w, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("knots must be a pair (knot [K], w [K,2]) as mppi_knots returns it") from None
        if knot.shape != (K,) or knot.dtype.kind not in "iu" or w.shape != (K, 2):
            raise ValueError("knots must be (knot: %d integers, w: shape (%d, 2)), got shapes %s and %s"
                             % (K, K, knot.shape, w.shape))
        if int(knot.min()) < 1 or int(knot.max()) + 1 > MPPI_MAX_KNOT:
            raise ValueError("knot numbers must lie in [1, %d]" % (MPPI_MAX_KNOT - 1))
        w = w.astype(np.float32)
        if not np.isfinite(w).all():
            raise ValueError("knot weights must be finite")
        # (int32 on the device: the same 32 bits; knot numbers are far below 2^31)
        return np.ascontiguousarray(knot.astype(np.uint32)).view(np.int32), w
    return _wire.uploaded(env, "mppi_knots", check)


def _mppi_ext(env, knots, K):
    """(cs_rollout_mppi_ext with the knot table filled in, the tensors it points to)."""
    ext = _wire.block(_lib.RolloutMppiExt)
    keep = []
    if knots is not None:
        kn, kw = keep = _mppi_knots(env, knots, K)
        ext.knot_dev, ext.knot_weights_dev = kn.data_ptr(), kw.data_ptr()
    return ext, keep


def _costs_tape(env, costs):
    """costs [P,N], rollout_mppi_costs' result, checked; returns P."""
    torch = _torch()
    n = env.num_envs
    if not isinstance(costs, torch.Tensor) or costs.dim() != 2 or not 1 <= costs.shape[0] <= _lib.MPPI_MAX_SAMPLES:
        raise ValueError("costs must be the [P,%d] float64 device tensor of rollout_mppi_costs" % n)
    P = int(costs.shape[0])
    _wire.check_tape(env, "rollout_mppi_costs", (costs, "costs", (P, n), torch.float64))
    return P


def rollout_mppi_costs(self, actions, sigma, samples, x_ref, Q, R, Q_final=None, a_ref=None, reward_weight=0.0,
                       stream=0, state=None, knots=None):
    """The costs of P = `samples` noisy copies of the action tape `actions` [K,N,A] per env, one kernel: sample p
    takes a_k = actions[k-1] + sigma * eps(p, k) in float32 (one multiply, one add), eps the library's counter-based
    noise -- Irwin-Hall of order 4, mean 0, variance 1 - 2**-32, a pure function of (seed, global env id, `stream`,
    k, p, component): tests/mppi_ref.py restates it in NumPy bit for bit -- and sample 0 is `actions` itself.  Each
    copy is rolled out as rollout_states would (same start rules: state=None or get_state()'s layout; the step clips
    the motors itself) and scored in float64, in registers:

        S = sum_k 1/2 (x_k - x_ref)^T Q_k (x_k - x_ref) + 1/2 (a_k - a_ref)^T R (a_k - a_ref) - reward_weight reward_k

    with Q_K = Q_final when given.  sigma: a scalar or [A], >= 0; x_ref: [12], [N,12] or [K,N,12]; Q [12,12] and
    R [A,A] symmetric positive semidefinite, shared; a_ref [A] or None (zero); reward_weight >= 0 brings in the
    task's own reward (rollout_states' float64 reward); `stream` is a nonce in [0, 2**32), for example the MPC
    iteration.  No state tape and no noise tensor exist.

    knots=(knot [K], w [K,2]) (mppi_knots(K, hold)) makes the noise smooth: step k takes
    eps~ = float32(float32(w[k][0] eps(p, knot[k])) + float32(w[k][1] eps(p, knot[k] + 1))) in place of eps(p, k) --
    tests/mppi_smooth_ref.py restates it bit for bit; None, or the white table mppi_knots(K, 1), is the noise above.

    Returns MppiCosts(costs [P,N] float64, best [N] int32: the arg-min over the env's finite costs, the lowest index
    on ties, -1 if none is finite).  Asynchronous on the current stream; the tensors are buffers of this env,
    overwritten by its next call with the same P.  No env state changes."""
    self._check_open()
    torch = _torch()
    # (the MPPI loop calls this three times an iteration on small batches, so it is wired by hand: inline scalar checks,
    # the blocks filled member by member and the library called directly -- what _wire.int_in, finite, block's keywords
    # and launch do, without their calls; profiles/host_wrappers_refactor_ab.txt)
    if not isinstance(samples, (int, np.integer)) or isinstance(samples, bool) \
            or not 1 <= int(samples) <= _lib.MPPI_MAX_SAMPLES:
        raise ValueError("samples must be %s, got %r" % (_SAMPLES, samples))
    P = int(samples)
    wr = float(reward_weight)
    if not (wr >= 0.0) or wr == float("inf"):
        raise ValueError("reward_weight must be finite and >= 0, got %r" % (reward_weight,))
    Qd, Rd, Qfd = _lqr_weights(self, Q, R, Q_final, definite=False)
    sg = _mppi_small(self, sigma, "sigma", np.float32, True)
    ar = None if a_ref is None else _mppi_small(self, a_ref, "a_ref", np.float64, False)
    io, K, keep = _rollout._rollout_io(self, actions, state)
    n = self.num_envs
    xr = x_ref if isinstance(x_ref, torch.Tensor) else torch.from_numpy(np.asarray(x_ref, dtype=np.float64))
    if tuple(xr.shape) == (12,):
        xr = xr.expand(n, 12)
    if tuple(xr.shape) not in ((n, 12), (K, n, 12)) or not xr.dtype.is_floating_point:
        raise ValueError("x_ref must be a floating-point array of shape (12,), (%d, 12) or (%d, %d, 12), got %s"
                         % (n, K, n, tuple(xr.shape)))
    xr = xr.detach().to(device=self.device, dtype=torch.float64).contiguous()
    keep.append(xr)
    if not isinstance(stream, (int, np.integer)) or isinstance(stream, bool) or not 0 <= int(stream) < _wire.U32:
        raise ValueError("stream must be %s, got %r" % (_wire.IN_U32, stream))
    out = _wire.rollout_cache(self, ("mppi_costs", P), lambda: MppiCosts(
        _wire.empty(self, (P, n), torch.float64), _wire.empty(self, n, torch.int32)))
    mio = _wire.block(_lib.RolloutMppiIO)
    mio.num_samples, mio.noise_stream = P, int(stream)
    mio.x_ref_steps = 1 if xr.dim() == 3 else 0
    mio.reward_weight = wr
    mio.sigma_dev, mio.x_ref_dev = sg.data_ptr(), xr.data_ptr()
    mio.a_ref_dev = None if ar is None else ar.data_ptr()
    mio.Q_dev, mio.R_dev = Qd.data_ptr(), Rd.data_ptr()
    mio.Q_final_dev = None if Qfd is None else Qfd.data_ptr()
    mio.costs_dev, mio.best_dev = out.costs.data_ptr(), out.best.data_ptr()
    keep += [Qd, Rd, Qfd, sg, ar]
    with torch.cuda.device(self.device):
        if knots is None:
            _lib.check(self._lib.cs_rollout_mppi_costs(self._ctx, C.byref(io), C.byref(mio), self._stream()))
        else:
            ext, kept = _mppi_ext(self, knots, K)
            keep += kept
            _lib.check(self._lib.cs_rollout_mppi_costs_ex(self._ctx, C.byref(io), C.byref(mio), C.byref(ext),
                                                          self._stream()))
    self._keep = keep
    return out


def rollout_mppi_update(self, actions, costs, sigma, lam, stream=0, knots=None):
    """The MPPI update, one kernel: per env, with beta = its minimum finite cost, w_p = exp(-(costs[p] - beta) / lam)
    (0 for a cost that is not finite) and eta = sum_p w_p,

        actions_out[k-1] = clip01(float32(actions[k-1] + (1 / eta) sum_p w_p sigma eps(p, k)))

    in float64 with p ascending, eps drawn again from the counter: `costs` [P,N] float64 is what
    rollout_mppi_costs(actions, sigma, P, ..., stream=stream) returned for the same actions, sigma and stream.
    lam > 0 is the temperature: a scalar, or an [N] float64 device tensor with one temperature per env
    (rollout_mppi_temperature's); an env whose entry is not finite and > 0 keeps its actions and reports ess = 0.
    knots: the table rollout_mppi_costs was given.  Returns MppiUpdate(actions [K,N,A] float32, ess [N] float64 = eta^2 / sum_p w_p^2:
    the effective sample size, cost_min [N] = beta).  An env without a finite cost keeps its actions (the same
    bits) and reports ess = 0, cost_min = inf.  Every sum runs inside one lane in a fixed order: two calls give the
    same bits.  Asynchronous on the current stream; the tensors are buffers of this env (two sets, so that the
    result of one call can be the `actions` of the next), overwritten by its second next call with the same K.  No
    env state changes."""
    self._check_open()
    torch = _torch()
    lam_t = lam if isinstance(lam, torch.Tensor) and lam.dim() > 0 else None
    if lam_t is None:
        lam = _wire.finite(float(lam), "lam", 0, above=True)
    sg = _mppi_small(self, sigma, "sigma", np.float32, True)
    io, K, keep = _rollout._rollout_io(self, actions, None)
    n, ad = self.num_envs, self.action_dim
    if lam_t is not None:
        _wire.check_tape(self, "rollout_mppi_update", (lam_t, "lam", (n,), torch.float64))
    P = _costs_tape(self, costs)
    nonce = _wire.int_in(stream, "stream", 0, _wire.U32, _wire.IN_U32)
    sets = _wire.rollout_cache(self, ("mppi_update", K), lambda: [MppiUpdate(
        _wire.empty(self, (K, n, ad), torch.float32), _wire.empty(self, n, torch.float64),
        _wire.empty(self, n, torch.float64)) for _ in range(2)])
    out = sets[1] if sets[0].actions.data_ptr() == io.actions_dev else sets[0]
    mio = _wire.block(_lib.RolloutMppiIO, num_samples=P, noise_stream=nonce,
                      lam=0.0 if lam_t is not None else lam, sigma_dev=sg.data_ptr(), costs_dev=costs.data_ptr(),
                      actions_out_dev=out.actions.data_ptr(), ess_dev=out.ess.data_ptr(),
                      cost_min_dev=out.cost_min.data_ptr())
    keep = keep + [sg, costs, lam_t]
    if knots is None and lam_t is None:
        _wire.launch(self, "cs_rollout_mppi_update", io, mio, keep=keep)
    else:
        ext, kept = _mppi_ext(self, knots, K)
        if lam_t is not None:
            ext.lam_dev = lam_t.data_ptr()
        _wire.launch(self, "cs_rollout_mppi_update_ex", io, mio, ext, keep=keep + kept)
    return out


def rollout_mppi_temperature(self, costs, ess_target, lam_min=1e-6, lam_max=1e6):
    """The temperature per env at which the MPPI weights of `costs` [P,N] (rollout_mppi_costs') have the effective
    sample size ess_target, one kernel: with E(lam) = (sum_p w_p)^2 / sum_p w_p^2 over the env's finite costs, 48
    bisections of ln lam between ln lam_min and ln lam_max, keeping E >= ess_target at the upper end; lam_max where
    even E(lam_max) < ess_target, lam_min where E(lam_min) >= ess_target, lam_max (and ess 0) for an env without a
    finite cost.  ess_target >= 1, 0 < lam_min < lam_max.  Returns MppiTemperature(lam [N] float64, for
    rollout_mppi_update(lam=), ess [N] float64 = E(lam)).  Two calls give the same bits.  Asynchronous on the
    current stream; the tensors are buffers of this env, overwritten by its next call.  No env state changes."""
    self._check_open()
    torch = _torch()
    n = self.num_envs
    target = _wire.finite(ess_target, "ess_target", 1)
    lo, hi = float(lam_min), float(lam_max)
    if not (0.0 < lo < hi) or hi == float("inf"):
        raise ValueError("0 < lam_min < lam_max, both finite, is required, got %r and %r" % (lam_min, lam_max))
    P = _costs_tape(self, costs)
    out = _wire.rollout_cache(self, ("mppi_temperature",), lambda: MppiTemperature(
        _wire.empty(self, n, torch.float64), _wire.empty(self, n, torch.float64)))
    mio = _wire.block(_lib.RolloutMppiIO, num_samples=P, costs_dev=costs.data_ptr())
    ext = _wire.block(_lib.RolloutMppiExt, ess_target=target, lam_min=lo, lam_max=hi, lam_out_dev=out.lam.data_ptr(),
                      ess_out_dev=out.ess.data_ptr())
    _wire.launch(self, "cs_rollout_mppi_temperature", mio, ext, keep=[costs])
    return out


def mppi(env, actions0, x_ref, Q, R, Q_final=None, a_ref=None, reward_weight=0.0, samples=256, sigma=0.1, lam=1.0,
         iters=10, state=None, stream0=0, hold=1, ess_target=None, lam_range=(1e-6, 1e6)):
    """Minimise the cost above over the actions [K,N,A] of env's rollout from `state` (None: its stored state),
    starting from actions0.  x_ref is [12], [N,12] or [K,N,12]; a_ref [A] or None (zero); sigma a scalar or [A]; lam the
    temperature.  hold: the steps between two noise knots (mppi_knots(K, hold); 1 is white noise) -- sigma is the
    standard deviation at every step either way; set it against the hover motor value (0.0166 for the default vehicle),
    not against the action range.  ess_target: None, or the effective sample size the temperature is solved for per env
    and iteration within lam_range (`lam` is then unused) -- it removes the dependence on the cost's scale, and it hurts
    where the cost is bimodal (the Lander's landing bonus: DESIGN.md section 15), so it is not the default.

    Iteration t: rollout_mppi_costs with stream = stream0 + t, (rollout_mppi_temperature,) rollout_mppi_update, then the
    cost of the candidate plan alone (samples = 1: the nominal).  Each env takes the candidate only where its cost is
    lower, else it keeps its plan (ilqr's rule: the cost history is non-increasing per env by construction).  No host
    read happens inside the loop.

    Returns MppiResult(actions [K,N,A] float32, cost [iters+1,N] float64: per env, before the first iteration and after
    each, ess [iters,N] float64: the effective sample size of each update)."""
    torch = _torch()
    dev = env.device
    acts = actions0.detach() if isinstance(actions0, torch.Tensor) else torch.as_tensor(actions0)
    acts = acts.to(device=dev, dtype=torch.float32).clone().contiguous()
    n = acts.shape[1]
    knots = None if hold == 1 else mppi_knots(int(acts.shape[0]), hold)
    kw = dict(Q_final=Q_final, a_ref=a_ref, reward_weight=reward_weight, state=state)
    cost = env.rollout_mppi_costs(acts, sigma, 1, x_ref, Q, R, **kw).costs[0].clone()
    history, sizes = [cost], []
    for t in range(iters):
        costs = env.rollout_mppi_costs(acts, sigma, samples, x_ref, Q, R, stream=stream0 + t, knots=knots, **kw).costs
        if ess_target is not None:
            lam = env.rollout_mppi_temperature(costs, ess_target, lam_range[0], lam_range[1]).lam
        up = env.rollout_mppi_update(acts, costs, sigma, lam, stream=stream0 + t, knots=knots)
        sizes.append(up.ess.clone())
        c = env.rollout_mppi_costs(up.actions, sigma, 1, x_ref, Q, R, **kw).costs[0]
        better = c < cost                              # (a non-finite candidate compares False)
        acts = torch.where(better[None, :, None], up.actions, acts).contiguous()
        cost = torch.where(better, c, cost)
        history.append(cost)
    ess = torch.stack(sizes) if sizes else torch.zeros((0, n), dtype=torch.float64, device=dev)
    return MppiResult(acts, torch.stack(history), ess)
