"""The closed-loop rollouts under the fused MLP policy of gym_copter_amd.mlp:
CopterVecEnv.rollout_mlp_states, rollout_mlp_vjp and mlp_param_grad, bound to the class by vecenv.py.  (mlp.py itself
stays free of the library: it works on CPU tensors.)"""
import collections

from . import _lib, _wire
from . import mlp as _mlp
from . import rollout as _rollout
from ._wire import _torch

# a closed-loop rollout (rollout_mlp_states): Rollout's fields plus the observation and action tapes
MlpRollout = collections.namedtuple("MlpRollout", "x reward terminated truncated status obs actions")


def _mlp_io(self, params, hidden, num_steps, offsets, keep):
    """The cs_rollout_mlp_io of rollout_mlp_states / rollout_mlp_vjp (its tapes not yet set) and the device params."""
    torch = _torch()
    if not isinstance(num_steps, int) or isinstance(num_steps, bool) or num_steps < 1:
        raise ValueError("num_steps must be an int >= 1, got %r" % (num_steps,))
    P = _mlp.num_params(self.obs_dim, self.action_dim, hidden)    # (checks hidden)
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.dim() != 1:
        raise ValueError("params must be a 1-D float32 torch tensor of %d values (gym_copter_amd.mlp), got %s"
                         % (P, getattr(params, "dtype", type(params).__name__)))
    if params.shape[0] != P:
        raise ValueError("params must have %d values for obs_dim %d, action_dim %d, hidden %d, got %d"
                         % (P, self.obs_dim, self.action_dim, hidden, params.shape[0]))
    p = params.detach().to(self.device).contiguous()
    keep.append(p)
    mio = _wire.block(_lib.RolloutMlpIO, hidden=hidden, params_dev=p.data_ptr())
    if offsets is not None:
        u, _ = self._dev_f32(offsets, (num_steps, self.num_envs, self.action_dim), "offsets")
        keep.append(u)
        mio.offsets_dev = u.data_ptr()
    return mio, p


def rollout_mlp_states(self, params, num_steps, hidden, offsets=None, state=None):
    """K = num_steps calls of step() with auto-reset DISABLED under a fused MLP policy, as a pure function (DESIGN
    section 12): step k takes a_k = float32(pi(o_{k-1}) + offsets[k-1]), where o_{k-1} is the float32 observation
    step() returns for the state before step k (the start's for k = 1) and pi the MLP of `params` ([P] float32, the
    layout of gym_copter_amd.mlp; hidden = 0 is linear, 1..64 one tanh layer).  offsets [K,N,A] (None = 0) is an
    open-loop term added to the policy's action.  The start point, the pending perturbation, a pending NEXT_STEP
    reset, prev_shaping and the step counter are rollout_states'; no env state changes.

    Returns MlpRollout(x, reward, terminated, truncated, status -- rollout_states' fields, bit-identical to a twin
    env stepped with `actions` --, obs [K,N,OBS] float32 (o_{k-1}), actions [K,N,A] float32 (a_k)).  Asynchronous on
    the current stream; the tensors are buffers of this env, overwritten by its next call with the same K."""
    self._check_open()
    torch = _torch()
    keep = []
    mio, _ = _mlp_io(self, params, hidden, num_steps, offsets, keep)
    io, K, k2 = _rollout._rollout_io(self, None, state, num_steps)
    keep += k2
    n = self.num_envs
    out = _wire.rollout_cache(self, ("mlp_states", K), lambda: MlpRollout(
        *_rollout._rollout_tensors(self, K), _wire.empty(self, (K, n, self.obs_dim), torch.float32),
        _wire.empty(self, (K, n, self.action_dim), torch.float32)))
    _rollout._wire_rollout(io, out)
    mio.obs_out_dev, mio.actions_out_dev = out.obs.data_ptr(), out.actions.data_ptr()
    _wire.launch(self, "cs_rollout_mlp_states", io, mio, keep=keep)
    return out


def mlp_param_grad(self, params, hidden, obs, g_actions, out=None):
    """g_params [P] float64 = sum_{k,n} J_params pi(obs[k,n])^T g_actions[k,n], reduced ON THE DEVICE by one HIP
    kernel (cs_mlp_param_grad): the device counterpart of gym_copter_amd.mlp.param_grad, the
    same sums term by term in float64 (h recomputed with the device library's tanh), in an order of its own that
    is fixed -- the same inputs give the same bits on every call.  obs [K,N,OBS] float32 is the forward's obs tape,
    g_actions [K,N,A] float64 or float32 what rollout_mlp_vjp returned; both contiguous tensors on this env's
    device.  Asynchronous on the current stream; the result is written (not accumulated) into `out`, a contiguous
    [P] float64 tensor on this env's device, or into a new tensor."""
    self._check_open()
    torch = _torch()
    keep = []
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3 or obs.shape[0] < 1:
        raise ValueError("obs must be the [K,%d,%d] obs tape of rollout_mlp_states" % (self.num_envs, self.obs_dim))
    K = int(obs.shape[0])
    _, p = _mlp_io(self, params, hidden, K, None, keep)
    n = self.num_envs
    _wire.check_tape(self, "rollout_mlp_states", (obs, "obs", (K, n, self.obs_dim), torch.float32))
    if not isinstance(g_actions, torch.Tensor) or g_actions.dtype not in (torch.float64, torch.float32):
        raise ValueError("g_actions must be a float64 or float32 device tensor of shape (%d, %d, %d)"
                         % (K, n, self.action_dim))
    _wire.check_tape(self, "rollout_mlp_vjp", (g_actions, "g_actions", (K, n, self.action_dim), g_actions.dtype))
    if out is None:
        out = _wire.empty(self, p.shape[0], torch.float64)
    else:
        _wire.check_tape(self, "mlp_param_grad", (out, "out", (p.shape[0],), torch.float64))
    gio = _wire.block(_lib.MlpGradIO, ga_dtype=_wire.dtype_code(g_actions.dtype), hidden=hidden, num_steps=K,
                      params_dev=p.data_ptr(), obs_dev=obs.data_ptr(), g_actions_dev=g_actions.data_ptr(),
                      g_params_dev=out.data_ptr())
    _wire.launch(self, "cs_mlp_param_grad", gio, keep=keep + [obs, g_actions])
    return out


def rollout_mlp_vjp(self, params, rollout, gx=None, gr=None, state=None, hidden=None, offsets=None, dtype=None,
                    param_grad=True, g_actions_in=None, reduce="torch"):
    """Reverse-mode gradient of a closed-loop rollout: given the cotangents gx [K,N,12] (on rollout.x) and gr [K,N]
    (on rollout.reward), either None (zero), returns (g_params [P] float64, g_actions [K,N,A], g_x0 [12,N] or None).

    g_actions = dL / d a_k including every later step's dependence on a_k through the policy -- which is also
    dL / d offsets; g_x0 = dL / d state["x"] of an explicit start (including the path through o_0), None for the
    stored one; g_params = sum over envs and steps of J_params pi^T g_actions, reduced by torch from rollout.obs
    (gym_copter_amd.mlp.param_grad; param_grad=False skips it and returns None).  `rollout` is what
    rollout_mlp_states(params, K, hidden, offsets, state) returned (its x, status, obs and actions are the tape;
    with the stored start the env must not have been stepped since); `hidden` must be that call's.  The float32
    rounding of o and a is straight-through.  dtype: torch.float64 (default) or torch.float32 for g_actions and
    g_x0.  Asynchronous on the current stream; g_actions and g_x0 are buffers of this env, overwritten by its next
    call with the same K and dtype.  (`offsets` is accepted for symmetry with the forward; the backward reads the
    action tape, not the offsets.)

    g_actions_in [K,N,A] (None = zero) is a cotangent taken directly on the action tape rollout.actions -- a loss on
    the actions themselves, such as a control-effort penalty: a_k is the action as step() receives it, before the
    clip, so it adds to the step's own g_a_k without a mask, and the total is what g_actions returns, what the
    policy carries back into the state and what g_params is reduced from.  An env that resets in step 1 returns
    g_actions[0] = g_actions_in[0].  reduce="torch" (default) makes g_params with gym_copter_amd.mlp.param_grad,
    reduce="device" with mlp_param_grad (one HIP kernel; the same sums in another, fixed, order)."""
    self._check_open()
    torch = _torch()
    if hidden is None:
        raise ValueError("hidden is required (the forward's)")
    if reduce not in ("torch", "device"):
        raise ValueError("reduce must be 'torch' or 'device', got %r" % (reduce,))
    dtype = _wire.out_dtype(dtype)
    n, ad, od = self.num_envs, self.action_dim, self.obs_dim
    acts = getattr(rollout, "actions", None)
    if not isinstance(acts, torch.Tensor) or acts.dim() != 3:
        raise ValueError("rollout.actions must be the [K,N,A] action tape of rollout_mlp_states")
    K = int(acts.shape[0])
    keep = []
    mio, p = _mlp_io(self, params, hidden, K, None, keep)
    io, _, k2 = _rollout._rollout_io(self, None, state, K)
    keep += k2
    io.out_dtype = _wire.dtype_code(dtype)
    obs = getattr(rollout, "obs", None)
    _wire.check_tape(self, "rollout_mlp_states", (rollout.x, "rollout.x", (K, n, 12), torch.float64),
                     (rollout.status, "rollout.status", (K, n), torch.uint8),
                     (acts, "rollout.actions", (K, n, ad), torch.float32),
                     (obs, "rollout.obs", (K, n, od), torch.float32))
    io.x_dev, io.status_dev = rollout.x.data_ptr(), rollout.status.data_ptr()
    mio.actions_out_dev = acts.data_ptr()
    _rollout._cotangents(self, io, gx, gr, K, keep)
    xio = None
    if g_actions_in is not None:
        gin = _wire.tensor(self, g_actions_in, (K, n, ad), torch.float64, "g_actions_in", keep, host=False,
                           floating=True, foreign=False)
        xio = _wire.block(_lib.RolloutMlpExIO, g_actions_in_dev=gin.data_ptr())
    ga, g0 = _rollout._grad_out(self, io, "mlp_", K, dtype, state is not None)
    # (xio = None is a NULL block: exactly cs_rollout_mlp_vjp)
    _wire.launch(self, "cs_rollout_mlp_vjp_ex", io, mio, xio, keep=keep)
    gp = None
    if param_grad:
        with torch.cuda.device(self.device):
            gp = self.mlp_param_grad(p, hidden, obs, ga) if reduce == "device" else _mlp.param_grad(p, hidden, obs, ga)
        self._keep = keep
    return gp, ga, g0
