"""torch.autograd over K-step rollouts: differentiable_rollout(env, actions, state) is CopterVecEnv.rollout_states
as a differentiable function of the actions (and of an explicit start's x, and optionally of the vehicle and the start's
pending force), its backward CopterVecEnv.rollout_vjp (rollout_vjp_params); differentiable_mlp_rollout(env, params, K,
hidden) is the closed-loop CopterVecEnv.rollout_mlp_states under an MLP policy, its backward rollout_mlp_vjp.  See
DESIGN.md sections 10 to 12 and INTEGRATION.md."""
from .rollout import _vjp
from .vecenv import MlpRollout, Rollout, _torch

_FN = None
_FN_MLP = None
_FN_PPO = None


def _function():
    global _FN
    if _FN is not None:
        return _FN
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class RolloutFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, actions, x0, vehicle, force, env, state):
            r = env.rollout_states(actions, state, vehicle=vehicle)
            x, reward = r.x.clone(), r.reward.clone()           # (the env's buffers are overwritten by its next call)
            term, trunc, status = r.terminated.clone(), r.truncated.clone(), r.status.clone()
            ctx.mark_non_differentiable(term, trunc, status)
            # (the vehicle is saved, not kept as an attribute: autograd then refuses a backward after an in-place change
            # of it, so the backward may skip re-checking the table the forward's rollout_states checked)
            ctx.save_for_backward(actions, x, status, vehicle)
            ctx.save_for_forward(actions, x, status, vehicle)   # (what jvp needs: the same tape)
            ctx.env, ctx.state = env, state
            ctx.params = vehicle is not None or force is not None
            ctx.want = (x0 is not None, vehicle is not None and vehicle.requires_grad, force is not None)
            return x, reward, term, trunc, status

        @staticmethod
        @once_differentiable
        def backward(ctx, gx, gr, *_):
            actions, x, status, vehicle = ctx.saved_tensors
            tape = Rollout(x, None, None, None, status)
            if ctx.params:                                      # the parameter VJP: g_vehicle and g_force as well
                ga, g0, gv, gf = _vjp(ctx.env, actions, tape, gx, gr, ctx.state, torch.float64, params=True,
                                      vehicle=vehicle, check_vehicle=False)
            else:
                ga, g0 = ctx.env.rollout_vjp(actions, tape, gx=gx, gr=gr, state=ctx.state, dtype=torch.float64)
                gv = gf = None
            want_x0, want_v, want_f = ctx.want
            # (copies: the env's buffers are overwritten by its next call)
            return (ga.to(actions.dtype), g0.clone() if (want_x0 and g0 is not None) else None,
                    gv.clone() if want_v else None, gf.clone() if want_f else None, None, None)

        @staticmethod
        def jvp(ctx, t_actions, t_x0, t_vehicle, t_force, *_):
            # forward mode (torch.autograd.forward_ad): the tangents of x and reward, CopterVecEnv.rollout_jvp
            actions, x, status, vehicle = ctx.saved_tensors
            if t_actions is None and t_x0 is None and t_vehicle is None and t_force is None:
                return torch.zeros_like(x), torch.zeros_like(x[..., 0]), None, None, None
            t = ctx.env.rollout_jvp(actions, Rollout(x, None, None, None, status), t_actions=t_actions, t_x0=t_x0,
                                    t_vehicle=t_vehicle, t_force=t_force, state=ctx.state, vehicle=vehicle,
                                    dtype=torch.float64, check_vehicle=False)
            # (copies: the env's buffers are overwritten by its next call)
            return t.x.clone(), t.reward.clone(), None, None, None

    _FN = RolloutFunction
    return _FN


def differentiable_rollout(env, actions, state=None, vehicle=None):
    """K steps of `env` with auto-reset disabled (CopterVecEnv.rollout_states), differentiable: returns a Rollout of
    x [K,N,12] float64 and reward [K,N] float64 that carry gradients, and terminated / truncated / status that do not.
    `actions` [K,N,A] is a float32 device tensor; it and an explicit start's state["x"] ([12,N] float64, when it
    requires grad) receive gradients from the backward (CopterVecEnv.rollout_vjp).  An observation is a slice of x
    (env.STATE_NAMES), so a loss on observations needs nothing more.  The start is the env's stored state (state=None;
    the env must not step between the forward and the backward) or an explicit point as rollout_states takes it.  The
    outputs are copies, the env's buffers are free for its next call.  Once differentiable: a double backward raises.

    vehicle: a [12,N] float64 device tensor of the vehicle rows (env.VEHICLE_ROWS) to roll out with instead of the env's
    own (rollout_states(..., vehicle=)); when it requires grad it receives dL / d vehicle, and a state["force"] that
    requires grad (float64 [3,N]) receives dL / d force (CopterVecEnv.rollout_vjp_params).  With
    neither, the rollout is differentiated with respect to the actions and x0 only, as without them.

    Forward mode: under torch.autograd.forward_ad.dual_level(), duals on `actions`, state["x"], `vehicle` or
    state["force"] come out with tangents on x and reward (CopterVecEnv.rollout_jvp)."""
    torch = _torch()
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.float32:
        raise ValueError("actions must be a float32 torch tensor of shape (K, %d, %d)" % (env.num_envs, env.action_dim))
    if actions.device != env.device:
        raise ValueError("actions must be on %s, got %s" % (env.device, actions.device))

    def wanted(t):  # a gradient (reverse mode) or a tangent (a dual tensor of torch.autograd.forward_ad) is asked for
        return isinstance(t, torch.Tensor) and (t.requires_grad or
                                                torch.autograd.forward_ad.unpack_dual(t).tangent is not None)
    x0 = None
    if state is not None and wanted(state.get("x")):
        if state["x"].dtype != torch.float64:
            raise ValueError("state['x'] must be float64 to receive a gradient, got %s" % state["x"].dtype)
        x0 = state["x"]
    force = None
    if state is not None and wanted(state.get("force")):
        if state["force"].dtype != torch.float64:
            raise ValueError("state['force'] must be float64 to receive a gradient, got %s" % state["force"].dtype)
        force = state["force"]
    if vehicle is not None:
        if not isinstance(vehicle, torch.Tensor) or vehicle.dtype != torch.float64:
            raise ValueError("vehicle must be a float64 torch tensor of shape (%d, %d)"
                             % (len(env.VEHICLE_ROWS), env.num_envs))
    return Rollout(*_function().apply(actions, x0, vehicle, force, env, state))


def _function_mlp():
    global _FN_MLP
    if _FN_MLP is not None:
        return _FN_MLP
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class MlpRolloutFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, params, offsets, x0, env, num_steps, hidden, state, action_grad, reduce):
            r = env.rollout_mlp_states(params, num_steps, hidden, offsets=offsets, state=state)
            out = tuple(t.clone() for t in r)                   # (the env's buffers are overwritten by its next call)
            x, reward, term, trunc, status, obs, actions = out
            if action_grad:                                     # (the action tape carries a gradient: its cotangent is
                ctx.mark_non_differentiable(term, trunc, status, obs)       # the backward's g_actions_in)
            else:
                ctx.mark_non_differentiable(term, trunc, status, obs, actions)
            ctx.action_grad, ctx.reduce = action_grad, reduce
            # (params is saved, not kept as an attribute: autograd refuses a backward after an in-place change of it)
            ctx.save_for_backward(params, x, status, obs, actions)
            ctx.env, ctx.state, ctx.hidden = env, state, hidden
            ctx.want = (offsets is not None, x0 is not None)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, gx, gr, *rest):
            params, x, status, obs, actions = ctx.saved_tensors
            gact = rest[4] if ctx.action_grad else None         # (the cotangent of the action tape, the seventh output)
            gp, ga, g0 = ctx.env.rollout_mlp_vjp(params, MlpRollout(x, None, None, None, status, obs, actions), gx=gx,
                                                 gr=gr, state=ctx.state, hidden=ctx.hidden, dtype=torch.float64,
                                                 g_actions_in=gact, reduce=ctx.reduce)
            want_u, want_x0 = ctx.want
            return (gp.to(params.dtype), ga.to(torch.float32) if want_u else None,
                    g0.clone() if (want_x0 and g0 is not None) else None, None, None, None, None, None, None)

    _FN_MLP = MlpRolloutFunction
    return _FN_MLP


def differentiable_mlp_rollout(env, params, num_steps, hidden, offsets=None, state=None, action_grad=False,
                               reduce="torch"):
    """K = num_steps closed-loop steps of `env` under the MLP policy `params` (CopterVecEnv.rollout_mlp_states: step k
    takes a_k = float32(pi(o_{k-1}) + offsets[k-1]), auto-reset disabled), differentiable: returns an MlpRollout whose
    x [K,N,12] float64 and reward [K,N] float64 carry gradients, and whose terminated / truncated / status and the obs /
    actions tapes do not.  `params` ([P] float32 device tensor, gym_copter_amd.mlp's layout) receives dL / d params,
    `offsets` ([K,N,A] float32, optional) dL / d offsets, an explicit start's state["x"] ([12,N] float64, when it
    requires grad) dL / d x0 -- all through one backward kernel (CopterVecEnv.rollout_mlp_vjp) and one reduction for the
    parameters: torch matrix products (reduce="torch", the default) or one HIP kernel (reduce="device",
    CopterVecEnv.mlp_param_grad).  The outputs are copies; an in-place change of params between the forward and the
    backward is refused, and a double backward raises (once differentiable).  With the stored start the env must not
    step between the forward and the backward.  With action_grad=True the returned `actions` tape ([K,N,A] float32)
    carries a gradient too: a loss on the actions themselves (control effort, action rate) is differentiated, its
    cotangent entering the backward as rollout_mlp_vjp's g_actions_in.  With the default the action tape is an output
    without gradient, and a loss on it is not differentiated."""
    torch = _torch()
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.dim() != 1:
        raise ValueError("params must be a 1-D float32 torch tensor (gym_copter_amd.mlp)")
    if params.device != env.device:
        raise ValueError("params must be on %s, got %s" % (env.device, params.device))
    if offsets is not None:
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.float32:
            raise ValueError("offsets must be a float32 torch tensor of shape (%d, %d, %d)"
                             % (num_steps, env.num_envs, env.action_dim))
        if offsets.device != env.device:
            raise ValueError("offsets must be on %s, got %s" % (env.device, offsets.device))
    x0 = None
    if state is not None and isinstance(state.get("x"), torch.Tensor) and state["x"].requires_grad:
        if state["x"].dtype != torch.float64:
            raise ValueError("state['x'] must be float64 to receive a gradient, got %s" % state["x"].dtype)
        x0 = state["x"]
    if reduce not in ("torch", "device"):
        raise ValueError("reduce must be 'torch' or 'device', got %r" % (reduce,))
    out = _function_mlp().apply(params, offsets, x0, env, num_steps, hidden, state, bool(action_grad), reduce)
    return MlpRollout(*out)


def _function_ppo():
    global _FN_PPO
    if _FN_PPO is not None:
        return _FN_PPO
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class PpoLossFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, actor, critic, log_std, env, hidden, critic_hidden, tapes, kw):
            g = env.ppo_grad(actor, critic, log_std, hidden, critic_hidden, *tapes, **kw)
            stats = g.stats
            ctx.mark_non_differentiable(stats)
            ctx.sizes = (actor.shape[0], 0 if critic is None else critic.shape[0])
            ctx.dtypes = (actor.dtype, None if critic is None else critic.dtype, log_std.dtype)
            ctx.save_for_backward(g.grad)
            return stats[4].clone(), stats

        @staticmethod
        @once_differentiable
        def backward(ctx, g_loss, _g_stats):
            grad, = ctx.saved_tensors
            P, Pv = ctx.sizes
            g = g_loss * grad
            return (g[:P].to(ctx.dtypes[0]), g[P:P + Pv].to(ctx.dtypes[1]) if ctx.dtypes[1] is not None else None,
                    g[P + Pv:].to(ctx.dtypes[2]), None, None, None, None, None)

    _FN_PPO = PpoLossFunction
    return _FN_PPO


def ppo_loss(env, actor, critic, log_std, hidden, critic_hidden, obs, actions, logp, advantages, returns, **kw):
    """PPO's clipped-surrogate minibatch loss L as a differentiable float64 scalar, for a caller with an optimizer of
    their own: one CopterVecEnv.ppo_grad call (its arguments and keywords: live, index, row_base, num_samples, clip,
    vf_coef, ent_coef, normalize) makes the loss and its gradient together, and the backward hands grad_output x
    gradient to `actor`, `critic` (None: no value term) and `log_std` in their dtype.  Returns (L, stats [8] float64 --
    vecenv.PPO_STATS, without gradient).  Once differentiable: a double backward raises.  The tapes carry no gradient."""
    for name in ("out", "stats_out"):
        if name in kw:
            raise ValueError("ppo_loss makes its own outputs: %s is not accepted" % name)
    return _function_ppo().apply(actor, critic, log_std, env, hidden, critic_hidden,
                                 (obs, actions, logp, advantages, returns), kw)
