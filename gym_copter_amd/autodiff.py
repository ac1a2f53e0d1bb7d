"""torch.autograd over K-step rollouts: differentiable_rollout(env, actions, state) is CopterVecEnv.rollout_states
as a differentiable function of the actions (and of an explicit start's x, and optionally of the vehicle and the start's
pending force), its backward CopterVecEnv.rollout_vjp (rollout_vjp_params).  See DESIGN.md sections 10 and 11 and
INTEGRATION.md."""
from .vecenv import Rollout, _torch

_FN = None
_FN_PARAMS = None


def _function():
    global _FN
    if _FN is not None:
        return _FN
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class RolloutFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, actions, x0, env, state):
            r = env.rollout_states(actions, state)
            x, reward = r.x.clone(), r.reward.clone()           # (the env's buffers are overwritten by its next call)
            term, trunc, status = r.terminated.clone(), r.truncated.clone(), r.status.clone()
            ctx.mark_non_differentiable(term, trunc, status)
            ctx.save_for_backward(actions, x, status)
            ctx.env, ctx.state, ctx.want_x0 = env, state, x0 is not None
            return x, reward, term, trunc, status

        @staticmethod
        @once_differentiable
        def backward(ctx, gx, gr, *_):
            actions, x, status = ctx.saved_tensors
            env = ctx.env
            ga, g0 = env.rollout_vjp(actions, Rollout(x, None, None, None, status), gx=gx, gr=gr, state=ctx.state,
                                     dtype=torch.float64)
            ga = ga.to(actions.dtype)                           # (a copy: the env's buffer is overwritten next call)
            g0 = g0.clone() if (ctx.want_x0 and g0 is not None) else None
            return ga, g0, None, None

    _FN = RolloutFunction
    return _FN


def _function_params():
    global _FN_PARAMS
    if _FN_PARAMS is not None:
        return _FN_PARAMS
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class RolloutParamsFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, actions, x0, vehicle, force, env, state):
            r = env.rollout_states(actions, state, vehicle=vehicle)
            x, reward = r.x.clone(), r.reward.clone()
            term, trunc, status = r.terminated.clone(), r.truncated.clone(), r.status.clone()
            ctx.mark_non_differentiable(term, trunc, status)
            # (the vehicle is saved, not kept as an attribute: autograd then refuses a backward after an in-place change
            # of it, so the backward may skip re-checking the table the forward's rollout_states checked)
            ctx.save_for_backward(actions, x, status, vehicle)
            ctx.env, ctx.state = env, state
            ctx.want = (x0 is not None, vehicle is not None and vehicle.requires_grad, force is not None)
            return x, reward, term, trunc, status

        @staticmethod
        @once_differentiable
        def backward(ctx, gx, gr, *_):
            actions, x, status, vehicle = ctx.saved_tensors
            ga, g0, gv, gf = ctx.env._vjp(actions, Rollout(x, None, None, None, status), gx, gr, ctx.state,
                                          torch.float64, params=True, vehicle=vehicle, check_vehicle=False)
            want_x0, want_v, want_f = ctx.want
            return (ga.to(actions.dtype), g0.clone() if (want_x0 and g0 is not None) else None,
                    gv.clone() if want_v else None, gf.clone() if want_f else None, None, None)

    _FN_PARAMS = RolloutParamsFunction
    return _FN_PARAMS


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
    neither, the rollout is differentiated with respect to the actions and x0 only, as without them."""
    torch = _torch()
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.float32:
        raise ValueError("actions must be a float32 torch tensor of shape (K, %d, %d)" % (env.num_envs, env.action_dim))
    if actions.device != env.device:
        raise ValueError("actions must be on %s, got %s" % (env.device, actions.device))
    x0 = None
    if state is not None and isinstance(state.get("x"), torch.Tensor) and state["x"].requires_grad:
        if state["x"].dtype != torch.float64:
            raise ValueError("state['x'] must be float64 to receive a gradient, got %s" % state["x"].dtype)
        x0 = state["x"]
    force = None
    if state is not None and isinstance(state.get("force"), torch.Tensor) and state["force"].requires_grad:
        if state["force"].dtype != torch.float64:
            raise ValueError("state['force'] must be float64 to receive a gradient, got %s" % state["force"].dtype)
        force = state["force"]
    if vehicle is not None:
        if not isinstance(vehicle, torch.Tensor) or vehicle.dtype != torch.float64:
            raise ValueError("vehicle must be a float64 torch tensor of shape (%d, %d)"
                             % (len(env.VEHICLE_ROWS), env.num_envs))
    if vehicle is None and force is None:
        out = _function().apply(actions, x0, env, state)
    else:
        out = _function_params().apply(actions, x0, vehicle, force, env, state)
    return Rollout(*out)
