"""torch.autograd over K-step rollouts: differentiable_rollout(env, actions, state) is CopterVecEnv.rollout_states
as a differentiable function of the actions (and of an explicit start's x), its backward CopterVecEnv.rollout_vjp.
See DESIGN.md section 10 and INTEGRATION.md."""
from .vecenv import Rollout, _torch

_FN = None


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


def differentiable_rollout(env, actions, state=None):
    """K steps of `env` with auto-reset disabled (CopterVecEnv.rollout_states), differentiable: returns a Rollout of
    x [K,N,12] float64 and reward [K,N] float64 that carry gradients, and terminated / truncated / status that do not.
    `actions` [K,N,A] is a float32 device tensor; it and an explicit start's state["x"] ([12,N] float64, when it
    requires grad) receive gradients from the backward (CopterVecEnv.rollout_vjp).  An observation is a slice of x
    (env.STATE_NAMES), so a loss on observations needs nothing more.  The start is the env's stored state (state=None;
    the env must not step between the forward and the backward) or an explicit point as rollout_states takes it.  The
    outputs are copies, the env's buffers are free for its next call.  Once differentiable: a double backward raises."""
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
    out = _function().apply(actions, x0, env, state)
    return Rollout(*out)
