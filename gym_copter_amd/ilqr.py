"""A small iLQR driver on CopterVecEnv.rollout_lqr / rollout_feedback_states: batched
trajectory optimisation of open-loop actions for a quadratic tracking cost, one independent problem per env.

    J = sum_{k=1..K} 1/2 (x_k - x_ref)^T Q_k (x_k - x_ref) + 1/2 (a_k - a_ref)^T R (a_k - a_ref),   Q_K = Q_final

Every iteration is one backward kernel (the Riccati sweep over the nominal tape) and one forward kernel per line-search
candidate; the cost and its gradients at the tape are a few torch expressions on the device."""
import collections

import numpy as np

IlqrResult = collections.namedtuple("IlqrResult", "actions cost alpha rollout mu")


def _torch():
    import torch
    return torch


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
         alphas=(1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125), mu0=0.0, state=None):
    """Minimise the tracking cost above over the actions [K,N,A] of env's rollout from `state` (None: its stored
    state), starting from actions0.  x_ref and a_ref broadcast against [K,N,12] and [K,N,A] (a_ref=None: zero).

    Per iteration: q, r at the nominal tape (torch), rollout_lqr, then a per-env backtracking line search with
    rollout_feedback_states: each env keeps the first alpha of `alphas` whose ACTUAL cost is below its current one,
    else its nominal (alpha 0).  The Levenberg term mu starts at mu0 and is raised tenfold (from at least 1e-6) for the
    next call whenever rollout_lqr reported a failed factorisation anywhere; those envs' candidates are not finite and
    are never accepted.  The host reads one small tensor per line-search candidate (have all envs accepted?) and
    nothing else.

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
    n = acts.shape[1]
    from .vecenv import Rollout

    ro = env.rollout_states(acts, state=state)
    x, status = ro.x.clone(), ro.status.clone()      # (the env's buffers are overwritten by its next call)
    cost = tracking_cost(x, acts, xr, ar, Qd, Rd, Qfd)
    history, taken = [cost], []
    mu = float(mu0)
    zero = torch.zeros(n, **f64)
    for _ in range(iters):
        q, r = tracking_gradients(x, acts, xr, ar, Qd, Rd, Qfd)
        nominal = Rollout(x, None, None, None, status)
        gains = env.rollout_lqr(acts, nominal, Qh, Rh, q=q, r=r, Q_final=Qfh, mu=mu, state=state)
        accepted = torch.zeros(n, dtype=torch.bool, device=dev)
        step = zero.clone()
        new_x, new_status, new_acts, new_cost = x, status, acts, cost
        all_ok = True
        for al in alphas:
            alpha = torch.where(accepted, zero, torch.full_like(zero, float(al)))
            fro, fa = env.rollout_feedback_states(acts, nominal, gains, alpha, state=state)
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
