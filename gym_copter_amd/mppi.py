"""A small MPPI driver on CopterVecEnv.rollout_mppi_costs / rollout_mppi_update: batched
sampling-based trajectory optimisation of open-loop actions, one independent problem per env.

    S = sum_{k=1..K} 1/2 (x_k - x_ref)^T Q_k (x_k - x_ref) + 1/2 (a_k - a_ref)^T R (a_k - a_ref) - reward_weight reward_k

with Q_K = Q_final.  Every iteration is three kernels -- the costs of `samples` noisy copies of the plan, their weighted
average, the cost of that candidate -- and a few torch selections on the device; nothing is read by the host."""
import collections

MppiResult = collections.namedtuple("MppiResult", "actions cost ess")


def _torch():
    import torch
    return torch


def mppi(env, actions0, x_ref, Q, R, Q_final=None, a_ref=None, reward_weight=0.0, samples=256, sigma=0.1, lam=1.0,
         iters=10, state=None, stream0=0):
    """Minimise the cost above over the actions [K,N,A] of env's rollout from `state` (None: its stored state),
    starting from actions0.  x_ref is [12], [N,12] or [K,N,12]; a_ref [A] or None (zero); sigma a scalar or [A]; lam the
    temperature.

    Iteration t: rollout_mppi_costs with stream = stream0 + t, rollout_mppi_update, then the cost of the candidate plan
    alone (samples = 1: the nominal).  Each env takes the candidate only where its cost is lower, else it keeps its plan
    (ilqr's rule: the cost history is non-increasing per env by construction).  No host read happens inside the loop.

    Returns MppiResult(actions [K,N,A] float32, cost [iters+1,N] float64: per env, before the first iteration and after
    each, ess [iters,N] float64: the effective sample size of each update)."""
    torch = _torch()
    dev = env.device
    acts = actions0.detach() if isinstance(actions0, torch.Tensor) else torch.as_tensor(actions0)
    acts = acts.to(device=dev, dtype=torch.float32).clone().contiguous()
    n = acts.shape[1]
    kw = dict(Q_final=Q_final, a_ref=a_ref, reward_weight=reward_weight, state=state)
    cost = env.rollout_mppi_costs(acts, sigma, 1, x_ref, Q, R, **kw).costs[0].clone()
    history, sizes = [cost], []
    for t in range(iters):
        costs = env.rollout_mppi_costs(acts, sigma, samples, x_ref, Q, R, stream=stream0 + t, **kw).costs
        up = env.rollout_mppi_update(acts, costs, sigma, lam, stream=stream0 + t)
        sizes.append(up.ess.clone())
        c = env.rollout_mppi_costs(up.actions, sigma, 1, x_ref, Q, R, **kw).costs[0]
        better = c < cost                              # (a non-finite candidate compares False)
        acts = torch.where(better[None, :, None], up.actions, acts).contiguous()
        cost = torch.where(better, c, cost)
        history.append(cost)
    ess = torch.stack(sizes) if sizes else torch.zeros((0, n), dtype=torch.float64, device=dev)
    return MppiResult(acts, torch.stack(history), ess)
