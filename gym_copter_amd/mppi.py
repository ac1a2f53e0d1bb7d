"""A small MPPI driver on CopterVecEnv.rollout_mppi_costs / rollout_mppi_update (DESIGN.md sections 14 and 15): batched
sampling-based trajectory optimisation of open-loop actions, one independent problem per env.

    S = sum_{k=1..K} 1/2 (x_k - x_ref)^T Q_k (x_k - x_ref) + 1/2 (a_k - a_ref)^T R (a_k - a_ref) - reward_weight reward_k

with Q_K = Q_final.  Every iteration is three kernels -- the costs of `samples` noisy copies of the plan, their weighted
average, the cost of that candidate -- and a few torch selections on the device; nothing is read by the host.  With
hold > 1 the noise is smooth (piecewise linear between knots `hold` steps apart); with ess_target a fourth kernel solves a
temperature per env between the costs and the update."""
import collections

MppiResult = collections.namedtuple("MppiResult", "actions cost ess")


def _torch():
    import torch
    return torch


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
    knots = None
    if hold != 1:
        from .vecenv import mppi_knots
        knots = mppi_knots(int(acts.shape[0]), hold)
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
