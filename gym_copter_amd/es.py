"""A small evolution-strategies driver on CopterVecEnv.es_perturb / rollout_mlp_population / es_gradient (DESIGN.md
section 16): the MLP policy of the closed-loop rollouts trained on episode returns alone, without a derivative of the
simulator -- touchdowns, crashes, tilt terminations and the motor clip, whose derivatives are zero or one-sided, are
plain events of the return here.

Every iteration is five kernels -- the mirrored population, its rollouts, the members' mean returns, the search gradient
and its fixed-order sum -- and a few torch operations on [M] and [P] tensors; nothing is read by the host."""
import collections

EsResult = collections.namedtuple("EsResult", "params history")


def _torch():
    import torch
    return torch


def shape_fitness(fitness):
    """The centred ranks of the members' fitness [M] float64: rank / (M - 1) - 1/2, the worst member -1/2 and the best
    +1/2; a fitness that is not finite ranks below every finite one."""
    torch = _torch()
    f = fitness.to(torch.float64)
    f = torch.where(torch.isfinite(f), f, torch.full_like(f, float("-inf")))
    M = f.shape[0]
    ranks = torch.empty(M, dtype=torch.float64, device=f.device)
    ranks[torch.argsort(f, stable=True)] = torch.arange(M, dtype=torch.float64, device=f.device)
    return ranks / max(M - 1, 1) - 0.5


def es(env, params0, hidden, K, pairs, sigma, lr, iterations, envs_per_member=64, gamma=1.0, start_x=None,
       shaping="centered_rank"):
    """Maximise the mean K-step return of the MLP policy theta (gym_copter_amd.mlp's layout for `hidden`) by an
    evolution strategy with mirrored sampling, starting from params0 [P].  env holds M E envs, M = 2 `pairs` members of
    E = envs_per_member envs (a multiple of 64) each.  Iteration t:

      1. table = env.es_perturb(theta, sigma, M, t)                    theta +- sigma eps_i
      2. f = env.rollout_mlp_population(table, K, hidden, E, gamma, ..).member_returns
      3. w = shape_fitness(f)                                   centred ranks: an argsort, torch's
      4. g = env.es_gradient(w, t, P) / (M sigma)               the noise drawn again
      5. an Adam step of size lr on theta (betas 0.9 and 0.999), towards larger returns

    start_x: None -- every env starts from its stored state, so the members see DIFFERENT envs (their start points and
    pending perturbations differ: the fitness differences carry that noise) -- or explicit airborne start points, [12,E]
    float64, tiled over the members so that every member sees the SAME E starts (common random numbers), or [12,M E]
    as they are.  No host read happens inside the loop and no env state changes.

    Returns EsResult(params [P] float32: theta after the last step, history [iterations] float64: the mean of
    member_returns -- the perturbed population's, not theta's own -- at every iteration)."""
    torch = _torch()
    dev = env.device
    if not isinstance(pairs, int) or isinstance(pairs, bool) or pairs < 1:
        raise ValueError("pairs must be an int >= 1, got %r" % (pairs,))
    if not isinstance(iterations, int) or isinstance(iterations, bool) or iterations < 0:
        raise ValueError("iterations must be an int >= 0, got %r" % (iterations,))
    if shaping != "centered_rank":
        raise ValueError("shaping must be 'centered_rank', got %r" % (shaping,))
    sigma, lr = float(sigma), float(lr)
    if not sigma > 0.0 or sigma == float("inf"):
        raise ValueError("sigma must be finite and > 0, got %r" % (sigma,))
    M, E = 2 * pairs, envs_per_member
    if M * E != env.num_envs:
        raise ValueError("2 x pairs x envs_per_member = %d x %d is not env.num_envs = %d" % (M, E, env.num_envs))
    theta = (params0.detach() if isinstance(params0, torch.Tensor) else torch.as_tensor(params0))
    theta = theta.to(device=dev, dtype=torch.float64).clone()
    P = int(theta.shape[0])
    if start_x is not None:
        x = start_x if isinstance(start_x, torch.Tensor) else torch.as_tensor(start_x)
        x = x.detach().to(device=dev, dtype=torch.float64)
        if tuple(x.shape) == (12, E) and M > 1:
            x = x.repeat(1, M)
        elif tuple(x.shape) != (12, M * E):
            raise ValueError("start_x must have shape (12, %d) or (12, %d), got %s" % (E, M * E, tuple(x.shape)))
        start_x = x.contiguous()
    m1, m2 = torch.zeros_like(theta), torch.zeros_like(theta)
    history = []
    for t in range(iterations):
        table = env.es_perturb(theta.to(torch.float32), sigma, M, t)
        pop = env.rollout_mlp_population(table, K, hidden, E, gamma, start_x=start_x)
        history.append(pop.member_returns.mean())
        w = shape_fitness(pop.member_returns)
        g = env.es_gradient(w, t, P) / (M * sigma)
        m1 = 0.9 * m1 + 0.1 * g
        m2 = 0.999 * m2 + 0.001 * g * g
        step = (m1 / (1.0 - 0.9 ** (t + 1))) / ((m2 / (1.0 - 0.999 ** (t + 1))).sqrt() + 1e-8)
        theta = theta + lr * step
    hist = torch.stack(history) if history else torch.zeros(0, dtype=torch.float64, device=dev)
    return EsResult(theta.to(torch.float32), hist)
