"""A small evolution-strategies driver on CopterVecEnv.es_perturb / rollout_mlp_population / es_gradient (DESIGN.md
section 16): the MLP policy of the closed-loop rollouts trained on episode returns alone, without a derivative of the
simulator -- touchdowns, crashes, tilt terminations and the motor clip, whose derivatives are zero or one-sided, are
plain events of the return here.

Every iteration is five kernels -- the mirrored population, its rollouts, the members' mean returns, the search gradient
and its fixed-order sum -- and a few torch operations on [M] and [P] tensors; nothing is read by the host."""
import collections

import numpy as np

from . import _lib, _wire
from . import mlp as _mlp
from . import rollout as _rollout
from ._wire import _torch

EsResult = collections.namedtuple("EsResult", "params history")
# CopterVecEnv.rollout_mlp_population's result
Population = collections.namedtuple("Population", "returns lengths end_flags end_status member_returns")


# -- population rollouts and evolution strategies: CopterVecEnv's methods, bound in vecenv.py -------
def rollout_mlp_population(self, table, K, hidden, envs_per_member, gamma=1.0, start_x=None, start_status=None,
                           state=None):
    """M = table.shape[0] policies, each rolled out closed-loop for K steps on its own E = envs_per_member envs and
    scored by its episode return, one kernel and no tape: env i runs under theta = table[i // E] ([M,P] float32,
    every row in gym_copter_amd.mlp's layout for `hidden`); N = M E, E a multiple of 64.  With the outputs
    rollout_mlp_states(table[m], K, hidden) gives for the same start, and d the first step at which an env is
    terminated or truncated (K if none):

        returns[i] = sum_{k=1..d} gamma^(k-1) reward_k   (float64, k ascending, the discount a running product)
        lengths[i] = d,  end_flags[i] = terminated_d | truncated_d << 1,  end_status[i] = status_d

    exactly (the policy's float32 arithmetic and the step are rollout_mlp_states'), and member_returns[m] = the mean
    of returns over the member's envs, summed in a fixed order (the same bits on every call).  The start is
    rollout_mlp_states': the stored state (its pending perturbation; a pending NEXT_STEP reset is performed in step
    1), or an explicit one -- start_x [12,N] float64 with start_status [N] (None: all airborne), or `state`,
    get_state()'s layout.  With stored starts the members see different envs; give every member the same E start
    points for common random numbers (gym_copter_amd.es does).

    Returns Population(returns [N] float64, lengths [N] int32, end_flags [N] uint8, end_status [N] uint8,
    member_returns [M] float64).  Asynchronous on the current stream; the tensors are buffers of this env,
    overwritten by its next call with the same M.  No env state changes."""
    self._check_open()
    torch = _torch()
    n, dev = self.num_envs, self.device
    K = _wire.int_in(K, "K", 1, None, "an int >= 1")
    P = _mlp.num_params(self.obs_dim, self.action_dim, hidden)    # (checks hidden)
    E = _wire.int_in(envs_per_member, "envs_per_member", 64, None, "a positive multiple of 64",
                     ok=lambda e: e % 64 == 0)
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 \
            or table.shape[1] != P or table.shape[0] < 1:
        raise ValueError("table must be a [M,%d] float32 torch tensor (one gym_copter_amd.mlp vector of hidden %d per "
                         "member), got %s" % (P, hidden, getattr(table, "shape", type(table).__name__)))
    M = int(table.shape[0])
    if M * E != n:
        raise ValueError("members x envs_per_member = %d x %d is not num_envs = %d" % (M, E, n))
    g = _wire.finite(gamma, "gamma")
    if start_x is not None:
        if state is not None:
            raise ValueError("give start_x (with start_status) or state, not both")
        state = {"x": start_x,
                 "status": np.full(n, _lib.STATUS_AIRBORNE, np.uint8) if start_status is None else start_status}
    elif start_status is not None:
        raise ValueError("start_status describes an explicit start: start_x is required")
    tb = table.detach().to(dev).contiguous()
    io, K, keep = _rollout._rollout_io(self, None, state, K)
    out = _wire.rollout_cache(self, ("population", M), lambda: Population(
        _wire.empty(self, n, torch.float64), _wire.empty(self, n, torch.int32), _wire.empty(self, n, torch.uint8),
        _wire.empty(self, n, torch.uint8), _wire.empty(self, M, torch.float64)))
    pio = _wire.block(_lib.RolloutPopulationIO, hidden=hidden, members=M, envs_per_member=E, gamma=g,
                      params_table_dev=tb.data_ptr())
    pio.returns_dev, pio.lengths_dev, pio.end_flags_dev, pio.end_status_dev, pio.member_returns_dev = (
        t.data_ptr() for t in out)
    _wire.launch(self, "cs_rollout_mlp_population", io, pio, keep=keep + [tb])
    return out


def _es_io(members, num_params, nonce, pair_base):
    return _wire.block(
        _lib.EsIO,
        members=_wire.int_in(members, "members", 2, _lib.ES_MAX_MEMBERS + 1, "an even int in [2, %d]" % _lib.ES_MAX_MEMBERS,
                             ok=lambda m: m % 2 == 0),
        num_params=_wire.int_in(num_params, "num_params", 1, _lib.ES_MAX_PARAMS + 1,
                                "an int in [1, %d]" % _lib.ES_MAX_PARAMS),
        noise_stream=_wire.int_in(nonce, "nonce", 0, _wire.U32, _wire.IN_U32),
        pair_base=_wire.int_in(pair_base, "pair_base", 0, _wire.U32, _wire.IN_U32))


def es_perturb(self, params, sigma, members, nonce, pair_base=0):
    """The mirrored population of an evolution strategy around the centre `params` ([P] float32), one kernel:

        table[2i] = float32(params + float32(sigma eps_i)),   table[2i+1] = float32(params - float32(sigma eps_i))

    for the pairs i = 0 .. members/2 - 1, eps_i [P] the library's counter-based noise -- Irwin-Hall of order 4, mean
    0, variance 1 - 2**-32, a pure function of (seed, `nonce`, the global pair index pair_base + i, the parameter
    index): tests/es_ref.py restates it in NumPy bit for bit.  sigma >= 0; members even; nonce and pair_base in
    [0, 2**32) (pair_base: where this call's pairs sit in a population split over several calls or devices).
    Returns table [members,P] float32, a buffer of this env overwritten by its next call with the same shape.
    Asynchronous on the current stream."""
    self._check_open()
    torch = _torch()
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.dim() != 1:
        raise ValueError("params must be a 1-D float32 torch tensor, got %s"
                         % (getattr(params, "dtype", type(params).__name__),))
    sg = _wire.finite(sigma, "sigma", 0)
    eio = _es_io(members, int(params.shape[0]), nonce, pair_base)
    th = params.detach().to(self.device).contiguous()
    table = _wire.rollout_cache(self, ("es_table", eio.members, eio.num_params),
                                lambda: _wire.empty(self, (eio.members, eio.num_params), torch.float32))
    eio.sigma, eio.params_dev, eio.table_dev = sg, th.data_ptr(), table.data_ptr()
    _wire.launch(self, "cs_es_perturb", eio, keep=[th])
    return table


def es_gradient(self, weights, nonce, num_params, pair_base=0):
    """The search gradient of an evolution strategy, g[p] = sum_i (weights[2i] - weights[2i+1]) eps_i[p] in float64,
    two kernels: `weights` [M] float64 (a device tensor: the shaped fitness of es_perturb's members, for example
    their centred ranks) and the noise of es_perturb(.., nonce, pair_base) drawn again -- no table is read.  The sum
    runs in a fixed order (the same bits on every call) and the result is written, not accumulated; the scale
    1 / (M sigma) is the caller's.  Returns g [num_params] float64, a buffer of this env overwritten by its next call
    with the same num_params.  Asynchronous on the current stream."""
    self._check_open()
    torch = _torch()
    if not isinstance(weights, torch.Tensor) or weights.dim() != 1:
        raise ValueError("weights must be a [M] float64 device tensor")
    M = int(weights.shape[0])
    eio = _es_io(M, num_params, nonce, pair_base)
    _wire.check_tape(self, "the shaped fitness", (weights, "weights", (M,), torch.float64))
    g = _wire.rollout_cache(self, ("es_grad", eio.num_params), lambda: _wire.empty(self, eio.num_params, torch.float64))
    eio.weights_dev, eio.grad_dev = weights.data_ptr(), g.data_ptr()
    _wire.launch(self, "cs_es_gradient", eio, keep=[weights])
    return g


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
