"""The MLP policy of the closed-loop rollouts (CopterVecEnv.rollout_mlp_states / rollout_mlp_vjp,
gym_copter_amd.differentiable_mlp_rollout; include/copterstep.h cs_rollout_mlp_io): one flat
float32 parameter vector theta shared by every env,

    hidden = 0:         a = W o + b                          theta = [W (A x OBS, row-major), b (A)]
    1 <= hidden <= 64:  h = tanh(W1 o + b1), a = W2 h + b2   theta = [W1 (H x OBS), b1 (H), W2 (A x H), b2 (A)]

and the host side of its gradient: g_theta = sum_{k,n} J_theta pi(o_{k-1,n})^T g_a_{k,n}, a reduction over every env
and step that torch runs as matrix products (param_grad).  Works on CPU and device tensors alike."""
import math

MAX_HIDDEN = 64   # CS_MLP_MAX_HIDDEN


def _torch():
    import torch
    return torch


def _check_hidden(hidden):
    if not isinstance(hidden, int) or isinstance(hidden, bool) or not 0 <= hidden <= MAX_HIDDEN:
        raise ValueError("hidden must be an int in [0, %d], got %r" % (MAX_HIDDEN, hidden))


def num_params(obs_dim, act_dim, hidden):
    """P, the length of theta."""
    _check_hidden(hidden)
    if hidden == 0:
        return act_dim * (obs_dim + 1)
    return hidden * (obs_dim + 1) + act_dim * (hidden + 1)


def _shapes(obs_dim, act_dim, hidden):
    if hidden == 0:
        return (("W", (act_dim, obs_dim)), ("b", (act_dim,)))
    return (("W1", (hidden, obs_dim)), ("b1", (hidden,)), ("W2", (act_dim, hidden)), ("b2", (act_dim,)))


def unpack(params, obs_dim, act_dim, hidden):
    """theta -> {"W", "b"} (hidden = 0) or {"W1", "b1", "W2", "b2"}: views of `params` in its dtype."""
    P = num_params(obs_dim, act_dim, hidden)
    if params.dim() != 1 or params.shape[0] != P:
        raise ValueError("params must have shape (%d,) for obs_dim %d, act_dim %d, hidden %d, got %s"
                         % (P, obs_dim, act_dim, hidden, tuple(params.shape)))
    out, at = {}, 0
    for name, shape in _shapes(obs_dim, act_dim, hidden):
        size = math.prod(shape)
        out[name] = params[at:at + size].view(shape)
        at += size
    return out


def pack(parts, hidden, dtype=None, device=None):
    """The inverse of unpack: {"W", "b"} or {"W1", "b1", "W2", "b2"} (tensors or arrays) -> theta [P] (float32 unless
    `dtype` says otherwise)."""
    torch = _torch()
    _check_hidden(hidden)
    dtype = torch.float32 if dtype is None else dtype
    names = ("W", "b") if hidden == 0 else ("W1", "b1", "W2", "b2")
    if set(parts) != set(names):
        raise ValueError("hidden = %d packs the parts %s, got %s" % (hidden, names, sorted(parts)))
    ts = [torch.as_tensor(parts[k]) for k in names]
    W = ts[0] if hidden == 0 else ts[2]
    act_dim, obs_dim = (W.shape[0], W.shape[1]) if hidden == 0 else (ts[2].shape[0], ts[0].shape[1])
    for (name, shape), t in zip(_shapes(obs_dim, act_dim, hidden), ts):
        if tuple(t.shape) != shape:
            raise ValueError("%s must have shape %s, got %s" % (name, shape, tuple(t.shape)))
    dev = device if device is not None else ts[0].device
    return torch.cat([t.reshape(-1).to(device=dev, dtype=dtype) for t in ts])


def pack_module(module, dtype=None, device=None):
    """theta of a torch module laid out as the policy: nn.Linear(OBS, A) (hidden = 0) or nn.Sequential(nn.Linear(OBS,
    H), nn.Tanh(), nn.Linear(H, A)).  Returns (theta, hidden)."""
    torch = _torch()
    lin = [m for m in module.modules() if isinstance(m, torch.nn.Linear)]
    if len(lin) == 1:
        return pack({"W": lin[0].weight.detach(), "b": lin[0].bias.detach()}, 0, dtype, device), 0
    if len(lin) == 2 and any(isinstance(m, torch.nn.Tanh) for m in module.modules()):
        H = lin[0].out_features
        return pack({"W1": lin[0].weight.detach(), "b1": lin[0].bias.detach(), "W2": lin[1].weight.detach(),
                     "b2": lin[1].bias.detach()}, H, dtype, device), H
    raise ValueError("pack_module takes nn.Linear or nn.Sequential(nn.Linear, nn.Tanh, nn.Linear)")


def init(obs_dim, act_dim, hidden, generator=None, device=None, out_bias=None, out_scale=1.0):
    """A fresh theta [P] float32 with nn.Linear's default initialisation (uniform in +-1/sqrt(fan_in)); `out_scale`
    scales the output layer's weights and `out_bias` (a float or [A]) replaces its bias -- e.g. the hover motor value,
    so that the untrained policy starts near hover."""
    torch = _torch()
    _check_hidden(hidden)
    g = generator

    def u(shape, fan_in):
        bound = 1.0 / math.sqrt(fan_in)
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * bound
    if hidden == 0:
        parts = {"W": u((act_dim, obs_dim), obs_dim) * out_scale, "b": u((act_dim,), obs_dim)}
        ob = "b"
    else:
        parts = {"W1": u((hidden, obs_dim), obs_dim), "b1": u((hidden,), obs_dim),
                 "W2": u((act_dim, hidden), hidden) * out_scale, "b2": u((act_dim,), hidden)}
        ob = "b2"
    if out_bias is not None:
        parts[ob] = torch.as_tensor(out_bias, dtype=torch.float64).expand(act_dim).clone()
    return pack(parts, hidden, device=device)


def forward64(params, obs, hidden, act_dim):
    """pi_theta(obs) in float64 (obs [..., OBS]): the exact function the kernel's float32 arithmetic rounds."""
    torch = _torch()
    o = obs.to(torch.float64)
    p = unpack(params.to(torch.float64), o.shape[-1], act_dim, hidden)
    if hidden == 0:
        return o @ p["W"].T + p["b"]
    return torch.tanh(o @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]


def _outer_sum(a, b, rows=4096):
    """sum_r a[r] (x) b[r] for a [R, p], b [R, q] -> [p, q], as a batch of [p, rows] x [rows, q] products summed after:
    one GEMM with R as its inner dimension has a p x q output -- one tile, one workgroup reducing all R rows serially."""
    torch = _torch()
    R = a.shape[0]
    pad = (-R) % rows
    if pad:
        a = torch.cat([a, a.new_zeros((pad, a.shape[1]))])
        b = torch.cat([b, b.new_zeros((pad, b.shape[1]))])
    B = a.shape[0] // rows
    return torch.bmm(a.view(B, rows, -1).transpose(1, 2), b.view(B, rows, -1)).sum(0)


def param_grad(params, hidden, obs, g_actions, chunk=None):
    """g_theta = sum_{k,n} J_theta pi(obs[k,n])^T g_actions[k,n] in float64: obs [K,N,OBS] (the forward's obs tape),
    g_actions [K,N,A] (rollout_mlp_vjp's).  The hidden units are recomputed in float64 from the obs tape, as the
    backward kernel recomputes them, in chunks of `chunk` steps (default: about 2^22 env-steps' worth) so that the
    temporaries stay bounded.  Returns [P] float64 on params' device."""
    torch = _torch()
    if obs.dim() != 3 or g_actions.dim() != 3 or obs.shape[:2] != g_actions.shape[:2]:
        raise ValueError("obs [K,N,OBS] and g_actions [K,N,A] must agree in K and N, got %s and %s"
                         % (tuple(obs.shape), tuple(g_actions.shape)))
    K, N, OBS = obs.shape
    A = g_actions.shape[2]
    dev = params.device
    p = unpack(params.detach().to(torch.float64), OBS, A, hidden)
    if chunk is None:
        chunk = max(1, (1 << 22) // max(N, 1))
    if hidden == 0:
        gW = torch.zeros((A, OBS), dtype=torch.float64, device=dev)
        gb = torch.zeros(A, dtype=torch.float64, device=dev)
    else:
        gW1 = torch.zeros((hidden, OBS), dtype=torch.float64, device=dev)
        gb1 = torch.zeros(hidden, dtype=torch.float64, device=dev)
        gW2 = torch.zeros((A, hidden), dtype=torch.float64, device=dev)
        gb2 = torch.zeros(A, dtype=torch.float64, device=dev)
    for k0 in range(0, K, chunk):
        o = obs[k0:k0 + chunk].to(device=dev, dtype=torch.float64).reshape(-1, OBS)
        ga = g_actions[k0:k0 + chunk].to(device=dev, dtype=torch.float64).reshape(-1, A)
        if hidden == 0:
            gW += _outer_sum(ga, o)
            gb += ga.sum(0)
            continue
        h = torch.tanh(o @ p["W1"].T + p["b1"])
        gW2 += _outer_sum(ga, h)
        gb2 += ga.sum(0)
        gp = (ga @ p["W2"]) * (1.0 - h * h)
        gW1 += _outer_sum(gp, o)
        gb1 += gp.sum(0)
    if hidden == 0:
        return torch.cat([gW.reshape(-1), gb])
    return torch.cat([gW1.reshape(-1), gb1, gW2.reshape(-1), gb2])
