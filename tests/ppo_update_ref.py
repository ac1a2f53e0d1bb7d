"""The reference of cs_ppo_grad, independent of the kernel's hand-derived backward:

  1. evaluate(): the minibatch loss of gym_copter_amd/ppo.py's loop body (the same torch expressions, gym_copter_amd.mlp's
     forward) in a chosen dtype, differentiated by torch AUTOGRAD.  In float64 it is the reference; in float32 it is the
     arithmetic the kernel replaces, whose distance from the float64 result the kernel has to beat.
  2. reference(): that in float64 together with the eight statistics, the per-parameter term magnitudes T (in the manner
     of _term_magnitudes of tests/test_gpu_mlp_param_grad.py, from the per-row |g_mu|, |g_V| and |dL/dlogp (z^2 - 1)|), the
     derived error budget of the gradient bar and the conditions a test asserts on the reference alone.
  3. synthetic(): tapes that need no rollout.

Everything here runs on the CPU (or on whatever device the tensors are on)."""
import math

import numpy as np

import ppo_ref

TASK_SHAPE = {"lander3d": (10, 4), "hover3d": (12, 4), "lander2d": (6, 2), "hover1d": (2, 1), "lander1d": (2, 1),
              "hover2d": (6, 2)}
U64 = 2.0 ** -53
LN_2PI = math.log(2.0 * math.pi)
STATS = ("live_samples", "policy_loss", "value_loss", "entropy", "loss", "approx_kl", "clip_fraction",
         "max_ratio_error")


# task, H, Hv (None: no critic), R, B, seed, options: the cases of tests/test_gpu_ppo_grad.py's first test -- a ragged last
# tile (1 000 = 15 x 64 + 40), every width class with idle lanes in both networks (33 / 3), less than one tile (37), every
# task shape, more tiles than workgroups (70 000 samples: 1 094 tiles on 1 024 workgroups at most), no critic with the
# minibatch given as a row range and every row live, and the advantages taken as they are.  The seeds are the first for
# which the conditions of check_conditions() hold, found on the CPU.
CASES = [("lander3d", 16, 16, 4096, 1000, 1, {}), ("lander3d", 0, 0, 4096, 1000, 1, {}),
         ("lander3d", 64, 64, 4096, 1000, 1, {}), ("lander3d", 33, 3, 4096, 37, 1, {}),
         ("hover3d", 16, 64, 4096, 1000, 1, {}), ("lander2d", 33, 16, 4096, 1000, 1, {}),
         ("hover1d", 3, 0, 4096, 1000, 1, {}), ("lander3d", 16, 16, 80000, 70000, 1, {}),
         ("lander3d", 1, None, 200, 200, 1, {"range": True}), ("lander3d", 16, 16, 4096, 1000, 1, {"normalize": False})]


# The constant c of the gradient bar c (2 B + 64) 2^-53 T (tests/test_gpu_ppo_grad.py derives it): the least power of two
# that covers reference()'s budget, c_needed, over the cases above -- 54.3 at the smallest minibatch (B = 37, where 2 B +
# 64 = 138 is least against the per-term errors, which do not shrink with B), 3.0 to 9.4 at B >= 200.
BAR_C = 64.0


def width_class(H):
    """The kernel's HP of a hidden width (head_launch in copterstep_ppo_grad.hip): 0 = linear, else H rounded up to
    8, 16, 32 or 64 lanes per row."""
    return 0 if H == 0 else 8 if H <= 8 else 16 if H <= 16 else 32 if H <= 32 else 64


# The instantiation matrix of tests/test_gpu_ppo_grad_matrix.py: task, H, Hv, R, B, seed.  cs_ppo_grad is one template
# <OBS, A, HP, head> with 4 shapes x 5 width classes x {policy, value} = 40 instantiations; five width pairs per shape
# reach every (shape, class, head), and over the matrix each class runs at its full width (no idle lanes) and at a
# ragged one, for both heads (tests/test_ppo_grad_cpu.py asserts both from this list).  lander1d and hover2d share
# hover1d's and lander2d's kernels and run once each, by name.  R = 512, B = 300: four full tiles and a ragged one of 44.
# The seeds are the first for which check_conditions() holds and the bar's constant covers the budget (clip 0.2, vf_coef
# 0.5, ent_coef 0.01), found on the CPU.
MATRIX_R, MATRIX_B = 512, 300
_LANDER_PAIRS = [(0, 24), (5, 64), (16, 0), (32, 8), (40, 12)]
_HOVER_PAIRS = [(0, 32), (8, 33), (9, 0), (17, 5), (64, 16)]
_MATRIX_SEEDS = {("lander2d", 0, 24): 2}
MATRIX = [(task, H, Hv, MATRIX_R, MATRIX_B, _MATRIX_SEEDS.get((task, H, Hv), 1))
          for task, pairs in (("lander3d", _LANDER_PAIRS), ("lander2d", _LANDER_PAIRS), ("hover3d", _HOVER_PAIRS),
                              ("hover1d", _HOVER_PAIRS), ("lander1d", [(17, 5)]), ("hover2d", [(17, 5)]))
          for H, Hv in pairs]

# Two minibatches of 200 000 samples: 3 125 tiles, 4 per workgroup on 782 workgroups, so that all four wavefronts of a
# workgroup take a tile and the last workgroup holds one tile only.  task, H, Hv, R, B, seed (found as above).
LARGE = [("hover1d", 12, 33, 210000, 200000, 1), ("lander3d", 40, 12, 210000, 200000, 1)]


# Degenerate minibatches (tests/test_gpu_ppo_grad_matrix.py), R = 512: task, H, Hv, seed.
#   ONE_LIVE: 65 samples of which one is live (one_live()).  With normalize the normalised advantage is exactly 0; without,
#     the case is compared with the reference, and the seed is the first whose reference has c_needed, c_stats <= BAR_C
#     (one live row cannot meet check_conditions(): its clipped share is 0 or 1).
#   EQUAL_ADV: 256 samples, every advantage 0.5 (equal_advantages()).  With normalize m = 0.5 and Ahat = 0 exactly; without,
#     an ordinary case: the first seed that meets check_conditions() and the bar's constant.
#   RANGE_LIVE: rows 100 .. 399 as a row range WITH the live mask: the first seed as for EQUAL_ADV.
DEGENERATE_R = 512
ONE_LIVE = [("lander3d", 16, 16, 1), ("hover1d", 5, 0, 1)]
EQUAL_ADV = [("lander3d", 16, 16, 1), ("hover1d", 5, 0, 1), ("hover3d", 0, 33, 1)]
RANGE_LIVE = ("lander3d", 16, 16, 1)
RANGE_BASE, RANGE_B = 100, 300


def one_live(task, H, Hv, seed, B=65, at=37):
    """synthetic() with every row dead but the one sample `at` of the minibatch perm[:B].  Returns (tapes, index)."""
    import torch
    s = synthetic(task, H, Hv, DEGENERATE_R, seed)
    idx = s["perm"][:B].contiguous()
    s["live"] = torch.zeros_like(s["live"])
    s["live"][idx[at]] = True
    return s, idx


def equal_advantages(task, H, Hv, seed, B=256):
    """synthetic() with every advantage 0.5 (sums of 0.5 are exact in any order).  Returns (tapes, index = perm[:B])."""
    import torch
    s = synthetic(task, H, Hv, DEGENERATE_R, seed)
    s["advantages"] = torch.full_like(s["advantages"], 0.5)
    return s, s["perm"][:B].contiguous()


def check_conditions(ref, need_dead=True):
    """What a test asserts of the reference alone before it looks at the device: at least 1 % of the live samples
    clipped and at least 50 % not, no ratio within 1e-8 of 1 +- clip (no sample can change branch between two float64
    evaluations), at least one dead row."""
    assert 0.01 <= ref["clip_fraction"] <= 0.5, ref["clip_fraction"]
    assert ref["edge"] >= 1e-8, ref["edge"]
    assert not need_dead or ref["dead"] >= 1


def synthetic(task, H, Hv, R, seed):
    """Tapes of R rows and the parameters of a PPO minibatch step, CPU tensors: obs ~ N(0, 1); actions drawn from an
    "old" Gaussian policy (mlp.init with the hover motor value as output bias and an output layer scaled by 0.3,
    sigma = 0.05) with their float32 log-probabilities (ppo_ref.logp); the CURRENT actor = old + 0.02 mean|theta_old|
    N(0, 1) per parameter, log_std = old + 0.05 N(0, 1); a critic from mlp.init; adv ~ 0.3 + N(0, 1), ret ~ N(0, 1),
    live ~ Bernoulli(0.9); perm a permutation of the rows (a minibatch is a prefix of it).  Hv None: no critic."""
    import torch
    from gym_copter_amd import mlp
    from jacobian_fd import hover_action
    od, A = TASK_SHAPE[task]
    gen = torch.Generator().manual_seed(seed)
    obs = torch.randn((R, od), generator=gen, dtype=torch.float64).to(torch.float32)
    old = mlp.init(od, A, H, generator=gen, out_bias=float(hover_action()), out_scale=0.3)
    ls_old = torch.full((A,), math.log(0.05), dtype=torch.float32)
    mu_old = mlp.forward64(old, obs, H, A)
    eps = torch.randn((R, A), generator=gen, dtype=torch.float64)
    actions = (mu_old + torch.exp(ls_old.double()) * eps).to(torch.float32)
    logp = torch.from_numpy(ppo_ref.logp(actions.numpy(), mu_old.to(torch.float32).numpy(), ls_old.numpy())
                            .astype(np.float32))
    shift = 0.02 * float(old.double().abs().mean())
    actor = (old.double() + shift * torch.randn(old.shape, generator=gen, dtype=torch.float64)).to(torch.float32)
    log_std = (ls_old.double() + 0.05 * torch.randn((A,), generator=gen, dtype=torch.float64)).to(torch.float32)
    critic = mlp.init(od, 1, Hv, generator=gen) if Hv is not None else None
    adv = (0.3 + torch.randn(R, generator=gen, dtype=torch.float64)).to(torch.float32)
    ret = torch.randn(R, generator=gen, dtype=torch.float64).to(torch.float32)
    live = torch.rand(R, generator=gen, dtype=torch.float64) < 0.9
    perm = torch.randperm(R, generator=gen)
    return dict(task=task, hidden=H, critic_hidden=Hv, actor=actor, critic=critic, log_std=log_std, obs=obs,
                actions=actions, logp=logp, advantages=adv, returns=ret, live=live, perm=perm)


def _forward(torch, params, obs, hidden, act_dim):
    from gym_copter_amd import mlp
    p = mlp.unpack(params, obs.shape[-1], act_dim, hidden)
    if hidden == 0:
        return obs @ p["W"].T + p["b"]
    return torch.tanh(obs @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]


def evaluate(s, index, clip=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True, dtype=None, live=True):
    """The loss of ppo.py's minibatch step on the rows `index` (int64 tensor, every entry in range) of the tapes `s`, in
    `dtype` (default float64), with autograd.  Returns a dict: loss, grad (actor | critic | log_std, in `dtype`), and the
    intermediate tensors a caller may want (ratio, logp, w, ahat, z, mu, value, clipped)."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    A = s["actions"].shape[-1]
    H, Hv = s["hidden"], s["critic_hidden"]
    actor = s["actor"].to(dtype).clone().requires_grad_(True)
    log_std = s["log_std"].to(dtype).clone().requires_grad_(True)
    critic = s["critic"].to(dtype).clone().requires_grad_(True) if s["critic"] is not None else None
    one = torch.ones((), dtype=dtype, device=actor.device)
    w = s["live"][index].to(dtype) if (live and s["live"] is not None) else torch.ones(index.shape[0], dtype=dtype,
                                                                                       device=actor.device)
    wsum = torch.maximum(w.sum(), one)
    a_mb = s["advantages"][index].to(dtype)
    if normalize:
        a_mean = (a_mb * w).sum() / wsum
        a_std = (((a_mb - a_mean) ** 2 * w).sum() / wsum).sqrt()
        a_mb = (a_mb - a_mean) / (a_std + 1e-8)
    o_mb = s["obs"][index].to(dtype)
    mu = _forward(torch, actor, o_mb, H, A)
    z = (s["actions"][index].to(dtype) - mu) * torch.exp(-log_std)
    logp = -0.5 * (z * z).sum(-1) - log_std.sum() - 0.5 * A * LN_2PI
    logp_old = s["logp"][index].to(dtype)
    ratio = torch.exp(logp - logp_old)
    surr = torch.minimum(ratio * a_mb, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_mb)
    pol_loss = -(surr * w).sum() / wsum
    if critic is not None:
        value = _forward(torch, critic, o_mb, Hv, 1)[:, 0]
        val_loss = 0.5 * (((value - s["returns"][index].to(dtype)) ** 2) * w).sum() / wsum
    else:
        value, val_loss = None, torch.zeros((), dtype=dtype, device=actor.device)
    entropy = log_std.sum() + 0.5 * A * (1.0 + LN_2PI)
    loss = pol_loss + vf_coef * val_loss - ent_coef * entropy
    leaves = [actor, log_std] + ([critic] if critic is not None else [])
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    gz = [g if g is not None else torch.zeros_like(p) for g, p in zip(grads, leaves)]
    grad = torch.cat([gz[0]] + ([gz[2]] if critic is not None else []) + [gz[1]])
    r = ratio.detach()
    clipped = ((a_mb > 0) & (r > 1.0 + clip)) | ((a_mb < 0) & (r < 1.0 - clip))
    return dict(loss=loss.detach(), grad=grad, pol_loss=pol_loss.detach(), val_loss=val_loss.detach(),
                entropy=entropy.detach(), ratio=r, logp=logp.detach(), logp_old=logp_old, w=w, wsum=wsum, ahat=a_mb,
                z=z.detach(), mu=mu.detach(), value=None if value is None else value.detach(), clipped=clipped, obs=o_mb)


def _layer_magnitudes(torch, params, hidden, o, g):
    """sum over the rows of the bound of |term| per parameter of one network, for the per-row cotangent magnitudes g
    [B, outs] (test_gpu_mlp_param_grad._term_magnitudes on rows)."""
    from gym_copter_amd import mlp
    outs = g.shape[1]
    ao = o.abs()
    if hidden == 0:
        return torch.cat([(g.T @ ao).reshape(-1), g.sum(0)])
    p = mlp.unpack(params.double(), o.shape[1], outs, hidden)
    h = torch.tanh(o @ p["W1"].T + p["b1"]).abs()
    gh = g @ p["W2"].abs()
    return torch.cat([(gh.T @ ao).reshape(-1), gh.sum(0), (g.T @ h).reshape(-1), g.sum(0)])


def _output_budget(torch, params, hidden, o, outs):
    """[B, outs], in units of u = 2^-53: a bound of the difference of two float64 evaluations of the network's outputs
    in different summation orders (each within (terms + 1) u of the exact sum of its terms' magnitudes), including what
    the hidden units' own arguments ((OBS + 1) terms, tanh' <= 1) and two tanh implementations (2 u |h| each) add."""
    from gym_copter_amd import mlp
    od = o.shape[1]
    p = mlp.unpack(params.double(), od, outs, hidden)
    if hidden == 0:
        return 2.0 * (od + 2) * (o.abs() @ p["W"].abs().T + p["b"].abs())
    pre = o.abs() @ p["W1"].abs().T + p["b1"].abs()
    h = torch.tanh(o @ p["W1"].T + p["b1"]).abs()
    dh = 2.0 * ((od + 2) * pre + 2.0 * h)
    return dh @ p["W2"].abs().T + 2.0 * (hidden + 2) * (h @ p["W2"].abs().T + p["b2"].abs())


def reference(s, index, clip=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True, live=True):
    """The float64 reference on the minibatch `index`.  Returns a dict:
      grad [P + Pv + A], stats [8] (cs_ppo_grad's);
      T [P + Pv + A], the term magnitudes: per parameter the sum over the rows of |term|, from the per-row |g_mu|, |g_V|
        and |dL/dlogp (z^2 - 1)| (+ |ent_coef| for log_std);
      S [8], the same for the statistics that are sums (sum |term| / W);
      c_needed: the least c for which c (2 B + 64) u T covers, for every parameter, the derived error budget of TWO float64
        evaluations (tests/test_gpu_ppo_grad.py states the derivation); c_stats the same for the summed statistics;
      ratio_err: the bound of |max|rho - 1|| between two evaluations, in units of u;
      the conditions a test asserts on the reference alone: clip_fraction, edge (the least distance of a live sample's
        ratio from 1 +- clip), dead (rows with w = 0), ratio_range, max_dlogp."""
    import torch
    r = evaluate(s, index, clip, vf_coef, ent_coef, normalize, torch.float64, live)
    A = s["actions"].shape[-1]
    H, Hv = s["hidden"], s["critic_hidden"]
    B = int(index.shape[0])
    w, W, ahat, ratio, z, o = r["w"], r["wsum"], r["ahat"], r["ratio"], r["z"], r["obs"]
    on = w > 0
    ls = s["log_std"].double()
    els = torch.exp(-ls)
    zero = torch.zeros_like(ratio)
    active = on & ~r["clipped"]
    dl = torch.where(active, -(ahat * ratio) / W, zero)
    g_mu = (dl[:, None] * z * els).abs()
    g_ls = (dl[:, None] * (z * z - 1.0)).abs()
    T = [_layer_magnitudes(torch, s["actor"], H, o, g_mu)]
    # ---- the error budget per row, in units of u ----
    d_mu = _output_budget(torch, s["actor"], H, o, A)                       # [B, A] absolute
    d_z = els * d_mu + 6.0 * z.abs()                                        # (a - mu, exp(-ls), the product: two sides)
    logp_terms = 0.5 * (z * z).sum(-1) + ls.abs().sum() + 0.5 * A * LN_2PI + r["logp_old"].abs()
    d_logp = (z.abs() * d_z).sum(-1) + 2.0 * (A + 4) * logp_terms           # absolute, of exp's argument
    rel_rho = d_logp + 2.0                                                  # (+ one ulp of exp on either side)
    adv = s["advantages"][index].double()
    if normalize:
        den = ((((adv - (adv * w).sum() / W) ** 2) * w).sum() / W).sqrt() + 1e-8
        a1 = (adv.abs() * w).sum() / W
        d_ahat = 3.0 * (B + 8) * (a1 / den + ahat.abs())                     # m's and sd's own summations, two sides
    else:
        d_ahat = zero
    d_dl = torch.where(active, ratio / W * (d_ahat + ahat.abs() * (rel_rho + 4.0)), zero)
    e_mu = els * (d_dl[:, None] * z.abs() + dl.abs()[:, None] * (d_z + 2.0 * z.abs()))
    e_ls = d_dl[:, None] * (z * z - 1.0).abs() + dl.abs()[:, None] * (2.0 * z.abs() * d_z + 2.0 * z * z + 1.0)
    budget = [_layer_magnitudes(torch, s["actor"], H, o, e_mu)]
    v_terms = zero
    if s["critic"] is not None:
        dv = r["value"] - s["returns"][index].double()
        g_v = (vf_coef * w * dv / W).abs()
        T.append(_layer_magnitudes(torch, s["critic"], Hv, o, g_v[:, None]))
        d_v = _output_budget(torch, s["critic"], Hv, o, 1)[:, 0]
        e_v = abs(vf_coef) * w / W * (d_v + 6.0 * dv.abs())
        budget.append(_layer_magnitudes(torch, s["critic"], Hv, o, e_v[:, None]))
        v_terms = 0.5 * w * dv * dv
        e_vt = w * dv.abs() * (d_v + 4.0 * dv.abs())
    T.append(g_ls.sum(0) + abs(ent_coef))
    budget.append(e_ls.sum(0) + 2.0 * abs(ent_coef))
    T = torch.cat(T)
    # two summations of B terms in any orders, and the backward's own roundings per term (section 12's 2 R + 64)
    budget = torch.cat(budget) + (2 * B + 64) * T
    c_needed = float((budget / ((2 * B + 64) * T).clamp_min(1e-300))[T > 0].max()) if bool((T > 0).any()) else 1.0
    used = torch.where(r["clipped"], torch.clamp(ratio, 1.0 - clip, 1.0 + clip), ratio)
    dlogp = r["logp_old"] - r["logp"]
    nil = torch.zeros((), dtype=torch.float64, device=w.device)
    stats = torch.stack([w.sum(), r["pol_loss"], r["val_loss"], r["entropy"], r["loss"], (w * dlogp).sum() / W,
                         (w * r["clipped"].double()).sum() / W, torch.where(on, (ratio - 1.0).abs(), zero).max()])
    S = torch.stack([nil, (w * (ahat * used).abs()).sum() / W, v_terms.sum() / W,
                     ls.abs().sum() + 0.5 * A * (1.0 + LN_2PI), nil, (w * logp_terms).sum() / W, nil, nil])
    S[4] = S[1] + abs(vf_coef) * S[2] + abs(ent_coef) * S[3]
    e_s = torch.stack([nil, (w * used * (d_ahat + ahat.abs() * torch.where(r["clipped"], zero, rel_rho))).sum() / W,
                       (e_vt.sum() / W if s["critic"] is not None else nil), 2.0 * (A + 2) * S[3], nil,
                       (w * d_logp).sum() / W, nil, nil])
    e_s[4] = e_s[1] + abs(vf_coef) * e_s[2] + abs(ent_coef) * e_s[3] + 6.0 * S[4]
    e_s = e_s + (2 * B + 64) * S
    c_stats = float((e_s / ((2 * B + 64) * S).clamp_min(1e-300))[S > 0].max())
    rows = on if bool(on.any()) else torch.ones_like(on)
    return dict(grad=r["grad"], stats=stats, T=T, S=S, c_needed=c_needed, c_stats=c_stats,
                ratio_err=float(torch.where(on, ratio * rel_rho + 2.0, zero).max()),
                max_dlogp=float(dlogp[rows].abs().max()), count=float(w.sum()),
                edge=float(torch.minimum((ratio - (1.0 + clip)).abs(), (ratio - (1.0 - clip)).abs())[rows].min()),
                clip_fraction=float(stats[6]), ratio_range=(float(ratio[rows].min()), float(ratio[rows].max())),
                dead=int((~on).sum()), parts=r)


def float32_distance(s, index, ref_grad, **kw):
    """The scaled distance max |g32 - g64| / max(1, |g64|) of the float32 autograd gradient (ppo.py's present arithmetic
    on the same minibatch) from the float64 reference."""
    import torch
    g32 = evaluate(s, index, dtype=torch.float32, **kw)["grad"].double()
    return scaled(g32, ref_grad)


def scaled(got, want):
    import torch
    return float(((got - want).abs() / torch.clamp(want.abs(), min=1.0)).max())


def bound_ratio(dev, ref, T, B, c):
    """max over the parameters of |device - reference| / (c (2 B + 64) 2^-53 T)."""
    import torch
    bound = c * (2 * B + 64) * U64 * T
    diff = (dev - ref).abs()
    assert bool(torch.isfinite(dev).all())
    assert bool(((bound > 0) | (diff == 0)).all())
    return float((diff / bound.clamp_min(1e-300)).max())


def to_device(s, device):
    import torch
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in s.items()}
