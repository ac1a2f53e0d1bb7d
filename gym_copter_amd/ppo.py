"""A small PPO driver on CopterVecEnv.rollout_actor_critic / gae: the MLP policy of the
closed-loop rollouts with a state-independent Gaussian and an MLP value head, trained on-policy.

Every iteration is two library kernels -- the K-step collection with its log-probabilities and values, and the
advantages -- followed by the clipped-surrogate update in plain torch autograd on a float32 restatement of the two
networks (gym_copter_amd.mlp.unpack).  Nothing is read by the host inside the loop; the per-iteration statistics stay on
the device until the caller reads them."""
import collections
import ctypes as C
import math

import numpy as np

from . import _lib, _wire, mlp
from ._wire import _torch

PpoResult = collections.namedtuple("PpoResult", "actor critic log_std history stats")
# the columns of PpoResult.stats [iterations, 6] float32
STATS = ("mean_reward_per_live_step", "live_samples", "first_ratio_error", "policy_loss", "value_loss", "done_rate")
# CopterVecEnv.rollout_actor_critic's result
ActorCritic = collections.namedtuple("ActorCritic", "obs actions means logp values reward terminated truncated live")
# ppo_grad: grad [P + Pv + A] float64 (actor | critic | log_std), stats [8] float64 (PPO_STATS)
PpoGrad = collections.namedtuple("PpoGrad", "grad stats")
_ON_DEVICE = "%(name)s must be a [%(size)d] float32 tensor on %(device)s, got %(got)s"
PPO_STATS = ("live_samples", "policy_loss", "value_loss", "entropy", "loss", "approx_kl", "clip_fraction",
             "max_ratio_error")


# -- on-policy actor-critic collection and GAE, the fused PPO minibatch gradient (section 18):
#    CopterVecEnv's methods, bound in vecenv.py --------
def rollout_actor_critic(self, actor, critic, log_std, K, hidden, critic_hidden=None, nonce=0, deterministic=False,
                         means=False):
    """K closed-loop steps under a Gaussian MLP policy with a value head, one kernel, with everything a PPO / A2C
    learner needs of them.  The env ADVANCES (its own auto-reset mode), exactly as step_many would under the
    returned actions.  actor [P] float32 is a gym_copter_amd.mlp vector of `hidden`; critic [Pv] float32 one with
    act_dim = 1 and `critic_hidden` (None: `hidden`), or None for no values; log_std [A] float32.  Per step, on the
    observation o the previous step returned (step 1: the stored state's):

        mu = actor(o), V = critic(o), a = float32(mu + float32(exp(log_std) eps)), eps ~ N(0, 1)

    (deterministic=True: a = mu) and logp = log N(a; mu, exp(log_std)^2) computed in float64 from the stored a and
    mu.  eps is the library's counter-based Box-Muller draw, a pure function of (seed, `nonce`, global env id, step,
    component): tests/ppo_ref.py restates it.  Returns ActorCritic(obs [K+1,N,OBS] -- row 0 the stored state's
    observation, row K the bootstrap observation --, actions [K,N,A], means [K,N,A] or None (means=True), logp [K,N],
    values [K+1,N] or None, reward [K,N], terminated [K,N], truncated [K,N], live [K,N] bool: False for a next_step
    reset step, whose action the env ignores).  Asynchronous on the current stream; the tensors are buffers of this
    env, overwritten by its next call with the same K."""
    self._check_open()
    torch = _torch()
    n, A, od = self.num_envs, self.action_dim, self.obs_dim
    K = _wire.int_in(K, "K", 1, None, "an int >= 1")
    P = mlp.num_params(od, A, hidden)                                # (checks hidden)
    if critic_hidden is None:
        critic_hidden = hidden
    Pv = mlp.num_params(od, 1, critic_hidden)
    nonce = _wire.int_in(nonce, "nonce", 0, _wire.U32, _wire.IN_U32)
    keep = []
    wording = "%(name)s must be a [%(size)d] float32 torch tensor, got %(got)s"
    th = _wire.exact_vector(self, actor, P, "actor", keep, wording)
    tv = _wire.exact_vector(self, critic, Pv, "critic", keep, wording) if critic is not None else None
    ls = _wire.exact_vector(self, log_std, A, "log_std", keep, wording)

    def make():
        return {"obs": _wire.empty(self, (K + 1, n, od), torch.float32),
                "actions": _wire.empty(self, (K, n, A), torch.float32), "logp": _wire.empty(self, (K, n), torch.float32),
                "reward": _wire.empty(self, (K, n), torch.float32),
                "flags": _wire.empty(self, (K, n, 2), torch.uint8),        # interleaved flags
                "live": _wire.empty(self, (K, n), torch.uint8)}
    buf = _wire.rollout_cache(self, ("actor_critic", K), make)
    if means and "means" not in buf:
        buf["means"] = _wire.empty(self, (K, n, A), torch.float32)
    if tv is not None and "values" not in buf:
        buf["values"] = _wire.empty(self, (K + 1, n), torch.float32)
    aio = _wire.block(_lib.RolloutAcIO, num_steps=K, hidden=hidden, critic_hidden=critic_hidden, nonce=nonce,
                      deterministic=1 if deterministic else 0, actor_dev=th.data_ptr(), log_std_dev=ls.data_ptr(),
                      critic_dev=tv.data_ptr() if tv is not None else None,
                      means_dev=buf["means"].data_ptr() if means else None,
                      values_dev=buf["values"].data_ptr() if tv is not None else None,
                      **{k + "_dev": buf[k].data_ptr() for k in ("obs", "actions", "logp", "reward", "flags", "live")})
    _wire.launch(self, "cs_rollout_actor_critic", aio, keep=keep)
    flags = buf["flags"]
    return ActorCritic(buf["obs"], buf["actions"], buf["means"] if means else None, buf["logp"],
                       buf["values"] if tv is not None else None, buf["reward"], flags[:, :, 0].view(torch.bool),
                       flags[:, :, 1].view(torch.bool), buf["live"].view(torch.bool))


def gae(self, reward, values, terminated, truncated, gamma=0.99, lam=0.95):
    """Generalised advantage estimation over rollout_actor_critic's tapes, one kernel: reward [K,N] float32, values
    [K+1,N] float32, terminated and truncated [K,N] bool or uint8 (device tensors) -> (advantages, returns), both
    [K,N] float32:

        delta_k = r_k + gamma V_{k+1} nd_k - V_k,   adv_k = delta_k + gamma lam nd_k adv_{k+1},   ret_k = adv_k + V_k

    with nd_k = 0 where step k terminated OR truncated its episode (truncation cuts the bootstrap as termination
    does: the K-step forms return no final observation to bootstrap from) and 1 elsewhere.  float32 in a fixed order,
    no fused operation: tests/ppo_ref.py gives the same bits in NumPy.  Asynchronous on the current stream; the
    results are buffers of this env, overwritten by its next call with the same K."""
    self._check_open()
    torch = _torch()
    n, dev = self.num_envs, self.device
    if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
        raise ValueError("reward must be a [K,%d] float32 device tensor" % n)
    K = int(reward.shape[0])
    _wire.check_tape(self, "rollout_actor_critic", (reward, "reward", (K, n), torch.float32),
                     (values, "values", (K + 1, n), torch.float32))
    g, l = float(gamma), float(lam)
    with np.errstate(over="ignore"):
        narrowed = (np.float32(g), np.float32(l), np.float32(g) * np.float32(l))
    if not np.isfinite(g) or not np.isfinite(l) or not np.all(np.isfinite(narrowed)):
        raise ValueError("gamma and lam must be finite (in float32, and their product too), got %r and %r"
                         % (gamma, lam))
    flags = []
    for t, name in ((terminated, "terminated"), (truncated, "truncated")):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (K, n) or t.dtype not in (torch.bool, torch.uint8) \
                or t.device != dev:
            raise ValueError("%s must be a [%d,%d] bool or uint8 tensor on %s" % (name, K, n, dev))
        flags.append(t.view(torch.uint8) if t.dtype == torch.bool else t)
    # the two columns of one interleaved [K,N,2] array (what rollout_actor_critic returns) are read in place
    stride = 2 if all(t.stride() == (2 * n, 2) for t in flags) else 1
    if stride == 1:
        flags = [t.contiguous() for t in flags]
    out = _wire.rollout_cache(self, ("gae", K), lambda: (_wire.empty(self, (K, n), torch.float32),
                                                         _wire.empty(self, (K, n), torch.float32)))
    gio = _wire.block(_lib.GaeIO, num_steps=K, flag_stride=stride, gamma=g, lam=l, reward_dev=reward.data_ptr(),
                      values_dev=values.data_ptr(), terminated_dev=flags[0].data_ptr(),
                      truncated_dev=flags[1].data_ptr(), advantages_dev=out[0].data_ptr(), returns_dev=out[1].data_ptr())
    _wire.launch(self, "cs_gae", gio, keep=[reward, values] + flags)
    return out


def ppo_grad(self, actor, critic, log_std, hidden, critic_hidden, obs, actions, logp, advantages, returns, live=None,
             index=None, row_base=0, num_samples=None, clip=0.2, vf_coef=0.5, ent_coef=0.0, normalize=True, out=None,
             stats_out=None):
    """PPO's clipped-surrogate minibatch loss and its gradient, ON THE DEVICE (cs_ppo_grad): what
    the minibatch step of gym_copter_amd.ppo differentiates, evaluated in float64 from the float32 tapes,

        L = -mean_w min(r A, clip(r, 1 - clip, 1 + clip) A) + vf_coef mean_w (V - ret)^2 / 2 - ent_coef H

    over the minibatch's live samples (w = live), r = exp(logp_new - logp), A the advantages normalised over the
    minibatch's live samples (normalize=True), H the Gaussian's entropy.  actor [P], critic [Pv] (None: no value
    term) and log_std [A] are float32 device tensors in gym_copter_amd.mlp's layout for `hidden` / `critic_hidden`.
    The tapes are what rollout_actor_critic and gae returned -- obs [K,N,OBS] or the [K+1,N,OBS] tape (its first K
    rows are used), actions [K,N,A], logp, advantages, returns [K,N] float32, live [K,N] bool or uint8 (None: every
    row live) -- or the same flattened to R rows: obs [R,OBS], actions [R,A], the others [R].  The minibatch is
    `index`, a contiguous int64 device tensor of row numbers (a slice of torch.randperm; an entry outside [0, R) is
    skipped by the kernel, a duplicate counts twice), or, with index=None, the `num_samples` (default: all) rows
    from `row_base` on.  A row is live iff its `live` byte is nonzero: a uint8 tape holding 2 or 255 gives the bits
    of one holding 1; a dead row, a row the index does not name and an out-of-range sample are never read.  The
    tapes may be contiguous views that start inside larger buffers (`buf[k:]`), with one condition the library
    checks: obs must start on a 16-byte boundary.  Every row of a [R,12] tape does; of a [R,10], [R,6] or [R,2] tape
    only every second row does, and a view from another row is refused with a CopterStepError that names
    the alignment, before any launch.

    Returns PpoGrad(grad [P + Pv + A] float64: dL / d(actor | critic | log_std), stats [8] float64: PPO_STATS of this
    module -- live samples, policy loss, value loss, entropy, L, the approximate KL, the clipped share, max |r - 1|),
    written into `out` / `stats_out` or into new tensors.  The sums run in a fixed order: the same inputs give the
    same bits.  Asynchronous on the current stream; nothing is read by the host."""
    self._check_open()
    torch = _torch()
    dev, A, od = self.device, self.action_dim, self.obs_dim
    P = mlp.num_params(od, A, hidden)                                # (checks hidden)
    Pv = mlp.num_params(od, 1, critic_hidden) if critic is not None else 0
    if critic is None:
        critic_hidden = 0 if critic_hidden is None else critic_hidden
        mlp.num_params(od, 1, critic_hidden)
    keep = []
    th = _wire.exact_vector(self, actor, P, "actor", keep, _ON_DEVICE, foreign=False)
    tv = _wire.exact_vector(self, critic, Pv, "critic", keep, _ON_DEVICE, foreign=False) if critic is not None else None
    ls = _wire.exact_vector(self, log_std, A, "log_std", keep, _ON_DEVICE, foreign=False)
    if not isinstance(actions, torch.Tensor) or actions.dim() not in (2, 3):
        raise ValueError("actions must be the [K,N,%d] action tape of rollout_actor_critic or its rows [R,%d]"
                         % (A, A))
    lead = tuple(actions.shape[:-1])
    R = math.prod(lead)
    if R < 1:
        raise ValueError("the tapes hold no rows")
    if not isinstance(obs, torch.Tensor):
        raise ValueError("obs must be the obs tape of rollout_actor_critic, a device tensor")
    if len(lead) == 2 and tuple(obs.shape) == (lead[0] + 1, lead[1], od):
        obs = obs[:lead[0]]                                           # (the [K+1,N,OBS] tape: a contiguous prefix)
    tapes = [(obs, "obs", lead + (od,), torch.float32), (actions, "actions", lead + (A,), torch.float32),
             (logp, "logp", lead, torch.float32), (advantages, "advantages", lead, torch.float32)]
    if tv is not None or returns is not None:
        tapes.append((returns, "returns", lead, torch.float32))
    _wire.check_tape(self, "rollout_actor_critic / gae", *tapes)
    if live is not None:
        if not isinstance(live, torch.Tensor) or live.dtype not in (torch.bool, torch.uint8):
            raise ValueError("live must be a bool or uint8 device tensor of shape %s" % (lead,))
        _wire.check_tape(self, "rollout_actor_critic", (live, "live", lead, live.dtype))
        live = live.view(torch.uint8) if live.dtype == torch.bool else live
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype != torch.int64 \
                or index.device != dev or not index.is_contiguous() or index.shape[0] < 1:
            raise ValueError("index must be a contiguous 1-D int64 tensor on %s with at least one entry" % (dev,))
        if num_samples is not None and int(num_samples) != int(index.shape[0]):
            raise ValueError("num_samples = %r disagrees with index [%d]" % (num_samples, index.shape[0]))
        B, base = int(index.shape[0]), 0
    else:
        if not isinstance(row_base, (int, np.integer)) or isinstance(row_base, bool):
            raise ValueError("row_base must be an int, got %r" % (row_base,))
        base = int(row_base)
        B = R - base if num_samples is None else num_samples
        if not isinstance(B, (int, np.integer)) or isinstance(B, bool) or B < 1 or base < 0 or base + B > R:
            raise ValueError("rows row_base .. row_base + num_samples - 1 must lie in [0, %d), got row_base %r, "
                             "num_samples %r" % (R, row_base, num_samples))
        B = int(B)
    cl, vf, en = float(clip), float(vf_coef), float(ent_coef)
    if not math.isfinite(cl) or not cl > 0.0:
        raise ValueError("clip must be finite and > 0, got %r" % (clip,))
    if not math.isfinite(vf) or not math.isfinite(en):
        raise ValueError("vf_coef and ent_coef must be finite, got %r and %r" % (vf_coef, ent_coef))
    if out is None:
        out = _wire.empty(self, P + Pv + A, torch.float64)
    else:
        _wire.check_tape(self, "ppo_grad", (out, "out", (P + Pv + A,), torch.float64))
    if stats_out is None:
        stats_out = _wire.empty(self, 8, torch.float64)
    else:
        _wire.check_tape(self, "ppo_grad", (stats_out, "stats_out", (8,), torch.float64))
    # (a minibatch step is host-bound, so this wrapper is wired by hand: inline scalar checks above, the block filled
    # member by member and the library called directly -- what _wire.block's keywords and _wire.launch do, without their
    # calls; profiles/host_wrappers_refactor_ab.txt)
    pio = _wire.block(_lib.PpoGradIO)
    pio.hidden, pio.critic_hidden, pio.normalize = hidden, critic_hidden, 1 if normalize else 0
    pio.num_rows, pio.num_samples, pio.row_base = R, B, base
    pio.clip, pio.vf_coef, pio.ent_coef = cl, vf, en
    pio.actor_dev, pio.log_std_dev = th.data_ptr(), ls.data_ptr()
    pio.critic_dev = tv.data_ptr() if tv is not None else None
    pio.obs_dev, pio.actions_dev, pio.logp_dev = obs.data_ptr(), actions.data_ptr(), logp.data_ptr()
    pio.advantages_dev = advantages.data_ptr()
    pio.returns_dev = returns.data_ptr() if returns is not None else None
    pio.live_dev = live.data_ptr() if live is not None else None
    pio.index_dev = index.data_ptr() if index is not None else None
    pio.grad_dev, pio.stats_dev = out.data_ptr(), stats_out.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(self._lib.cs_ppo_grad(self._ctx, C.byref(pio), self._stream()))
    keep += [obs, actions, logp, advantages, returns, live, index]
    self._keep = keep
    return PpoGrad(out, stats_out)


def _forward(torch, params, obs, hidden, obs_dim, act_dim):
    """pi_theta(obs) in float32 with autograd: obs [B, OBS] -> [B, act_dim]."""
    p = mlp.unpack(params, obs_dim, act_dim, hidden)
    if hidden == 0:
        return obs @ p["W"].T + p["b"]
    return torch.tanh(obs @ p["W1"].T + p["b1"]) @ p["W2"].T + p["b2"]


def gaussian_logp(torch, actions, means, log_std):
    """log N(a; mu, exp(log_std)^2) summed over the components, in the dtype of its arguments."""
    z = (actions - means) * torch.exp(-log_std)
    return -0.5 * (z * z).sum(-1) - log_std.sum() - 0.5 * actions.shape[-1] * math.log(2.0 * math.pi)


def ppo(env, actor0, critic0, log_std0, hidden, critic_hidden, K, iterations, epochs=4, minibatches=4, clip=0.2,
        lr=3e-4, gamma=0.99, lam=0.95, vf_coef=0.5, ent_coef=0.0, seed=0, update="torch"):
    """Proximal policy optimisation of the Gaussian MLP policy (actor0 [P], log_std0 [A]) and the MLP value function
    (critic0 [Pv]; gym_copter_amd.mlp's layout for `hidden` / `critic_hidden`, the critic with act_dim = 1) on `env`,
    which keeps stepping under its own auto-reset mode from wherever it stands.  Iteration t:

      1. roll = env.rollout_actor_critic(actor, critic, log_std, K, hidden, critic_hidden, nonce=t)
      2. adv, ret = env.gae(roll.reward, roll.values, roll.terminated, roll.truncated, gamma, lam)
      3. `epochs` passes over the K N samples in `minibatches` random minibatches each: an Adam step of size lr on
             -min(r A, clip(r, 1 - clip, 1 + clip) A) + vf_coef (V - ret)^2 / 2 - ent_coef H
         averaged over the minibatch's LIVE samples (roll.live: a next_step reset step, whose action the env ignores,
         carries no weight), r = exp(logp_new - roll.logp), A the advantages normalised over the minibatch's live
         samples, H the Gaussian's entropy.

    The update is plain torch autograd on a float32 restatement of the two networks; roll.logp is computed by the kernel
    from the stored actions, so r = 1 up to float32 rounding in the first minibatch of every iteration (recorded in
    stats).  `seed` seeds the minibatch permutations.  No host read happens inside the loop.

    update="torch" (the default) is the above; update="device" makes every minibatch's loss and gradient with one
    library call instead (env.ppo_grad, DESIGN.md section 18: the same function in float64, reduced on the device in a
    fixed order), copies the gradient into the three leaves' .grad as float32 and takes the same Adam step.  The
    permutations, the optimizer and the statistics columns are the same; the two paths differ by rounding.

    Returns PpoResult(actor [P], critic [Pv], log_std [A] float32 after the last update, history [iterations] float32:
    the mean reward per live step of every iteration's collection, stats [iterations, 6] float32: the columns
    STATS of this module)."""
    torch = _torch()
    if update not in ("torch", "device"):
        raise ValueError("update must be 'torch' or 'device', got %r" % (update,))
    dev = env.device
    for v, name in ((iterations, "iterations"), (epochs, "epochs")):
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ValueError("%s must be an int >= 0, got %r" % (name, v))
    if not isinstance(minibatches, int) or isinstance(minibatches, bool) or minibatches < 1:
        raise ValueError("minibatches must be an int >= 1, got %r" % (minibatches,))
    if not isinstance(K, int) or isinstance(K, bool) or K < 1:
        raise ValueError("K must be an int >= 1, got %r" % (K,))
    od, A, n = env.obs_dim, env.action_dim, env.num_envs
    B = K * n
    if minibatches > B:
        raise ValueError("minibatches = %d exceeds the K N = %d samples of an iteration" % (minibatches, B))

    def leaf(t, size, name):
        t = t.detach() if isinstance(t, torch.Tensor) else torch.as_tensor(t)
        if tuple(t.shape) != (size,):
            raise ValueError("%s must have shape (%d,), got %s" % (name, size, tuple(t.shape)))
        return t.to(device=dev, dtype=torch.float32).clone().requires_grad_(True)
    actor = leaf(actor0, mlp.num_params(od, A, hidden), "actor0")
    critic = leaf(critic0, mlp.num_params(od, 1, critic_hidden), "critic0")
    log_std = leaf(log_std0, A, "log_std0")
    opt = torch.optim.Adam([actor, critic, log_std], lr=float(lr), eps=1e-5)
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    one = torch.ones((), dtype=torch.float32, device=dev)
    rows = []
    P, Pv = actor.shape[0], critic.shape[0]
    if update == "device":
        grad64 = torch.empty(P + Pv + A, dtype=torch.float64, device=dev)
        grad32 = torch.zeros(P + Pv + A, dtype=torch.float32, device=dev)
        actor.grad, critic.grad, log_std.grad = grad32[:P], grad32[P:P + Pv], grad32[P + Pv:]
        mb_stats = torch.empty(8, dtype=torch.float64, device=dev)
    for t in range(iterations):
        with torch.no_grad():
            roll = env.rollout_actor_critic(actor, critic, log_std, K, hidden, critic_hidden, nonce=t)
            adv, ret = env.gae(roll.reward, roll.values, roll.terminated, roll.truncated, gamma, lam)
            obs = roll.obs[:K].reshape(B, od)
            act = roll.actions.reshape(B, A)
            logp_old, adv, ret = roll.logp.reshape(B), adv.reshape(B), ret.reshape(B)
            live = roll.live.reshape(B).to(torch.float32)
            count = live.sum()
            mean_reward = (roll.reward.reshape(B) * live).sum() / torch.maximum(count, one)
            done_rate = (roll.terminated | roll.truncated).to(torch.float32).mean()
        first_err = pol_loss = val_loss = torch.zeros((), dtype=torch.float32, device=dev)
        for ep in range(epochs):
            perm = torch.randperm(B, device=dev, generator=gen)
            for mb in range(minibatches):
                idx = perm[mb * B // minibatches:(mb + 1) * B // minibatches]
                if update == "device":
                    with torch.no_grad():
                        env.ppo_grad(actor, critic, log_std, hidden, critic_hidden, obs, act, logp_old, adv, ret,
                                     live=roll.live.reshape(B), index=idx, clip=clip, vf_coef=vf_coef,
                                     ent_coef=ent_coef, out=grad64, stats_out=mb_stats)
                        grad32.copy_(grad64)
                        if ep == 0 and mb == 0:
                            first_err = mb_stats[7].to(torch.float32)
                        pol_loss, val_loss = mb_stats[1].to(torch.float32), mb_stats[2].to(torch.float32)
                    opt.step()
                    continue
                w = live[idx]
                wsum = torch.maximum(w.sum(), one)
                a_mb = adv[idx]
                a_mean = (a_mb * w).sum() / wsum
                a_std = (((a_mb - a_mean) ** 2 * w).sum() / wsum).sqrt()
                a_mb = (a_mb - a_mean) / (a_std + 1e-8)
                o_mb = obs[idx]
                logp = gaussian_logp(torch, act[idx], _forward(torch, actor, o_mb, hidden, od, A), log_std)
                ratio = torch.exp(logp - logp_old[idx])
                surr = torch.minimum(ratio * a_mb, torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * a_mb)
                pol_loss = -(surr * w).sum() / wsum
                value = _forward(torch, critic, o_mb, critic_hidden, od, 1)[:, 0]
                val_loss = 0.5 * (((value - ret[idx]) ** 2) * w).sum() / wsum
                entropy = log_std.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
                loss = pol_loss + vf_coef * val_loss - ent_coef * entropy
                if ep == 0 and mb == 0:
                    first_err = ((ratio.detach() - 1.0).abs() * w).max()
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
        rows.append(torch.stack([mean_reward, count, first_err.detach(), pol_loss.detach(), val_loss.detach(),
                                 done_rate]))
    stats = torch.stack(rows) if rows else torch.zeros((0, len(STATS)), dtype=torch.float32, device=dev)
    return PpoResult(actor.detach(), critic.detach(), log_std.detach(), stats[:, 0].clone(), stats)
