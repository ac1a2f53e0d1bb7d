"""A small PPO driver on CopterVecEnv.rollout_actor_critic / gae: the MLP policy of the
closed-loop rollouts with a state-independent Gaussian and an MLP value head, trained on-policy.

Every iteration is two library kernels -- the K-step collection with its log-probabilities and values, and the
advantages -- followed by the clipped-surrogate update in plain torch autograd on a float32 restatement of the two
networks (gym_copter_amd.mlp.unpack).  Nothing is read by the host inside the loop; the per-iteration statistics stay on
the device until the caller reads them."""
import collections
import math

from . import mlp

PpoResult = collections.namedtuple("PpoResult", "actor critic log_std history stats")
# the columns of PpoResult.stats [iterations, 6] float32
STATS = ("mean_reward_per_live_step", "live_samples", "first_ratio_error", "policy_loss", "value_loss", "done_rate")


def _torch():
    import torch
    return torch


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
