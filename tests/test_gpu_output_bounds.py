"""The memory contract of every rollout entry point of CopterVecEnv, with tests/guarded_outputs.py: no call writes outside
the arrays it is given, every call writes every element of every tensor it returns, and no call modifies an input tensor.
The values are the business of the families' own tests; every comparison here is exact and there is no tolerance.

The wrappers allocate their outputs with torch.empty, so a store past the end of an output lands in a neighbouring block of
the caching allocator, where no value test looks: a padding lane that stores row j of an env index >= N hits the head of row
j + 1, which the right value overwrites later, and only the overflow of the last row written leaves the tensor.  Here
every output sits between two bands of the byte 0xA5, 256 envs' worth of the tensor each.

Sizes: N = 1 (a single lane), 64 (exactly one wavefront: the back band begins right behind a whole-wavefront run), 65 (one
whole wavefront and one lane: both store paths in one call) and 191 (a last wavefront of 63 lanes); K = 1 (the shortest
horizon: no "row j + 1" exists) and 3.  Task lander3d throughout, and lander1d where an output is action-shaped: its rows
are 4 bytes (float32) or 8 bytes (float64) wide, the width at which a vectorised store would overrun.  Every method that
takes dtype= runs once more with torch.float32 at N = 65, K = 3.  One env per case (the wrappers cache their output
buffers by key); where a case calls a method twice, the first call's payloads are given the fill again in between.

No exemption from "fully written" is used: no docstring, INTEGRATION.md or DESIGN.md says of any returned tensor that the
call leaves part of it as it was."""
import numpy as np
import pytest

import model_variants
import ppo_update_ref as pur
import test_gpu_rollout_ac as AC
import test_gpu_rollout_ekf as E
import test_gpu_rollout_es as ES
import test_gpu_rollout_lqr as L
import test_gpu_rollout_mlp as M
import test_gpu_rollout_mppi as MP
from gpu_util import have_gpu
from guarded_outputs import guarded
from jacobian_fd import hover_action

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

AH = hover_action()
NS, KS = (1, 64, 65, 191), (1, 3)
SIZES = [(n, K) for n in NS for K in KS]
WIDE, NARROW = "lander3d", "lander1d"
# (n, K, task, dtype): every size on both tasks, and float32 outputs once
ACTION_CASES = [(n, K, t, None) for t in (WIDE, NARROW) for n, K in SIZES] + [(65, 3, WIDE, "float32")]
WIDE_CASES = [(n, K, WIDE, None) for n, K in SIZES] + [(65, 3, WIDE, "float32")]

# method of CopterVecEnv -> the test below that calls it under a guard (tests/test_guarded_outputs_cpu.py compares this
# list with the class, so that a later entry point is not forgotten)
COVERED = {
    "step_many": "test_stepping_forms", "rollout_random": "test_stepping_forms", "rollout_pid": "test_stepping_forms",
    "step_jacobian": "test_step_jacobian",
    "rollout_states": "test_rollout_states_and_vjps", "rollout_vjp": "test_rollout_states_and_vjps",
    "rollout_vjp_params": "test_rollout_states_and_vjps",
    "rollout_mlp_states": "test_mlp_rollouts", "rollout_mlp_vjp": "test_mlp_rollouts",
    "mlp_param_grad": "test_mlp_rollouts",
    "rollout_lqr": "test_lqr_and_feedback", "rollout_feedback_states": "test_lqr_and_feedback",
    "rollout_mppi_costs": "test_mppi", "rollout_mppi_update": "test_mppi", "rollout_mppi_temperature": "test_mppi",
    "rollout_mlp_population": "test_population", "es_perturb": "test_es_perturb_and_gradient",
    "es_gradient": "test_es_perturb_and_gradient",
    "rollout_actor_critic": "test_actor_critic_and_gae", "gae": "test_actor_critic_and_gae",
    "ppo_grad": "test_ppo_grad",
    "rollout_ekf": "test_ekf_and_rts", "rollout_rts": "test_ekf_and_rts",
    # the families whose guarded test lives with their own tests: "<module>::<test>"
    "rollout_pf": "test_gpu_rollout_pf::test_outputs_are_written_fully_and_nothing_else",
    "rollout_lqg": "test_gpu_lqg_output_bounds::test_lqg_outputs_are_written_exactly",
    "rollout_ukf": "test_gpu_ukf_output_bounds::test_ukf_outputs_are_written_exactly",
}
SKIPPED = {
    "rollout_policy": "needs a policy functor compiled with hipcc at run time; it goes through _rollout, whose buffers and "
                      "K-step kernel rollout_random and rollout_pid cover",
}


def _env(task, n, mode="float64", autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    return gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _dtype(name):
    import torch
    return None if name is None else getattr(torch, name)


def _fields(prefix, nt):
    """the tensors of a named tuple as keyword arguments of _run (inputs to freeze)"""
    return {"%s_%s" % (prefix, f): t for f, t in zip(nt._fields, nt) if t is not None}


def _run(g, call, except_=(), **inputs):
    """One guarded call: `inputs` frozen, call(), then the three assertions.  Returns what call() returned."""
    import torch
    g.release()
    g.freeze(**{k: v for k, v in inputs.items() if isinstance(v, torch.Tensor)})
    result = call()
    torch.cuda.synchronize()
    g.assert_bands_intact()
    g.assert_fully_written(result, except_=except_)
    g.assert_inputs_unchanged()
    return result


def _start(env, rng, force=False):
    """an explicit airborne start on the device (tests/test_gpu_rollout_mppi.py's points), get_state()'s layout"""
    x, st = MP._random_point(env.num_envs, rng)
    state = {"x": _dev(x, env), "status": _dev(st, env)}
    if force:
        state["force"] = _dev(rng.uniform(-1.0, 1.0, (3, env.num_envs)), env)
    return state


def _actions(env, K, rng):
    return _dev((AH * rng.uniform(0.7, 1.3, (K, env.num_envs, env.action_dim))).astype(np.float32), env)


# ---------------------------------------------------------------------------------------------------------------------
# the guard on the device itself
# ---------------------------------------------------------------------------------------------------------------------
def test_the_guard_intercepts_and_sees_a_stray_write_on_the_device():
    """tests/test_guarded_outputs_cpu.py's negative cases once on the device: the wrapper's own torch.empty is
    intercepted, and one float stored through the backing buffer right behind a payload, one stored right in front of it
    and one element given the fill again are each reported (the stores stay inside the helper's own allocation)."""
    import torch
    n = 65
    env = _env(WIDE, n)
    try:
        env.reset()
        acts = _actions(env, 3, np.random.default_rng(0))
        real = torch.empty
        with guarded(n) as g:
            ro = _run(g, lambda: env.rollout_states(acts), actions=acts)
        assert len(g.allocations) == 5 and all(a.backing.device == env.device for a in g.allocations)
        x = g.allocations[0]
        assert x.shape == (3, n, 12) and x.ptr == ro.x.data_ptr() and x.ptr % 512 == 0 and x.front == 256 * 3 * 96
        end = x.front + x.nbytes
        x.backing[end:end + 8] = 0
        with pytest.raises(AssertionError, match=r"the back band of allocation #0 .* bytes 0 \.\. 7 past the payload's end"):
            g.assert_bands_intact()
        x.backing[end:end + 8] = g.fill
        g.assert_bands_intact()
        x.backing[x.front - 8:x.front] = 0
        with pytest.raises(AssertionError, match=r"the front band of allocation #0 .* bytes 8 \.\. 1 before"):
            g.assert_bands_intact()
        x.backing[x.front - 8:x.front] = g.fill
        at = x.front + (2 * n + 64) * 12 * 8                       # the last env's row of the last step
        x.backing[at:at + 96] = g.fill
        with pytest.raises(AssertionError, match=r"result.x .* 12 of 2340 elements were not written, the first at index "
                                                 r"\[2, 64, 0\]"):
            g.assert_fully_written(ro)
        acts[1, 7, 2] += 1.0
        with pytest.raises(AssertionError, match="input 'actions'"):
            g.assert_inputs_unchanged()
        assert torch.empty is real                                   # (the patch is gone)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# the K-step stepping forms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,task", [c[:3] for c in ACTION_CASES if c[3] is None])
def test_stepping_forms(n, K, task):
    """step_many, rollout_random and rollout_pid (the lander heuristic: lander3d), with and without the action tape.  The
    three share one set of buffers per K."""
    rng = np.random.default_rng(1000 * n + K)
    env = _env(task, n, mode="float32", autoreset="next_step", seed=3)
    try:
        env.reset()
        acts = _dev(rng.uniform(-1, 1, (K, n, env.action_dim)).astype(np.float32), env)
        with guarded(n) as g:
            _run(g, lambda: env.step_many(acts), actions=acts)
            r = _run(g, lambda: env.rollout_random(K), actions=acts)
            g.refill(r)
            r = _run(g, lambda: env.rollout_random(K, return_actions=True), actions=acts)
            assert len(r) == 5 and tuple(r[4].shape) == (K, n, env.action_dim)
            if task == WIDE:
                g.refill(r)
                r4 = _run(g, lambda: env.rollout_pid(K), actions=acts)
                g.refill(r)
                r = _run(g, lambda: env.rollout_pid(K, return_actions=True), actions=acts)
                assert len(r4) == 4 and len(r) == 5
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# step_jacobian
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,task,dtype", [(n, t, None) for t in (WIDE, NARROW) for n in NS] + [(65, WIDE, "float32")])
def test_step_jacobian(n, task, dtype):
    """At the stored state and at an explicit one with a pending force; du [N,12,A] and reward_du [N,A] are action-shaped."""
    rng = np.random.default_rng(2000 + n)
    env = _env(task, n)
    try:
        env.reset()
        a = _actions(env, 1, rng)[0].contiguous()
        state = _start(env, rng, force=True)
        with guarded(n) as g:
            j = _run(g, lambda: env.step_jacobian(a, dtype=_dtype(dtype)), actions=a)
            g.refill(j)
            _run(g, lambda: env.step_jacobian(a, state=state, dtype=_dtype(dtype)), actions=a, **state)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# open-loop rollouts and their gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,task,dtype", ACTION_CASES)
def test_rollout_states_and_vjps(n, K, task, dtype):
    """rollout_states from the stored start, from an explicit one and under a vehicle override; rollout_vjp with both
    cotangents, with gr alone and with neither; rollout_vjp_params with gx alone under the override."""
    rng = np.random.default_rng(3000 + 10 * n + K)
    env = _env(task, n)
    try:
        env.reset()
        dt = _dtype(dtype)
        acts = _actions(env, K, rng)
        gx, gr = _dev(rng.standard_normal((K, n, 12)), env), _dev(rng.standard_normal((K, n)), env)
        plain, forced = _start(env, rng), _start(env, rng, force=True)
        table = _dev(model_variants.vehicle_table(rng, n, mars=False), env)
        with guarded(n) as g:
            ro = _run(g, lambda: env.rollout_states(acts), actions=acts)
            v = _run(g, lambda: env.rollout_vjp(acts, ro, gx, gr, dtype=dt), actions=acts, gx=gx, gr=gr, **_fields("ro", ro))
            assert v[1] is None
            g.refill(v)
            _run(g, lambda: env.rollout_vjp(acts, ro, dtype=dt), actions=acts, **_fields("ro", ro))
            g.refill(ro)
            ro = _run(g, lambda: env.rollout_states(acts, state=plain), actions=acts, **plain)
            g.refill(v)
            v = _run(g, lambda: env.rollout_vjp(acts, ro, gr=gr, state=plain, dtype=dt), actions=acts, gr=gr,
                     **plain, **_fields("ro", ro))
            assert tuple(v[1].shape) == (12, n)
            g.refill(ro)
            ro = _run(g, lambda: env.rollout_states(acts, state=forced, vehicle=table), actions=acts, vehicle=table,
                      **forced)
            g.refill(v)
            v = _run(g, lambda: env.rollout_vjp_params(acts, ro, gx=gx, state=forced, vehicle=table, dtype=dt),
                     actions=acts, gx=gx, vehicle=table, **forced, **_fields("ro", ro))
            assert len(v) == 4 and tuple(v[2].shape) == (12, n) and tuple(v[3].shape) == (3, n)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# closed-loop rollouts under the fused MLP policy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden", [0, 33])
@pytest.mark.parametrize("n,K,task,dtype", ACTION_CASES)
def test_mlp_rollouts(n, K, task, dtype, hidden):
    """rollout_mlp_states (stored start; explicit start with offsets), rollout_mlp_vjp with the parameter gradient reduced
    on the device (with and without the action-tape cotangent) and mlp_param_grad on its own.  hidden 0 is the linear
    policy; 33 is no multiple of 64 and leaves idle lanes in the row stages."""
    rng = np.random.default_rng(4000 + 10 * n + K + hidden)
    env = _env(task, n)
    try:
        env.reset()
        dt = _dtype(dtype)
        theta = M._theta(task, hidden, seed=7, env=env)
        x, st = M._point(n, rng)
        state = {"x": _dev(x, env), "status": _dev(st, env)}
        off = _dev((0.01 * AH * rng.standard_normal((K, n, env.action_dim))).astype(np.float32), env)
        gx, gr = _dev(rng.standard_normal((K, n, 12)), env), _dev(rng.standard_normal((K, n)), env)
        gin = _dev(rng.standard_normal((K, n, env.action_dim)), env)
        with guarded(n) as g:
            r = _run(g, lambda: env.rollout_mlp_states(theta, K, hidden), theta=theta)
            v = _run(g, lambda: env.rollout_mlp_vjp(theta, r, gx, gr, hidden=hidden, dtype=dt, reduce="device"),
                     theta=theta, gx=gx, gr=gr, **_fields("r", r))
            assert tuple(v[0].shape) == tuple(theta.shape) and v[2] is None
            g.refill(r)
            r = _run(g, lambda: env.rollout_mlp_states(theta, K, hidden, offsets=off, state=state), theta=theta,
                     offsets=off, **state)
            g.refill(v[1])
            v = _run(g, lambda: env.rollout_mlp_vjp(theta, r, gr=gr, state=state, hidden=hidden, dtype=dt,
                                                    g_actions_in=gin, reduce="device"),
                     theta=theta, gr=gr, g_actions_in=gin, **state, **_fields("r", r))
            assert tuple(v[2].shape) == (12, n)
            _run(g, lambda: env.mlp_param_grad(theta, hidden, r.obs, v[1]), theta=theta, obs=r.obs, g_actions=v[1])
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# the iLQR backward pass and its feedback rollout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,task,dtype", ACTION_CASES)
def test_lqr_and_feedback(n, K, task, dtype):
    """rollout_lqr (K [K,N,A,12] and d [K,N,A] are action-shaped) and rollout_feedback_states (actions_out).  The feedback
    takes float64 gains, so the float32 case guards the gains alone."""
    rng = np.random.default_rng(5000 + 10 * n + K)
    env = _env(task, n)
    try:
        env.reset()
        A = env.action_dim
        acts, state = _actions(env, K, rng), _start(env, rng)
        Q, Qf, R, q, r = L._cost_model(rng, A, K, n)
        q, r = _dev(q, env), _dev(r, env)
        ro = env.rollout_states(acts, state=state)
        ro = type(ro)(*(t.clone() for t in ro))
        alpha = _dev(rng.uniform(0.1, 1.0, n), env)
        with guarded(n) as g:
            gains = _run(g, lambda: env.rollout_lqr(acts, ro, Q, R, q=q, r=r, Q_final=Qf, mu=1e-3, state=state,
                                                   dtype=_dtype(dtype)),
                         actions=acts, q=q, r=r, **state, **_fields("ro", ro))
            if dtype is None:
                fb = _run(g, lambda: env.rollout_feedback_states(acts, ro, gains, alpha, state=state), actions=acts,
                          alpha=alpha, **state, **_fields("ro", ro), **_fields("gains", gains))
                assert tuple(fb[1].shape) == (K, n, A)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# MPPI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,task", [c[:3] for c in ACTION_CASES if c[3] is None])
def test_mppi(n, K, task):
    """rollout_mppi_costs, rollout_mppi_update and rollout_mppi_temperature with 37 samples (no multiple of 64), white
    noise and knots.  The update alternates between two buffer sets: three calls write the first, the second and the first
    again, the last with one temperature per env."""
    import torch
    import gym_copter_amd
    rng = np.random.default_rng(6000 + 10 * n + K)
    env = _env(task, n)
    try:
        env.reset()
        A, P, sigma = env.action_dim, 37, 0.2 * AH
        acts, state = _actions(env, K, rng), _start(env, rng)
        Q, Qf, R, x_ref, a_ref = MP._cost_model(rng, A, n)
        x_ref = _dev(x_ref, env)
        knots = gym_copter_amd.mppi_knots(K, 2)
        with guarded(n) as g:
            c = _run(g, lambda: env.rollout_mppi_costs(acts, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref,
                                                      reward_weight=0.1, stream=3, state=state),
                     actions=acts, x_ref=x_ref, **state)
            assert tuple(c.costs.shape) == (P, n)
            u0 = _run(g, lambda: env.rollout_mppi_update(acts, c.costs, sigma, 50.0, stream=3), actions=acts, costs=c.costs)
            g.refill(c)
            c = _run(g, lambda: env.rollout_mppi_costs(u0.actions, sigma, P, x_ref, Q, R, stream=4, state=state, knots=knots),
                     actions=u0.actions, x_ref=x_ref, **state)
            u1 = _run(g, lambda: env.rollout_mppi_update(u0.actions, c.costs, sigma, 50.0, stream=4, knots=knots),
                      actions=u0.actions, costs=c.costs)
            assert u1.actions.data_ptr() != u0.actions.data_ptr()
            t = _run(g, lambda: env.rollout_mppi_temperature(c.costs, 8.0), costs=c.costs)
            g.refill(u0)
            u2 = _run(g, lambda: env.rollout_mppi_update(u1.actions, c.costs, sigma, t.lam, stream=4, knots=knots),
                      actions=u1.actions, costs=c.costs, lam=t.lam)
            assert u2.actions.data_ptr() == u0.actions.data_ptr()
            # an env without a finite cost and one without a usable temperature "keep their actions": written all the same
            bad, lam = c.costs.clone(), t.lam.clone()
            bad[:, 0], lam[n - 1] = float("inf"), float("nan")
            g.refill(u1)
            u3 = _run(g, lambda: env.rollout_mppi_update(u2.actions, bad, sigma, lam, stream=4, knots=knots),
                      actions=u2.actions, costs=bad, lam=lam)
            assert u3.actions.data_ptr() == u1.actions.data_ptr()
            for i in (0, n - 1):
                assert torch.equal(u3.actions[:, i], u2.actions[:, i]) and float(u3.ess[i]) == 0.0
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# population rollouts and evolution strategies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members,E_,K,hidden", [(1, 64, 1, 0), (1, 64, 3, 33), (3, 64, 3, 33), (3, 64, 1, 0),
                                                 (2, 128, 3, 33)])
def test_population(members, E_, K, hidden):
    """rollout_mlp_population takes N = members x envs_per_member with envs_per_member a multiple of 64, so of the sizes
    above only N = 64 exists for it: one wavefront; and 192 = 3 x 64 and 256 = 2 x 128, where member_returns [3] and [2]
    end far inside a wavefront's width."""
    n = members * E_
    rng = np.random.default_rng(7000 + n + K)
    env = _env(WIDE, n, mode="float32")
    try:
        env.reset()
        table = _dev(ES._table(WIDE, members, hidden, rng), env)
        x, st = ES._low_starts(n, rng)
        x, st = _dev(x, env), _dev(st, env)
        with guarded(n) as g:
            p = _run(g, lambda: env.rollout_mlp_population(table, K, hidden, E_, gamma=0.99), table=table)
            assert tuple(p.member_returns.shape) == (members,)
            g.refill(p)
            _run(g, lambda: env.rollout_mlp_population(table, K, hidden, E_, start_x=x, start_status=st), table=table,
                 start_x=x, start_status=st)
    finally:
        env.close()


@pytest.mark.parametrize("members,num_params", [(2, 1), (6, 65), (6, 257), (70, 300), (2, 64)])
def test_es_perturb_and_gradient(members, num_params):
    """es_perturb launches (pairs, ceil(P / 256)) workgroups of 256 lanes and es_gradient (ceil(P / 64), ceil(pairs / 32)):
    P = 1, 65, 257 and 300 leave the last workgroup ragged in the parameter dimension of both, 35 pairs leave the last
    chunk of pairs with 3; P = 64 is one whole wavefront."""
    rng = np.random.default_rng(8000 + members + num_params)
    env = _env(WIDE, 64, mode="float32")
    try:
        theta = _dev(rng.standard_normal(num_params).astype(np.float32), env)
        w = _dev(rng.standard_normal(members), env)
        with guarded(env.num_envs) as g:
            t = _run(g, lambda: env.es_perturb(theta, 0.05, members, nonce=9, pair_base=5), params=theta)
            assert tuple(t.shape) == (members, num_params)
            gr = _run(g, lambda: env.es_gradient(w, 9, num_params, pair_base=5), weights=w)
            assert tuple(gr.shape) == (num_params,)
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# actor-critic collection, GAE and the PPO gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["lean", "full"])
@pytest.mark.parametrize("n,K,task", [c[:3] for c in ACTION_CASES if c[3] is None])
def test_actor_critic_and_gae(n, K, task, full):
    """rollout_actor_critic in the kernel's lean form (the common configuration) and its full-featured one (episode
    statistics, ticks, time-limit truncation), first without critic and means, then with both (the action, mean and logp
    tapes are action-shaped or one float per env), and gae on the tapes."""
    rng = np.random.default_rng(9000 + 10 * n + K)
    kw = dict(episode_stats=True, track_time=True, time_limit_truncates=True) if full else {}
    env = _env(task, n, mode="float32", autoreset="next_step", seed=11, **kw)
    try:
        env.reset()
        H, Hv = 33, 16
        actor, critic, log_std = AC._policy(task, H, Hv, int(rng.integers(1 << 30)), env)
        with guarded(n) as g:
            r = _run(g, lambda: env.rollout_actor_critic(actor, None, log_std, K, H), actor=actor, log_std=log_std)
            assert r.means is None and r.values is None
            g.refill(r)
            r = _run(g, lambda: env.rollout_actor_critic(actor, critic, log_std, K, H, critic_hidden=Hv, nonce=5,
                                                        means=True),
                     actor=actor, critic=critic, log_std=log_std)
            assert tuple(r.means.shape) == (K, n, env.action_dim) and tuple(r.values.shape) == (K + 1, n)
            _run(g, lambda: env.gae(r.reward, r.values, r.terminated, r.truncated), reward=r.reward, values=r.values,
                 terminated=r.terminated, truncated=r.truncated)
    finally:
        env.close()


@pytest.mark.parametrize("task,H,Hv,B,ranged", [(WIDE, 16, 16, 37, False), (WIDE, 0, 0, 101, False),
                                                (NARROW, 33, 3, 1, False), (WIDE, 64, None, 200, True),
                                                (WIDE, 16, 16, 65, False)])
def test_ppo_grad(task, H, Hv, B, ranged):
    """ppo_grad on minibatches that are no multiple of the 64-row tile (1, 37, 65, 101, 200), through an index and through a
    row range; the gradient [P + Pv + A] and the statistics [8] are both the wrapper's allocations."""
    env = _env(task, 64, mode="float32", autoreset="next_step")
    try:
        s = pur.to_device(pur.synthetic(task, H, Hv, pur.DEGENERATE_R, 1), env.device)
        idx = None if ranged else s["perm"][:B].contiguous()
        tapes = {k: s[k] for k in ("actor", "critic", "log_std", "obs", "actions", "logp", "advantages", "returns", "live")}
        with guarded(env.num_envs) as g:
            if ranged:
                call = lambda: env.ppo_grad(s["actor"], s["critic"], s["log_std"], H, Hv, s["obs"], s["actions"], s["logp"],
                                            s["advantages"], s["returns"], live=s["live"], row_base=100, num_samples=B,
                                            ent_coef=0.01)
            else:
                call = lambda: env.ppo_grad(s["actor"], s["critic"], s["log_std"], H, Hv, s["obs"], s["actions"], s["logp"],
                                            s["advantages"], s["returns"], live=s["live"], index=idx, ent_coef=0.01)
            got = _run(g, call, index=idx, **tapes)
            assert tuple(got.stats.shape) == (8,) and got.grad.dim() == 1
    finally:
        env.close()


# ---------------------------------------------------------------------------------------------------------------------
# the extended Kalman filter and the RTS smoother
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,task,dtype", WIDE_CASES)
def test_ekf_and_rts(n, K, task, dtype):
    """rollout_ekf with and without the covariance tape (starts of every branch, tests/test_gpu_rollout_ekf.py's problem),
    rollout_rts with the tape and, given the last row through end=, without.  The smoother reads a float64 filter, so the
    float32 case filters once more in float64 for it."""
    rng = np.random.default_rng(10000 + 10 * n + K)
    env = _env(task, n)
    try:
        dt = _dtype(dtype)
        p = E._problem(env, task, rng, steps=K)
        ins = dict(actions=p["acts"], z=p["z"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        with guarded(n) as g:
            f = _run(g, lambda: env.rollout_ekf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"],
                                                status0=p["st0"], dtype=dt), **ins)
            assert f.P_tape is None
            ft = _run(g, lambda: env.rollout_ekf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"],
                                                 status0=p["st0"], tape=True, dtype=dt), **ins)
            assert tuple(ft.P_tape.shape) == (K, n, 12, 12)
            if dt is not None:
                ft = _run(g, lambda: env.rollout_ekf(p["acts"], p["z"], p["H"], p["r"], p["Q"], p["x0"], p["P0"],
                                                     status0=p["st0"], tape=True), **ins)
            del ins["z"]
            ins.update(_fields("filt", ft))
            s = _run(g, lambda: env.rollout_rts(p["acts"], ft, p["Q"], p["x0"], p["P0"], status0=p["st0"], dtype=dt), **ins)
            assert tuple(s.P_tape.shape) == (K, n, 12, 12)
            end = (ft.x[K - 1].t().contiguous(), ft.P.clone())
            s = _run(g, lambda: env.rollout_rts(p["acts"], ft, p["Q"], p["x0"], p["P0"], status0=p["st0"], end=end,
                                                tape=False, dtype=dt), end_x=end[0], end_P=end[1], **ins)
            assert s.P_tape is None
    finally:
        env.close()

