"""Every rollout entry point with its optional outputs NULL (tests/null_outputs.py has the table and the interposer).

include/copterstep.h promises of most outputs that they "may be NULL (not written)", and the kernels keep that with some
340 pointer tests; the wrappers of gym_copter_amd wire every output, so none of those branches runs in any other test.
In the kernels that stage rows through the LDS for their neighbours' lanes (filter_step.h, cov_tile.h, the smoother, the
particle filter, the iLQR pass), which outputs are present also decides which wave_sync() / __syncthreads() execute.

Per entry point, inside guarded(N): the full call through the wrapper, every output present, its results cloned; then,
the result buffers given the 0xA5 fill again each time, the same call with a subset of the optional outputs nulled --
each one alone (m calls), each one present alone (m calls), all nulled (1 call), and nothing nulled (1 call: the full
call is repeatable, the split-K reductions cs_mlp_param_grad, cs_es_gradient and cs_ppo_grad included).  Every such call
must return 0, leave every byte of a nulled tensor at the fill, give every other output bit-identical to the clone
(integer views: NaN payloads count), leave no element of a present output at the fill, touch no band of any allocation,
no input tensor, and leave get_state() as the full call left it (unchanged, for every entry point but
cs_rollout_actor_critic, which advances the env: its env is set back before every call).  Each family's "each nulled
alone" runs once more with float32 outputs.  Then every `required` output in turn is nulled on the live context: the
call must be refused with CS_ERR_ARG and the pointer's name in cs_last_error(), with every output buffer still at the
fill (nothing was launched) and the env state untouched.

Shapes: N = 65 (a whole wavefront and one lane of the next: both store paths), K = 3 (a first, a middle and a last row),
lander3d, float64 storage.  Filters: M = 3 with a tenth of z missing, starts of every branch
(test_gpu_rollout_ekf._points: AIRBORNE, LANDED and CRASHED lanes), once more with the rotor-gyro term.  Where a launcher
picks a kernel or a launch by a pointer, the subsets reach each: cs_rollout_vjp_ex (neither gradient: the plain sweep;
either: the parameter sweep; g_vehicle: the unfold kernel behind it), cs_rollout_mppi_costs (best_dev: the arg-min
kernel), cs_rollout_mlp_population (member_returns_dev: the reduction kernel), cs_rollout_actor_critic (with and without
a critic), cs_rollout_rts (with and without end_x / end_P), cs_rollout_pf (both start forms).

Measured on an MI355X: 501 calls with outputs nulled and 34 refusals, all as required; the file takes 5.0 s, 2.3 s of
them inside the test functions (each prints its calls and its time, the module its total, under pytest -s).

Mutants this file was seen to fail for on an MI355X (uncommitted builds of the library, this file alone; the current
library passes it):
  - filter_step.h, filter_store_row: the nis store moved inside the var guard -- test_ekf, test_lqg and test_ukf fail
    (all six cases) at "cs_rollout_ekf, cs_rollout_ekf_io.var_dev nulled: result.nis still holds the fill" and its
    cs_rollout_lqg and cs_rollout_ukf twins;
  - rollout_sweep.h, rollout_forward: the status_dev store placed under the reward_dev guard -- test_open_loop_rollouts
    fails at "cs_rollout_states, cs_rollout_io.reward_dev nulled: result.status still holds the fill", and
    test_lqr_and_feedback at the same for cs_rollout_feedback_states, which runs that loop;
  - cs_rollout_ekf's launcher returning CS_ERR_ARG when x_pred_dev is NULL -- both cases of test_ekf fail with
    "CopterStepError: libcopterstep error -1: cs_rollout_ekf: x_pred_dev is required".
"""
import time

import numpy as np
import pytest

import model_variants
import null_outputs as NO
import ppo_update_ref as pur
import test_gpu_rollout_ac as AC
import test_gpu_rollout_ekf as E
import test_gpu_rollout_es as ES
import test_gpu_rollout_lqg as LQ
import test_gpu_rollout_lqr as L
import test_gpu_rollout_mlp as M
import test_gpu_rollout_mppi as MP
import test_gpu_rollout_ukf as U
from gpu_util import have_gpu
from guarded_outputs import _int_view, _walk, guarded
from jacobian_fd import hover_action

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

AH = hover_action()
N, K, TASK = 65, 3, "lander3d"
COUNT = {"calls": 0, "refusals": 0, "seconds": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _total():
    yield
    print("\ntest_gpu_null_outputs: %d calls with outputs nulled, %d refusals, %.1f s in the test functions"
          % (COUNT["calls"], COUNT["refusals"], COUNT["seconds"]))


@pytest.fixture(autouse=True)
def _timed(request):
    t0, c0 = time.perf_counter(), COUNT["calls"]
    yield
    dt = time.perf_counter() - t0
    COUNT["seconds"] += dt
    print("\n%s: %d calls, %.2f s" % (request.node.name, COUNT["calls"] - c0, dt))


def _env(n=N, autoreset="disabled", **kw):
    import gym_copter_amd
    kw.setdefault("max_steps", 100000)
    kw.setdefault("seed", 3)
    return gym_copter_amd.CopterVecEnv(task=TASK, num_envs=n, state_dtype="float64", autoreset_mode=autoreset, **kw)


def _dev(a, env, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device, dtype=dtype)


def _f32():
    import torch
    return torch.float32


def _state(env):
    return {k: np.asarray(v).tobytes() for k, v in env.get_state().items()}


def _holds_fill(g, t):
    pattern = int.from_bytes(bytes([g.fill]) * t.element_size(), "little", signed=True)
    return bool((_int_view(t) == pattern).all())


def _sweep(env, g, entry, call, inputs, via=None, subsets=("alone", "only", "none"), absent=(), prepare=None):
    """The module docstring's procedure for one entry point and one form of its call.  call() makes the wrapper's call;
    inputs: the tensors it reads; via: the attribute the wrapper reaches `entry` through when that is another entry
    point; absent: optional members this form of the call does not wire; prepare(): run before every call."""
    import torch
    from gym_copter_amd import _lib
    row = NO.TABLE[entry]
    null = lambda fields: NO.nulling(env._lib, via or entry, fields, forward_to=entry if via else None)   # noqa: E731
    g.release()
    g.freeze(**{k: v for k, v in inputs.items() if isinstance(v, torch.Tensor)})
    if prepare is not None:
        prepare()
    before = _state(env)
    with null(()) as calls:
        res = call()
    torch.cuda.synchronize()
    assert calls[-1].rc == 0
    seen = calls[-1].seen
    after = _state(env)
    if prepare is None:
        assert after == before, "%s changed the env state" % entry
    g.assert_bands_intact()
    g.assert_fully_written(res)
    g.assert_inputs_unchanged()
    full = [(path, t, t.clone()) for path, t in _walk(res)]
    ptrs = {t.data_ptr() for _, t, _ in full}
    optional = NO.of_class(entry, NO.OPTIONAL)
    wired = [f for f in optional if seen[f]]
    assert set(optional) - set(wired) == set(absent), (entry, sorted(set(optional) - set(wired)))
    for f in wired + [f for f in NO.of_class(entry, NO.REQUIRED) if seen[f]]:
        assert seen[f] in ptrs, "%s: %s is no tensor of the wrapper's result" % (entry, f)

    plans = [()]
    if "alone" in subsets:
        plans += [(f,) for f in wired]
    if "only" in subsets:
        plans += [tuple(o for o in wired if o != f) for f in wired]
    if "none" in subsets:
        plans += [tuple(wired)]
    done = set()
    for nulled in plans:
        if nulled in done:
            continue
        done.add(nulled)
        what = "%s, %s nulled" % (entry, " ".join(nulled) if nulled else "nothing")
        g.refill(res)
        if prepare is not None:
            prepare()
        with null(nulled) as calls:
            again = call()
        torch.cuda.synchronize()
        COUNT["calls"] += 1
        assert calls[-1].rc == 0, what
        gone = {seen[f] for f in nulled}
        found = list(_walk(again))
        assert [(p, t.data_ptr()) for p, t in found] == [(p, t.data_ptr()) for p, t, _ in full], what
        left = []
        for (path, t), (_, _, clone) in zip(found, full):
            if t.data_ptr() in gone:
                assert _holds_fill(g, t), "%s: %s was written" % (what, path)
                left.append(t)
            else:
                unwritten = _holds_fill(g, t) and t.numel() > 0
                assert not unwritten, "%s: %s still holds the fill" % (what, path)
                assert torch.equal(_int_view(t), _int_view(clone)), "%s: %s differs from the full call's" % (what, path)
        g.assert_fully_written(again, except_=left)
        g.assert_bands_intact()
        g.assert_inputs_unchanged()
        assert _state(env) == after, "%s: the env state differs" % what

    for f in NO.of_class(entry, NO.REQUIRED):
        if not seen[f]:
            continue
        g.refill(res)
        if prepare is not None:
            prepare()
        with null((f,)) as calls:
            with pytest.raises(_lib.CopterStepError) as err:
                call()
        torch.cuda.synchronize()
        COUNT["refusals"] += 1
        assert calls[-1].rc == _lib.ERR_ARG == err.value.code and f.split(".")[1] in calls[-1].message, (f, calls[-1])
        for path, t, _ in full:
            assert _holds_fill(g, t), "%s refused for %s, but %s was written" % (entry, f, path)
        g.assert_bands_intact()
        assert _state(env) == before, "%s refused for %s, but the env state changed" % (entry, f)
    for _, t, clone in full:             # the caller goes on with the full call's values
        t.copy_(clone)
    return res


def _start(env, rng, force=False):
    x, st = MP._random_point(env.num_envs, rng)
    state = {"x": _dev(x, env), "status": _dev(st, env)}
    if force:
        state["force"] = _dev(rng.uniform(-1.0, 1.0, (3, env.num_envs)), env)
    return state


def _actions(env, steps, rng):
    return _dev((AH * rng.uniform(0.7, 1.3, (steps, env.num_envs, env.action_dim))).astype(np.float32), env)


def _copy(nt):
    return type(nt)(*(None if t is None else t.clone() for t in nt))


def _fields(prefix, nt):
    return {"%s_%s" % (prefix, f): t for f, t in zip(nt._fields, nt) if t is not None}


# ---------------------------------------------------------------------------------------------------------------------
def test_step_jacobian():
    """cs_step_jacobian at the stored state and at an explicit point with a pending force: 5 optional outputs, 12 calls
    each, and 5 more in float32.  It has no required output."""
    rng = np.random.default_rng(1)
    env = _env()
    try:
        env.reset()
        a = _actions(env, 1, rng)[0].contiguous()
        state = _start(env, rng, force=True)
        with guarded(N) as g:
            _sweep(env, g, "cs_step_jacobian", lambda: env.step_jacobian(a), dict(actions=a))
            _sweep(env, g, "cs_step_jacobian", lambda: env.step_jacobian(a, state=state), dict(actions=a, **state))
            _sweep(env, g, "cs_step_jacobian", lambda: env.step_jacobian(a, state=state, dtype=_f32()),
                   dict(actions=a, **state), subsets=("alone",))
    finally:
        env.close()


def test_open_loop_rollouts():
    """cs_rollout_states (stored start), cs_rollout_states_ex (vehicle override, explicit start with a force): 5 optional
    outputs, 12 calls each; cs_rollout_vjp (2: 4 calls; the stored start wires no g_x0: 2 calls) and cs_rollout_vjp_ex
    (4: 10 calls, through the plain sweep, the parameter sweep and the unfold kernel); the backwards once more in
    float32."""
    rng = np.random.default_rng(2)
    env = _env()
    try:
        env.reset()
        acts = _actions(env, K, rng)
        gx, gr = _dev(rng.standard_normal((K, N, 12)), env), _dev(rng.standard_normal((K, N)), env)
        forced = _start(env, rng, force=True)
        table = _dev(model_variants.vehicle_table(rng, N, mars=False), env)
        with guarded(N) as g:
            ro = _sweep(env, g, "cs_rollout_states", lambda: env.rollout_states(acts), dict(actions=acts))
            tape = _copy(ro)
            ins = dict(actions=acts, gx=gx, gr=gr, **_fields("ro", tape))
            _sweep(env, g, "cs_rollout_vjp", lambda: env.rollout_vjp(acts, tape, gx, gr), ins,
                   absent=["cs_rollout_io.g_x0_dev"])
            ro = _sweep(env, g, "cs_rollout_states_ex", lambda: env.rollout_states(acts, state=forced, vehicle=table),
                        dict(actions=acts, vehicle=table, **forced))
            tape_v = _copy(ro)
            tape_p = _copy(env.rollout_states(acts, state=forced))
            ins = dict(actions=acts, gx=gx, gr=gr, **forced, **_fields("ro", tape_p))
            for dt, subsets in ((None, ("alone", "only", "none")), (_f32(), ("alone",))):
                _sweep(env, g, "cs_rollout_vjp", lambda: env.rollout_vjp(acts, tape_p, gx, gr, state=forced, dtype=dt), ins,
                       subsets=subsets)
            ins = dict(actions=acts, gx=gx, gr=gr, vehicle=table, **forced, **_fields("ro", tape_v))
            for dt, subsets in ((None, ("alone", "only", "none")), (_f32(), ("alone",))):
                _sweep(env, g, "cs_rollout_vjp_ex",
                       lambda: env.rollout_vjp_params(acts, tape_v, gx, gr, state=forced, vehicle=table, dtype=dt), ins,
                       subsets=subsets)
    finally:
        env.close()


def test_mlp_rollouts():
    """cs_rollout_mlp_states (hidden 33, offsets, an explicit start: 6 optional outputs, 14 calls, and the refusal of a
    NULL actions_out_dev), cs_rollout_mlp_vjp and cs_rollout_mlp_vjp_ex (2 each: 4 calls, and in float32), and
    cs_mlp_param_grad (its one output is required: the repeat of the full call -- bit-identical: a split-K reduction in
    a fixed order -- and the refusal)."""
    rng = np.random.default_rng(3)
    env = _env()
    try:
        env.reset()
        hidden = 33
        theta = M._theta(TASK, hidden, seed=7, env=env)
        x, st = M._point(N, rng)
        state = {"x": _dev(x, env), "status": _dev(st, env)}
        off = _dev((0.01 * AH * rng.standard_normal((K, N, env.action_dim))).astype(np.float32), env)
        gx, gr = _dev(rng.standard_normal((K, N, 12)), env), _dev(rng.standard_normal((K, N)), env)
        gin = _dev(rng.standard_normal((K, N, env.action_dim)), env)
        with guarded(N) as g:
            r = _sweep(env, g, "cs_rollout_mlp_states",
                       lambda: env.rollout_mlp_states(theta, K, hidden, offsets=off, state=state),
                       dict(theta=theta, offsets=off, **state))
            tape = _copy(r)
            ins = dict(theta=theta, gx=gx, gr=gr, **state, **_fields("r", tape))
            for dt, subsets in ((None, ("alone", "only", "none")), (_f32(), ("alone",))):
                _sweep(env, g, "cs_rollout_mlp_vjp",
                       lambda: env.rollout_mlp_vjp(theta, tape, gx, gr, state=state, hidden=hidden, dtype=dt,
                                                   param_grad=False), ins, via="cs_rollout_mlp_vjp_ex", subsets=subsets)
                v = _sweep(env, g, "cs_rollout_mlp_vjp_ex",
                           lambda: env.rollout_mlp_vjp(theta, tape, gx, gr, state=state, hidden=hidden, dtype=dt,
                                                       param_grad=False, g_actions_in=gin),
                           dict(g_actions_in=gin, **ins), subsets=subsets)
            ga = v[1].clone()
            buf = env.mlp_param_grad(theta, hidden, tape.obs, ga)        # (a new tensor per call unless out= is given)
            _sweep(env, g, "cs_mlp_param_grad", lambda: env.mlp_param_grad(theta, hidden, tape.obs, ga, out=buf),
                   dict(theta=theta, obs=tape.obs, g_actions=ga))
    finally:
        env.close()


def test_lqr_and_feedback():
    """cs_rollout_lqr (6 optional outputs: 14 calls, and 6 in float32) and cs_rollout_feedback_states (5: 12 calls, and
    the refusal of a NULL actions_out_dev)."""
    rng = np.random.default_rng(4)
    env = _env()
    try:
        env.reset()
        acts, state = _actions(env, K, rng), _start(env, rng)
        Q, Qf, R, q, r = L._cost_model(rng, env.action_dim, K, N)
        q, r = _dev(q, env), _dev(r, env)
        ro = _copy(env.rollout_states(acts, state=state))
        alpha = _dev(rng.uniform(0.1, 1.0, N), env)
        ins = dict(actions=acts, q=q, r=r, **state, **_fields("ro", ro))
        with guarded(N) as g:
            lqr = lambda dt: env.rollout_lqr(acts, ro, Q, R, q=q, r=r, Q_final=Qf, mu=1e-3, state=state, dtype=dt)  # noqa: E731
            gains = _copy(_sweep(env, g, "cs_rollout_lqr", lambda: lqr(None), ins))
            _sweep(env, g, "cs_rollout_lqr", lambda: lqr(_f32()), ins, subsets=("alone",))
            _sweep(env, g, "cs_rollout_feedback_states", lambda: env.rollout_feedback_states(acts, ro, gains, alpha, state=state),
                   dict(alpha=alpha, **ins, **_fields("gains", gains)))
    finally:
        env.close()


def _filter_problem(env, seed):
    return E._problem(env, TASK, np.random.default_rng(seed), M=3, missing=0.1, steps=K)


@pytest.mark.parametrize("gyro", [False, True], ids=["plain", "gyro"])
def test_ekf(gyro):
    """cs_rollout_ekf with the covariance tape: 10 optional outputs (x, status and the block's eight), 22 calls; 10 more
    in float32; the GYRO instantiation once (each nulled alone).  P_tape and P present or absent run the two wave_sync()
    sequences of filter_store_row on the last and on the other rows."""
    env = _env(**(model_variants.env_kwargs("gyro_only") if gyro else {}))
    try:
        p = _filter_problem(env, 5)
        grp = np.asarray(p["grp"])
        assert (grp == "landed").any() and (grp == "crashed").any() and (grp == "hover").any()
        assert bool(p["z"].isnan().any())
        ins = dict(actions=p["acts"], z=p["z"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        with guarded(N) as g:
            _sweep(env, g, "cs_rollout_ekf", lambda: E._run(env, p, tape=True), ins,
                   subsets=("alone",) if gyro else ("alone", "only", "none"))
            if not gyro:
                _sweep(env, g, "cs_rollout_ekf", lambda: E._run(env, p, tape=True, dtype=_f32()), ins, subsets=("alone",))
    finally:
        env.close()


@pytest.mark.parametrize("gyro", [False, True], ids=["plain", "gyro"])
def test_rts(gyro):
    """cs_rollout_rts over the filter's tapes, without and with the caller's end row: 6 optional outputs (x and the
    block's five), 14 calls each; 6 more in float32; the GYRO instantiation once (each nulled alone)."""
    env = _env(**(model_variants.env_kwargs("gyro_only") if gyro else {}))
    try:
        p = _filter_problem(env, 6)
        ft = _copy(E._run(env, p, tape=True))
        end = (ft.x[K - 1].t().contiguous(), ft.P.clone())
        ins = dict(actions=p["acts"], x0=p["x0"], P0=p["P0"], status0=p["st0"], **_fields("filt", ft))
        rts = lambda **kw: env.rollout_rts(p["acts"], ft, p["Q"], p["x0"], p["P0"], status0=p["st0"], **kw)   # noqa: E731
        with guarded(N) as g:
            _sweep(env, g, "cs_rollout_rts", lambda: rts(), ins, subsets=("alone",) if gyro else ("alone", "only", "none"))
            if not gyro:
                _sweep(env, g, "cs_rollout_rts", lambda: rts(end=end), dict(end_x=end[0], end_P=end[1], **ins))
                _sweep(env, g, "cs_rollout_rts", lambda: rts(dtype=_f32()), ins, subsets=("alone",))
    finally:
        env.close()


@pytest.mark.parametrize("gyro", [False, True], ids=["plain", "gyro"])
def test_pf(gyro):
    """cs_rollout_pf with 64 particles and every tape, from the Gaussian start and from carried particles: 17 optional
    outputs, 36 calls each; 17 more in float32; the GYRO instantiation once (each nulled alone).  P_dev present or absent
    changes the __syncthreads() of the last step."""
    env = _env(**(model_variants.env_kwargs("gyro_only") if gyro else {}))
    try:
        p = _filter_problem(env, 7)
        pf = lambda **kw: env.rollout_pf(p["acts"], p["z"], p["H"], p["r"], p["Q"], particles=64, nonce=7,      # noqa: E731
                                         ess_frac=0.5, tape=True, **kw)
        gauss = dict(x0=p["x0"], P0=p["P0"], status0=p["st0"])
        ins = dict(actions=p["acts"], z=p["z"])
        with guarded(N) as g:
            first = _sweep(env, g, "cs_rollout_pf", lambda: pf(**gauss), dict(ins, **gauss),
                           subsets=("alone",) if gyro else ("alone", "only", "none"))
            if not gyro:
                start = (first.part.clone(), first.pstatus.clone(), first.lw.clone())
                carried = dict(ins, part=start[0], pstatus=start[1], lw=start[2])
                _sweep(env, g, "cs_rollout_pf", lambda: pf(start=start, first_step=K + 1), carried)
                _sweep(env, g, "cs_rollout_pf", lambda: pf(dtype=_f32(), **gauss), dict(ins, **gauss), subsets=("alone",))
    finally:
        env.close()


@pytest.mark.parametrize("gyro", [False, True], ids=["plain", "gyro"])
def test_lqg(gyro):
    """cs_rollout_lqg with the covariance tape, an explicit start with a pending force: 16 optional outputs (the truth's
    five, z and the filter's ten), 34 calls; 16 more in float32; the GYRO instantiation once (each nulled alone); the
    refusal of a NULL actions_out_dev."""
    env = _env(**(model_variants.env_kwargs("gyro_only") if gyro else {}))
    try:
        env.reset()
        p = LQ._problem(env, TASK, np.random.default_rng(8), steps=K, M=3, missing=0.1)
        ins = dict(actions=p.abar, gains=p.gains, xbar=p.xbar, noise=p.e, xhat0=p.xhat0, P0=p.P0, status0=p.fst0,
                   **{"state_" + k: v for k, v in p.state.items()})
        with guarded(N) as g:
            _sweep(env, g, "cs_rollout_lqg", lambda: LQ._run(env, p, tape=True), ins,
                   subsets=("alone",) if gyro else ("alone", "only", "none"))
            if not gyro:
                _sweep(env, g, "cs_rollout_lqg", lambda: LQ._run(env, p, tape=True, dtype=_f32()), ins, subsets=("alone",))
    finally:
        env.close()


@pytest.mark.parametrize("gyro", [False, True], ids=["plain", "gyro"])
def test_ukf(gyro):
    """cs_rollout_ukf with the covariance tape and the point tapes: 13 optional outputs, 28 calls; 13 more in float32;
    the GYRO instantiation once (each nulled alone).  LANDED lanes write the point tapes on their other path."""
    env = _env(**(model_variants.env_kwargs("gyro_only") if gyro else {}))
    try:
        env.reset()
        p = U._problem(env, U.inputs(TASK, N, K, seed=9, M=3, missing=0.1))
        assert (np.asarray(p["grp"]) == "landed").any() and bool(p["z"].isnan().any())
        ins = dict(actions=p["acts"], z=p["z"], x0=p["x0"], P0=p["P0"], status0=p["st0"])
        with guarded(N) as g:
            _sweep(env, g, "cs_rollout_ukf", lambda: U._run(env, p, tape=True, points=True), ins,
                   subsets=("alone",) if gyro else ("alone", "only", "none"))
            if not gyro:
                _sweep(env, g, "cs_rollout_ukf", lambda: U._run(env, p, tape=True, points=True, dtype=_f32()), ins,
                       subsets=("alone",))
    finally:
        env.close()


def test_mppi():
    """5 samples, white noise (cs_rollout_mppi_costs / _update) and knots (the _ex forms): best_dev (1 optional output:
    with and without the arg-min kernel), ess_dev and cost_min_dev (2: 4 calls), cs_rollout_mppi_temperature's ess_out_dev
    (1); the refusals of a NULL costs_dev, actions_out_dev and lam_out_dev.  Their outputs are float64 or integers."""
    import gym_copter_amd
    rng = np.random.default_rng(10)
    env = _env()
    try:
        env.reset()
        A, P, sigma = env.action_dim, 5, 0.2 * AH
        acts, state = _actions(env, K, rng), _start(env, rng)
        Q, Qf, R, x_ref, a_ref = MP._cost_model(rng, A, N)
        x_ref = _dev(x_ref, env)
        knots = gym_copter_amd.mppi_knots(K, 2)
        with guarded(N) as g:
            for entry, kn in (("cs_rollout_mppi_costs", None), ("cs_rollout_mppi_costs_ex", knots)):
                c = _sweep(env, g, entry,
                           lambda: env.rollout_mppi_costs(acts, sigma, P, x_ref, Q, R, Q_final=Qf, a_ref=a_ref,
                                                          reward_weight=0.1, stream=3, state=state, knots=kn),
                           dict(actions=acts, x_ref=x_ref, **state))
                costs = c.costs.clone()
                _sweep(env, g, entry.replace("costs", "update"),
                       lambda: env.rollout_mppi_update(acts, costs, sigma, 50.0, stream=3, knots=kn),
                       dict(actions=acts, costs=costs))
            _sweep(env, g, "cs_rollout_mppi_temperature", lambda: env.rollout_mppi_temperature(costs, 3.0), dict(costs=costs))
    finally:
        env.close()


def test_population_and_es():
    """cs_rollout_mlp_population with 2 members x 64 envs, from the stored and from an explicit start: 4 optional outputs
    (member_returns_dev decides whether the reduction kernel is launched), 10 calls each, and the refusal of a NULL
    returns_dev; cs_es_perturb and cs_es_gradient (one required output each: the repeat -- cs_es_gradient's chunked sum
    is bit-repeatable -- and the refusal)."""
    members, E_, hidden, n = 2, 64, 33, 128
    rng = np.random.default_rng(11)
    env = _env(n)
    try:
        env.reset()
        table = _dev(ES._table(TASK, members, hidden, rng), env)
        x, st = ES._low_starts(n, rng)
        x, st = _dev(x, env), _dev(st, env)
        theta = _dev(rng.standard_normal(65).astype(np.float32), env)
        w = _dev(rng.standard_normal(6), env)
        with guarded(n) as g:
            _sweep(env, g, "cs_rollout_mlp_population", lambda: env.rollout_mlp_population(table, K, hidden, E_, gamma=0.99),
                   dict(table=table))
            _sweep(env, g, "cs_rollout_mlp_population",
                   lambda: env.rollout_mlp_population(table, K, hidden, E_, start_x=x, start_status=st),
                   dict(table=table, start_x=x, start_status=st))
            _sweep(env, g, "cs_es_perturb", lambda: env.es_perturb(theta, 0.05, 6, nonce=9, pair_base=5), dict(params=theta))
            _sweep(env, g, "cs_es_gradient", lambda: env.es_gradient(w, 9, 65, pair_base=5), dict(weights=w))
    finally:
        env.close()


def test_actor_critic_gae_and_ppo_grad():
    """cs_rollout_actor_critic without and with a critic (means_dev is its one optional output: 2 calls each; every
    other tape is required: 6 and 7 refusals, values_dev among them with the critic); the env is set back to its start
    before every call, and every call must leave it where the full call left it.  cs_gae and cs_ppo_grad (with and
    without a critic) have required outputs only: the repeat of the full call, bit-identical (cs_ppo_grad's partials are
    added in index order), and the refusals."""
    rng = np.random.default_rng(12)
    env = _env(autoreset="next_step")
    try:
        env.reset()
        H, Hv = 33, 16
        actor, critic, log_std = AC._policy(TASK, H, Hv, int(rng.integers(1 << 30)), env)
        start = env.get_state()
        back = lambda: env.set_state(**start)                                                        # noqa: E731
        with guarded(N) as g:
            _sweep(env, g, "cs_rollout_actor_critic", lambda: env.rollout_actor_critic(actor, None, log_std, K, H, means=True),
                   dict(actor=actor, log_std=log_std), prepare=back)
            r = _sweep(env, g, "cs_rollout_actor_critic",
                       lambda: env.rollout_actor_critic(actor, critic, log_std, K, H, critic_hidden=Hv, nonce=5, means=True),
                       dict(actor=actor, critic=critic, log_std=log_std), prepare=back)
            assert r.values is not None and r.means is not None
            tapes = dict(reward=r.reward.clone(), values=r.values.clone(), terminated=r.terminated.clone(),
                         truncated=r.truncated.clone())
            _sweep(env, g, "cs_gae", lambda: env.gae(tapes["reward"], tapes["values"], tapes["terminated"], tapes["truncated"]),
                   tapes)
            for hv in (16, None):
                s = pur.to_device(pur.synthetic(TASK, 16, hv, pur.DEGENERATE_R, 1), env.device)
                idx = s["perm"][:37].contiguous()
                ins = {k: s[k] for k in ("actor", "critic", "log_std", "obs", "actions", "logp", "advantages", "returns", "live")}
                ppo = lambda **kw: env.ppo_grad(s["actor"], s["critic"], s["log_std"], 16, hv, s["obs"], s["actions"],   # noqa: E731
                                                s["logp"], s["advantages"], s["returns"], live=s["live"], index=idx,
                                                ent_coef=0.01, **kw)
                buf = ppo()                                              # (new tensors per call unless out= is given)
                _sweep(env, g, "cs_ppo_grad", lambda: ppo(out=buf.grad, stats_out=buf.stats), dict(index=idx, **ins))
    finally:
        env.close()


def test_every_tabled_entry_point_was_swept():
    """the table's rows against the sweeps above: a later entry point is not forgotten here (cs_rollout_pid and
    cs_rollout_random take bare pointers and belong to the step family's tests)"""
    import inspect
    import sys
    source = inspect.getsource(sys.modules[__name__])
    for entry, row in NO.TABLE.items():
        if row.blocks:
            assert '"%s"' % entry in source or entry.replace("update", "costs") in source, entry
