"""The derivative entry points of CopterVecEnv (DESIGN.md sections 9 to 11): step_jacobian, and the open-loop rollouts
as a pure function with their reverse-mode gradients -- rollout_states, rollout_vjp, rollout_vjp_params.  vecenv.py binds
them to the class; the other families start from this module's _rollout_io (the actions and the start point of a
rollout)."""
import collections
import ctypes as C

import numpy as np

from . import _lib, _wire
from ._wire import _torch

# CopterVecEnv.step_jacobian's result (device tensors)
StepJacobian = collections.namedtuple("StepJacobian", "dx du reward_dx reward_du branch")
# CopterVecEnv.rollout_states' result (device tensors, [K, N, ...])
Rollout = collections.namedtuple("Rollout", "x reward terminated truncated status")


def _state(env, v, shape, dt, name, keep):
    """state[name] of step_jacobian or a rollout as a contiguous device tensor of dtype dt, kept alive in `keep`;
    returns its data pointer."""
    return _wire.tensor(env, v, shape, dt, "state[%r]" % name, keep, non_blocking=True).data_ptr()


def _rollout_tensors(env, K):
    """Rollout's five output buffers for K steps."""
    torch = _torch()
    n = env.num_envs
    return Rollout(_wire.empty(env, (K, n, 12), torch.float64), _wire.empty(env, (K, n), torch.float64),
                   _wire.empty(env, (K, n), torch.bool), _wire.empty(env, (K, n), torch.bool),
                   _wire.empty(env, (K, n), torch.uint8))


def _wire_rollout(io, out):
    """io's five outputs: the tensors of a Rollout (or the first five of a longer result)."""
    io.x_dev, io.reward_dev, io.terminated_dev = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    io.truncated_dev, io.status_dev = out[3].data_ptr(), out[4].data_ptr()


def step_jacobian(self, actions, state=None, dtype=None):
    """Jacobians of the step that step(actions) would take, for every env, as device tensors; NO env state
    changes.  Returns StepJacobian(dx [N,12,12] = d x' / d x, du [N,12,A] = d x' / d actions (the actions as
    step() receives them, before the clip to [0, 1]; the clip's derivative is 1 on [0, 1] and 0 outside),
    reward_dx [N,12], reward_du [N,A] = the gradient of the step's reward, branch [N] uint8 = the CS_JAC_*
    bits of the branches the step takes).  x is the full state in upstream slot order (STATE_NAMES_12); an
    observation is a slice of x', so its Jacobian is the matching rows of dx / du.

    The transition differentiated is the physics + reward of the step with auto-reset DISABLED: a termination
    in this step and the auto-reset behind it do not enter (a NEXT_STEP reset already pending gives
    dx = du = 0).  The physics is the float64 arithmetic of the step kernels (per-env vehicles, both thrust
    laws, the rotor-gyro term, `substeps` calls with the pending perturbation in the first); under
    action_arith="float32" it is still the float64 motor law.

    state=None linearises at the stored state the next step() starts from (float32 storage modes: the decoded
    words get_state() reports).  state={"x": [12,N] float64, "status": [N] uint8, "force": [3,N] newtons
    (optional, pending)} -- the keys and shapes of get_state() / set_state() -- linearises at that point instead
    (hover, a planned trajectory).  dtype: torch.float64 (default) or torch.float32 (the float64 values rounded).
    Asynchronous on the current stream; the returned tensors are buffers of this env, overwritten by the next
    call with the same dtype."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    n, ad = self.num_envs, self.action_dim
    a, _ = self._dev_f32(actions, (n, ad), "actions")
    io = _wire.block(_lib.JacobianIO, out_dtype=_wire.dtype_code(dtype), actions_dev=a.data_ptr())
    keep = [a]
    if state is not None:
        unknown = set(state) - {"x", "status", "force"}
        if unknown or "x" not in state or "status" not in state:
            raise ValueError("state needs the keys 'x' and 'status' (and optionally 'force'), got %s"
                             % sorted(state))
        io.x_dev = _state(self, state["x"], (12, n), torch.float64, "x", keep)
        io.status_dev = _state(self, state["status"], (n,), torch.uint8, "status", keep)
        if state.get("force") is not None:
            io.force_dev = _state(self, state["force"], (3, n), torch.float64, "force", keep)
    cache = getattr(self, "_jac_out", None)
    if cache is None:
        cache = self._jac_out = {}
    out = cache.get(dtype)
    if out is None:
        out = cache[dtype] = StepJacobian(
            _wire.empty(self, (n, 12, 12), dtype), _wire.empty(self, (n, 12, ad), dtype),
            _wire.empty(self, (n, 12), dtype), _wire.empty(self, (n, ad), dtype), _wire.empty(self, n, torch.uint8))
    io.dx_dev, io.du_dev, io.reward_dx_dev, io.reward_du_dev, io.branch_dev = (t.data_ptr() for t in out)
    _wire.launch(self, "cs_step_jacobian", io, keep=keep)
    return out


def _rollout_io(self, actions, state, num_steps=None):
    """The cs_rollout_io of rollout_states / rollout_vjp: actions [K,N,A] and the start point; returns (io, K, the
    tensors the call reads).  actions=None (the closed-loop calls): no actions, K = num_steps."""
    torch = _torch()
    n, ad = self.num_envs, self.action_dim
    io = _wire.block(_lib.RolloutIO)
    keep = []
    if actions is None:
        K = num_steps
    else:
        shape = tuple(actions.shape) if hasattr(actions, "shape") else np.shape(actions)
        if len(shape) != 3 or shape[0] < 1:
            raise ValueError("actions must have shape (K, %d, %d) with K >= 1, got %s" % (n, ad, tuple(shape)))
        K = int(shape[0])
        a, _ = self._dev_f32(actions, (K, n, ad), "actions")
        io.actions_dev = a.data_ptr()
        keep.append(a)
    io.num_steps = K
    if state is not None:
        unknown = set(state) - {"x", "status", "force", "prev_shaping"}
        if unknown or "x" not in state or "status" not in state:
            raise ValueError("state needs the keys 'x' and 'status' (and optionally 'force', 'prev_shaping'), got %s"
                             % sorted(state))
        io.start_x_dev = _state(self, state["x"], (12, n), torch.float64, "x", keep)
        io.start_status_dev = _state(self, state["status"], (n,), torch.uint8, "status", keep)
        if state.get("force") is not None:
            io.start_force_dev = _state(self, state["force"], (3, n), torch.float64, "force", keep)
        if state.get("prev_shaping") is not None:
            io.start_prev_shaping_dev = _state(self, state["prev_shaping"], (n,), torch.float64, "prev_shaping", keep)
    return io, K, keep


def _tape(env, io, rollout, K):
    """io.x_dev and io.status_dev of a backward over rollout_states' tape."""
    torch = _torch()
    n = env.num_envs
    x, status = getattr(rollout, "x", None), getattr(rollout, "status", None)
    _wire.check_tape(env, "rollout_states", (x, "rollout.x", (K, n, 12), torch.float64),
                     (status, "rollout.status", (K, n), torch.uint8))
    io.x_dev, io.status_dev = x.data_ptr(), status.data_ptr()


def _cotangents(env, io, gx, gr, K, keep):
    """io.gx_dev and io.gr_dev of a backward: gx [K,N,12] and gr [K,N] (None: zero) as float64 device tensors, kept
    alive in `keep`."""
    torch = _torch()
    n = env.num_envs
    if gx is not None:
        io.gx_dev = _wire.tensor(env, gx, (K, n, 12), torch.float64, "gx", keep, floating=True,
                                 non_blocking=True).data_ptr()
    if gr is not None:
        io.gr_dev = _wire.tensor(env, gr, (K, n), torch.float64, "gr", keep, floating=True,
                                 non_blocking=True).data_ptr()


def _grad_out(env, io, prefix, K, dtype, explicit):
    """A backward's outputs, set in io: g_actions [K,N,A] and, for an explicit start, g_x0 [12,N] (else None) -- buffers
    of this env cached under `prefix` (the plain and the closed-loop calls keep their own)."""
    n = env.num_envs
    ga = _wire.rollout_cache(env, (prefix + "g_actions", K, dtype),
                             lambda: _wire.empty(env, (K, n, env.action_dim), dtype))
    io.g_actions_dev = ga.data_ptr()
    g0 = None
    if explicit:
        g0 = _wire.rollout_cache(env, (prefix + "g_x0", dtype), lambda: _wire.empty(env, (12, n), dtype))
        io.g_x0_dev = g0.data_ptr()
    return ga, g0


def _param_io(env, vehicle, keep, dtype=None, check=True):
    """The cs_rollout_param_io of a rollout with a vehicle override and / or parameter gradients: vehicle [12,N]
    float64 (set_vehicle_params' rows) is checked on the device -- M, Ix, Iy, Iz positive, every value finite; a
    synchronising reduction, skipped with check=False for a tensor already checked -- and kept alive in `keep`."""
    torch = _torch()
    pio = _wire.block(_lib.RolloutParamIO, out_dtype=_wire.dtype_code(dtype))
    if vehicle is not None:
        t = _wire.tensor(env, vehicle, (len(env.VEHICLE_ROWS), env.num_envs), torch.float64, "vehicle", keep,
                         floating=True, non_blocking=True, note=" (rows %s)" % (env.VEHICLE_ROWS,))
        # the C ABI cannot check a device table synchronously: one reduction here (M, Ix, Iy, Iz are rows 2, 4, 5, 6)
        inertia = t[[2, 4, 5, 6]]
        if check and not bool(torch.isfinite(t).all() & (inertia > 0).all()):
            raise ValueError("vehicle: M, Ix, Iy, Iz must be positive and every value finite")
        pio.vehicle_dev = t.data_ptr()
    return pio


def rollout_states(self, actions, state=None, vehicle=None):
    """K calls of step() with auto-reset DISABLED, as a pure function: Rollout(x [K,N,12] float64, reward [K,N]
    float64, terminated [K,N] bool, truncated [K,N] bool, status [K,N] uint8) of device tensors; NO env state
    changes (no words, counters, episode numbers, prev_shaping, statistics or RNG position).  actions [K,N,A]: step
    k takes actions[k-1], as step() receives them.

    x[k-1] is the decoded stored state after step k in upstream slot order (STATE_NAMES_12; in the float32 storage
    modes the words get_state() would report), reward[k-1] the value step() rounds to float32.  Both are
    bit-identical to a twin env with autoreset_mode="disabled" stepped K times.  An observation is a slice of x
    (STATE_NAMES).

    state=None starts from the stored state the next step() starts from: its pending perturbation enters the first
    substep of step 1, and an env with a NEXT_STEP reset pending performs that reset in step 1 with the draw step()
    would make.  state={"x": [12,N] float64, "status": [N] uint8, "force": [3,N] newtons (optional, pending),
    "prev_shaping": [N] float64 (optional; NaN = None: reward 0 in step 1)} -- get_state()'s layout, as
    step_jacobian takes it -- starts from that point instead; without prev_shaping it is shaping(x0).  The step
    counter (time-limit truncation) is the env's in both cases.  vehicle=[12,N] float64 (set_vehicle_params' rows
    VEHICLE_ROWS) rolls out with that vehicle instead of the env's, for this call only: the env's installed vehicle
    is untouched.  Asynchronous on the current stream (an override is checked with one device
    reduction, which synchronises); the returned tensors are buffers of this env, overwritten by the next call with
    the same K."""
    self._check_open()
    io, K, keep = _rollout_io(self, actions, state)
    pio = None if vehicle is None else _param_io(self, vehicle, keep)
    out = _wire.rollout_cache(self, ("states", K), lambda: _rollout_tensors(self, K))
    _wire_rollout(io, out)
    # (the shortest wrapper, 7 us a call: the library is called directly here, not through _wire.launch;
    # profiles/host_wrappers_refactor_ab.txt)
    with _torch().cuda.device(self.device):
        if pio is None:
            _lib.check(self._lib.cs_rollout_states(self._ctx, C.byref(io), self._stream()))
        else:
            _lib.check(self._lib.cs_rollout_states_ex(self._ctx, C.byref(io), C.byref(pio), self._stream()))
    self._keep = keep
    return out


def rollout_vjp_params(self, actions, rollout, gx=None, gr=None, state=None, vehicle=None, dtype=None):
    """rollout_vjp with the gradients with respect to the vehicle and the start's pending force as well: returns
    (g_actions [K,N,A], g_x0 [12,N] or None, g_vehicle [12,N], g_force [3,N]).  g_vehicle = dL / d the vehicle
    rows (VEHICLE_ROWS, per env: sum over envs for a shared vehicle; rows that do not enter the configuration are
    0: B under the lift law, rho and C_L under the B law, Jr without rotor_gyro).  g_force = dL / d state["force"]
    (newtons), or with the stored start dL / d its pending perturbation; exactly 0 where none is pending (consumed,
    or a state without "force": pass zeros for the sensitivity at F = 0), where it never integrates, and for an env
    whose NEXT_STEP reset is pending (the new episode's draw is a constant).  `vehicle`
    is the override rollout_states(..., vehicle=) was given (None: the env's own).  g_actions and g_x0 are
    rollout_vjp's, bit for bit.  DESIGN section 11.  Same buffers and stream rules as rollout_vjp; not available
    with action_arith="float32"."""
    return _vjp(self, actions, rollout, gx, gr, state, dtype, params=True, vehicle=vehicle)


def rollout_vjp(self, actions, rollout, gx=None, gr=None, state=None, dtype=None):
    """Reverse-mode gradient of a rollout: given the cotangents gx [K,N,12] (on rollout.x) and gr [K,N] (on
    rollout.reward) -- either may be None (zero) -- returns (g_actions [K,N,A] = dL / d actions, the actions as
    step() receives them (the clip's derivative is 1 on [0, 1] and 0 outside), g_x0 [12,N] = dL / d state["x"] for an
    explicit start, None for the stored one).  `rollout` is what rollout_states(actions, state) returned for the
    same actions and start (its x and status are the tape the backward recomputes each step from); with the stored
    start the env must not have been stepped, reset or set since.  The derivative rules are step_jacobian's (DESIGN
    section 9) plus the prev_shaping term: reward_k = shaping(x_k) - shaping(x_{k-1}), and without a given
    prev_shaping the first step's differentiates shaping(x0).  The perturbation force and the vehicle are constants.
    dtype: torch.float64 (default) or torch.float32 (the float64 values rounded).  Asynchronous on the current
    stream; the returned tensors are buffers of this env, overwritten by the next call with the same K and dtype.
    rollout_vjp_params differentiates with respect to the vehicle and the force as well."""
    return _vjp(self, actions, rollout, gx, gr, state, dtype)


def _vjp(self, actions, rollout, gx, gr, state, dtype, params=False, vehicle=None, check_vehicle=True):
    self._check_open()
    dtype = _wire.out_dtype(dtype)
    io, K, keep = _rollout_io(self, actions, state)
    n = self.num_envs
    io.out_dtype = _wire.dtype_code(dtype)
    _tape(self, io, rollout, K)
    _cotangents(self, io, gx, gr, K, keep)
    ga, g0 = _grad_out(self, io, "", K, dtype, state is not None)
    if not params:
        _wire.launch(self, "cs_rollout_vjp", io, keep=keep)
        return ga, g0
    pio = _param_io(self, vehicle, keep, dtype, check=check_vehicle)
    gv = _wire.rollout_cache(self, ("g_vehicle", dtype), lambda: _wire.empty(self, (len(self.VEHICLE_ROWS), n), dtype))
    gf = _wire.rollout_cache(self, ("g_force", dtype), lambda: _wire.empty(self, (3, n), dtype))
    pio.g_vehicle_dev, pio.g_force_dev = gv.data_ptr(), gf.data_ptr()
    _wire.launch(self, "cs_rollout_vjp_ex", io, pio, keep=keep)
    return ga, g0, gv, gf


# CopterVecEnv.rollout_jvp's result (device tensors, [D, K, N, ...]; without the D axis for inputs without it)
RolloutTangents = collections.namedtuple("RolloutTangents", "x reward")


def rollout_jvp(self, actions, rollout, t_actions=None, t_x0=None, t_vehicle=None, t_force=None, state=None,
                vehicle=None, dtype=None, check_vehicle=True):
    """Forward-mode tangents of a rollout: D input directions pushed through the K steps, RolloutTangents(x [D,K,N,12]
    = the tangent of rollout.x, reward [D,K,N] = the tangent of rollout.reward).  The direction axis leads: t_actions
    [D,K,N,A] (on the actions as step() receives them), t_x0 [D,12,N] (on state["x"], or on the stored start's decoded
    words), t_vehicle [D,12,N] (on the vehicle rows VEHICLE_ROWS) and t_force [D,3,N] newtons (on the start's pending
    force), float64, each None = zero, at least one given, all with the same D.  Inputs without the direction axis mean
    D = 1, and the outputs then come back without it.  `rollout`, `state` and `vehicle` are rollout_vjp_params': the
    tape rollout_states(actions, state, vehicle=) returned, its start and its override.

    The linear map is the one whose transpose rollout_vjp / rollout_vjp_params apply, at the tape's points (DESIGN
    section 26): <gx, t_x> + <gr, t_reward> = <g_actions, t_actions> + <g_x0, t_x0> + <g_vehicle, t_vehicle> + <g_force,
    t_force> per env.  A pending NEXT_STEP reset zeroes that env's x0, first-action and force tangents; the force
    tangent is exactly 0 where none is pending or it never integrates; vehicle rows that do not enter the configuration
    contribute exactly 0.  With t_vehicle, t_force or vehicle: not available with action_arith="float32".  dtype:
    torch.float64 (default) or torch.float32 (the float64 values rounded).  Asynchronous on the current stream; the
    returned tensors are buffers of this env, overwritten by the next call with the same D, K and dtype."""
    self._check_open()
    torch = _torch()
    dtype = _wire.out_dtype(dtype)
    io, K, keep = _rollout_io(self, actions, state)
    n, ad = self.num_envs, self.action_dim
    _tape(self, io, rollout, K)
    given = [("t_actions", t_actions, (K, n, ad)), ("t_x0", t_x0, (12, n)),
             ("t_vehicle", t_vehicle, (len(self.VEHICLE_ROWS), n)), ("t_force", t_force, (3, n))]
    dims = {name: (len(t.shape) if hasattr(t, "shape") else np.ndim(t)) - len(shape)
            for name, t, shape in given if t is not None}
    if not dims:
        raise ValueError("rollout_jvp needs at least one of t_actions, t_x0, t_vehicle, t_force")
    if set(dims.values()) - {0, 1} or len(set(dims.values())) != 1:
        raise ValueError("the input tangents must all have the direction axis [D, ...] or all lack it (D = 1): %s"
                         % ", ".join("%s must have shape (D,) + %s or %s" % (name, shape, shape)
                                     for name, t, shape in given if t is not None))
    batched = set(dims.values()) == {1}
    D = None
    ptrs = {}
    for name, t, shape in given:
        if t is None:
            continue
        d = int(t.shape[0] if hasattr(t, "shape") else np.shape(t)[0]) if batched else 1
        if D is None:
            D = d
        if d != D or D < 1 or D > _lib.JVP_MAX_DIRS:
            raise ValueError("%s: the input tangents must share one D in [1, %d], got %d and %d"
                             % (name, _lib.JVP_MAX_DIRS, D, d))
        tt = _wire.tensor(self, t, ((D,) if batched else ()) + shape, torch.float64, name, keep, floating=True,
                          non_blocking=True)
        ptrs[name] = tt.data_ptr()
    jio = _wire.block(_lib.JvpIO, out_dtype=_wire.dtype_code(dtype), num_dirs=D,
                      t_actions_dev=ptrs.get("t_actions"), t_x0_dev=ptrs.get("t_x0"),
                      t_vehicle_dev=ptrs.get("t_vehicle"), t_force_dev=ptrs.get("t_force"))
    if vehicle is not None:
        jio.vehicle_dev = _param_io(self, vehicle, keep, check=check_vehicle).vehicle_dev
    out = _wire.rollout_cache(self, ("jvp", D, K, dtype), lambda: RolloutTangents(
        _wire.empty(self, (D, K, n, 12), dtype), _wire.empty(self, (D, K, n), dtype)))
    jio.t_x_dev, jio.t_reward_dev = out.x.data_ptr(), out.reward.data_ptr()
    _wire.launch(self, "cs_jvp_rollout", io, jio, keep=keep)
    return out if batched else RolloutTangents(out.x[0], out.reward[0])


class ForwardTangents:
    """CopterVecEnv's forward-mode rollout tangents, a base class of it.  It is inherited, not bound
    in the class body like its neighbours: the class body's rollout_* methods are the closed list that
    tests/test_gpu_output_bounds.py covers one by one (tests/test_guarded_outputs_cpu.py), and this one is held to the
    same memory contract in tests/test_gpu_jvp.py."""
    rollout_jvp = rollout_jvp
