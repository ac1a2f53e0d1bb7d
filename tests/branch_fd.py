"""Branch-aware central differences of the float64 oracle: the checker of the device gradients (step_jacobian,
rollout_vjp, rollout_vjp_params, rollout_mlp_vjp) through touchdowns, crashes, tilts, bounds, the |dz| penalty and
clipped motors -- the places where a derivative rule, not the smooth flight dynamics, decides the answer.

Layout as in tests/jacobian_fd.py / rollout_fd.py: every perturbed copy of every env is a lane of ONE oracle batch.
Here the batch holds the base run, the +-h copies and the +-2h copies of each of the D input directions:
lane = r n + env with r = 0 the base and r = 1 + 2 (j D + d) + s (j = 0: h, 1: 2h; s = 0: +, 1: -).

The per-lane stability verdict is the oracle's alone, never the device's answer.  An env is kept only if
  - every copy has the base run's discrete signature: the status, terminated and truncated flags after every step,
    the outcome of every setMotors call inside every step (RecordingOracle: integrated, froze on contact, levelled,
    took off, held), the clip side of every action, and the out-of-bounds, tilt, |dz| > dz_max and inside-radius
    tests of the stored state after every step (and of the start);
  - the central differences at h and at 2h agree within AGREE, scaled by max(1, |gradient|).
Where both hold, the function is smooth through the step sequence of the base run, and its central difference is the
derivative the branch rules of DESIGN sections 9-12 define."""
from collections import namedtuple

import numpy as np

from jacobian_fd import VEHICLE_FIELDS
from mlp_rollout_fd import OBS_SHAPE, policy64
from oracle.refcpu import AIRBORNE, CRASHED, DJI_PHANTOM, G, LANDED, LEVELING, TaskParams, VehicleParams, \
    task_action_dim
from oracle.refvec import VecOracle

AGREE = 1e-7
# the step of the K-step differences: at 1e-6 the rounding of 16 float64 steps (~1e-7 scaled at 10 m, 10 m/s) alone
# fills the h / 2h agreement budget; at 4e-6 both it and the truncation error stay well inside it
H_ROLLOUT = 4e-6
INACTIVE = 255            # a call of a lane whose step does not run the physics (LANDED at the start)
TOOK_OFF = LANDED * 4 + AIRBORNE      # call code (status before) * 4 + (status after)
LEVELLED = LEVELING * 4 + LANDED
ROWS = ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm", "G", "rho", "C_L")   # set_vehicle_params' rows


class RecordingOracle(VecOracle):
    """VecOracle that records, for every Dynamics.setMotors call, (status before) * 4 + (status after) per lane, or
    INACTIVE.  The pair names the call's branch: AIRBORNE -> AIRBORNE integrated, AIRBORNE -> LEVELING / CRASHED froze
    on contact (soft / hard), LEVELING -> LANDED levelled, CRASHED -> CRASHED held, LANDED -> LANDED held, LANDED ->
    AIRBORNE took off and integrated, LANDED -> LEVELING / CRASHED took off into a contact."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.calls = []

    def _physics(self, x, status, pend, k, motors, active):
        before = status.astype(np.int64)
        super()._physics(x, status, pend, k, motors, active)
        self.calls.append(np.where(active, before * 4 + status, INACTIVE))


def state_events(x, tp=TaskParams()):
    """The discrete tests of judge_step and the shaping on a stored state x [12,L]: (oob, tilt (not oob), |dz| >
    dz_max, inside the target radius), bool [L] each."""
    x = np.asarray(x, np.float64)
    oob = (np.abs(x[0]) >= tp.bounds) | (np.abs(x[2]) >= tp.bounds)
    ma = np.radians(tp.max_angle)
    tilt = ~oob & ((np.abs(x[6]) >= ma) | (np.abs(x[8]) >= ma))
    dzpen = np.abs(x[5]) > tp.dz_max
    inside = np.sqrt(x[0] ** 2 + x[2] ** 2) < tp.target_radius
    return oob, tilt, dzpen, inside


def tile_lanes(v, reps):
    """an array with the lane axis last (or a scalar / None) -> reps copies along that axis"""
    if v is None or np.ndim(v) == 0:
        return v
    v = np.asarray(v)
    return np.tile(v, (1,) * (v.ndim - 1) + (reps,))


def vehicle_of(table, mars):
    """a raw [12, L] vehicle table (ROWS) -> (VehicleParams, g, mars) as VecOracle takes them"""
    t = np.asarray(table, np.float64)
    vp = VehicleParams(**{k: t[ROWS.index(k)] for k in VEHICLE_FIELDS})
    return vp, t[ROWS.index("G")], ((t[ROWS.index("rho")], t[ROWS.index("C_L")]) if mars else None)


def run_rollout(task, x, status, actions, force=None, prev_shaping=None, steps=1, substeps=1, vp=DJI_PHANTOM, g=G,
                mars=None, tp=TaskParams(), time_limit_truncates=False, policy=None):
    """K steps of RecordingOracle(task, float64 storage, auto-reset disabled) on L lanes from x [12,L] / status [L].
    actions [K,L,A] are the actions step() receives, or with policy = (params [P,L], hidden) the offsets u_k of
    a_k = pi(o_{k-1}) + u_k.  prev_shaping None = shaping(x0), else the given [L] values (NaN = None); force [3,L]
    newtons pending; steps = the step counter.  Returns (tape, sig): tape = dict of x [K,L,12], reward [K,L], status,
    terminated, truncated [K,L], calls [K,substeps,L], actions [K,L,A] (the ones taken), oob / tilt / dzpen / inside
    [K+1,L] (start first); sig [S,L] int64 = the discrete signature of each lane."""
    x = np.asarray(x, np.float64)
    L = x.shape[1]
    A = task_action_dim(task)
    orc = RecordingOracle(task, L, tp, vp=vp, substeps=substeps, store_mode="float64", g=g, mars=mars,
                          time_limit_truncates=time_limit_truncates)
    orc.x[:] = x
    orc.status[:] = np.asarray(status, np.uint8)
    orc.steps[:] = steps
    orc.prev_shaping[:] = orc._shaping(x) if prev_shaping is None else prev_shaping
    if force is not None:
        orc.force[:] = np.asarray(force, np.float64)
        orc.pending[:] = True
    tape = {k: [] for k in ("x", "reward", "status", "terminated", "truncated", "calls", "actions")}
    ev = [[e] for e in state_events(x, tp)]
    sig = [np.asarray(status, np.int64)] + [e[0] for e in ev]
    first, od = OBS_SHAPE[task]
    for k, u in enumerate(np.asarray(actions, np.float64)):
        a = u if policy is None else policy64(policy[0], orc.x[first:first + od].T, policy[1], A) + u
        orc.calls = []
        _, r, term, trunc = orc.step(a)
        xk = orc.x.astype(np.float64)
        for lst, v in zip(ev, state_events(xk, tp)):
            lst.append(v)
        calls = np.array(orc.calls)
        clip = (a < 0).astype(np.int64) + 2 * (a > 1)
        sig += [orc.status.copy(), term, trunc, *calls, *clip.T, *(e[-1] for e in ev)]
        for key, v in (("x", xk.T), ("reward", r), ("status", orc.status), ("terminated", term),
                       ("truncated", trunc), ("calls", calls), ("actions", a)):
            tape[key].append(np.array(v, copy=True))
    tape = {k: np.array(v) for k, v in tape.items()}
    for name, e in zip(("oob", "tilt", "dzpen", "inside"), ev):
        tape[name] = np.array(e)
    return tape, np.array([np.asarray(s, np.int64) for s in sig])


FD = namedtuple("FD", "grad grad2 out keep same agree tape")


def branch_fd(run, Z, hs):
    """Central differences of run's outputs with respect to its inputs Z [D,n] (steps hs [D] or [D,n]), at h and 2h,
    with the stability verdict.  run(Z [D,L]) -> (out [M,L], sig [S,L], tape dict of arrays with the lane axis last).
    Returns FD(grad [M,D,n] (at h), grad2 (at 2h), out [M,n] of the base run, keep = same & agree [n], same (every
    copy has the base's signature), agree (h and 2h within AGREE), tape of the base run)."""
    Z = np.asarray(Z, np.float64)
    D, n = Z.shape
    hs = np.asarray(hs, np.float64)
    hs = np.broadcast_to(hs if hs.ndim == 2 else hs.reshape(-1, 1), (D, n))
    reps = 1 + 4 * D
    Zl = np.tile(Z, (1, reps))
    for j, mult in enumerate((1.0, 2.0)):
        for d in range(D):
            for s, sign in enumerate((1.0, -1.0)):
                r = 1 + 2 * (j * D + d) + s
                Zl[d, r * n:(r + 1) * n] += sign * mult * hs[d]
    out, sig, tape = run(Zl)
    M = out.shape[0]
    o = out.reshape(M, reps, n)
    op = o[:, 1:].reshape(M, 2, D, 2, n)
    grad = (op[:, 0, :, 0] - op[:, 0, :, 1]) / (2 * hs)
    grad2 = (op[:, 1, :, 0] - op[:, 1, :, 1]) / (4 * hs)
    sg = sig.reshape(sig.shape[0], reps, n)
    same = np.all(sg == sg[:, :1], axis=(0, 1))
    with np.errstate(invalid="ignore"):
        dev = np.abs(grad - grad2) / np.maximum(1.0, np.abs(grad))
    agree = np.all(dev <= AGREE, axis=(0, 1))
    tape0 = {k: (v[:, :n] if k in ("x", "actions") else v[..., :n]) for k, v in tape.items()}
    return FD(grad, grad2, o[:, 0], same & agree, same, agree, tape0)


def _loss(tape, gx, gr, reps):
    """L = sum(gx X) + sum(gr R) of every lane MINUS its env's base-run value (lanes 0 .. n-1 are the base run): the
    differences of the tapes are taken before the contraction, so the rounding of L's large terms (a -100 penalty, x of
    10 m) does not enter the central differences, only the rounding of the tapes themselves."""
    n = tape["reward"].shape[1] // reps
    L = np.zeros(tape["reward"].shape[1])
    if gx is not None:
        dx = tape["x"] - np.tile(tape["x"][:, :n], (1, reps, 1))
        L += np.einsum("knj,knj->n", dx, np.tile(np.asarray(gx, np.float64), (1, reps, 1)))
    if gr is not None:
        dr = tape["reward"] - np.tile(tape["reward"][:, :n], (1, reps))
        L += np.einsum("kn,kn->n", dr, np.tile(np.asarray(gr, np.float64), (1, reps)))
    return L[None]


def fd_step(task, x, status, actions, force=None, substeps=1, vp=DJI_PHANTOM, g=G, mars=None, h=1e-6):
    """One step (step_jacobian's transition: prev_shaping a defined constant, 0).  Returns (FD, dx [n,12,12],
    du [n,12,A], reward_dx [n,12], reward_du [n,A]) of the h differences; FD.tape is the base run's."""
    x = np.asarray(x, np.float64)
    n, A = x.shape[1], task_action_dim(task)
    Z = np.concatenate([x, np.asarray(actions, np.float64).reshape(n, A).T])

    def run(Zl):
        reps = Zl.shape[1] // n
        tape, sig = run_rollout(task, Zl[:12], tile_lanes(status, reps), Zl[12:].T[None], force=tile_lanes(force, reps),
                                prev_shaping=np.zeros(Zl.shape[1]), substeps=substeps, vp=_tile_vp(vp, reps),
                                g=tile_lanes(g, reps), mars=_tile_mars(mars, reps))
        return np.concatenate([tape["x"][0].T, tape["reward"]]), sig, tape

    fd = branch_fd(run, Z, h)
    J = np.moveaxis(fd.grad, 2, 0)                 # [n, 13, D]
    return fd, J[:, :12, :12], J[:, :12, 12:], J[:, 12, :12], J[:, 12, 12:]


def fd_rollout(task, x, status, actions, gx=None, gr=None, force=None, prev_shaping=None, steps=1, substeps=1,
               vp=DJI_PHANTOM, g=G, mars=None, tp=TaskParams(), time_limit_truncates=False, h=H_ROLLOUT):
    """L = sum(gx X) + sum(gr R) over K open-loop steps (run_rollout).  Returns (FD, g_actions [K,n,A], g_x0 [12,n])."""
    x = np.asarray(x, np.float64)
    actions = np.asarray(actions, np.float64)
    K, n, A = actions.shape
    Z = np.concatenate([x, actions.transpose(0, 2, 1).reshape(K * A, n)])

    def run(Zl):
        reps = Zl.shape[1] // n
        acts = Zl[12:].reshape(K, A, -1).transpose(0, 2, 1)
        tape, sig = run_rollout(task, Zl[:12], tile_lanes(status, reps), acts, force=tile_lanes(force, reps),
                                prev_shaping=tile_lanes(prev_shaping, reps), steps=tile_lanes(steps, reps),
                                substeps=substeps, vp=_tile_vp(vp, reps), g=tile_lanes(g, reps),
                                mars=_tile_mars(mars, reps), tp=tp, time_limit_truncates=time_limit_truncates)
        return _loss(tape, gx, gr, reps), sig, tape

    fd = branch_fd(run, Z, h)
    return fd, fd.grad[0, 12:].reshape(K, A, n).transpose(0, 2, 1), fd.grad[0, :12]


def fd_params(task, x, status, actions, table, force, gx=None, gr=None, prev_shaping=None, substeps=1, mars=False,
              h=H_ROLLOUT):
    """L over K open-loop steps with respect to the [12,n] vehicle table (ROWS) and the pending force [3,n].  The rows
    span 1e-6 .. 1e4, so they are differentiated in units of |p| (a row that is 0: units of 1) -- the log-scaled
    comparison of the device's g_vehicle -- and the force in units of 10 N; the verdict applies to those scaled
    gradients.  Returns (FD, g_vehicle [12,n], g_force [3,n]) in the rows' own units."""
    x = np.asarray(x, np.float64)
    n = x.shape[1]
    table = np.asarray(table, np.float64)
    scale = np.concatenate([np.where(table != 0, np.abs(table), 1.0), np.full((3, n), 10.0)])
    Z = np.concatenate([table, np.asarray(force, np.float64)]) / scale

    def run(Zl):
        reps = Zl.shape[1] // n
        P = Zl * np.tile(scale, (1, reps))
        vp, g, mp = vehicle_of(P[:12], mars)
        tape, sig = run_rollout(task, tile_lanes(x, reps), tile_lanes(status, reps),
                                np.tile(np.asarray(actions, np.float64), (1, reps, 1)), force=P[12:],
                                prev_shaping=tile_lanes(prev_shaping, reps), substeps=substeps, vp=vp, g=g, mars=mp)
        return _loss(tape, gx, gr, reps), sig, tape

    fd = branch_fd(run, Z, h)
    return fd, fd.grad[0, :12] / scale[:12], fd.grad[0, 12:] / scale[12:]


def fd_mlp(task, x, status, params, hidden, offsets, gx=None, gr=None, substeps=1, h=H_ROLLOUT, h_p=1e-6):
    """L over K closed-loop steps a_k = pi(o_{k-1}) + u_k (pi in float64 on the float64 observation), with respect to
    x0, u and theta.  Returns (FD, g_params [P,n] per env, g_u [K,n,A], g_x0 [12,n]).  theta's step h_p is smaller:
    a weight moves the action by h_p |o|."""
    x = np.asarray(x, np.float64)
    u = np.asarray(offsets, np.float64)
    K, n, A = u.shape
    p = np.asarray(params, np.float64)
    P = p.shape[0]
    Z = np.concatenate([x, u.transpose(0, 2, 1).reshape(K * A, n), np.repeat(p[:, None], n, axis=1)])

    def run(Zl):
        reps = Zl.shape[1] // n
        uu = Zl[12:12 + K * A].reshape(K, A, -1).transpose(0, 2, 1)
        tape, sig = run_rollout(task, Zl[:12], tile_lanes(status, reps), uu, substeps=substeps,
                                policy=(Zl[12 + K * A:], hidden))
        return _loss(tape, gx, gr, reps), sig, tape

    fd = branch_fd(run, Z, np.array([h] * (12 + K * A) + [h_p] * P))
    g = fd.grad[0]
    return fd, g[12 + K * A:], g[12:12 + K * A].reshape(K, A, n).transpose(0, 2, 1), g[:12]


def _tile_vp(vp, reps):
    return VehicleParams(**{k: tile_lanes(getattr(vp, k), reps) for k in VEHICLE_FIELDS})


def _tile_mars(mars, reps):
    return None if mars is None else tuple(tile_lanes(m, reps) for m in mars)


def event_classes(tape, status0):
    """The event classes of a base run (bool [n] each): what a lane went through inside the horizon."""
    st, calls = tape["status"], tape["calls"]
    s0 = np.asarray(status0)
    seen = lambda s: (st == s).any(axis=0)                                        # noqa: E731
    changes = lambda e: (e != e[:1]).any(axis=0)                                  # noqa: E731
    froze_soft = (calls == AIRBORNE * 4 + LEVELING).any(axis=(0, 1))
    levelled = (calls == LEVELLED).any(axis=(0, 1))
    took_off = (calls[0] == TOOK_OFF).any(axis=0)
    clipped = (tape["actions"] < 0).any(axis=(0, 2)) | (tape["actions"] > 1).any(axis=(0, 2))
    trunc = tape["truncated"]
    return {
        "soft_touchdown": (s0 == AIRBORNE) & froze_soft & levelled & (st[-1] == LANDED),
        "hard_touchdown": (s0 != CRASHED) & seen(CRASHED),
        "tilt_crossed": changes(tape["tilt"]),
        "oob_crossed": changes(tape["oob"]),
        "dz_crossed": changes(tape["dzpen"]),
        "clipped": clipped,
        "landed_start": s0 == LANDED,
        "crashed_start": s0 == CRASHED,
        "leveling_takeoff": (s0 == LEVELING) & took_off,
        "truncated_mid": trunc[1:].any(axis=0) & ~trunc[0],
    }
