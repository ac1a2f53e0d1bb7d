"""The checker of CopterVecEnv.step_jacobian: central differences of one float64 VecOracle step (oracle/refvec.py,
bit-exact to the reference) from a given point, for a batch of envs at once.  Every env's 2 x (12 + A) perturbed
copies run as lanes of ONE oracle batch."""
import numpy as np

from oracle.refcpu import AIRBORNE, DJI_PHANTOM, G, VehicleParams, task_action_dim
from oracle.refvec import VecOracle

VEHICLE_FIELDS = ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm")


def _tile(v, reps):
    """a per-env array [n] -> [reps * n] lanes (lane = rep * n + env); scalars stay scalars"""
    return np.tile(np.asarray(v, dtype=np.float64), reps) if np.ndim(v) else v


def fd_jacobian(task, x, status, actions, force=None, substeps=1, vp=DJI_PHANTOM, g=G, mars=None,
                h_x=1e-6, h_a=1e-6):
    """Central differences of one step of VecOracle(task, store_mode="float64", auto-reset disabled).

    x [12,n] float64, status [n] uint8, actions [n,A] (the values step() receives), force [3,n] newtons pending
    (None: no perturbation), vp / g / mars as VecOracle takes them (fields may be arrays [n]).  prev_shaping is 0
    (a defined constant).  Returns (dx [n,12,12], du [n,12,A], reward_dx [n,12], reward_du [n,A])."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    A = task_action_dim(task)
    D = 12 + A
    reps = 2 * D                                    # lane = (2 d + s) n + env, s = 0: +h, 1: -h
    vpl = VehicleParams(**{k: _tile(getattr(vp, k), reps) for k in VEHICLE_FIELDS})
    marsl = None if mars is None else tuple(_tile(m, reps) for m in mars)
    orc = VecOracle(task, reps * n, vp=vpl, substeps=substeps, store_mode="float64", g=_tile(g, reps), mars=marsl)
    X = np.tile(x, (1, reps))
    act = np.tile(np.asarray(actions, dtype=np.float64).reshape(n, A), (reps, 1))
    for d in range(D):
        for s, sign in ((0, 1.0), (1, -1.0)):
            sl = slice((2 * d + s) * n, (2 * d + s + 1) * n)
            if d < 12:
                X[d, sl] += sign * h_x
            else:
                act[sl, d - 12] += sign * h_a
    orc.x[:] = X
    orc.status[:] = np.tile(np.asarray(status, dtype=np.uint8), reps)
    orc.steps[:] = 1
    orc.prev_shaping[:] = 0.0
    if force is not None:
        orc.force[:] = np.tile(np.asarray(force, dtype=np.float64), (1, reps))
        orc.pending[:] = True
    _, r, _, _ = orc.step(act)
    xs = orc.x.astype(np.float64).reshape(12, D, 2, n)
    rs = r.reshape(D, 2, n)
    hs = np.array([h_x] * 12 + [h_a] * A)[:, None]
    J = (xs[:, :, 0, :] - xs[:, :, 1, :]) / (2 * hs[None])      # [12, D, n]
    gr = (rs[:, 0, :] - rs[:, 1, :]) / (2 * hs)                 # [D, n]
    J = np.moveaxis(J, 2, 0)                                    # [n, 12, D]
    return J[:, :, :12], J[:, :, 12:], gr[:12].T, gr[12:].T


def hover_action(vp=DJI_PHANTOM, g=G):
    """The motor value a* at which the four motors of the B thrust law hold the vehicle (bz = -G)."""
    w = vp.maxrpm * np.pi / 30
    return np.sqrt(g * vp.M / (4 * vp.B * w * w))


def hover_point(n, altitude=10.0):
    x = np.zeros((12, n))
    x[4] = -altitude
    return x, np.full(n, AIRBORNE, np.uint8)


def lqr_gain(A, B, q, r, iters=5000):
    """Discrete-time LQR gain K (u = -K x) by Riccati iteration: P = Q + A'P(A - BK), K = (R + B'PB)^-1 B'PA."""
    Q, R = np.diag(q), np.diag(r)
    P = Q.copy()
    for _ in range(iters):
        K = np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
        Pn = Q + A.T @ P @ (A - B @ K)
        if np.max(np.abs(Pn - P)) <= 1e-12 * max(1.0, np.max(np.abs(P))):
            P = Pn
            break
        P = Pn
    return np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A)
