"""The checker of CopterVecEnv.rollout_vjp: central differences of K float64 VecOracle steps (oracle/refvec.py, auto-reset
disabled) from a given point, for a batch of envs at once.  Every env's 2 x (12 + K A) perturbed copies run as lanes of
ONE oracle batch, as in tests/jacobian_fd.py."""
import numpy as np

from oracle.refcpu import DJI_PHANTOM, G, VehicleParams, task_action_dim
from oracle.refvec import VecOracle

from jacobian_fd import VEHICLE_FIELDS, _tile


def oracle_rollout(task, x, status, actions, force=None, prev_shaping=None, substeps=1, vp=DJI_PHANTOM, g=G,
                   mars=None, steps=1, store_mode="float64"):
    """K steps of VecOracle(task, auto-reset disabled) from x [12,n] / status [n]; actions [K,n,A].  prev_shaping None =
    shaping(x0) (differentiated by a perturbation of x0), else the given [n] values; force [3,n] newtons pending.
    Returns (x [K,n,12], reward [K,n], terminated [K,n], truncated [K,n], the oracle)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    orc = VecOracle(task, n, vp=vp, substeps=substeps, store_mode=store_mode, g=g, mars=mars)
    orc.x[:] = x
    orc.status[:] = np.asarray(status, dtype=np.uint8)
    orc.steps[:] = steps
    orc.prev_shaping[:] = orc._shaping(x) if prev_shaping is None else prev_shaping
    if force is not None:
        orc.force[:] = np.asarray(force, dtype=np.float64)
        orc.pending[:] = True
    xs, rs, ts, us = [], [], [], []
    for a in np.asarray(actions, dtype=np.float64):
        _, r, term, trunc = orc.step(a)
        xs.append(orc.x.astype(np.float64).T.copy())
        rs.append(r.copy())
        ts.append(term.copy())
        us.append(trunc.copy())
    return np.array(xs), np.array(rs), np.array(ts), np.array(us), orc


def fd_rollout_vjp(task, x, status, actions, gx=None, gr=None, force=None, prev_shaping=None, substeps=1,
                   vp=DJI_PHANTOM, g=G, mars=None, h_x=1e-6, h_a=1e-6):
    """Central differences of L = sum(gx * X) + sum(gr * R) over a K-step oracle rollout (oracle_rollout, float64
    storage).  x [12,n], status [n], actions [K,n,A], gx [K,n,12], gr [K,n] (None = zero).  Returns (g_actions [K,n,A],
    g_x0 [12,n])."""
    x = np.asarray(x, dtype=np.float64)
    actions = np.asarray(actions, dtype=np.float64)
    K, n, A = actions.shape
    assert A == task_action_dim(task)
    D = 12 + K * A
    reps = 2 * D                                    # lane = (2 d + s) n + env, s = 0: +h, 1: -h
    vpl = VehicleParams(**{k: _tile(getattr(vp, k), reps) for k in VEHICLE_FIELDS})
    marsl = None if mars is None else tuple(_tile(m, reps) for m in mars)
    X = np.tile(x, (1, reps))
    act = np.tile(actions, (1, reps, 1))
    for d in range(D):
        for s, sign in ((0, 1.0), (1, -1.0)):
            sl = slice((2 * d + s) * n, (2 * d + s + 1) * n)
            if d < 12:
                X[d, sl] += sign * h_x
            else:
                k, j = divmod(d - 12, A)
                act[k, sl, j] += sign * h_a
    fl = None if force is None else np.tile(np.asarray(force, dtype=np.float64), (1, reps))
    pl = None if prev_shaping is None else np.tile(np.asarray(prev_shaping, dtype=np.float64), reps)
    xs, rs, _, _, _ = oracle_rollout(task, X, np.tile(np.asarray(status, np.uint8), reps), act, force=fl,
                                     prev_shaping=pl, substeps=substeps, vp=vpl, g=_tile(g, reps), mars=marsl)
    L = np.zeros(reps * n)
    if gx is not None:
        L += np.einsum("knj,knj->n", xs, np.tile(np.asarray(gx, dtype=np.float64), (1, reps, 1)))
    if gr is not None:
        L += np.einsum("kn,kn->n", rs, np.tile(np.asarray(gr, dtype=np.float64), (1, reps)))
    L = L.reshape(D, 2, n)
    hs = np.array([h_x] * 12 + [h_a] * (K * A))[:, None]
    grad = (L[:, 0, :] - L[:, 1, :]) / (2 * hs)      # [D, n]
    g_x0 = grad[:12]
    g_act = grad[12:].reshape(K, A, n).transpose(0, 2, 1)
    return g_act, g_x0


def shaping_grad(x, xyz_pen=25.0, yaw_pen=50.0):
    """Gradient of the Lander shaping potential (lander.py:48-57) at x [12,n]: the rule of DESIGN section 9."""
    x = np.asarray(x, dtype=np.float64)
    g = np.zeros_like(x)
    r6 = np.sqrt(np.sum(x[:6] ** 2, axis=0))
    r2 = np.sqrt(x[10] ** 2 + x[11] ** 2)
    f6 = np.where(r6 > 0, -xyz_pen / np.where(r6 > 0, r6, 1.0), 0.0)
    f2 = np.where(r2 > 0, -yaw_pen / np.where(r2 > 0, r2, 1.0), 0.0)
    g[:6] = f6 * x[:6]
    g[10] = f2 * x[10]
    g[11] = f2 * x[11]
    return g
