"""The checker of CopterVecEnv.rollout_mlp_vjp: central differences of a K-step CLOSED-LOOP float64 oracle rollout
(VecOracle with auto-reset disabled, tests/rollout_fd.py's setup) in which step k takes a_k = pi(o_{k-1}) + u_k, pi
evaluated in float64 on the float64 observation (the float32 roundings of the device are what the adjoint treats as
straight-through).  Every env's 2 x (12 + K A + P) perturbed copies -- of x0, of u and of theta -- run as lanes of ONE
oracle batch, each lane with its own theta."""
import numpy as np

from oracle.refcpu import DJI_PHANTOM, G, VehicleParams, task_action_dim
from oracle.refvec import VecOracle

from jacobian_fd import VEHICLE_FIELDS, _tile


# (first observed state slot, obs_dim) of each task: gym_copter_amd.vecenv._TASK_SHAPES
OBS_SHAPE = {"lander3d": (0, 10), "hover3d": (0, 12), "lander2d": (2, 6), "hover2d": (2, 6), "lander1d": (4, 2),
             "hover1d": (4, 2)}


def policy64(params, obs, hidden, act_dim):
    """pi(obs) in float64 for lanes with their own theta: params [P, L] (or [P]), obs [L, OBS] -> [L, A]."""
    p = np.asarray(params, np.float64)
    o = np.asarray(obs, np.float64)
    L, OBS = o.shape
    if p.ndim == 1:
        p = np.repeat(p[:, None], L, axis=1)
    if hidden == 0:
        W = p[:act_dim * OBS].reshape(act_dim, OBS, L)
        b = p[act_dim * OBS:].reshape(act_dim, L)
        return (np.einsum("cjl,lj->lc", W, o) + b.T)
    H = hidden
    W1 = p[:H * OBS].reshape(H, OBS, L)
    b1 = p[H * OBS:H * OBS + H]
    W2 = p[H * OBS + H:H * OBS + H + act_dim * H].reshape(act_dim, H, L)
    b2 = p[H * OBS + H + act_dim * H:]
    h = np.tanh(np.einsum("hjl,lj->lh", W1, o) + b1.T)
    return np.einsum("chl,lh->lc", W2, h) + b2.T


def oracle_mlp_rollout(task, x, status, params, hidden, K, offsets=None, substeps=1, vp=DJI_PHANTOM, g=G, steps=1,
                       mars=None):
    """K closed-loop steps of VecOracle(task, auto-reset disabled, float64 storage) from x [12,n] / status [n]
    (prev_shaping = shaping(x0)); params [P] or [P,n]; offsets [K,n,A] or None; vp / g / mars as VecOracle takes them
    (fields may be arrays [n]).  Returns (x [K,n,12], reward [K,n], obs [K,n,OBS] (o_{k-1}), actions [K,n,A])."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    first, od = OBS_SHAPE[task]
    A = task_action_dim(task)
    orc = VecOracle(task, n, vp=vp, substeps=substeps, store_mode="float64", g=g, mars=mars)
    orc.x[:] = x
    orc.status[:] = np.asarray(status, dtype=np.uint8)
    orc.steps[:] = steps
    orc.prev_shaping[:] = orc._shaping(x)
    xs, rs, os_, acts = [], [], [], []
    for k in range(K):
        o = orc.x[first:first + od].astype(np.float64).T.copy()
        a = policy64(params, o, hidden, A)
        if offsets is not None:
            a = a + np.asarray(offsets[k], np.float64)
        _, r, _, _ = orc.step(a)
        xs.append(orc.x.astype(np.float64).T.copy())
        rs.append(r.copy())
        os_.append(o)
        acts.append(a)
    return np.array(xs), np.array(rs), np.array(os_), np.array(acts)


def fd_mlp_rollout_vjp(task, x, status, params, hidden, K, offsets=None, gx=None, gr=None, substeps=1, h_x=1e-6,
                       h_u=1e-6, h_p=1e-6, vp=DJI_PHANTOM, g=G, mars=None):
    """Central differences of L = sum(gx * X) + sum(gr * R) over oracle_mlp_rollout; vp / g / mars (fields may be arrays
    [n]) are tiled over the perturbed copies as tests/rollout_fd.py tiles them.  Returns (g_params [P] summed over the
    envs, g_u [K,n,A], g_x0 [12,n])."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    A = task_action_dim(task)
    params = np.asarray(params, np.float64)
    P = params.shape[0]
    u = np.zeros((K, n, A)) if offsets is None else np.asarray(offsets, np.float64)
    D = 12 + K * A + P
    reps = 2 * D                                    # lane = (2 d + s) n + env, s = 0: +h, 1: -h
    vpl = VehicleParams(**{k: _tile(getattr(vp, k), reps) for k in VEHICLE_FIELDS})
    marsl = None if mars is None else tuple(_tile(m, reps) for m in mars)
    X = np.tile(x, (1, reps))
    U = np.tile(u, (1, reps, 1))
    Pl = np.repeat(params[:, None], reps * n, axis=1)
    for d in range(D):
        for s, sign in ((0, 1.0), (1, -1.0)):
            sl = slice((2 * d + s) * n, (2 * d + s + 1) * n)
            if d < 12:
                X[d, sl] += sign * h_x
            elif d < 12 + K * A:
                k, j = divmod(d - 12, A)
                U[k, sl, j] += sign * h_u
            else:
                Pl[d - 12 - K * A, sl] += sign * h_p
    xs, rs, _, _ = oracle_mlp_rollout(task, X, np.tile(np.asarray(status, np.uint8), reps), Pl, hidden, K, offsets=U,
                                      substeps=substeps, vp=vpl, g=_tile(g, reps), mars=marsl)
    L = np.zeros(reps * n)
    if gx is not None:
        L += np.einsum("knj,knj->n", xs, np.tile(np.asarray(gx, dtype=np.float64), (1, reps, 1)))
    if gr is not None:
        L += np.einsum("kn,kn->n", rs, np.tile(np.asarray(gr, dtype=np.float64), (1, reps)))
    L = L.reshape(D, 2, n)
    hs = np.array([h_x] * 12 + [h_u] * (K * A) + [h_p] * P)[:, None]
    grad = (L[:, 0, :] - L[:, 1, :]) / (2 * hs)      # [D, n]
    g_x0 = grad[:12]
    g_u = grad[12:12 + K * A].reshape(K, A, n).transpose(0, 2, 1)
    g_p = grad[12 + K * A:].sum(axis=1)
    return g_p, g_u, g_x0
