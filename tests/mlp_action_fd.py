"""The checker of CopterVecEnv.rollout_mlp_vjp's cotangent on the action tape (g_actions_in): central differences of
L = sum(gx * X) + sum(gr * R) + sum(gact * A) over the float64 closed-loop oracle rollout of tests/mlp_rollout_fd.py,
where A [K,n,A] is the action tape a_k = pi(o_{k-1}) + u_k as step() receives it (before the clip).  With gact=None it
is fd_mlp_rollout_vjp, operation for operation."""
import numpy as np

from mlp_rollout_fd import oracle_mlp_rollout
from oracle.refcpu import task_action_dim


def fd_mlp_action_vjp(task, x, status, params, hidden, K, offsets=None, gx=None, gr=None, gact=None, substeps=1,
                      h_x=1e-6, h_u=1e-6, h_p=1e-6):
    """Returns (g_params [P] summed over the envs, g_u [K,n,A], g_x0 [12,n]); the lanes of fd_mlp_rollout_vjp: every
    env's 2 x (12 + K A + P) perturbed copies run as one oracle batch."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[1]
    A = task_action_dim(task)
    params = np.asarray(params, np.float64)
    P = params.shape[0]
    u = np.zeros((K, n, A)) if offsets is None else np.asarray(offsets, np.float64)
    D = 12 + K * A + P
    reps = 2 * D                                    # lane = (2 d + s) n + env, s = 0: +h, 1: -h
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
    xs, rs, _, acts = oracle_mlp_rollout(task, X, np.tile(np.asarray(status, np.uint8), reps), Pl, hidden, K,
                                         offsets=U, substeps=substeps)
    L = np.zeros(reps * n)
    if gx is not None:
        L += np.einsum("knj,knj->n", xs, np.tile(np.asarray(gx, dtype=np.float64), (1, reps, 1)))
    if gr is not None:
        L += np.einsum("kn,kn->n", rs, np.tile(np.asarray(gr, dtype=np.float64), (1, reps)))
    if gact is not None:
        L += np.einsum("knj,knj->n", acts, np.tile(np.asarray(gact, dtype=np.float64), (1, reps, 1)))
    L = L.reshape(D, 2, n)
    hs = np.array([h_x] * 12 + [h_u] * (K * A) + [h_p] * P)[:, None]
    grad = (L[:, 0, :] - L[:, 1, :]) / (2 * hs)      # [D, n]
    g_x0 = grad[:12]
    g_u = grad[12:12 + K * A].reshape(K, A, n).transpose(0, 2, 1)
    g_p = grad[12 + K * A:].sum(axis=1)
    return g_p, g_u, g_x0
