"""NumPy references of the forward-mode rollout tangents (cs_jvp_rollout): a restatement of the
fold tangent (rollout_tangent.h: fold_tangent, the forward derivative of fold_vehicle and the transpose partner of
unfold_vehicle_kernel), central-difference rollout tangents of the float64 oracle, and the identification problem of
tests/test_gpu_identify.py with a Levenberg-Marquardt loop on the oracle's central-difference Jacobian (the algorithm of
gym_copter_amd.identify, restated), so that no device sees a problem the reference does not solve."""
import numpy as np

from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, G, VehicleParams
from rollout_fd import oracle_rollout

ROWS = ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm", "G", "rho", "C_L")


def fold_tangent(t, p, lift, gyro):
    """raw tangents t [12, n] at the raw rows p [12, n] -> the tangents of the 11 coefficients [11, n]"""
    B, D, M, L, Ix, Iy, Iz, Jr, maxrpm, _, rho, C_L = p
    ws = maxrpm * np.pi / 30.0
    ws2 = ws * ws
    t_ws = t[8] * (np.pi / 30.0)
    t_ws2 = 2.0 * ws * t_ws
    if lift:
        base = 0.5 * (0.05 * L * 4.0) * (L / 2.0) ** 2
        kt = kr = base * rho * C_L * ws2
        t_kt = t_kr = base * C_L * ws2 * t[10] + base * rho * ws2 * t[11] + 0.075 * L * L * rho * C_L * ws2 * t[3] + \
            base * rho * C_L * t_ws2
    else:
        kt, kr = B * ws2, L * B * ws2
        t_kt = ws2 * t[0] + B * t_ws2
        t_kr = B * ws2 * t[3] + L * ws2 * t[0] + L * B * t_ws2
    z = np.zeros_like(M)
    return np.array([
        -t_kt / M + kt / (M * M) * t[2],
        t_kr / Ix - kr / (Ix * Ix) * t[4],
        t_kr / Iy - kr / (Iy * Iy) * t[5],
        ws2 / Iz * t[1] + D / Iz * t_ws2 - D * ws2 / (Iz * Iz) * t[6],
        t[9] + z,
        (t[5] - t[6]) / Ix - (Iy - Iz) / (Ix * Ix) * t[4],
        (t[6] - t[4]) / Iy - (Iz - Ix) / (Iy * Iy) * t[5],
        (t[4] - t[5]) / Iz - (Ix - Iy) / (Iz * Iz) * t[6],
        -2.0 / (M * M) * t[2],
        (ws / Ix * t[7] + Jr / Ix * t_ws - Jr * ws / (Ix * Ix) * t[4]) if gyro else z,
        (ws / Iy * t[7] + Jr / Iy * t_ws - Jr * ws / (Iy * Iy) * t[5]) if gyro else z])


def _oracle(task, x, status, actions, table, force, prev_shaping, substeps, mars):
    vp = VehicleParams(**{k: table[ROWS.index(k)] for k in ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm")})
    mp = (table[ROWS.index("rho")], table[ROWS.index("C_L")]) if mars else None
    xs, rs, _, _, _ = oracle_rollout(task, x, status, actions, force=force, prev_shaping=prev_shaping,
                                     substeps=substeps, vp=vp, g=table[ROWS.index("G")], mars=mp)
    return xs, rs


def fd_tangents(task, x, status, actions, table, force, t_a, t_x0, t_v, t_f, prev_shaping=None, substeps=1,
                mars=False, h=1e-6):
    """Central differences (oracle(theta + h t) - oracle(theta - h t)) / 2h of a K-step float64 oracle rollout in D mixed
    directions: t_a [D,K,n,A], t_x0 [D,12,n], t_v [D,12,n], t_f [D,3,n].  Every direction's two copies run as lanes of
    one oracle batch.  Returns (t_x [D,K,n,12], t_reward [D,K,n])."""
    D, n = t_x0.shape[0], x.shape[1]
    reps = 2 * D
    X, A = np.tile(x, (1, reps)), np.tile(np.asarray(actions, np.float64), (1, reps, 1))
    T, F = np.tile(table, (1, reps)), np.tile(force, (1, reps))
    for d in range(D):
        for s, sign in ((0, 1.0), (1, -1.0)):
            sl = slice((2 * d + s) * n, (2 * d + s + 1) * n)
            X[:, sl] += sign * h * t_x0[d]
            A[:, sl] += sign * h * t_a[d]
            T[:, sl] += sign * h * t_v[d]
            F[:, sl] += sign * h * t_f[d]
    pl = None if prev_shaping is None else np.tile(prev_shaping, reps)
    xs, rs = _oracle(task, X, np.tile(status, reps), A, T, F, pl, substeps, mars)
    K = xs.shape[0]
    xs, rs = xs.reshape(K, D, 2, n, 12), rs.reshape(K, D, 2, n)
    return ((xs[:, :, 0] - xs[:, :, 1]) / (2 * h)).transpose(1, 0, 2, 3), \
        ((rs[:, :, 0] - rs[:, :, 1]) / (2 * h)).transpose(1, 0, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the identification problem (tests/test_gpu_rollout_param_grad.py's, at n = 256) and its reference solution
# ---------------------------------------------------------------------------------------------------------------------
FIT = ("M", "Ix", "Iy")
IDENTIFY_N, IDENTIFY_K = 256, 50


def identify_problem(n=IDENTIFY_N, K=IDENTIFY_K, seed=2024, shared=False, rho=1.225, C_L=0.0):
    """Lander3D envs with hidden M, Ix, Iy at +-20 % around the DJI Phantom (one common hidden vehicle when `shared`) and
    a hidden +-30 N pending force, K steps of exciting open-loop actions from 30 m.  Returns a dict of NumPy arrays:
    nominal, hidden [12,n], force [3,n], x0 [12,n], status [n], actions [K,n,4] float32."""
    rng = np.random.default_rng(seed)
    nominal = np.array([np.full(n, v) for v in (5e-3, 2e-6, 1.38, 0.35, 2.0, 2.0, 3.0, 38e-4, 15000.0, G, rho, C_L)])
    idx = [ROWS.index(k) for k in FIT]
    hidden = nominal.copy()
    hidden[idx] *= rng.uniform(0.8, 1.2, (3, 1 if shared else n))
    x0 = np.zeros((12, n))
    x0[4] = -30.0
    actions = (hover_action() * (1.0 + 0.15 * rng.standard_normal((K, n, 4)))).astype(np.float32)
    return dict(nominal=nominal, hidden=hidden, force=rng.uniform(-30.0, 30.0, (3, n)), x0=x0,
                status=np.full(n, AIRBORNE, np.uint8), actions=actions, idx=idx)


def lm_reference(pb, x_obs, fit_force=False, iterations=6, damping=1e-3, shared=False, h=1e-6):
    """gym_copter_amd.identify's algorithm on the float64 oracle with a central-difference Jacobian (steps h in the log
    parameters, h x 10 N in the force).  Returns (vehicle [12,n], force [3,n] or None, accepted [iterations, m])."""
    n = pb["x0"].shape[1]
    idx, pv = pb["idx"], len(pb["idx"])
    p = pv + (3 if fit_force else 0)
    w = 1.0 / np.maximum(np.abs(x_obs).max(axis=0, keepdims=True), 1e-3)
    f0 = np.zeros((3, n))
    acts = pb["actions"].astype(np.float64)

    def point(theta):
        veh = pb["nominal"].copy()
        veh[idx] = pb["nominal"][idx] * np.exp(theta[:pv])
        return veh, (f0 + theta[pv:]) if fit_force else None

    def rollouts(thetas):  # [R, p, n] -> x [R, K, n, 12], as lanes of one oracle batch
        R = len(thetas)
        pts = [point(t) for t in thetas]
        force = np.concatenate([f for _, f in pts], axis=1) if fit_force else None
        xs, _ = _oracle("lander3d", np.tile(pb["x0"], (1, R)), np.tile(pb["status"], R), np.tile(acts, (1, R, 1)),
                        np.concatenate([v for v, _ in pts], axis=1), force, None, 1, False)
        return xs.reshape(xs.shape[0], R, n, 12).transpose(1, 0, 2, 3)

    def linearise(theta):
        hs = np.array([h] * pv + [10.0 * h] * (p - pv))
        pts = [theta]
        for j in range(p):
            for sign in (1.0, -1.0):
                t = theta.copy()
                t[j] += sign * hs[j]
                pts.append(t)
        xs = rollouts(pts)
        res = (xs[0] - x_obs) * w
        J = np.array([(xs[1 + 2 * j] - xs[2 + 2 * j]) / (2 * hs[j]) for j in range(p)]) * w
        cost, jtj, jtr = (res * res).sum(axis=(0, 2)), np.einsum("aknj,bknj->nab", J, J), np.einsum("aknj,knj->na", J, res)
        if shared:
            cost, jtj, jtr = cost.sum(keepdims=True), jtj.sum(axis=0, keepdims=True), jtr.sum(axis=0, keepdims=True)
        return cost, jtj, jtr

    m = 1 if shared else n
    theta = np.zeros((p, m))
    lam = np.full(m, damping)
    cost, jtj, jtr = linearise(np.broadcast_to(theta, (p, n)).copy())
    accepted = []
    for _ in range(iterations):
        diag = np.einsum("nii->ni", jtj)
        A = jtj + np.eye(p) * (lam[:, None] * diag)[:, :, None]
        delta = -np.linalg.solve(A, jtr[:, :, None])[:, :, 0]
        delta[:, :pv] = np.clip(delta[:, :pv], -1.0, 1.0)
        trial = theta + delta.T
        cost_t, jtj_t, jtr_t = linearise(np.broadcast_to(trial, (p, n)).copy())
        acc = cost_t < cost
        theta = np.where(acc[None], trial, theta)
        cost = np.where(acc, cost_t, cost)
        jtj, jtr = np.where(acc[:, None, None], jtj_t, jtj), np.where(acc[:, None], jtr_t, jtr)
        lam = np.where(acc, lam / 3.0, lam * 10.0)
        accepted.append(acc)
    veh, force = point(np.broadcast_to(theta, (p, n)))
    return veh, force, np.array(accepted)


def oracle_observation(pb, with_force=False):
    """x_obs [K,n,12] of the hidden vehicle (and hidden force) on the float64 oracle"""
    xs, _ = _oracle("lander3d", pb["x0"], pb["status"], pb["actions"].astype(np.float64), pb["hidden"],
                    pb["force"] if with_force else None, None, 1, False)
    return xs
