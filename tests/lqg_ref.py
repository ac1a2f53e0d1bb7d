"""A plain NumPy restatement of the two formulas cs_rollout_lqg (include/copterstep.h) adds to its parts -- the affine
feedback law at the filter's estimate and the formation of the measurement (gym_copter_amd/csrc/lqg_law.h) -- in the
kernel's own order of operations, so that the values are the device's bit for bit (NumPy's element-wise operations never
fuse a multiply with an add).  tests/test_rollout_lqg_cpu.py holds it to the header compiled for the host.

Also: the starts and inputs of the GPU tests (points, problem), the whole closed loop restated on the CPU (closed_loop: the
float64 oracle as the truth, tests/ekf_ref.py with central-difference Jacobians as the filter), and the application of
DESIGN.md section 22 (app_inputs, app_gains, app_conditions), whose inputs the CPU and the GPU test share."""
import numpy as np

import ekf_ref
from oracle.refcpu import AIRBORNE, CRASHED, LANDED

TASK_A = {"lander3d": 4, "hover3d": 4, "lander2d": 2, "hover2d": 2, "lander1d": 1, "hover1d": 1}


def law(abar, gains, xhat, xbar):
    """a = fl32(abar + sum_j K[c][j] (xhat[j] - xbar[j])): from (double) abar, j ascending, a subtraction, a multiply and
    an add each, one rounding.  abar [N,A] float32, gains [N,A,12], xhat [N,12], xbar [N,12] -> [N,A] float32."""
    abar = np.asarray(abar)
    assert abar.dtype == np.float32
    gains, xhat, xbar = (np.asarray(v, np.float64) for v in (gains, xhat, xbar))
    dx = xhat - xbar
    t = abar.astype(np.float64)
    for j in range(12):
        p = gains[:, :, j] * dx[:, None, j]
        t = t + p
    return t.astype(np.float32)


def measure(H, x, e):
    """z[i] = sum_j H[i][j] x[j] + e[i]: the first product starts the sum, j ascending, one multiply and one add per
    term, then the noise; a NaN e gives a NaN z.  H [M,12], x [N,12], e [N,M] -> [N,M]."""
    H, x, e = (np.asarray(v, np.float64) for v in (H, x, e))
    acc = H[None, :, 0] * x[:, None, 0]
    for j in range(1, 12):
        p = H[None, :, j] * x[:, None, j]
        acc = acc + p
    return acc + e


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
GROUPS = ("hover", "soft0", "hard0", "soft_mid", "hard_mid", "landed", "crashed", "clip")


def points(n, steps, A, rng, ah):
    """The truth's starts, one group of envs per branch: high hover; descents in ground contact at the first call
    (z > 0), soft and hard; low descents that touch down inside the horizon, soft and hard; LANDED and CRASHED starts;
    and a group whose nominal motors are below 0 half of the time.  Every nominal motor value is <= 1.  Returns (x
    [12,n], status [n], abar [steps,n,A] float32, group names [n])."""
    grp = np.array([GROUPS[i % len(GROUPS)] for i in range(n)])
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[1], x[3] = rng.uniform(-0.3, 0.3, (2, n))
    x[4] = rng.uniform(-8, -4, n)
    x[5] = rng.uniform(-0.5, 0.5, n)
    x[6], x[8] = rng.uniform(-0.05, 0.05, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-0.3, 0.3, (4, n))
    st = np.full(n, AIRBORNE, np.uint8)
    a = ah * rng.uniform(0.8, 1.2, (steps, n, A))
    for name, dz in (("soft0", (0.1, 0.6)), ("hard0", (1.5, 3.0)), ("soft_mid", (0.2, 0.6)), ("hard_mid", (1.5, 3.0))):
        m = grp == name
        k = int(m.sum())
        x[5, m] = rng.uniform(*dz, k)
        if name.endswith("0"):
            x[4, m] = rng.uniform(1e-3, 0.05, k)
        else:                                    # z passes 0 after 3 .. 9 steps of 0.01 s at this descent rate
            x[4, m] = -x[5, m] * rng.uniform(3, 9, k) / 100.0
    m = grp == "landed"
    x[4, m], x[5, m], st[m] = 0.0, 0.0, LANDED
    st[grp == "crashed"] = CRASHED
    m = grp == "clip"
    k = int(m.sum())
    a[:, m] = np.where(rng.uniform(size=(steps, k, A)) < 0.5, rng.uniform(-0.4, -0.01, (steps, k, A)), a[:, m])
    return x, st, a.astype(np.float32), grp


def problem(task, n, steps, rng, ah, M=6, dense=True, missing=0.0, gain_sd=0.02):
    """Everything cs_rollout_lqg reads but the reference tape, as host arrays: the truth's start (x0 [12,n], st0, force
    [3,n] newtons), abar, random gains [steps,n,A,12] of standard deviation gain_sd (the deviations are a few tenths, the
    hover motor value is 0.0166: the law moves every motor by its own size and pushes some below 0), the filter's start
    xhat0 = x0 + an error with altitude errors of up to 0.3 m -- so that an estimate is on the other side of a touchdown
    from the truth -- its status (the truth's), a random SPD P0 per env, H [M,12], r [M], the noise e [steps,n,M] scaled by
    sqrt(r) with NaN entries (probability `missing`), and ekf_ref.test_Q()."""
    A = TASK_A[task]
    x0, st0, abar, grp = points(n, steps, A, rng, ah)
    force = rng.uniform(-1.0, 1.0, (3, n))
    gains = gain_sd * rng.standard_normal((steps, n, A, 12))
    err = np.zeros((12, n))
    err[[0, 2]] = 0.2 * rng.standard_normal((2, n))
    err[[1, 3, 5]] = 0.2 * rng.standard_normal((3, n))
    err[4] = rng.uniform(-0.3, 0.3, n)
    err[[6, 8, 10]] = 0.02 * rng.standard_normal((3, n))
    err[[7, 9, 11]] = 0.1 * rng.standard_normal((3, n))
    held = (st0 != AIRBORNE)
    err[:, held] = 0.0
    err[[0, 2], :] += np.where(held, 0.1 * rng.standard_normal((2, n)), 0.0)
    xhat0 = x0 + err
    m = rng.standard_normal((n, 12, 12))
    P0 = 0.1 * (m @ np.swapaxes(m, 1, 2) / 12 + 0.2 * np.eye(12))
    P0 = (P0 + np.swapaxes(P0, 1, 2)) / 2
    if dense:
        H = rng.standard_normal((M, 12)) / np.sqrt(12)
    else:
        H = np.zeros((M, 12))
        H[np.arange(M), rng.permutation(12)[:M]] = 1.0
    r = rng.uniform(0.01, 0.1, M)
    e = np.sqrt(r) * rng.standard_normal((steps, n, M))
    if missing > 0.0:
        e[rng.uniform(size=e.shape) < missing] = np.nan
    return dict(x0=x0, st0=st0, force=force, abar=abar, gains=gains, xhat0=xhat0, fst0=st0.copy(), P0=P0, H=H, r=r, e=e,
                Q=ekf_ref.test_Q(), grp=grp)


def reference_tape(x0, nominal_x):
    """xbar [K,N,12]: the start, then the nominal tape's rows 0 .. K-2 (row k-1 = the reference before step k)"""
    return np.concatenate([np.asarray(x0).T[None], np.asarray(nominal_x)[:-1]])


# ---------------------------------------------------------------------------------------------------------------------
# the closed loop on the CPU: the float64 oracle as the truth, ekf_ref with central-difference Jacobians as the filter
# ---------------------------------------------------------------------------------------------------------------------
def closed_loop(task, x0, st0, abar, gains, xbar, e, H, r, Q, xhat0, P0, fst0, force=None, substeps=1):
    """cs_rollout_lqg's recursion in NumPy.  Returns dict of x, status (the truth's tapes [K,N,..]), actions [K,N,A]
    float32, z, xhat, fstatus, nis [K,N], P (the last posterior)."""
    from branch_fd import fd_step, run_rollout
    K, n = abar.shape[:2]
    xt, stt = np.array(x0, np.float64), np.array(st0, np.uint8)
    xh, Pm, fst = np.array(xhat0, np.float64).T.copy(), np.array(P0, np.float64), np.array(fst0, np.uint8)
    out = {k: [] for k in ("x", "status", "actions", "z", "xhat", "fstatus", "nis")}
    for k in range(K):
        a = law(abar[k], gains[k], xh, xbar[k])
        tape, _ = run_rollout(task, xt, stt, a[None].astype(np.float64), force=force if k == 0 else None,
                              substeps=substeps)
        xt, stt = tape["x"][0].T.copy(), tape["status"][0].astype(np.uint8)
        z = measure(H, xt.T, e[k])
        fd, Aj, *_ = fd_step(task, xh.T, fst, a.astype(np.float64), substeps=substeps)
        step = ekf_ref.one_step(Aj, Pm, fd.tape["x"][0][:n], Q, H, r, z)
        xh, Pm, fst = step["x"], step["P"], fd.tape["status"][0][:n].astype(np.uint8)
        for key, v in (("x", xt.T), ("status", stt), ("actions", a), ("z", z), ("xhat", xh), ("fstatus", fst),
                       ("nis", step["nis"])):
            out[key].append(np.array(v, copy=True))
    out = {k: np.array(v) for k, v in out.items()}
    out["P"] = Pm
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the application: Hover3D held at its reference from measured positions and angles
# ---------------------------------------------------------------------------------------------------------------------
# K = 192 steps (1.92 s), not the filter application's 48: a lateral position error is corrected through a tilt, and in
# 0.48 s even a controller that is told the true state leaves 0.21 m of the open loop's 0.22 m (measured on this
# restatement with xhat0 = x0 and no noise); the altitude, which the thrust reaches directly, is back within 0.01 m by then
APP_N, APP_K = 300, 192
APP_QC = np.diag([1000.0, 30.0] * 3 + [10.0, 1.0] * 3)      # the LQR's state weights: position, velocity; angle, rate
APP_RC = 3e6 * np.eye(4)                                    # ... and its action weights (a motor value is 0.0166 at hover)
APP_QF = APP_QC.copy()


def app_inputs(hover, seed=1):
    """(abar [K,N,4] float32 = the hover action, true start x0 [12,N] perturbed in velocity, xhat0 = x0 + N(0, P0),
    xbar [K,N,12] = the hover point, e [K,N,6] = sigma N(0, 1), H [6,12], r [6]) from NumPy seed `seed`; P0 and Q are
    ekf_ref's APP_P0 and APP_Q"""
    rng = np.random.default_rng(seed)
    n, K = APP_N, APP_K
    abar = np.full((K, n, 4), hover, np.float32)
    x0 = np.zeros((12, n))
    x0[4] = -10.0
    x0[[1, 3, 5]] = 0.5 * rng.standard_normal((3, n))
    xhat0 = x0 + np.sqrt(np.diag(ekf_ref.APP_P0))[:, None] * rng.standard_normal((12, n))
    H = np.zeros((6, 12))
    H[np.arange(6), ekf_ref.APP_SLOTS] = 1.0
    r = ekf_ref.APP_SIGMA ** 2
    e = ekf_ref.APP_SIGMA * rng.standard_normal((K, n, 6))
    ref = np.zeros(12)
    ref[4] = -10.0
    xbar = np.broadcast_to(ref, (K, n, 12)).copy()
    return abar, x0, xhat0, xbar, e, H, r


def app_gains(hover, K=APP_K):
    """One finite-horizon LQR recursion at hover, on the host: A, B = the central-difference Jacobians of the float64
    oracle's Hover3D step at the hover point under the hover action; S_K = Qf, then for k = K-1 .. 0
    L_k = (R + B^T S B)^-1 B^T S A,  S = Q + A^T S (A - B L_k).  Returns the law's gains [K,4,12] = -L_k."""
    from branch_fd import fd_step
    x = np.zeros((12, 1))
    x[4] = -10.0
    _, A, B, *_ = fd_step("hover3d", x, np.array([AIRBORNE], np.uint8), np.full((1, 4), hover, np.float64))
    A, B = A[0], B[0]
    S = APP_QF.copy()
    gains = np.zeros((K, 4, 12))
    for k in range(K - 1, -1, -1):
        L = np.linalg.solve(APP_RC + B.T @ S @ B, B.T @ S @ A)
        S = APP_QC + A.T @ S @ (A - B @ L)
        S = (S + S.T) / 2
        gains[k] = -L
    return gains


def app_conditions(nis, x_closed, x_open):
    """the application's two conditions on a result: nis [K,N], the closed loop's and the open-loop nominal's truth tapes
    [K,N,12]; returns the figures (asserts inside)"""
    mean_nis = float(np.mean(nis))
    assert abs(mean_nis - 6.0) <= 0.3, mean_nis
    ref = np.array([0.0, 0.0, -10.0])
    rmse = lambda x: float(np.sqrt(np.mean((x[-1][:, [0, 2, 4]] - ref) ** 2)))          # noqa: E731
    closed, opened = rmse(np.asarray(x_closed)), rmse(np.asarray(x_open))
    assert closed < 0.5 * opened, (closed, opened)
    return dict(mean_nis=mean_nis, rmse_closed=closed, rmse_open=opened, ratio=closed / opened)
