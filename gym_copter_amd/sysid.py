"""System identification on the device: identify() fits vehicle rows (and optionally the start's pending force) to an
observed trajectory by Levenberg-Marquardt, its Jacobian the forward-mode tangents of CopterVecEnv.rollout_jvp -- one
rollout_states and one rollout_jvp per iteration, the p x p normal equations reduced and solved with torch.  DESIGN.md
section 26."""
import collections

from ._wire import _torch

# identify()'s result: vehicle [12,N] float64 (the fitted table), force [3,N] newtons (None without fit_force),
# cost [N] (the weighted squared trajectory error at the result; [1] with shared=True), history = {"cost":
# [iterations + 1, N], "accepted": [iterations, N] bool, "damping": [iterations, N]} (device tensors)
IdentifyResult = collections.namedtuple("IdentifyResult", "vehicle force cost history")

_MAX_LOG_STEP = 1.0     # a step changes a vehicle row by at most a factor e
_ACCEPT_DIV, _REJECT_MUL = 3.0, 10.0


def identify(env, actions_k, x_obs, fit=("M", "Ix", "Iy"), vehicle0=None, fit_force=False, state=None, weights=None,
             iterations=8, damping=1e-3, shared=False):
    """Fit the vehicle rows `fit` (names of env.VEHICLE_ROWS), per env, to the observed states x_obs [K,N,12] of the
    rollout of actions_k [K,N,A] from `state` (rollout_states' start: None = the stored state): Levenberg-Marquardt on
    the weighted trajectory error sum(((x - x_obs) * w)^2), w = `weights` (broadcastable to [K,N,12]) or, by default,
    1 / max_k |x_obs| per env and slot, clamped at 1e-3.  The unknowns are the logs of the chosen rows (they stay
    positive) and, with fit_force=True, the start's pending force in newtons (state is then required; state["force"],
    or zero, is the first guess).  vehicle0 [12,N] float64 is the first guess and the known rows (None: the env's
    configured vehicle for every env).

    Each iteration makes one rollout_states(vehicle=) at the trial point and one rollout_jvp with D = p directions (the
    log-parameter directions theta_j e_j, the force's unit directions); J^T J [N,p,p] and J^T r are reduced with torch
    on the device and solved by a batched Cholesky factorisation with Marquardt's diagonal scaling, (J^T J + damping
    diag(J^T J)) delta = -J^T r.  Acceptance is per env: a trial point with a smaller cost is taken and that env's
    damping divided by 3, any other is dropped and the damping multiplied by 10.  shared=True sums the normal equations
    over the envs for ONE common vehicle (vehicle0's columns must then be equal; not with fit_force).  Returns
    IdentifyResult(vehicle, force, cost, history).  Not available with action_arith="float32".  A
    ShardedCopterVecEnv is fitted shard-locally; shared=True on a sharded env is out of scope and refused."""
    torch = _torch()
    local = getattr(env, "local", env)
    if shared and local is not env:
        raise ValueError("identify(shared=True) is not available on a sharded env")
    if shared and fit_force:
        raise ValueError("identify(shared=True) fits one common vehicle: fit_force is not available with it")
    if fit_force and state is None:
        raise ValueError("fit_force=True needs an explicit start `state` (its 'force' is what is fitted)")
    rows = local.VEHICLE_ROWS
    fit = tuple(fit)
    unknown = [k for k in fit if k not in rows]
    if unknown or len(set(fit)) != len(fit) or (not fit and not fit_force):
        raise ValueError("fit must name distinct rows of %s (or fit_force=True), got %s" % (rows, fit))
    if not isinstance(iterations, int) or iterations < 1:
        raise ValueError("iterations must be an int >= 1, got %r" % (iterations,))
    if not float(damping) > 0.0:
        raise ValueError("damping must be > 0, got %r" % (damping,))
    dev, n = local.device, local.num_envs
    f64 = dict(dtype=torch.float64, device=dev)
    x_obs = torch.as_tensor(x_obs, **f64)
    if x_obs.dim() != 3 or x_obs.shape[1:] != (n, 12):
        raise ValueError("x_obs must have shape (K, %d, 12), got %s" % (n, tuple(x_obs.shape)))
    K = x_obs.shape[0]
    if vehicle0 is None:
        base = torch.tensor([float(getattr(local.config, k)) for k in rows], **f64)[:, None].repeat(1, n)
    else:
        base = torch.as_tensor(vehicle0, **f64).clone()
        if tuple(base.shape) != (len(rows), n):
            raise ValueError("vehicle0 must have shape (%d, %d), got %s" % (len(rows), n, tuple(base.shape)))
    idx = torch.tensor([rows.index(k) for k in fit], dtype=torch.long, device=dev)
    pv = len(fit)
    p = pv + (3 if fit_force else 0)
    if (base[idx] <= 0).any():
        raise ValueError("vehicle0: the rows to fit must be positive (their logs are the unknowns)")
    if shared and not bool((base == base[:, :1]).all()):
        raise ValueError("identify(shared=True): vehicle0's columns must be equal")
    if weights is None:
        w = 1.0 / x_obs.abs().amax(dim=0, keepdim=True).clamp_min(1e-3)
    else:
        w = torch.as_tensor(weights, **f64)
    w = w.expand(K, n, 12)
    state = None if state is None else dict(state)
    force0 = None
    if fit_force:
        force0 = state.get("force")
        force0 = torch.zeros((3, n), **f64) if force0 is None else torch.as_tensor(force0, **f64).clone()

    def point(theta):
        """theta [p, n] -> the vehicle table and the start of that point"""
        veh = base.clone()
        veh[idx] = base[idx] * torch.exp(theta[:pv])
        st = state
        if fit_force:
            st = dict(state)
            st["force"] = force0 + theta[pv:]
        return veh, st

    def linearise(theta, jac=True):
        """the cost [n], J^T J [n, p, p] and J^T r [n, p] at theta: one rollout, one rollout_jvp (jac=False: the cost
        alone, the last iteration's trial point)"""
        veh, st = point(theta)
        r = env.rollout_states(actions_k, state=st, vehicle=veh)
        res = (r.x - x_obs) * w
        cost = (res * res).sum(dim=(0, 2))
        if not jac:
            return (cost.sum(0, keepdim=True) if shared else cost), None, None
        t_v = torch.zeros((p, len(rows), n), **f64)
        t_v[torch.arange(pv, device=dev), idx] = veh[idx]       # d / d log p_j = p_j d / d p_j
        t_f = None
        if fit_force:
            t_f = torch.zeros((p, 3, n), **f64)
            t_f[pv + torch.arange(3, device=dev), torch.arange(3, device=dev)] = 1.0
        J = env.rollout_jvp(actions_k, r, t_vehicle=t_v, t_force=t_f, state=st, vehicle=veh, check_vehicle=False).x
        Jw = J * w
        jtj = torch.einsum("aknj,bknj->nab", Jw, Jw)
        jtr = torch.einsum("aknj,knj->na", Jw, res)
        if shared:
            cost, jtj, jtr = cost.sum(0, keepdim=True), jtj.sum(0, keepdim=True), jtr.sum(0, keepdim=True)
        return cost, jtj, jtr

    m = 1 if shared else n                                      # independent problems
    theta = torch.zeros((p, m), **f64)
    lam = torch.full((m,), float(damping), **f64)
    cost, jtj, jtr = linearise(theta.expand(p, n))
    hist_cost, hist_acc, hist_lam = [cost.clone()], [], []
    eye = torch.eye(p, **f64)
    for it in range(iterations):
        diag = torch.diagonal(jtj, dim1=1, dim2=2).clamp_min(1e-300)
        A = jtj + eye * (lam[:, None] * diag)[:, :, None]
        L, info = torch.linalg.cholesky_ex(A)
        ok = info == 0
        L = torch.where(ok[:, None, None], L, eye)
        delta = -torch.cholesky_solve(jtr[:, :, None], L)[:, :, 0]         # [m, p]
        delta = torch.where(ok[:, None] & torch.isfinite(delta).all(dim=1, keepdim=True), delta,
                            torch.zeros_like(delta))
        delta[:, :pv] = delta[:, :pv].clamp(-_MAX_LOG_STEP, _MAX_LOG_STEP)
        trial = theta + delta.t()
        last = it == iterations - 1
        cost_t, jtj_t, jtr_t = linearise(trial.expand(p, n), jac=not last)
        accept = ok & (cost_t < cost)                           # (a NaN cost is not smaller)
        theta = torch.where(accept[None, :], trial, theta)
        cost = torch.where(accept, cost_t, cost)
        if not last:
            jtj = torch.where(accept[:, None, None], jtj_t, jtj)
            jtr = torch.where(accept[:, None], jtr_t, jtr)
        hist_lam.append(lam.clone())
        lam = torch.where(accept, lam / _ACCEPT_DIV, lam * _REJECT_MUL)
        hist_acc.append(accept)
        hist_cost.append(cost.clone())
    veh, st = point(theta.expand(p, n))
    history = {"cost": torch.stack(hist_cost), "accepted": torch.stack(hist_acc), "damping": torch.stack(hist_lam)}
    return IdentifyResult(veh, st["force"] if fit_force else None, cost, history)
