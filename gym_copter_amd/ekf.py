"""A small streaming driver on CopterVecEnv.rollout_ekf: an extended Kalman filter per env whose
measurements arrive a chunk of steps at a time, the synthetic measurements to try it on, and the chunked driver of the
smoother over its tapes, CopterVecEnv.rollout_rts.

    z = H x + e,  e ~ N(0, diag(r));     x- = step(xhat, a),  P- = A P A^T + Q;     sequential scalar updates

The filter's state (mean, covariance, flight status) is carried from call to call on the device; nothing is read by the
host."""
from .vecenv import EkfResult, RtsResult


def _torch():
    import torch
    return torch


def measure(x_tape, H, r, seed, missing=0.0):
    """Synthetic measurements of a rollout_states tape: z [K,N,M] float64 = H x + sqrt(r) N(0, 1) on x_tape's device, from
    a torch generator seeded with `seed` on that device; where a Bernoulli(missing) draw says so the entry is NaN ("no
    measurement", which rollout_ekf skips).  x_tape [K,N,12]; H [M,12]; r [M] > 0 the variances."""
    torch = _torch()
    if not isinstance(x_tape, torch.Tensor) or x_tape.dim() != 3 or x_tape.shape[2] != 12:
        raise ValueError("x_tape must be a tensor of shape (K, N, 12) (rollout_states' x)")
    if not 0.0 <= float(missing) <= 1.0:
        raise ValueError("missing must be a probability, got %r" % (missing,))
    dev = x_tape.device
    Hd = torch.as_tensor(H, dtype=torch.float64).to(dev)
    rd = torch.as_tensor(r, dtype=torch.float64).to(dev)
    if Hd.dim() != 2 or Hd.shape[1] != 12 or tuple(rd.shape) != (Hd.shape[0],):
        raise ValueError("H must have shape (M, 12) and r shape (M,), got %s and %s" % (tuple(Hd.shape), tuple(rd.shape)))
    if not bool((rd > 0).all()):
        raise ValueError("r must be positive: the measurement variances")
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    K, n, M = x_tape.shape[0], x_tape.shape[1], Hd.shape[0]
    noise = torch.randn((K, n, M), generator=gen, dtype=torch.float64, device=dev)
    z = x_tape.to(torch.float64) @ Hd.T + noise * torch.sqrt(rd)
    if missing > 0.0:
        gone = torch.rand((K, n, M), generator=gen, dtype=torch.float64, device=dev) < float(missing)
        z = torch.where(gone, torch.full_like(z, float("nan")), z)
    return z


def _chunked(actions, z, chunk, taped, state, call, carry):
    """The chunk loop of ekf(), ukf() and pf(): call(actions' chunk, z's chunk, k0, state) runs the chunk that starts at
    step k0 from the carried `state` and returns its result (buffers of the env); its fields `taped` are cloned, and
    carry(result) is the state that starts the next chunk.  Returns (the taped fields concatenated over the chunks, by
    name; the state after the last chunk; loglik, the sum of the chunks'; ok, their conjunction)."""
    torch = _torch()
    K = int(actions.shape[0])
    chunk = K if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %r" % (chunk,))
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[0] != K:
        raise ValueError("z must be a tensor of shape (K, N, M) with K = %d steps" % K)
    parts = {name: [] for name in taped}
    loglik, ok = None, None
    for k0 in range(0, K, chunk):
        res = call(actions[k0:k0 + chunk], z[k0:k0 + chunk], k0, state)
        for name in taped:
            parts[name].append(getattr(res, name).clone())
        state = carry(res)
        loglik = res.loglik.clone() if loglik is None else loglik + res.loglik
        ok = res.ok.clone() if ok is None else ok & res.ok
    return {name: torch.cat(parts[name]) for name in taped}, state, loglik, ok


def _carry_gaussian(res):
    """What a Kalman filter carries from chunk to chunk: the last mean as [12,N], the last covariance and the status."""
    return res.x[-1].T.contiguous(), res.P.clone(), res.status[-1].clone()


def ekf(env, actions, z, H, r, Q, x0, P0, status0=None, chunk=None):
    """Run env.rollout_ekf over actions [K,N,A] and z [K,N,M] in chunks of `chunk` steps (None: one call), as a filter
    whose measurements arrive `chunk` at a time: the mean, the covariance and the status after each chunk start the next.
    Returns EkfResult with the tapes of all K steps concatenated (P_tape included), P the last posterior, loglik the sum
    of the chunks' and ok their conjunction -- tensors of their own, not the env's buffers.  Every tape, P and ok are
    bit-identical to the single call's: a chunk boundary rounds nothing (float64 throughout).  loglik equals the single
    call's to rounding only: it is the sum of the chunks' sums.  The arguments are rollout_ekf's."""
    cat, (_, P, _), loglik, ok = _chunked(
        actions, z, chunk, ("x", "x_pred", "var", "nis", "status", "branch", "P_tape"), (x0, P0, status0),
        lambda a, zc, k0, s: env.rollout_ekf(a, zc, H, r, Q, s[0], s[1], status0=s[2], tape=True), _carry_gaussian)
    return EkfResult(cat["x"], cat["x_pred"], P, cat["var"], cat["nis"], loglik, cat["status"], cat["branch"], ok,
                     cat["P_tape"])


def smooth(env, actions, filt, Q, x0, P0, status0=None, chunk=None):
    """Run env.rollout_rts over the K steps of a filter's tapes in chunks of `chunk` steps (None: one call), last chunk
    first: a chunk starts from the filter's row before it (the caller's x0, P0, status0 for the first chunk) and ends in
    the smoothed starting point the chunk after it returned.  Returns RtsResult with the tapes of all K steps
    concatenated (P_tape included), x0 and P0 the smoothed starting point and ok the chunks' conjunction -- tensors of
    their own, not the env's buffers.  Every tape, x0, P0 and ok are bit-identical to the single call's: a chunk boundary
    rounds nothing (float64 throughout).  filt is the EkfResult of the whole filter with its float64 P_tape
    (rollout_ekf(..., tape=True) or ekf()); the other arguments are rollout_rts'."""
    torch = _torch()
    K = int(actions.shape[0])
    chunk = K if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be >= 1, got %r" % (chunk,))
    if not isinstance(filt, EkfResult) or filt.P_tape is None:
        raise ValueError("filt must be an EkfResult with its P_tape (rollout_ekf(..., tape=True))")
    for t, name in ((filt.x, "x"), (filt.x_pred, "x_pred"), (filt.status, "status"), (filt.P_tape, "P_tape")):
        if not isinstance(t, torch.Tensor) or t.shape[0] != K:
            raise ValueError("filt.%s must be a tensor of K = %d rows" % (name, K))
    parts, end, ok, res = [], None, None, None
    for k0 in reversed(range(0, K, chunk)):
        k1 = min(k0 + chunk, K)
        if k0 == 0:
            start = (x0, P0, status0)
        else:
            start = (filt.x[k0 - 1].T.contiguous(), filt.P_tape[k0 - 1], filt.status[k0 - 1])
        sub = EkfResult(filt.x[k0:k1], filt.x_pred[k0:k1], None, None, None, None, filt.status[k0:k1], None, None,
                        filt.P_tape[k0:k1])
        res = env.rollout_rts(actions[k0:k1], sub, Q, start[0], start[1], status0=start[2], end=end, tape=True)
        parts.append([t.clone() for t in (res.x, res.P_tape, res.var)])
        end = (res.x0.clone(), res.P0.clone())
        ok = res.ok.clone() if ok is None else ok & res.ok
    xs, pt, var = (torch.cat([p[j] for p in reversed(parts)]) for j in range(3))
    return RtsResult(xs, pt, var, end[0], end[1], ok)
