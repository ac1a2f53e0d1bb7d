"""CPU-side checks of control-limited iLQR (cs_ilqr_box_backward / cs_ilqr_box_forward): the box
programme's header compiled for the host (tests/host/boxqp_host) against its NumPy restatement bit for bit; the
restatement against brute-force enumeration of the active sets; tests/ilqr_box_ref.py's identities; both entry points
declared, exported and bound, the ctypes struct mirroring the header; bad argument blocks refused without touching a
device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boxqp_ref
import ilqr_box_ref
import lqr_ref
from gym_copter_amd import _lib
from test_rollout_lqr_cpu import _fio, _io, _lio, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "boxqp_host")
INF = np.inf


def _spd(rng, n, A):
    m = rng.standard_normal((n, A, A))
    return m @ np.swapaxes(m, 1, 2) / A + 0.2 * np.eye(A)


def _cases(A, rng):
    """(H, g, l, u) batches that reach every path of the iteration; the names say which"""
    n = 40
    H, g = _spd(rng, n, A), rng.standard_normal((n, A))
    x0 = -np.linalg.solve(H, g[..., None])[..., 0]
    # every control clamped at l: the gradient at l is w > 0 in every component
    pushed = x0 + np.linalg.solve(H, rng.uniform(0.5, 1.5, (n, A))[..., None])[..., 0]
    out = {
        "interior": (H, g, x0 - 1.0, x0 + 1.0),
        "all_clamped": (H, g, pushed, pushed + 1.0),
        "mixed": (H, g, x0 - rng.uniform(-0.5, 0.5, (n, A)) - 0.25, x0 + rng.uniform(-0.5, 0.5, (n, A)) + 0.25),
        "infinite": (H, g, np.full((n, A), -INF), np.full((n, A), INF)),
        "half_infinite": (H, g, x0 + rng.uniform(-0.3, 0.3, (n, A)), np.full((n, A), INF)),
    }
    l, u = out["mixed"][2:]
    out["mixed"] = (H, g, np.minimum(l, u), np.maximum(l, u))
    # a bound equal to the start: the unconstrained minimiser as the device computes it sits exactly on l (or u)
    fac, _ = lqr_ref.cholesky(H)
    start = -lqr_ref.chol_solve(fac, g)
    out["bound_is_start"] = (H, g, np.where(np.arange(A) % 2 == 0, start, start - 1.0),
                             np.where(np.arange(A) % 2 == 0, start + 1.0, start))
    pin = rng.uniform(-1, 1, (n, A))
    out["lo_equals_hi"] = (H, g, pin, pin.copy())
    bad = H.copy()
    bad[:, A - 1, A - 1] = -1.0                               # a non-positive pivot (of H and of most free blocks)
    out["bad_pivot"] = (bad, g, x0 - 0.3, x0 + 0.3)
    gn = g.copy()
    gn[:, 0] = np.nan
    out["nan_in_g"] = (H, gn, x0 - 0.3, x0 + 0.3)
    return out


def _run_host(A, H, g, l, u, k, cap):
    fmt = lambda v: " ".join("nan" if np.isnan(x) else ("inf" if x == INF else "-inf" if x == -INF else float(x).hex())
                             for x in np.ravel(v))
    lines = ["%d %s %s %s %s %s %d" % (A, fmt(H[i]), fmt(g[i]), fmt(l[i]), fmt(u[i]), fmt(k[i]), cap[i])
             for i in range(len(g))]
    p = subprocess.run([HOST], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    rows = [ln.split() for ln in p.stdout.strip().split("\n")]
    assert len(rows) == len(g)
    ints = np.array([[int(v) for v in r[:5]] for r in rows])
    vals = np.array([[float.fromhex(v) if v not in ("nan", "-nan", "inf", "-inf") else float(v.replace("-nan", "nan"))
                      for v in r[5:]] for r in rows])
    return ints, vals[:, :A], vals[:, A:A + A * A].reshape(-1, A, A), vals[:, A + A * A:]


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)                      # (a NaN's sign and payload are not the arithmetic's)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())


@pytest.mark.parametrize("A", [1, 2, 4])
def test_host_program_matches_the_restatement_bit_for_bit(A):
    """Fails without the feature: tests/host/boxqp_host is boxqp_solve.h compiled for the host."""
    assert os.path.exists(HOST), "make -C gym_copter_amd/csrc host"
    rng = np.random.default_rng(240 + A)
    seen_iters, seen_sets = set(), set()
    for name, (H, g, l, u) in _cases(A, rng).items():
        k = rng.standard_normal(g.shape)
        cap = np.where(np.arange(len(g)) % 8 == 7, 0, 16)     # every eighth problem: the clamped start only
        ref = boxqp_ref.solve(H, g, l, u, cap)
        ints, x, fac, kk = _run_host(A, H, g, l, u, k, cap)
        assert np.array_equal(ints[:, 0], ref["pd"].astype(int)), name
        assert np.array_equal(ints[:, 1], ref["ok"].astype(int)), name
        assert np.array_equal(ints[:, 2], ref["iters"]), name
        assert np.array_equal(ints[:, 3], ref["lower"]) and np.array_equal(ints[:, 4], ref["upper"]), name
        assert _same_bits(x, ref["x"]), name
        assert _same_bits(np.tril(fac), ref["fac"]), name
        assert _same_bits(kk, boxqp_ref.gain(ref, k)), name
        seen_iters |= set(ref["iters"].tolist())
        seen_sets |= set((ref["lower"] | (ref["upper"] << 4)).tolist())
        full = cap > 0
        if name == "infinite":                                # the unconstrained arithmetic bit for bit
            fach, _ = lqr_ref.cholesky(H)
            assert _same_bits(x, -lqr_ref.chol_solve(fach, g)) and _same_bits(np.tril(fac)[full], np.tril(fach)[full])
            assert _same_bits(kk[full], -lqr_ref.chol_solve(fach, k)[full])
            assert (ints[full, 2] == 1).all() and (ints[:, 3:] == 0).all() and ints[:, 1].all()
        if name == "interior":
            assert (ints[:, 3:] == 0).all() and ints[:, 1].all()
        if name == "all_clamped":
            assert (ints[full, 3] == (1 << A) - 1).all() and (kk[full] == 0).all() and _same_bits(x[full], l[full])
        if name == "lo_equals_hi":
            assert _same_bits(x, l) and (kk[full] == 0).all()
        if name == "bad_pivot":
            assert not ints[:, 0].any() and not ints[full, 1].all()
        if name == "nan_in_g":
            assert np.isnan(x).any(axis=1).all()
    # (one control: the clamped start is the minimiser, and the first iteration says so)
    assert {0, 1} <= seen_iters and (A == 1 or (max(seen_iters) >= 2 and len(seen_sets) > 4))


@pytest.mark.parametrize("A", [1, 2, 4])
def test_restatement_finds_the_enumerated_minimiser(A):
    """Passes without the feature (NumPy only): boxqp_ref against brute-force enumeration of the 3^A active sets on
    random SPD problems -- the solution to 1e-12 scaled, the same clamp set wherever the enumerated multipliers exceed
    1e-9, the iteration cap never reached."""
    rng = np.random.default_rng(77 + A)
    n = 400
    H, g = _spd(rng, n, A), 2.0 * rng.standard_normal((n, A))
    c = rng.standard_normal((n, A))
    w = rng.uniform(0.0, 1.5, (n, A))
    l, u = c - w, c + w
    l[rng.random((n, A)) < 0.1] = -INF
    u[rng.random((n, A)) < 0.1] = INF
    sol = boxqp_ref.solve(H, g, l, u)
    assert sol["ok"].all() and sol["iters"].max() < boxqp_ref.ITERS
    assert ((sol["x"] >= l) & (sol["x"] <= u)).all()
    sets = 0
    for i in range(n):
        x, st, mult = boxqp_ref.brute_force(H[i], g[i], l[i], u[i])
        assert np.max(np.abs(sol["x"][i] - x)) <= 1e-12 * max(1.0, np.abs(x).max()), i
        strict = (st == 0) | (mult > 1e-9 * max(1.0, np.abs(g[i]).max()))
        if strict.all():
            assert np.array_equal(sol["clamped"][i], st != 0), i
            assert sol["lower"][i] == sum(1 << a for a in range(A) if st[a] == -1), i
            sets += 1
    assert sets > 0.9 * n
    assert sol["clamped"].any(-1).mean() > 0.3                # the box binds often enough to mean something
    ld = boxqp_ref.solve(H, g, l, u, dtype=np.longdouble)     # the dtype is a parameter
    assert ld["x"].dtype == np.longdouble and np.max(np.abs(ld["x"].astype(np.float64) - sol["x"])) < 1e-10


@pytest.mark.parametrize("A", [1, 2, 4])
def test_backward_restatement_identities(A):
    """Passes without the feature (NumPy only): with infinite bounds ilqr_box_ref.lqr_box_backward equals
    lqr_ref.lqr_backward exactly, and for K = 1 its d is the dense box-QP optimum of the step's own model."""
    rng = np.random.default_rng(900 + A)
    K, N = 5, 6
    probs = [_problem(rng, K, A) for _ in range(N)]
    Ab = np.stack([p[0] for p in probs], 1)
    Bb = np.stack([p[1] for p in probs], 1)
    Q, Qf, R = probs[0][2], probs[0][3], probs[0][4]
    q = np.stack([p[5] for p in probs], 1)
    r = np.stack([p[6] for p in probs], 1)
    abar = rng.uniform(0.2, 0.8, (K, N, A)).astype(np.float32)
    free = lqr_ref.lqr_backward(Ab, Bb, Q, R, q, r, Q_final=Qf, mu=0.25)
    box = ilqr_box_ref.lqr_box_backward(Ab, Bb, Q, R, abar, -INF, INF, q, r, Q_final=Qf, mu=0.25)
    for key in ("K", "d", "dV", "S0", "s0", "ok"):
        assert np.array_equal(free[key], box[key]), key
    assert not box["clamped"].any() and (box["iters"] == 1).all()
    # K = 1: one step's model is 1/2 d^T (R + B^T Q_f B) d + (r + B^T q)^T d, minimised over the box by enumeration
    one = ilqr_box_ref.lqr_box_backward(Ab[:1], Bb[:1], Q, R, abar[:1], 0.45, 0.55, q[:1], r[:1], Q_final=Qf)
    binding = 0
    for i in range(N):
        B = Bb[0, i]
        H, g = R + B.T @ Qf @ B, r[0, i] + B.T @ q[0, i]
        l, u = np.float32(0.45).astype(np.float64) - abar[0, i], np.float32(0.55).astype(np.float64) - abar[0, i]
        x, st, _ = boxqp_ref.brute_force(H, g, l, u)
        assert np.max(np.abs(one["d"][0, i] - x)) <= 1e-12
        assert (np.abs(one["K"][0, i][st != 0]) == 0).all()
        binding += int((st != 0).any())
    assert binding > 0 and one["ok"].all()
    # a resetting lane takes the clamped start and no iteration
    rs = ilqr_box_ref.lqr_box_backward(Ab, Bb, Q, R, abar, 0.45, 0.55, q, r, resetting=np.arange(N) < 2)
    assert (rs["iters"][0, :2] == 0).all() and (rs["iters"][0, 2:] > 0).all() and (rs["iters"][1:] > 0).all()


def test_forward_clamp_restatement():
    """Passes without the feature (NumPy only)."""
    a = np.array([[0.1, 0.5, np.nan, 0.9], [0.3, 0.7, 0.300001, 0.2]], np.float32)
    out, bits = ilqr_box_ref.clamp_actions(a, 0.3, np.array([0.7, 0.6, 0.7, 0.7], np.float32))
    assert out.dtype == np.float32 and np.isnan(out[0, 2])
    assert out[0, [0, 1, 3]].tolist() == [np.float32(0.3), 0.5, np.float32(0.7)]
    assert bits.tolist() == [0b10000001, 0b00101000]


def _bio(**kw):
    bio = _lib.RolloutIlqrBoxIO()
    bio.struct_size = C.sizeof(bio)
    bio.lo_dev, bio.hi_dev, bio.clamped_dev = 0x8000, 0x9000, 0xa000
    for k, v in kw.items():
        setattr(bio, k, v)
    return bio


def test_entry_points_are_declared_exported_and_bound():
    """Fails without the feature."""
    lib = _lib.load()
    for name, second in (("cs_ilqr_box_backward", "cs_rollout_lqr_io"), ("cs_ilqr_box_forward", "cs_rollout_feedback_io")):
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const %s\* \w+,\s*"
                         r"const cs_ilqr_box_io\* bio,\s*void\* stream\);" % (name, second), HEADER)
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes[3] is C.POINTER(_lib.RolloutIlqrBoxIO)
    body = re.search(r"typedef struct cs_ilqr_box_io \{(.*?)\} cs_ilqr_box_io;", HEADER, re.S).group(1)
    plain = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"([\w \*]+?)\b(\w+);", plain)
    M = _lib.RolloutIlqrBoxIO
    assert [m for _, m in fields] == [f for f, _ in M._fields_]
    at = 0
    for (ctype, member), (_, mirror) in zip(fields, M._fields_):                 # field by field: type, offset, size
        size = 8 if "*" in ctype else 4
        assert (mirror is C.c_void_p) == ("*" in ctype) and C.sizeof(mirror) == size, member
        at = (at + size - 1) // size * size
        assert getattr(M, member).offset == at, member
        at += size
    assert C.sizeof(M) == at == 8 + 4 * 8
    assert lib.cs_version() == _lib.ABI_VERSION == 5
    import gym_copter_amd
    from gym_copter_amd import sharded
    assert gym_copter_amd.BoxGains._fields == ("K", "d", "dV", "S0", "s0", "ok", "clamped", "iters")
    for name in ("rollout_lqr_box", "rollout_feedback_box_states"):
        assert callable(getattr(gym_copter_amd.CopterVecEnv, name)) and name in sharded._LOCAL_ROLLOUTS


def test_backward_refuses_bad_arguments_without_a_device():
    """Fails without the feature.  Every block is checked before the context, bio last."""
    lib = _lib.load()
    fn = lib.cs_ilqr_box_backward
    who = b"cs_ilqr_box_backward: "
    assert fn(None, None, None, None, None) == _lib.ERR_ARG and lib.cs_last_error() == who + b"null io"
    assert fn(None, C.byref(_io(x_dev=None)), C.byref(_lio()), C.byref(_bio()), None) == _lib.ERR_ARG
    assert b"tape" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), None, C.byref(_bio()), None) == _lib.ERR_ARG and b"null lio" in lib.cs_last_error()
    bad = _lio(struct_size=C.sizeof(_lib.RolloutLqrIO) - 8)
    assert fn(None, C.byref(_io()), C.byref(bad), C.byref(_bio()), None) == _lib.ERR_ABI
    for mu in (-1.0, float("nan")):
        assert fn(None, C.byref(_io()), C.byref(_lio(mu=mu)), C.byref(_bio()), None) == _lib.ERR_ARG
        assert lib.cs_last_error().startswith(who + b"mu must be")
    assert fn(None, C.byref(_io()), C.byref(_lio()), None, None) == _lib.ERR_ARG and b"null bio" in lib.cs_last_error()
    # a wrong struct_size is reported first, whatever else is wrong with the block
    bad = _bio(struct_size=C.sizeof(_lib.RolloutIlqrBoxIO) + 8, lo_dev=None)
    assert fn(None, C.byref(_io()), C.byref(_lio()), C.byref(bad), None) == _lib.ERR_ABI
    assert lib.cs_last_error().startswith(who + b"bio->struct_size 48 != 40")
    for key in ("lo_dev", "hi_dev"):
        assert fn(None, C.byref(_io()), C.byref(_lio()), C.byref(_bio(**{key: None})), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == who + b"lo_dev and hi_dev are required"
    assert fn(None, C.byref(_io()), C.byref(_lio()), C.byref(_bio(reserved_=1)), None) == _lib.ERR_ARG
    assert b"reserved_" in lib.cs_last_error()
    for extra in (dict(), dict(iters_dev=0xb000), dict(clamped_dev=None)):      # ... as far as the context
        assert fn(None, C.byref(_io()), C.byref(_lio(mu=0.5)), C.byref(_bio(**extra)), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"


def test_forward_refuses_bad_arguments_without_a_device():
    """Fails without the feature."""
    lib = _lib.load()
    fn = lib.cs_ilqr_box_forward
    who = b"cs_ilqr_box_forward: "
    assert fn(None, None, None, None, None) == _lib.ERR_ARG and lib.cs_last_error() == who + b"null io"
    assert fn(None, C.byref(_io()), None, C.byref(_bio()), None) == _lib.ERR_ARG and b"null fio" in lib.cs_last_error()
    bad = _fio(struct_size=C.sizeof(_lib.RolloutFeedbackIO) + 8)
    assert fn(None, C.byref(_io()), C.byref(bad), C.byref(_bio()), None) == _lib.ERR_ABI
    for key in ("K_dev", "d_dev", "alpha_dev", "actions_out_dev"):
        assert fn(None, C.byref(_io()), C.byref(_fio(**{key: None})), C.byref(_bio()), None) == _lib.ERR_ARG
        assert lib.cs_last_error().startswith(who) and b"required" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_fio(xbar_dev=None)), C.byref(_bio()), None) == _lib.ERR_ARG
    assert b"xbar_dev" in lib.cs_last_error()
    assert fn(None, C.byref(_io()), C.byref(_fio()), None, None) == _lib.ERR_ARG and b"null bio" in lib.cs_last_error()
    bad = _bio(struct_size=C.sizeof(_lib.RolloutIlqrBoxIO) - 8, iters_dev=0xb000)
    assert fn(None, C.byref(_io()), C.byref(_fio()), C.byref(bad), None) == _lib.ERR_ABI
    assert lib.cs_last_error().startswith(who + b"bio->struct_size 32 != 40")
    assert fn(None, C.byref(_io()), C.byref(_fio()), C.byref(_bio(hi_dev=None)), None) == _lib.ERR_ARG
    assert lib.cs_last_error() == who + b"lo_dev and hi_dev are required"
    assert fn(None, C.byref(_io()), C.byref(_fio()), C.byref(_bio(iters_dev=0xb000)), None) == _lib.ERR_ARG
    assert lib.cs_last_error().startswith(who + b"iters_dev") and b"must be NULL" in lib.cs_last_error()
    for extra in (dict(), dict(clamped_dev=None)):
        assert fn(None, C.byref(_io(num_steps=1)), C.byref(_fio(xbar_dev=None)), C.byref(_bio(**extra)), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"
