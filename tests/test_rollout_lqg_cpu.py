"""CPU-side checks of cs_rollout_lqg: the entry point declared, exported and bound, the ctypes struct mirroring the header
field by field; bad argument blocks refused without touching a device; the feedback law and the measurement formation of
the kernel's own header compiled for the host (tests/host/lqg_law_host) against the NumPy restatement the GPU tests use
(tests/lqg_ref.py), bit for bit; and the inputs of the GPU tests on the CPU restatement of the whole loop -- the float64
oracle as the truth, tests/ekf_ref.py with central-difference Jacobians as the filter: the starts put an estimate on the
other side of a touchdown from the truth, and the application's conditions hold with their margins."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ekf_ref
import lqg_ref
from gym_copter_amd import _lib
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
HOST = os.path.join(ROOT, "tests", "host", "lqg_law_host")


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_rollout_lqg\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_rollout_lqg_io\* \w+,"
                     r"\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_rollout_lqg") and "cs_rollout_lqg" in _lib.SYMBOLS
    assert lib.cs_rollout_lqg.argtypes[2] is C.POINTER(_lib.RolloutLqgIO)
    import gym_copter_amd
    assert callable(gym_copter_amd.lqg) and callable(gym_copter_amd.measurement_noise)
    assert callable(gym_copter_amd.CopterVecEnv.rollout_lqg)
    assert gym_copter_amd.LqgResult._fields == ("rollout", "actions", "z", "filter")


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_rollout_lqg_io \{(.*?)\} cs_rollout_lqg_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.RolloutLqgIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.RolloutLqgIO._fields_):
        size = 8 if "*" in ctype else 4
        assert C.sizeof(mirror) == size, name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.RolloutLqgIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.RolloutLqgIO) == offset == 16 + 21 * 8


def test_the_abi_version_is_unchanged():
    assert _lib.load().cs_version() == 5 == _lib.ABI_VERSION
    assert re.search(r"#define CS_ABI_VERSION 5\b", HEADER)


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev, io.x_dev, io.status_dev = 0x1000, 0x4000, 0x5000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


REQUIRED = ("K_dev", "xbar_dev", "e_dev", "H_dev", "r_dev", "Q_dev", "P0_dev", "xhat0_dev", "status0_dev",
            "actions_out_dev")


def _lio(**kw):
    lio = _lib.RolloutLqgIO()
    lio.struct_size = C.sizeof(lio)
    lio.num_meas = 6
    for j, key in enumerate(REQUIRED):
        setattr(lio, key, 0x10000 + 0x1000 * j)
    for k, v in kw.items():
        setattr(lio, k, v)
    return lio


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_lqg
    err = lib.cs_last_error
    assert fn(None, None, None, None) == _lib.ERR_ARG and b"null io" in err()
    assert fn(None, C.byref(_io(struct_size=8)), C.byref(_lio()), None) == _lib.ERR_ABI
    assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG and b"null lio" in err()
    # a wrong struct_size is reported before anything else in the block
    bad = _lio(struct_size=C.sizeof(_lib.RolloutLqgIO) - 8, num_meas=99, H_dev=None, out_dtype=7)
    assert fn(None, C.byref(_io(gx_dev=0xb000)), C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in err()
    assert fn(None, C.byref(_io(num_steps=0)), C.byref(_lio()), None) == _lib.ERR_ARG and b"num_steps" in err()
    assert fn(None, C.byref(_io(actions_dev=None)), C.byref(_lio()), None) == _lib.ERR_ARG and b"actions_dev" in err()
    # the truth's start is cs_rollout_states': stored (no start pointer at all) or explicit (x and status, then the rest)
    assert fn(None, C.byref(_io(start_force_dev=0xb000)), C.byref(_lio()), None) == _lib.ERR_ARG
    assert b"start_x_dev is required" in err()
    assert fn(None, C.byref(_io(start_x_dev=0x2000)), C.byref(_lio()), None) == _lib.ERR_ARG
    assert b"start_status_dev" in err()
    for key in ("gx_dev", "gr_dev", "g_actions_dev", "g_x0_dev"):
        assert fn(None, C.byref(_io(**{key: 0xb000})), C.byref(_lio()), None) == _lib.ERR_ARG
        assert b"must be NULL" in err()
    assert fn(None, C.byref(_io()), C.byref(_lio(out_dtype=5)), None) == _lib.ERR_ARG and b"out_dtype" in err()
    for m in (0, -1, 13):
        assert fn(None, C.byref(_io()), C.byref(_lio(num_meas=m)), None) == _lib.ERR_ARG and b"num_meas" in err()
    for key in REQUIRED:
        assert fn(None, C.byref(_io()), C.byref(_lio(**{key: None})), None) == _lib.ERR_ARG and b"required" in err(), key
    for key in ("K_dev", "xbar_dev", "e_dev", "H_dev", "r_dev", "Q_dev", "P0_dev", "xhat0_dev", "z_dev", "xhat_dev",
                "x_pred_dev", "P_tape_dev", "nis_dev", "loglik_dev", "var_dev", "P_dev"):
        assert fn(None, C.byref(_io()), C.byref(_lio(**{key: 0xc004})), None) == _lib.ERR_ARG and b"aligned" in err(), key
    for key in ("x_dev", "reward_dev"):
        assert fn(None, C.byref(_io(**{key: 0x4004})), C.byref(_lio()), None) == _lib.ERR_ARG and b"aligned" in err()
    full = dict(start_x_dev=0x2000, start_status_dev=0x3001)
    for key in ("start_x_dev", "start_force_dev", "start_prev_shaping_dev"):
        io = _io(**dict(full, **{key: 0x2004}))
        assert fn(None, C.byref(io), C.byref(_lio()), None) == _lib.ERR_ARG and b"aligned" in err(), key
    assert fn(None, C.byref(_io(actions_dev=0x1002)), C.byref(_lio()), None) == _lib.ERR_ARG and b"4-B aligned" in err()
    assert fn(None, C.byref(_io()), C.byref(_lio(actions_out_dev=0xc002)), None) == _lib.ERR_ARG
    assert b"4-B aligned" in err()
    # float32 outputs need 4 bytes only; the byte arrays need none
    ok32 = _lio(out_dtype=_lib.JAC_F32, P_tape_dev=0xc004, nis_dev=0xc004, fstatus_dev=0xc001, status0_dev=0xc003)
    assert fn(None, C.byref(_io()), C.byref(ok32), None) == _lib.ERR_ARG and err() == b"null context"
    # every output is optional, both start forms and the truth's reward and flags are accepted ... as far as the context
    assert fn(None, C.byref(_io(x_dev=None, status_dev=None)), C.byref(_lio()), None) == _lib.ERR_ARG
    assert err() == b"null context"
    io = _io(reward_dev=0x6000, terminated_dev=0x7001, truncated_dev=0x7003, start_force_dev=0x8000,
             start_prev_shaping_dev=0x9000, **full)
    assert fn(None, C.byref(io), C.byref(_lio()), None) == _lib.ERR_ARG and err() == b"null context"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the law and the measurement on the host, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _host(A, M, xhat, xbar, x, abar, gains, H, e):
    args = [repr(float(v)) for v in np.concatenate([xhat, xbar, x])]
    for c in range(A):
        args += [repr(float(abar[c]))] + [repr(float(v)) for v in gains[c]]
    for i in range(M):
        args += [repr(float(v)) for v in H[i]] + [repr(float(e[i]))]
    out = subprocess.run([HOST, str(A), str(M)] + args, check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == A + M
    v = np.array([float.fromhex(s) if "nan" not in s else np.nan for s in out])
    return v[:A].astype(np.float32), v[A:]


@pytest.mark.parametrize("A", [1, 2, 4])
@pytest.mark.parametrize("M", [1, 6, 12])
def test_host_law_and_measurement_match_the_restatement_bit_for_bit(A, M):
    rng = np.random.default_rng(100 * A + M)
    for trial in range(4):
        xhat, xbar, x = rng.standard_normal((3, 12)) * np.array([[3.0], [3.0], [5.0]])
        abar = rng.uniform(-0.2, 1.2, A).astype(np.float32)
        gains = rng.standard_normal((A, 12)) * 10.0 ** rng.integers(-3, 1)
        H = rng.standard_normal((M, 12))
        e = rng.standard_normal(M) * 0.3
        e[trial % M] = np.nan                                      # (one "no measurement" per trial)
        a, z = _host(A, M, xhat, xbar, x, abar, gains, H, e)
        want_a = lqg_ref.law(abar[None], gains[None], xhat[None], xbar[None])[0]
        want_z = lqg_ref.measure(H, x[None], e[None])[0]
        assert a.dtype == want_a.dtype == np.float32 and np.array_equal(a.view(np.uint32), want_a.view(np.uint32))
        assert np.isnan(z[trial % M]) and np.isnan(want_z[trial % M])
        keep = ~np.isnan(e)
        assert np.array_equal(z[keep].view(np.uint64), want_z[keep].view(np.uint64))
        if M > 1:
            assert np.isfinite(z[keep]).all()


def test_the_measurement_restatement_is_order_sensitive():
    """the bit-for-bit comparison of the float64 measurement can tell the kernel's order from another: summing from the
    last term gives other bits (the law's one rounding to float32 hides such a difference; its order is the header's)"""
    rng = np.random.default_rng(7)
    H, x = rng.standard_normal((6, 12)), rng.standard_normal((64, 12))
    zero = np.zeros((64, 6))
    assert (lqg_ref.measure(H, x, zero) != lqg_ref.measure(H[:, ::-1], x[:, ::-1], zero)).any()
    assert np.array_equal(lqg_ref.measure(H, x, zero), (H[None] * x[:, None]).cumsum(-1)[..., -1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. the GPU tests' inputs on the CPU restatement of the whole loop
# ---------------------------------------------------------------------------------------------------------------------
def test_the_starts_put_an_estimate_on_the_other_side_of_a_touchdown():
    """tests/test_gpu_rollout_lqg.py's Lander3D case (seed 901, N = 300, K = 16) restated on the oracle: the filter's
    status differs from the truth's somewhere, the law pushes motors outside [0, 1] that the nominal leaves inside, and
    the feedback moves nearly every action"""
    from branch_fd import run_rollout
    n, K = 300, 16
    p = lqg_ref.problem("lander3d", n, K, np.random.default_rng(901), hover_action())
    nominal, _ = run_rollout("lander3d", p["x0"], p["st0"], p["abar"].astype(np.float64), force=p["force"])
    xbar = lqg_ref.reference_tape(p["x0"], nominal["x"])
    out = lqg_ref.closed_loop("lander3d", p["x0"], p["st0"], p["abar"], p["gains"], xbar, p["e"], p["H"], p["r"], p["Q"],
                              p["xhat0"], p["P0"], p["fst0"], force=p["force"])
    differ = out["fstatus"] != out["status"]
    print("filter status != truth status in %d of %d (k, env) pairs, %d envs" % (differ.sum(), differ.size,
                                                                                differ.any(axis=0).sum()))
    assert differ.any(axis=0).sum() >= 10
    a, abar = out["actions"], p["abar"]
    inside = (abar >= 0) & (abar <= 1)
    assert (inside & ((a < 0) | (a > 1))).mean() >= 0.01
    assert (a != abar).mean() >= 0.9
    assert np.isfinite(out["x"]).all() and np.isfinite(out["xhat"]).all()


def test_application_conditions_hold_on_the_oracle_restatement():
    """The application of the GPU tests (Hover3D, 300 envs, 192 steps, positions and angles measured with sigma = 0.1 m
    and 0.01 rad, gains of one LQR recursion at hover) on the restatement, NumPy seed 1: mean NIS within 6 +- 0.3, and a
    final position RMSE <= 0.25 of the open-loop nominal's from the same starts (measured: mean NIS 5.978, 0.170 m against
    0.950 m, ratio 0.179; the device gives the same digits) -- half the bar the device must meet."""
    from branch_fd import run_rollout
    ah = hover_action()
    abar, x0, xhat0, xbar, e, H, r = lqg_ref.app_inputs(ah, seed=1)
    n, K = lqg_ref.APP_N, lqg_ref.APP_K
    gains = np.broadcast_to(lqg_ref.app_gains(ah)[:, None], (K, n, 4, 12)).copy()
    st = np.full(n, AIRBORNE, np.uint8)
    P0 = np.repeat(ekf_ref.APP_P0[None], n, axis=0)
    out = lqg_ref.closed_loop("hover3d", x0, st, abar, gains, xbar, e, H, r, ekf_ref.APP_Q, xhat0, P0, st)
    opened, _ = run_rollout("hover3d", x0, st, abar.astype(np.float64))
    assert (out["status"] == AIRBORNE).all() and (out["fstatus"] == AIRBORNE).all()
    fig = lqg_ref.app_conditions(out["nis"], out["x"], opened["x"])
    print("mean NIS %.3f rmse closed %.3f open %.3f ratio %.3f" % (fig["mean_nis"], fig["rmse_closed"], fig["rmse_open"],
                                                                   fig["ratio"]))
    assert fig["ratio"] <= 0.25, fig
