"""CPU-side checks of cs_jvp_rollout (forward-mode rollout tangents): the entry point is declared,
exported and bound, the ctypes struct mirrors cs_jvp_io, and bad argument blocks are refused without touching a device.

The fold-tangent tests hold a NumPy RESTATEMENT of rollout_tangent.h's fold_tangent (tests/jvp_ref.py) to central
differences of a NumPy fold_vehicle and to the transpose identity with the NumPy unfold of
tests/test_rollout_param_grad_cpu.py: they pin the closed form, not the device code, which tests/test_gpu_jvp.py holds
to central differences of the float64 oracle and to the adjoint kernels.

test_reference_solves_the_identification_problem PASSES WITHOUT THE FEATURE: it runs the inputs of
tests/test_gpu_identify.py on the float64 oracle with a central-difference Jacobian, so that no device sees a problem
the reference does not solve."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jvp_ref
from test_rollout_param_grad_cpu import fold, unfold

from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
WHO = b"cs_jvp_rollout:"


def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_jvp_rollout\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_jvp_io\* jio,\s*"
                     r"void\* stream\);", HEADER)
    assert hasattr(lib, "cs_jvp_rollout") and "cs_jvp_rollout" in _lib.SYMBOLS
    assert lib.cs_jvp_rollout.argtypes[1] is C.POINTER(_lib.RolloutIO)
    assert lib.cs_jvp_rollout.argtypes[2] is C.POINTER(_lib.JvpIO)
    assert not re.match(r"cs_rollout_", "cs_jvp_rollout")       # (tests/null_outputs.py tables every cs_rollout_*)
    import gym_copter_amd
    assert callable(gym_copter_amd.CopterVecEnv.rollout_jvp) and callable(gym_copter_amd.identify)
    from gym_copter_amd import sharded
    assert "rollout_jvp" in sharded._LOCAL_ROLLOUTS and callable(sharded.ShardedCopterVecEnv.rollout_jvp)


def test_jvp_io_layout_matches_its_mirror():
    body = re.search(r"typedef struct cs_jvp_io \{(.*?)\} cs_jvp_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [name for _, name in decls] == [f for f, _ in _lib.JvpIO._fields_]
    offset = 0
    for (ctype, name), (_, mirror) in zip(decls, _lib.JvpIO._fields_):
        size = 8 if "*" in ctype else 4
        assert C.sizeof(mirror) == size, name
        offset = (offset + size - 1) // size * size
        assert getattr(_lib.JvpIO, name).offset == offset, name
        offset += size
    assert C.sizeof(_lib.JvpIO) == offset == 16 + 7 * 8
    assert int(re.search(r"#define CS_JVP_MAX_DIRS (\d+)", HEADER).group(1)) == _lib.JVP_MAX_DIRS
    # the rollout block and the ABI version are as they were
    assert C.sizeof(_lib.RolloutIO) == 16 + 14 * 8 and C.sizeof(_lib.RolloutParamIO) == 8 + 3 * 8
    assert "CS_ABI_VERSION 5" in HEADER and _lib.ABI_VERSION == 5 and _lib.load().cs_version() == 5


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev = 0x1000
    io.x_dev, io.status_dev = 0x4000, 0x5000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _jio(**kw):
    jio = _lib.JvpIO()
    jio.struct_size = C.sizeof(jio)
    jio.num_dirs = 3
    jio.t_actions_dev, jio.t_x_dev, jio.t_reward_dev = 0x10000, 0x20000, 0x30000
    for k, v in kw.items():
        setattr(jio, k, v)
    return jio


def _refused(io, jio, code=_lib.ERR_ARG):
    lib = _lib.load()
    assert lib.cs_jvp_rollout(None, None if io is None else C.byref(io), None if jio is None else C.byref(jio),
                              None) == code
    msg = lib.cs_last_error()
    assert msg.startswith(WHO), msg
    return msg


def test_a_valid_block_gets_as_far_as_the_context():
    lib = _lib.load()
    for jio in (_jio(), _jio(t_actions_dev=None, t_x0_dev=0x100, t_reward_dev=None),
                _jio(t_vehicle_dev=0x100, t_force_dev=0x200, vehicle_dev=0x300, t_x_dev=None, out_dtype=_lib.JAC_F32),
                _jio(num_dirs=1), _jio(num_dirs=_lib.JVP_MAX_DIRS)):
        assert lib.cs_jvp_rollout(None, C.byref(_io()), C.byref(jio), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"
    explicit = _io(start_x_dev=0x100, start_status_dev=0x200, start_force_dev=0x300, start_prev_shaping_dev=0x400)
    assert lib.cs_jvp_rollout(None, C.byref(explicit), C.byref(_jio()), None) == _lib.ERR_ARG
    assert lib.cs_last_error() == b"null context"


@pytest.mark.parametrize("member", ["actions_dev", "x_dev", "status_dev"])
def test_every_required_member_missing_is_refused_by_name(member):
    msg = _refused(_io(**{member: None}), _jio())
    assert member.encode() in msg and b"required" in msg


@pytest.mark.parametrize("member", ["reward_dev", "terminated_dev", "truncated_dev", "gx_dev", "gr_dev",
                                    "g_actions_dev", "g_x0_dev"])
def test_every_must_be_null_member_set_is_refused_by_name(member):
    msg = _refused(_io(**{member: 0x9000}), _jio())
    assert member.encode() in msg and b"must be NULL" in msg


def test_the_block_cases():
    assert b"null io" in _refused(None, _jio())
    assert b"null jio" in _refused(_io(), None)
    assert b"num_steps" in _refused(_io(num_steps=0), _jio())
    for d in (0, -1, _lib.JVP_MAX_DIRS + 1):
        msg = _refused(_io(), _jio(num_dirs=d))
        assert b"num_dirs" in msg and b"CS_JVP_MAX_DIRS" in msg
    msg = _refused(_io(), _jio(t_actions_dev=None))
    assert b"required" in msg and all(m in msg for m in (b"t_actions_dev", b"t_x0_dev", b"t_vehicle_dev", b"t_force_dev"))
    msg = _refused(_io(), _jio(t_x_dev=None, t_reward_dev=None))
    assert b"required" in msg and b"t_x_dev" in msg and b"t_reward_dev" in msg
    msg = _refused(_io(), _jio(struct_size=C.sizeof(_lib.JvpIO) - 8), _lib.ERR_ABI)
    assert b"struct_size" in msg and b"cs_jvp_io" in msg
    assert b"struct_size" in _refused(_io(struct_size=8), _jio(), _lib.ERR_ABI)
    assert b"out_dtype" in _refused(_io(), _jio(out_dtype=7))
    assert b"start_x_dev" in _refused(_io(start_status_dev=0x100), _jio())
    assert b"aligned" in _refused(_io(), _jio(t_x_dev=0x20008))
    assert b"aligned" in _refused(_io(), _jio(t_x0_dev=0x104))


# ---------------------------------------------------------------------------------------------------------------------
# the fold tangent
# ---------------------------------------------------------------------------------------------------------------------
def _raw(rng, n):
    return np.array([5e-3, 2e-6, 1.38, 0.35, 2.0, 2.0, 3.0, 38e-4, 15000.0, 9.80665, 1.0, 0.5])[:, None] * \
        rng.uniform(0.8, 1.2, (12, n))


@pytest.mark.parametrize("lift", [False, True])
def test_fold_tangent_matches_central_differences_of_the_fold(lift):
    rng = np.random.default_rng(10 + int(lift))
    n = 64
    p = _raw(rng, n)
    for j in range(12):       # per log-parameter: the direction p_j e_j (the rows span 1e-6 .. 1e4)
        t = np.zeros((12, n))
        t[j] = p[j]
        got = jvp_ref.fold_tangent(t, p, lift, gyro=True)
        h = 1e-6
        want = (fold(p + h * t, lift) - fold(p - h * t, lift)) / (2 * h)
        err = np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))
        assert err <= 1e-6, (jvp_ref.ROWS[j], err)
    # rows that do not enter the configuration contribute exactly 0
    for k in (["B"] if lift else ["rho", "C_L"]):
        t = np.zeros((12, n))
        t[jvp_ref.ROWS.index(k)] = 1.0
        assert np.all(jvp_ref.fold_tangent(t, p, lift, gyro=True) == 0.0), k
    t = np.zeros((12, n))
    t[jvp_ref.ROWS.index("Jr")] = 1.0
    assert np.all(jvp_ref.fold_tangent(t, p, lift, gyro=False) == 0.0)
    assert np.any(jvp_ref.fold_tangent(t, p, lift, gyro=True) != 0.0)


@pytest.mark.parametrize("gyro", [False, True])
@pytest.mark.parametrize("lift", [False, True])
def test_fold_tangent_is_the_transpose_of_the_unfold(lift, gyro):
    rng = np.random.default_rng(20 + 2 * int(lift) + int(gyro))
    n = 64
    p = _raw(rng, n)
    g = rng.standard_normal((11, n))
    t = rng.standard_normal((12, n)) * p
    lhs = np.sum(unfold(g, p, lift, gyro) * t, axis=0)
    rhs = np.sum(g * jvp_ref.fold_tangent(t, p, lift, gyro), axis=0)
    scale = np.sum(np.abs(unfold(g, p, lift, gyro) * t), axis=0)
    assert np.max(np.abs(lhs - rhs) / scale) <= 1e-12, np.max(np.abs(lhs - rhs) / scale)


# ---------------------------------------------------------------------------------------------------------------------
# the identification problem is one the reference solves (passes without the feature)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["vehicle", "force", "shared"])
def test_reference_solves_the_identification_problem(case):
    pb = jvp_ref.identify_problem(shared=case == "shared")
    x_obs = jvp_ref.oracle_observation(pb, with_force=case == "force")
    veh, force, accepted = jvp_ref.lm_reference(pb, x_obs, fit_force=case == "force", iterations=6,
                                                shared=case == "shared")
    idx = pb["idx"]
    rel = np.max(np.abs(veh[idx] / pb["hidden"][idx] - 1.0))
    print("identify reference (%s): max relative error %.3g" % (case, rel))
    assert rel <= 1e-6, rel
    assert np.all(accepted.any(axis=0))
    if case == "force":
        err = np.max(np.abs(force - pb["force"]))
        print("identify reference: max force error %.3g N" % err)
        assert err <= 1e-4, err
