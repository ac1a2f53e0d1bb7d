"""CPU-side checks of cs_rollout_states_ex / cs_rollout_vjp_ex: both entry points are declared, exported and bound, the
ctypes struct mirrors cs_rollout_param_io, and bad argument blocks are refused without touching a device.

The unfold test holds a NumPy RESTATEMENT of the chain rule through fold_vehicle to central
differences of a NumPy fold_vehicle for both thrust laws: it pins the closed form, not the device kernel.  The kernel
(unfold_vehicle_kernel) is held to central differences of the float64 oracle by the GPU tests,
tests/test_gpu_rollout_param_grad.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
NAMES = ("cs_rollout_states_ex", "cs_rollout_vjp_ex")


def test_param_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    for name in NAMES:
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_rollout_param_io\* pio,\s*"
                         r"void\* stream\);" % name, HEADER)
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes[1] is C.POINTER(_lib.RolloutIO)
        assert getattr(lib, name).argtypes[2] is C.POINTER(_lib.RolloutParamIO)


def test_param_io_layout_matches_its_mirror():
    body = re.search(r"typedef struct cs_rollout_param_io \{(.*?)\} cs_rollout_param_io;", HEADER, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _lib.RolloutParamIO._fields_]
    assert C.sizeof(_lib.RolloutParamIO) == 8 + 3 * 8
    # the rollout block and the ABI version are as they were
    assert C.sizeof(_lib.RolloutIO) == 16 + 14 * 8
    assert "CS_ABI_VERSION 5" in HEADER


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev = 0x1000
    io.x_dev, io.status_dev = 0x4000, 0x5000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _pio(**kw):
    pio = _lib.RolloutParamIO()
    pio.struct_size = C.sizeof(pio)
    for k, v in kw.items():
        setattr(pio, k, v)
    return pio


def test_param_calls_refuse_bad_arguments_without_a_device():
    lib = _lib.load()
    for name in NAMES:
        fn = getattr(lib, name)
        assert fn(None, None, C.byref(_pio()), None) == _lib.ERR_ARG
        assert b"null io" in lib.cs_last_error()
        assert fn(None, C.byref(_io(num_steps=0)), C.byref(_pio()), None) == _lib.ERR_ARG
        assert b"num_steps" in lib.cs_last_error()
        assert fn(None, C.byref(_io()), C.byref(_pio(struct_size=C.sizeof(_lib.RolloutParamIO) - 8)), None) == \
            _lib.ERR_ABI
        assert b"cs_rollout_param_io" in lib.cs_last_error()
        assert fn(None, C.byref(_io()), C.byref(_pio(out_dtype=7)), None) == _lib.ERR_ARG
        assert b"out_dtype" in lib.cs_last_error()
        # a well-formed pair gets as far as the context; pio = NULL is the plain call's path
        assert fn(None, C.byref(_io()), C.byref(_pio(vehicle_dev=0x6000, g_vehicle_dev=0x7000)), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"
        assert fn(None, C.byref(_io()), None, None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"
    assert lib.cs_rollout_vjp_ex(None, C.byref(_io(x_dev=None)), C.byref(_pio()), None) == _lib.ERR_ARG
    assert b"tape" in lib.cs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the unfold chain rule
# ---------------------------------------------------------------------------------------------------------------------
def fold(p, lift):
    """fold_vehicle (copterstep_api.hip) in NumPy: raw rows [12, n] -> the 11 coefficients"""
    B, D, M, L, Ix, Iy, Iz, Jr, maxrpm, G, rho, C_L = p
    ws = maxrpm * np.pi / 30.0
    ws2 = ws * ws
    if lift:
        KL = 0.5 * rho * (0.05 * L * 4.0) * C_L * (L / 2.0) * (L / 2.0) * ws2
        kt = kr = KL
    else:
        kt, kr = B * ws2, L * B * ws2
    return np.array([-kt / M, kr / Ix, kr / Iy, D * ws2 / Iz, G + 0 * M, (Iy - Iz) / Ix, (Iz - Ix) / Iy,
                     (Ix - Iy) / Iz, 2.0 / M, Jr / Ix * ws, Jr / Iy * ws])


def unfold(a, p, lift, gyro):
    """the chain rule of unfold_vehicle_kernel (copterstep_rollout_grad.hip), restated: coefficient adjoints a [11, n]
    at the raw rows p [12, n] -> raw adjoints [12, n]"""
    B, D, M, L, Ix, Iy, Iz, Jr, maxrpm, G, rho, C_L = p
    ws = maxrpm * np.pi / 30.0
    ws2 = ws * ws
    g_kt = -a[0] / M
    g_kr = a[1] / Ix + a[2] / Iy
    z = np.zeros_like(M)
    if lift:
        base = 0.5 * (0.05 * L * 4.0) * (L / 2.0) ** 2
        kt = kr = base * rho * C_L * ws2
        g_KL = g_kt + g_kr
        g_B, g_rho, g_CL = z, g_KL * base * C_L * ws2, g_KL * base * rho * ws2
        g_L = g_KL * 0.075 * L * L * rho * C_L * ws2
        g_ws2 = g_KL * base * rho * C_L
    else:
        kt, kr = B * ws2, L * B * ws2
        g_B, g_rho, g_CL = (g_kt + g_kr * L) * ws2, z, z
        g_L = g_kr * B * ws2
        g_ws2 = g_kt * B + g_kr * L * B
    g_ws2 = g_ws2 + a[3] * D / Iz
    g_ws = 2.0 * ws * g_ws2
    a9, a10 = (a[9], a[10]) if gyro else (z, z)
    g_Jr = (a9 / Ix + a10 / Iy) * ws
    g_ws = g_ws + Jr * (a9 / Ix + a10 / Iy)
    return np.array([
        g_B, a[3] * ws2 / Iz, (a[0] * kt - 2.0 * a[8]) / (M * M), g_L,
        -(a[1] * kr + a[5] * (Iy - Iz) + a9 * Jr * ws) / (Ix * Ix) - a[6] / Iy + a[7] / Iz,
        -(a[2] * kr + a[6] * (Iz - Ix) + a10 * Jr * ws) / (Iy * Iy) + a[5] / Ix - a[7] / Iz,
        -(a[3] * D * ws2 + a[7] * (Ix - Iy)) / (Iz * Iz) - a[5] / Ix + a[6] / Iy,
        g_Jr, g_ws * np.pi / 30.0, a[4], g_rho, g_CL])


@pytest.mark.parametrize("lift", [False, True])
def test_unfold_chain_rule_matches_central_differences_of_the_fold(lift):
    rng = np.random.default_rng(int(lift))
    n = 64
    p = np.array([5e-3, 2e-6, 1.38, 0.35, 2.0, 2.0, 3.0, 38e-4, 15000.0, 9.80665, 1.0, 0.5])[:, None] * \
        rng.uniform(0.8, 1.2, (12, n))
    a = rng.standard_normal((11, n))
    got = unfold(a, p, lift, gyro=True)
    want = np.zeros_like(p)
    for j in range(12):
        h = 1e-6 * np.abs(p[j])
        pp, pm = p.copy(), p.copy()
        pp[j] += h
        pm[j] -= h
        want[j] = np.sum(a * (fold(pp, lift) - fold(pm, lift)), axis=0) / (2 * h)
    # compared as d / d log p: the rows span 1e-6 .. 1e4
    err = np.abs(got - want) * p / np.maximum(1.0, np.abs(want * p))
    assert err.max() < 1e-7, err.max()
    # rows that do not enter are exactly 0
    zero = ["B"] if lift else ["rho", "C_L"]
    for k in zero:
        assert np.all(got[("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm", "G", "rho", "C_L").index(k)] == 0)
    assert np.all(unfold(a, p, lift, gyro=False)[7] == 0)
