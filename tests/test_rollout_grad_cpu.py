"""CPU-side checks of cs_rollout_states / cs_rollout_vjp: both entry points are declared, exported and bound, the
ctypes struct mirrors the header; bad argument blocks are refused without touching a device; and the K-step
central-difference checker the GPU tests hold the backward kernel to (tests/rollout_fd.py) reproduces closed-form
derivatives of a rollout at hover and the telescoping of the Lander reward."""
import ctypes as C
import os
import re

import numpy as np

from gym_copter_amd import _lib
from jacobian_fd import hover_action, hover_point
from oracle.refcpu import G
from rollout_fd import fd_rollout_vjp, oracle_rollout, shaping_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
DU_DZ = -2.9609131841      # d dz' / d a_i of one step at hover (tests/test_jacobian_cpu.py)


def test_rollout_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    for name in ("cs_rollout_states", "cs_rollout_vjp"):
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, void\* stream\);" % name, HEADER)
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes[1] is C.POINTER(_lib.RolloutIO)
    body = re.search(r"typedef struct cs_rollout_io \{(.*?)\} cs_rollout_io;", HEADER, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _lib.RolloutIO._fields_]
    assert C.sizeof(_lib.RolloutIO) == 16 + 14 * 8
    assert "CS_ABI_VERSION 5" in HEADER


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    io.actions_dev = 0x1000
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_rollout_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    for fn in (lib.cs_rollout_states, lib.cs_rollout_vjp):
        assert fn(None, None, None) == -1                                # CS_ERR_ARG
        assert b"null io" in lib.cs_last_error()
        io = _io()
        io.struct_size = C.sizeof(io) - 8
        assert fn(None, C.byref(io), None) == _lib.ERR_ABI
        assert b"struct_size" in lib.cs_last_error()
        assert fn(None, C.byref(_io(num_steps=0)), None) == -1
        assert b"num_steps" in lib.cs_last_error()
        assert fn(None, C.byref(_io(actions_dev=None)), None) == -1
        assert b"actions_dev" in lib.cs_last_error()
        for key in ("start_status_dev", "start_force_dev", "start_prev_shaping_dev"):
            assert fn(None, C.byref(_io(**{key: 0x2000})), None) == -1
            assert b"start_x_dev is required" in lib.cs_last_error()
        assert fn(None, C.byref(_io(start_x_dev=0x2000)), None) == -1
        assert b"start_status_dev" in lib.cs_last_error()
    # the backward needs its tape, and a known output dtype
    for kw in ({"g_actions_dev": 0x3000}, {"g_x0_dev": 0x3000, "x_dev": 0x4000}, {"status_dev": 0x4000}):
        assert lib.cs_rollout_vjp(None, C.byref(_io(**kw)), None) == -1
        assert b"tape" in lib.cs_last_error()
    assert lib.cs_rollout_vjp(None, C.byref(_io(x_dev=0x4000, status_dev=0x5000, out_dtype=7)), None) == -1
    assert b"out_dtype" in lib.cs_last_error()
    # a well-formed block gets as far as the context
    assert lib.cs_rollout_states(None, C.byref(_io()), None) == -1
    assert lib.cs_last_error() == b"null context"
    assert lib.cs_rollout_vjp(None, C.byref(_io(x_dev=0x4000, status_dev=0x5000)), None) == -1
    assert lib.cs_last_error() == b"null context"


def test_checker_reproduces_the_closed_form_rollout_derivatives_at_hover():
    """From hover (z = -10, level, at rest, AIRBORNE) with a* on every motor for K = 10 steps of dt = 0.01:
    d z_K / d a_{0,i} = (K - 1) dt d dz' / d a_i (the first step's dz moves z in the K - 1 steps after it),
    d z_K / d a_{K-1} = 0, d dz_K / d a_{K-1,i} = d dz' / d a_i, d z_K / d dz_0 = K dt, and
    d X_K / d theta_0 = -G dt^2 K (K - 1) / 2 (theta holds, dX grows by -dt G theta a step)."""
    K, dt = 10, 0.01
    a = hover_action()
    x, st = hover_point(1)
    acts = np.full((K, 1, 4), a)
    for slot, want_last in ((4, 0.0), (5, DU_DZ)):
        gx = np.zeros((K, 1, 12))
        gx[K - 1, 0, slot] = 1.0
        ga, g0 = fd_rollout_vjp("lander3d", x, st, acts, gx=gx)
        assert ga.shape == (K, 1, 4) and g0.shape == (12, 1)
        np.testing.assert_allclose(ga[K - 1, 0], want_last, atol=1e-6, rtol=1e-6)
        if slot == 4:
            np.testing.assert_allclose(ga[0, 0], (K - 1) * dt * DU_DZ, rtol=1e-6)
            np.testing.assert_allclose(g0[5, 0], K * dt, rtol=1e-6)
    gx = np.zeros((K, 1, 12))
    gx[K - 1, 0, 0] = 1.0
    _, g0 = fd_rollout_vjp("lander3d", x, st, acts, gx=gx)
    np.testing.assert_allclose(g0[8, 0], -G * dt * dt * K * (K - 1) / 2, rtol=1e-6)


def test_lander_reward_telescopes_over_a_rollout():
    """Lander3D, no out-of-bounds penalty, landing bonus or tilt in the horizon: the rewards of a rollout whose
    prev_shaping starts as shaping(x0) sum to shaping(x_K) - shaping(x_0) -- the term the backward adds through
    prev_shaping is what makes its gradient that of this sum."""
    rng = np.random.default_rng(3)
    n, K = 64, 20
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    x[4] = rng.uniform(-8, -4, n)
    x[[1, 3, 5]] = rng.uniform(-1, 1, (3, n))
    x[[6, 8]] = rng.uniform(-0.1, 0.1, (2, n))
    x[10], x[11] = rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)
    st = np.full(n, 3, np.uint8)
    acts = hover_action() * rng.uniform(0.7, 1.3, (K, n, 4))
    xs, rs, term, _, orc = oracle_rollout("lander3d", x, st, acts)
    assert not term.any()
    total = rs.sum(axis=0)
    np.testing.assert_allclose(total, orc._shaping(xs[-1].T) - orc._shaping(x), atol=1e-9, rtol=1e-12)
    # ... and its central-difference gradient is that of shaping(x_K) - shaping(x_0)
    ga, g0 = fd_rollout_vjp("lander3d", x[:, :4], st[:4], acts[:8, :4], gr=np.ones((8, 4)))
    gx = np.zeros((8, 4, 12))
    xs8, _, _, _, _ = oracle_rollout("lander3d", x[:, :4], st[:4], acts[:8, :4])
    gx[-1] = shaping_grad(xs8[-1].T).T
    ga2, g02 = fd_rollout_vjp("lander3d", x[:, :4], st[:4], acts[:8, :4], gx=gx)
    np.testing.assert_allclose(g0 + shaping_grad(x[:, :4]), g02, atol=1e-5)
    np.testing.assert_allclose(ga, ga2, atol=1e-5)
