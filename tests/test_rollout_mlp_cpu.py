"""CPU-side checks of the closed-loop rollouts (cs_rollout_mlp_states / cs_rollout_mlp_vjp): both entry points are
declared, exported and bound and the ctypes struct mirrors the header; bad argument blocks are refused without a device;
the float64 closed-loop checker the GPU tests hold the backward to (tests/mlp_rollout_fd.py) is pinned to the open-loop
checker and to the host-side parameter gradient; and theta's pack / unpack round-trips."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_copter_amd import _lib, mlp
from jacobian_fd import hover_action
from mlp_rollout_fd import OBS_SHAPE, fd_mlp_rollout_vjp, oracle_mlp_rollout, policy64
from oracle.refcpu import AIRBORNE
from rollout_fd import fd_rollout_vjp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()


def test_mlp_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    for name in ("cs_rollout_mlp_states", "cs_rollout_mlp_vjp"):
        assert re.search(r"int %s\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, const cs_rollout_mlp_io\* mio, "
                         r"void\* stream\);" % name, HEADER)
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes[1] is C.POINTER(_lib.RolloutIO)
        assert getattr(lib, name).argtypes[2] is C.POINTER(_lib.RolloutMlpIO)
    body = re.search(r"typedef struct cs_rollout_mlp_io \{(.*?)\} cs_rollout_mlp_io;", HEADER, re.S).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f for f, _ in _lib.RolloutMlpIO._fields_]
    assert C.sizeof(_lib.RolloutMlpIO) == 8 + 4 * 8
    assert "#define CS_MLP_MAX_HIDDEN %d" % _lib.MLP_MAX_HIDDEN in HEADER
    assert "CS_ABI_VERSION 5" in HEADER                     # additive: the ABI version is unchanged


def _io(**kw):
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps = 4
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def _mio(**kw):
    m = _lib.RolloutMlpIO()
    m.struct_size = C.sizeof(m)
    m.hidden = 8
    m.params_dev = 0x1000
    m.actions_out_dev = 0x2000
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_mlp_rollout_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    for fn in (lib.cs_rollout_mlp_states, lib.cs_rollout_mlp_vjp):
        assert fn(None, None, C.byref(_mio()), None) == -1
        assert b"null io" in lib.cs_last_error()
        assert fn(None, C.byref(_io()), None, None) == -1
        assert b"null mio" in lib.cs_last_error()
        m = _mio()
        m.struct_size -= 8
        assert fn(None, C.byref(_io()), C.byref(m), None) == _lib.ERR_ABI
        assert b"struct_size" in lib.cs_last_error()
        for h in (-1, 65, 1000):
            assert fn(None, C.byref(_io()), C.byref(_mio(hidden=h)), None) == -1
            assert b"hidden" in lib.cs_last_error()
        assert fn(None, C.byref(_io()), C.byref(_mio(params_dev=None)), None) == -1
        assert b"params_dev" in lib.cs_last_error()
        assert fn(None, C.byref(_io()), C.byref(_mio(actions_out_dev=None)), None) == -1
        assert b"actions_out_dev" in lib.cs_last_error()
        assert fn(None, C.byref(_io(actions_dev=0x3000)), C.byref(_mio()), None) == -1
        assert b"actions_dev must be NULL" in lib.cs_last_error()
        # cs_rollout_io's own checks still apply
        assert fn(None, C.byref(_io(num_steps=0)), C.byref(_mio()), None) == -1
        assert b"num_steps" in lib.cs_last_error()
        assert fn(None, C.byref(_io(start_status_dev=0x4000)), C.byref(_mio()), None) == -1
        assert b"start_x_dev is required" in lib.cs_last_error()
    assert lib.cs_rollout_mlp_vjp(None, C.byref(_io()), C.byref(_mio()), None) == -1
    assert b"tape" in lib.cs_last_error()
    # well-formed blocks get as far as the context (hidden 0 and 64 are in range)
    for h in (0, 64):
        assert lib.cs_rollout_mlp_states(None, C.byref(_io()), C.byref(_mio(hidden=h)), None) == -1
        assert lib.cs_last_error() == b"null context"
        assert lib.cs_rollout_mlp_vjp(None, C.byref(_io(x_dev=0x5000, status_dev=0x6000)), C.byref(_mio(hidden=h)),
                                      None) == -1
        assert lib.cs_last_error() == b"null context"


@pytest.mark.parametrize("hidden", [0, 1, 5, 64])
def test_params_pack_unpack_round_trip(hidden):
    import torch
    od, ad = 10, 4
    p = mlp.init(od, ad, hidden, generator=torch.Generator().manual_seed(hidden))
    assert p.dtype == torch.float32 and p.shape == (mlp.num_params(od, ad, hidden),)
    parts = mlp.unpack(p, od, ad, hidden)
    assert torch.equal(mlp.pack(parts, hidden), p)
    if hidden == 0:
        assert parts["W"].shape == (ad, od) and parts["b"].shape == (ad,)
        module = torch.nn.Linear(od, ad)
    else:
        assert parts["W1"].shape == (hidden, od) and parts["W2"].shape == (ad, hidden)
        module = torch.nn.Sequential(torch.nn.Linear(od, hidden), torch.nn.Tanh(), torch.nn.Linear(hidden, ad))
    q, h = mlp.pack_module(module)
    assert h == hidden and q.shape == p.shape
    o = torch.randn(7, od, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        assert torch.allclose(mlp.forward64(q, o, hidden, ad), module.double()(o.double()), rtol=0, atol=1e-6)
    assert np.allclose(mlp.forward64(q, o, hidden, ad).numpy(), policy64(q.numpy(), o.numpy(), hidden, ad),
                       rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        mlp.unpack(p[:-1], od, ad, hidden)
    with pytest.raises(ValueError):
        mlp.num_params(od, ad, 65)
    b = mlp.init(od, ad, hidden, out_bias=0.6, out_scale=0.0)
    assert torch.equal(mlp.unpack(b, od, ad, hidden)["b" if hidden == 0 else "b2"], torch.full((ad,), 0.6))


def _point(n, rng):
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[1], x[3], x[5] = rng.uniform(-1, 1, (3, n))
    x[4] = rng.uniform(-15, -8, n)
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    x[7], x[9], x[11] = rng.uniform(-0.5, 0.5, (3, n))
    x[10] = rng.uniform(-0.5, 0.5, n)
    return x, np.full(n, AIRBORNE, np.uint8)


@pytest.mark.parametrize("task", ["lander3d", "hover2d"])
def test_checker_with_zero_policy_is_the_open_loop_checker(task):
    """theta = 0: the closed loop takes a_k = u_k, so its g_u is fd_rollout_vjp's g_actions, and g_x0 likewise."""
    n, K, A = 3, 4, {"lander3d": 4, "hover2d": 2}[task]
    rng = np.random.default_rng(3)
    x, st = _point(n, rng)
    u = hover_action() * rng.uniform(0.8, 1.2, (K, n, A))
    gx, gr = rng.normal(size=(K, n, 12)), rng.normal(size=(K, n))
    P = mlp.num_params(OBS_SHAPE[task][1], A, 3)
    gp, gu, g0 = fd_mlp_rollout_vjp(task, x, st, np.zeros(P), 3, K, offsets=u, gx=gx, gr=gr)
    ga, gx0 = fd_rollout_vjp(task, x, st, u, gx=gx, gr=gr)
    assert np.allclose(gu, ga, rtol=1e-9, atol=1e-9)
    assert np.allclose(g0, gx0, rtol=1e-9, atol=1e-9)
    assert np.all(np.isfinite(gp)) and np.abs(gp).max() > 0   # theta = 0 is no stationary point of the loss


@pytest.mark.parametrize("variant", ["mars_gyro", "vehicles", "vehicles_mars_gyro"])
def test_checker_passes_the_vehicle_model_through(variant):
    """vp / g / mars (per-env arrays included) reach the oracle tiled over the perturbed copies as tests/rollout_fd.py
    tiles them: with theta = 0 the closed-loop checker equals the open-loop one under the same model, and both differ
    from the default model's."""
    import model_variants
    task, n, K, A = "lander3d", 3, 4, 4
    rng = np.random.default_rng(5)
    model = model_variants.oracle_model(variant, model_variants.draw(variant, rng, n))
    x, st = _point(n, rng)
    u = model_variants.hover(variant) * rng.uniform(0.8, 1.2, (K, n, A))
    gx, gr = rng.normal(size=(K, n, 12)), rng.normal(size=(K, n))
    P = mlp.num_params(OBS_SHAPE[task][1], A, 3)
    gp, gu, g0 = fd_mlp_rollout_vjp(task, x, st, np.zeros(P), 3, K, offsets=u, gx=gx, gr=gr, **model)
    ga, gx0 = fd_rollout_vjp(task, x, st, u, gx=gx, gr=gr, **model)
    assert np.allclose(gu, ga, rtol=1e-9, atol=1e-9)
    assert np.allclose(g0, gx0, rtol=1e-9, atol=1e-9)
    _, plain, _ = fd_mlp_rollout_vjp(task, x, st, np.zeros(P), 3, K, offsets=u, gx=gx, gr=gr)
    assert np.all(np.abs(gu - plain).max(axis=(0, 2)) > 1e-3 * np.abs(plain).max(axis=(0, 2)))     # in every env
    xs, _, _, _ = oracle_mlp_rollout(task, x, st, np.zeros(P), 3, K, offsets=u, **model)
    xd, _, _, _ = oracle_mlp_rollout(task, x, st, np.zeros(P), 3, K, offsets=u)
    assert np.all(np.any(xs != xd, axis=(0, 2)))


@pytest.mark.parametrize("hidden", [0, 4])
def test_checker_theta_gradient_is_the_host_reduction_of_its_action_gradient(hidden):
    """Along one closed-loop trajectory, dL / d theta = sum_{k,n} J_theta pi(o_{k-1,n})^T dL / d a_k (the chain rule
    through a_k = pi(o_{k-1}) + u_k): central differences in theta == mlp.param_grad applied to the checker's own g_u
    and obs tape (CPU tensors)."""
    import torch
    task, n, K, A = "lander3d", 2, 4, 4
    rng = np.random.default_rng(11)
    x, st = _point(n, rng)
    od = OBS_SHAPE[task][1]
    theta = mlp.init(od, A, hidden, generator=torch.Generator().manual_seed(5), out_bias=hover_action(),
                     out_scale=0.05).double().numpy()
    gx, gr = rng.normal(size=(K, n, 12)), rng.normal(size=(K, n))
    gp, gu, _ = fd_mlp_rollout_vjp(task, x, st, theta, hidden, K, gx=gx, gr=gr)
    _, _, obs, _ = oracle_mlp_rollout(task, x, st, theta, hidden, K)
    want = mlp.param_grad(torch.from_numpy(theta), hidden, torch.from_numpy(obs), torch.from_numpy(gu)).numpy()
    scale = np.maximum(1.0, np.abs(want))
    assert np.max(np.abs(gp - want) / scale) < 1e-5, np.max(np.abs(gp - want) / scale)
