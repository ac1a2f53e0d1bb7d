"""CPU-side checks of the on-device policy-parameter gradient and the action-tape cotangent (cs_mlp_param_grad,
cs_rollout_mlp_vjp_ex): the entry points are declared, exported and bound and the ctypes structs mirror the header; bad
argument blocks are refused without a device; and the float64 checker the GPU tests hold the cotangent to
(tests/mlp_action_fd.py) is pinned to the checker without it, to the chain rule through the action tape and to the closed
form of a single step."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gym_copter_amd import _lib, mlp
from jacobian_fd import hover_action
from mlp_action_fd import fd_mlp_action_vjp
from mlp_rollout_fd import OBS_SHAPE, fd_mlp_rollout_vjp, oracle_mlp_rollout
from oracle.refcpu import AIRBORNE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()


def _header_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    return re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_mlp_param_grad\s*\(cs_ctx\* ctx, const cs_mlp_grad_io\* io, void\* stream\);", HEADER)
    assert re.search(r"int cs_rollout_mlp_vjp_ex\s*\(cs_ctx\* ctx, const cs_rollout_io\* io, "
                     r"const cs_rollout_mlp_io\* mio,\s*const cs_rollout_mlp_ex_io\* xio, void\* stream\);", HEADER)
    for name in ("cs_mlp_param_grad", "cs_rollout_mlp_vjp_ex"):
        assert hasattr(lib, name) and name in _lib.SYMBOLS
    assert lib.cs_mlp_param_grad.argtypes[1] is C.POINTER(_lib.MlpGradIO)
    assert lib.cs_rollout_mlp_vjp_ex.argtypes[1] is C.POINTER(_lib.RolloutIO)
    assert lib.cs_rollout_mlp_vjp_ex.argtypes[2] is C.POINTER(_lib.RolloutMlpIO)
    assert lib.cs_rollout_mlp_vjp_ex.argtypes[3] is C.POINTER(_lib.RolloutMlpExIO)
    assert _header_fields("cs_mlp_grad_io") == [f for f, _ in _lib.MlpGradIO._fields_]
    assert _header_fields("cs_mlp_grad_io") == ["struct_size", "ga_dtype", "hidden", "num_steps", "params_dev", "obs_dev",
                                                "g_actions_dev", "g_params_dev"]
    assert C.sizeof(_lib.MlpGradIO) == 16 + 4 * 8
    assert _header_fields("cs_rollout_mlp_ex_io") == [f for f, _ in _lib.RolloutMlpExIO._fields_]
    assert C.sizeof(_lib.RolloutMlpExIO) == 8 + 8
    # additive: the ABI version and the existing blocks are unchanged
    assert "CS_ABI_VERSION 5" in HEADER and _lib.ABI_VERSION == 5
    assert C.sizeof(_lib.RolloutMlpIO) == 8 + 4 * 8


def _gio(**kw):
    g = _lib.MlpGradIO()
    g.struct_size = C.sizeof(g)
    g.ga_dtype = _lib.JAC_F64
    g.hidden, g.num_steps = 8, 4
    g.params_dev, g.obs_dev, g.g_actions_dev, g.g_params_dev = 0x1000, 0x2000, 0x3000, 0x4000
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_param_grad_refuses_bad_blocks_without_a_device():
    lib = _lib.load()
    fn = lib.cs_mlp_param_grad
    assert fn(None, None, None) == _lib.ERR_ARG
    assert b"null io" in lib.cs_last_error()
    g = _gio()
    g.struct_size -= 8
    assert fn(None, C.byref(g), None) == _lib.ERR_ABI
    assert b"struct_size" in lib.cs_last_error()
    for name in ("params_dev", "obs_dev", "g_actions_dev", "g_params_dev"):
        assert fn(None, C.byref(_gio(**{name: None})), None) == _lib.ERR_ARG
        assert name.encode() in lib.cs_last_error()
    for h in (-1, 65, 1000):
        assert fn(None, C.byref(_gio(hidden=h)), None) == _lib.ERR_ARG
        assert b"hidden" in lib.cs_last_error()
    for k in (0, -3):
        assert fn(None, C.byref(_gio(num_steps=k)), None) == _lib.ERR_ARG
        assert b"num_steps" in lib.cs_last_error()
    assert fn(None, C.byref(_gio(ga_dtype=2)), None) == _lib.ERR_ARG
    assert b"ga_dtype" in lib.cs_last_error()
    # well-formed blocks get as far as the context (hidden 0 and 64 are in range, both dtypes)
    for h, dt in ((0, _lib.JAC_F64), (64, _lib.JAC_F32)):
        assert fn(None, C.byref(_gio(hidden=h, ga_dtype=dt)), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"


def test_vjp_ex_refuses_bad_blocks_without_a_device():
    lib = _lib.load()
    fn = lib.cs_rollout_mlp_vjp_ex
    io = _lib.RolloutIO()
    io.struct_size = C.sizeof(io)
    io.num_steps, io.x_dev, io.status_dev = 4, 0x5000, 0x6000
    m = _lib.RolloutMlpIO()
    m.struct_size = C.sizeof(m)
    m.hidden, m.params_dev, m.actions_out_dev = 8, 0x1000, 0x2000
    x = _lib.RolloutMlpExIO()
    x.struct_size = C.sizeof(x)
    x.g_actions_in_dev = 0x7000
    # NULL xio is cs_rollout_mlp_vjp: its own checks and messages
    assert fn(None, C.byref(io), None, None, None) == _lib.ERR_ARG
    assert b"cs_rollout_mlp_vjp: null mio" in lib.cs_last_error()
    assert fn(None, C.byref(io), C.byref(m), None, None) == _lib.ERR_ARG
    assert lib.cs_last_error() == b"null context"
    # with xio: the rollout blocks' checks first, then its own
    assert fn(None, None, C.byref(m), C.byref(x), None) == _lib.ERR_ARG
    assert b"null io" in lib.cs_last_error()
    m.hidden = 65
    assert fn(None, C.byref(io), C.byref(m), C.byref(x), None) == _lib.ERR_ARG
    assert b"hidden" in lib.cs_last_error()
    m.hidden = 8
    x.struct_size += 8
    assert fn(None, C.byref(io), C.byref(m), C.byref(x), None) == _lib.ERR_ABI
    assert b"xio->struct_size" in lib.cs_last_error()
    x.struct_size -= 8
    x.reserved_ = 1
    assert fn(None, C.byref(io), C.byref(m), C.byref(x), None) == _lib.ERR_ARG
    assert b"reserved_" in lib.cs_last_error()
    x.reserved_ = 0
    for ptr in (0x7000, None):                                  # (a NULL cotangent is zero)
        x.g_actions_in_dev = ptr
        assert fn(None, C.byref(io), C.byref(m), C.byref(x), None) == _lib.ERR_ARG
        assert lib.cs_last_error() == b"null context"


# ---------------------------------------------------------------------------------------------------------------------
# the checker of the action-tape cotangent, pinned on the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
def _point(n, rng):
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[1], x[3], x[5] = rng.uniform(-1, 1, (3, n))
    x[4] = rng.uniform(-15, -8, n)
    x[6], x[8] = rng.uniform(-0.2, 0.2, (2, n))
    x[7], x[9], x[11] = rng.uniform(-0.5, 0.5, (3, n))
    x[10] = rng.uniform(-0.5, 0.5, n)
    return x, np.full(n, AIRBORNE, np.uint8)


def _setup(hidden, K):
    """The set-up of test_checker_theta_gradient_is_the_host_reduction_of_its_action_gradient (test_rollout_mlp_cpu)."""
    import torch
    task, n, A = "lander3d", 2, 4
    rng = np.random.default_rng(11)
    x, st = _point(n, rng)
    od = OBS_SHAPE[task][1]
    theta = mlp.init(od, A, hidden, generator=torch.Generator().manual_seed(5), out_bias=hover_action(),
                     out_scale=0.05).double().numpy()
    gx, gr = rng.normal(size=(K, n, 12)), rng.normal(size=(K, n))
    gact = rng.normal(size=(K, n, A))
    return task, x, st, theta, gx, gr, gact


@pytest.mark.parametrize("hidden", [0, 4])
def test_checker_without_a_cotangent_is_the_plain_checker(hidden):
    task, x, st, theta, gx, gr, _ = _setup(hidden, 4)
    got = fd_mlp_action_vjp(task, x, st, theta, hidden, 4, gx=gx, gr=gr, gact=None)
    want = fd_mlp_rollout_vjp(task, x, st, theta, hidden, 4, gx=gx, gr=gr)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


@pytest.mark.parametrize("hidden", [0, 4])
def test_checker_theta_gradient_is_the_reduction_of_its_total_action_gradient(hidden):
    """With a cotangent on the action tape the chain rule still runs through a_k = pi(o_{k-1}) + u_k alone: central
    differences in theta == mlp.param_grad(obs, g_u) of the checker's own TOTAL g_u (which includes gact)."""
    import torch
    K = 4
    task, x, st, theta, gx, gr, gact = _setup(hidden, K)
    gp, gu, _ = fd_mlp_action_vjp(task, x, st, theta, hidden, K, gx=gx, gr=gr, gact=gact)
    _, _, obs, _ = oracle_mlp_rollout(task, x, st, theta, hidden, K)
    want = mlp.param_grad(torch.from_numpy(theta), hidden, torch.from_numpy(obs), torch.from_numpy(gu)).numpy()
    err = np.max(np.abs(gp - want) / np.maximum(1.0, np.abs(want)))
    print("chain identity with a cotangent, H = %d: %.2e" % (hidden, err))
    assert err < 1e-5, err
    # (and the cotangent is in g_u: without it the last step's g_u is the step's own alone)
    _, gu0, _ = fd_mlp_action_vjp(task, x, st, theta, hidden, K, gx=gx, gr=gr)
    assert np.max(np.abs((gu - gu0)[K - 1] - gact[K - 1])) < 1e-5


@pytest.mark.parametrize("hidden", [0, 4])
def test_checker_single_step_closed_form(hidden):
    """K = 1 with no other cotangent: L = sum(gact * a_1), so g_u = gact and g_theta = mlp.param_grad(obs, gact)."""
    import torch
    task, x, st, theta, _, _, gact = _setup(hidden, 1)
    gp, gu, _ = fd_mlp_action_vjp(task, x, st, theta, hidden, 1, gact=gact)
    _, _, obs, _ = oracle_mlp_rollout(task, x, st, theta, hidden, 1)
    want = mlp.param_grad(torch.from_numpy(theta), hidden, torch.from_numpy(obs), torch.from_numpy(gact)).numpy()
    err = max(np.max(np.abs(gu - gact)), np.max(np.abs(gp - want) / np.maximum(1.0, np.abs(want))))
    print("single-step closed form, H = %d: %.2e" % (hidden, err))
    assert err < 1e-9, err
