"""gym_copter_amd/_wire.py, the host kit of the rollout wrappers, without a device: a stand-in env on device "cpu" with a
fake library.  Every rule a call site asks of the coercion function, the io block, the scalar checks at their edges, the
upload-once cache and the launch; then the import direction (every family module imports alone in a fresh interpreter)
and the identity of the public names that moved out of vecenv.py."""
import contextlib
import ctypes as C
import subprocess
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gym_copter_amd                                  # noqa: E402
from gym_copter_amd import _lib, _wire                 # noqa: E402

N = 5
OTHER = torch.device("meta")                           # a device that is not the stand-in env's


class FakeLib:
    """cs_probe records its arguments and returns `rc`."""

    def __init__(self):
        self.calls, self.rc = [], 0
        self.cs_probe = self._probe

    def _probe(self, *args):
        self.calls.append(("first",) + args)
        return self.rc


def _env():
    return types.SimpleNamespace(device=torch.device("cpu"), num_envs=N, _lib=FakeLib(), _ctx=C.c_void_p(1234),
                                 _stream=lambda: C.c_void_p(77), _keep=None)


def _checked(t, shape, dtype, keep):
    assert isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert t.device == torch.device("cpu") and keep[-1] is t
    return t


# ---------------------------------------------------------------------------------------------------------------------
# the coercion function, rule by rule
# ---------------------------------------------------------------------------------------------------------------------
def test_state_rule_takes_any_dtype_from_host_or_tensor():
    """rollout's state[...]: any dtype, host array or tensor, moved and converted."""
    env, keep = _env(), []
    rule = dict(non_blocking=True)
    t = _wire.tensor(env, np.arange(3 * N).reshape(3, N), (3, N), torch.float64, "state['force']", keep, **rule)
    assert _checked(t, (3, N), torch.float64, keep)[2, 1].item() == 2 * N + 1
    t = _wire.tensor(env, [1, 0, 2, 0, 1], (N,), torch.uint8, "state['status']", keep, **rule)
    assert _checked(t, (N,), torch.uint8, keep).tolist() == [1, 0, 2, 0, 1]
    src = torch.arange(2 * N * 3, dtype=torch.int32).view(N, 6)[:, ::2].T          # a strided integer tensor
    t = _wire.tensor(env, src, (3, N), torch.float64, "state['x']", keep, **rule)
    assert torch.equal(_checked(t, (3, N), torch.float64, keep), src.double()) and len(keep) == 3
    with pytest.raises(ValueError, match=r"^state\['x'\] must have shape \(12, 5\), got \(3, 5\)$"):
        _wire.tensor(env, src, (12, N), torch.float64, "state['x']", keep, **rule)
    assert len(keep) == 3


def test_cotangent_and_vehicle_rule_require_a_floating_dtype():
    env, keep = _env(), []
    rule = dict(floating=True, non_blocking=True)
    t = _wire.tensor(env, np.ones((2, N), np.float32), (2, N), torch.float64, "gr", keep, **rule)
    _checked(t, (2, N), torch.float64, keep)
    _checked(_wire.tensor(env, torch.ones(2, N, dtype=torch.float16), (2, N), torch.float64, "gr", keep, **rule),
             (2, N), torch.float64, keep)
    with pytest.raises(ValueError, match=r"^gr must be a floating-point array$"):
        _wire.tensor(env, np.ones((2, N), np.int64), (2, N), torch.float64, "gr", keep, **rule)
    with pytest.raises(ValueError, match=r"^gr must be a floating-point array$"):
        _wire.tensor(env, torch.ones(2, N, dtype=torch.int32), (2, N), torch.float64, "gr", keep, **rule)
    # the shape comes first, and the vehicle's message carries its rows
    with pytest.raises(ValueError, match=r"^vehicle must have shape \(2, 5\) \(rows \('B', 'D'\)\), got \(5, 2\)$"):
        _wire.tensor(env, np.ones((N, 2), np.int64), (2, N), torch.float64, "vehicle", keep,
                     note=" (rows %s)" % (("B", "D"),), **rule)
    assert len(keep) == 2


def test_filter_rule_refuses_another_device_and_a_host_array_that_is_not_floating():
    env, keep = _env(), []
    rule = dict(floating=True, strict=True, foreign=False)
    _checked(_wire.tensor(env, np.ones((N, 2), np.float32)[:, ::-1], (N, 2), torch.float64, "z", keep, **rule),
             (N, 2), torch.float64, keep)
    _checked(_wire.tensor(env, torch.ones(N, 2, dtype=torch.float32), (N, 2), torch.float64, "z", keep, **rule),
             (N, 2), torch.float64, keep)
    with pytest.raises(ValueError, match=r"^z must have shape \(5, 2\), got \(2, 5\)$"):
        _wire.tensor(env, np.ones((2, N), np.int64), (N, 2), torch.float64, "z", keep, **rule)
    with pytest.raises(ValueError, match=r"^z must be a floating-point array, got dtype int64$"):
        _wire.tensor(env, np.ones((N, 2), np.int64), (N, 2), torch.float64, "z", keep, **rule)
    with pytest.raises(ValueError, match=r"^z must be a floating-point array, got dtype complex128$"):
        _wire.tensor(env, np.ones((N, 2), np.complex128), (N, 2), torch.float64, "z", keep, **rule)
    with pytest.raises(ValueError, match=r"^z must be a floating-point tensor, got torch.int32$"):
        _wire.tensor(env, torch.ones(N, 2, dtype=torch.int32), (N, 2), torch.float64, "z", keep, **rule)
    with pytest.raises(ValueError, match=r"^z must be on cpu, got meta$"):
        _wire.tensor(env, torch.ones(N, 2, device=OTHER), (N, 2), torch.float64, "z", keep, **rule)
    assert len(keep) == 2


def test_tensor_only_rule_checks_type_and_dtype_before_the_shape():
    """rollout_lqr's q and r, rollout_mlp_vjp's g_actions_in."""
    env, keep = _env(), []
    rule = dict(host=False, floating=True, foreign=False)
    src = torch.ones(2, N, 3, dtype=torch.float32).transpose(1, 2)
    t = _checked(_wire.tensor(env, src.transpose(1, 2), (2, N, 3), torch.float64, "q", keep, **rule), (2, N, 3),
                 torch.float64, keep)
    assert t.data_ptr() != src.data_ptr()
    same = torch.ones(2, N, 3, dtype=torch.float64)
    assert _wire.tensor(env, same, (2, N, 3), torch.float64, "q", keep, **rule).data_ptr() == same.data_ptr()
    for bad in (np.ones((2, N, 3)), torch.ones(2, N, 3, dtype=torch.int64), torch.ones(1, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"^q must be a floating-point torch tensor of shape \(2, 5, 3\)$"):
            _wire.tensor(env, bad, (2, N, 3), torch.float64, "q", keep, **rule)
    with pytest.raises(ValueError, match=r"^q must have shape \(2, 5, 3\), got \(2, 5\)$"):
        _wire.tensor(env, torch.ones(2, N), (2, N, 3), torch.float64, "q", keep, **rule)
    with pytest.raises(ValueError, match=r"^q must be on cpu, got meta$"):
        _wire.tensor(env, torch.ones(2, N, 3, device=OTHER), (2, N, 3), torch.float64, "q", keep, **rule)
    assert len(keep) == 2


@pytest.mark.parametrize("foreign", [True, False])
def test_exact_vector_is_one_check_with_the_call_sites_message(foreign):
    """The parameter vectors of rollout_actor_critic (moved to the device) and ppo_grad (required there)."""
    env, keep = _env(), []
    wording = "%(name)s must be a [%(size)d] float32 tensor on %(device)s, got %(got)s" if not foreign else \
        "%(name)s must be a [%(size)d] float32 torch tensor, got %(got)s"
    v = torch.arange(7, dtype=torch.float32, requires_grad=False)
    t = _checked(_wire.exact_vector(env, v, 7, "actor", keep, wording, foreign=foreign), (7,),
                 torch.float32, keep)
    assert t.data_ptr() == v.data_ptr()
    tail = " on cpu" if not foreign else ""
    word = "tensor" if not foreign else "torch tensor"
    for bad, got in ((v.double(), r"torch.Size\(\[7\]\)"), (v[:6], r"torch.Size\(\[6\]\)"), ([0.0] * 7, "list"),
                     (np.zeros(7, np.float32), r"\(7,\)")):
        with pytest.raises(ValueError, match=r"^actor must be a \[7\] float32 %s%s, got %s$" % (word, tail, got)):
            _wire.exact_vector(env, bad, 7, "actor", keep, wording, foreign=foreign)
    elsewhere = torch.zeros(7, dtype=torch.float32, device=OTHER)
    if foreign:       # passes the check and is moved (a meta tensor has no data to move: that is where it stops)
        with pytest.raises(NotImplementedError, match="meta tensor"):
            _wire.exact_vector(env, elsewhere, 7, "actor", keep, wording, foreign=True)
    else:
        with pytest.raises(ValueError, match=r"^actor must be a \[7\] float32 tensor on cpu, got torch.Size"):
            _wire.exact_vector(env, elsewhere, 7, "actor", keep, wording, foreign=False)
    assert len(keep) == 1


def test_check_tape():
    env = _env()
    x = torch.zeros(2, N, 12, dtype=torch.float64)
    _wire.check_tape(env, "rollout_states", (x, "rollout.x", (2, N, 12), torch.float64))
    with pytest.raises(ValueError, match=r"^rollout.x must be a device tensor of shape \(2, 5, 12\) \(rollout_states' result\)$"):
        _wire.check_tape(env, "rollout_states", (x.numpy(), "rollout.x", (2, N, 12), torch.float64))
    with pytest.raises(ValueError, match=r"^rollout.x must have shape \(3, 5, 12\), got \(2, 5, 12\)$"):
        _wire.check_tape(env, "rollout_states", (x, "rollout.x", (3, N, 12), torch.float64))
    for bad in (x.float(), x.transpose(0, 1).contiguous().transpose(0, 1), torch.zeros(2, N, 12, dtype=torch.float64,
                                                                                      device=OTHER)):
        with pytest.raises(ValueError, match=r"^rollout.x must be a contiguous torch.float64 tensor on cpu$"):
            _wire.check_tape(env, "rollout_states", (bad, "rollout.x", (2, N, 12), torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# io blocks, dtype codes and scalars
# ---------------------------------------------------------------------------------------------------------------------
def test_block_sets_the_size_and_the_fields_and_refuses_an_unknown_one():
    x = torch.zeros(3, dtype=torch.float64)
    io = _wire.block(_lib.RolloutIO, num_steps=3, x_dev=x.data_ptr(), status_dev=None)
    assert isinstance(io, _lib.RolloutIO) and io.struct_size == C.sizeof(_lib.RolloutIO) > 0
    assert io.num_steps == 3 and io.x_dev == x.data_ptr() and io.status_dev is None and io.actions_dev is None
    assert _wire.block(_lib.EsIO).struct_size == C.sizeof(_lib.EsIO)
    with pytest.raises(AttributeError, match="RolloutIO has no member 'x_device'"):
        _wire.block(_lib.RolloutIO, x_device=1)


def test_dtype_codes():
    assert _wire.out_dtype(None) is torch.float64 and _wire.out_dtype(torch.float32) is torch.float32
    with pytest.raises(ValueError, match="^dtype must be torch.float64 or torch.float32$"):
        _wire.out_dtype(torch.float16)
    assert _wire.dtype_code(torch.float64) == _lib.JAC_F64 == _wire.dtype_code(None)
    assert _wire.dtype_code(torch.float32) == _lib.JAC_F32 != _lib.JAC_F64


def test_int_in_at_its_boundaries():
    u32 = dict(lo=0, hi=_wire.U32, what=_wire.IN_U32)
    assert _wire.int_in(0, "nonce", **u32) == 0 and _wire.int_in(2 ** 32 - 1, "nonce", **u32) == 2 ** 32 - 1
    got = _wire.int_in(np.int64(7), "nonce", **u32)
    assert got == 7 and type(got) is int
    for bad in (True, False, 2 ** 32, -1, 1.0, "1", None, np.float32(1)):
        with pytest.raises(ValueError, match=r"^nonce must be an int in \[0, 2\*\*32\), got "):
            _wire.int_in(bad, "nonce", **u32)
    with pytest.raises(ValueError, match=r"^nonce must be an int in \[0, 2\*\*32\), got 4294967296$"):
        _wire.int_in(2 ** 32, "nonce", **u32)
    assert _wire.int_in(1, "K", 1, None, "an int >= 1") == 1 and _wire.int_in(10 ** 12, "K", 1, None, "an int >= 1")
    with pytest.raises(ValueError, match=r"^K must be an int >= 1, got 0$"):
        _wire.int_in(0, "K", 1, None, "an int >= 1")
    assert _wire.int_in(-5, "row_base", None, None, "an int") == -5
    with pytest.raises(ValueError, match=r"^row_base must be an int, got True$"):
        _wire.int_in(True, "row_base", None, None, "an int")
    even = dict(lo=2, hi=9, what="an even int in [2, 8]", ok=lambda m: m % 2 == 0)
    assert _wire.int_in(2, "members", **even) == 2 and _wire.int_in(8, "members", **even) == 8
    for bad in (0, 3, 10):
        with pytest.raises(ValueError, match=r"^members must be an even int in \[2, 8\], got %d$" % bad):
            _wire.int_in(bad, "members", **even)


def test_finite_at_its_boundaries():
    inf, nan = float("inf"), float("nan")
    assert _wire.finite(0, "mu", 0) == 0.0 and type(_wire.finite(0, "mu", 0)) is float
    assert _wire.finite(np.float32(2.5), "mu", 0) == 2.5 and _wire.finite(1, "ess_target", 1) == 1.0
    for bad in (-1e-300, inf, nan, -inf):
        with pytest.raises(ValueError, match=r"^mu must be finite and >= 0, got "):
            _wire.finite(bad, "mu", 0)
    with pytest.raises(ValueError, match=r"^ess_target must be finite and >= 1, got 0.5$"):
        _wire.finite(0.5, "ess_target", 1)
    assert _wire.finite(1e-300, "lam", 0, above=True) == 1e-300
    for bad in (0, -1, inf, nan):
        with pytest.raises(ValueError, match=r"^lam must be finite and > 0, got "):
            _wire.finite(bad, "lam", 0, above=True)
    assert _wire.finite(-3, "gamma") == -3.0
    for bad in (inf, -inf, nan):
        with pytest.raises(ValueError, match=r"^gamma must be finite, got "):
            _wire.finite(bad, "gamma")


# ---------------------------------------------------------------------------------------------------------------------
# the upload-once cache
# ---------------------------------------------------------------------------------------------------------------------
def test_uploaded_reuses_the_copies_while_the_bytes_are_equal():
    env = _env()
    q = np.eye(3)
    first = _wire.uploaded(env, "weights", lambda: (q, None, q[:, :2].T))
    assert first[1] is None and first[0].dtype == torch.float64 and first[2].is_contiguous()
    assert torch.equal(first[2], torch.from_numpy(q[:, :2].T.copy()))
    again = _wire.uploaded(env, "weights", lambda: (q.copy(), None, q[:, :2].T.copy()))
    assert again[0] is first[0] and again[2] is first[2]
    changed = _wire.uploaded(env, "weights", lambda: (q * 2, None, q[:, :2].T))
    assert changed[0] is not first[0] and float(changed[0][0, 0]) == 2.0
    with_third = _wire.uploaded(env, "weights", lambda: (q * 2, q, q[:, :2].T))        # None -> an array: another key
    assert with_third[0] is not changed[0] and with_third[1] is not None
    other = _wire.uploaded(env, "other", lambda: (q,))                                 # slots do not share
    assert other[0] is not first[0] and set(env._uploaded) == {"weights", "other"}
    # a check that raises leaves the slot as it was
    def refuse():
        raise ValueError("Q must be symmetric")
    with pytest.raises(ValueError, match="Q must be symmetric"):
        _wire.uploaded(env, "other", refuse)
    assert _wire.uploaded(env, "other", lambda: (q,))[0] is other[0]


def test_uploaded_recognises_the_same_device_tensors_without_a_host_copy():
    env = _env()
    H, r = torch.eye(2, 12, dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    checks = []

    def check():
        checks.append(1)
        return H.numpy(), r.numpy()
    first = _wire.uploaded(env, "ekf", check, given=(H, r))
    again = _wire.uploaded(env, "ekf", check, given=(H, r))
    assert len(checks) == 1 and again is first and again[0] is first[0]
    assert env._uploaded["ekf"][3][0] is H                                  # the caller's tensors are kept alive
    r.mul_(2.0)                                                             # modified in place: checked again, new copy
    third = _wire.uploaded(env, "ekf", check, given=(H, r))
    assert len(checks) == 2 and third[1] is not first[1] and float(third[1][0]) == 2.0
    # equal values in other tensors: checked (by value), and the copies are reused
    fourth = _wire.uploaded(env, "ekf", check, given=(H.clone(), r))
    assert len(checks) == 3 and fourth[0] is third[0] and fourth[1] is third[1]
    # host arrays are never recognised by identity
    h = H.numpy()
    _wire.uploaded(env, "host", lambda: checks.append(1) or (h,), given=(h,))
    _wire.uploaded(env, "host", lambda: checks.append(1) or (h,), given=(h,))
    assert len(checks) == 5 and env._uploaded["host"][2] is None


# ---------------------------------------------------------------------------------------------------------------------
# outputs and the launch
# ---------------------------------------------------------------------------------------------------------------------
def test_empty_and_the_rollout_cache():
    env = _env()
    seen = []
    real = torch.empty

    def spy(*size, **kw):
        seen.append((size, kw))
        return real(*size, **kw)
    torch.empty = spy
    try:
        t = _wire.empty(env, (2, N), torch.float32)
    finally:
        torch.empty = real
    assert seen == [(((2, N),), {"dtype": torch.float32, "device": env.device})]      # looked up at call time
    assert tuple(t.shape) == (2, N) and t.dtype == torch.float32
    made = []
    a = _wire.rollout_cache(env, ("states", 3), lambda: made.append(1) or object())
    assert _wire.rollout_cache(env, ("states", 3), lambda: made.append(1) or object()) is a and made == [1]
    assert _wire.rollout_cache(env, ("states", 4), lambda: made.append(1) or object()) is not a
    assert set(env._rollout_out) == {("states", 3), ("states", 4)}


def test_launch(monkeypatch):
    env = _env()
    entered = []

    @contextlib.contextmanager
    def device(dev):
        entered.append(("in", dev))
        try:
            yield
        finally:
            entered.append(("out", dev))
    monkeypatch.setattr(torch.cuda, "device", device)
    io, mio = _wire.block(_lib.RolloutIO, num_steps=3), _wire.block(_lib.RolloutMlpIO)
    keep = [torch.zeros(1)]
    _wire.launch(env, "cs_probe", io, mio, None, keep=keep)
    assert entered == [("in", env.device), ("out", env.device)] and env._keep is keep
    (tag, ctx, a, b, c, stream), = env._lib.calls
    assert tag == "first" and ctx is env._ctx and stream.value == 77 and c is None
    assert a._obj is io and b._obj is mio                                   # byref() of the blocks, in order
    # the entry point is looked up by name at call time: an attribute replaced between two calls is seen by the second
    second = []
    env._lib.cs_probe = lambda *args: second.append(args) or 0
    _wire.launch(env, "cs_probe", io, keep=[])
    assert len(env._lib.calls) == 1 and len(second) == 1 and len(second[0]) == 3 and env._keep == []
    # a non-zero status raises through _lib.check, inside the device context, and _keep stays
    env._lib.cs_probe = lambda *args: _lib.ERR_ABI
    with pytest.raises(_lib.CopterStepError):
        _wire.launch(env, "cs_probe", io, keep=[1])
    assert env._keep == [] and entered[-1] == ("out", env.device)
    with pytest.raises(AttributeError):
        _wire.launch(env, "cs_no_such_entry", io, keep=[])


# ---------------------------------------------------------------------------------------------------------------------
# the import direction, and the names that moved
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rollout", "mlp", "mlp_rollout", "ilqr", "mppi", "es", "ppo", "ekf", "pf", "lqg", "ukf",
                                  "autodiff", "sharded"])
def test_every_family_module_imports_alone(name):
    """A cycle among the family modules shows up when one of them is the first import of a fresh interpreter."""
    r = subprocess.run([sys.executable, "-c", "import gym_copter_amd.%s" % name], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_family_module_imports_vecenv():
    import os
    root = os.path.dirname(gym_copter_amd.__file__)
    for name in ("_wire", "rollout", "mlp", "mlp_rollout", "ilqr", "mppi", "es", "ppo", "ekf", "pf", "lqg", "ukf"):
        src = open(os.path.join(root, name + ".py")).read()
        assert "from .vecenv import" not in src and "from . import vecenv" not in src, name
        assert "struct_size = C.sizeof" not in src or name == "_wire", name


MOVED = {"rollout": ("Rollout", "StepJacobian"), "mlp_rollout": ("MlpRollout",), "ilqr": ("LqrGains",),
         "mppi": ("MppiCosts", "MppiUpdate", "MppiTemperature", "mppi_knots"), "es": ("Population",),
         "ppo": ("ActorCritic", "PpoGrad"), "ekf": ("EkfResult", "RtsResult"), "pf": ("PfResult",),
         "lqg": ("LqgResult",), "ukf": ("UkfResult",)}


def test_public_names_are_the_family_modules_objects():
    import importlib
    from gym_copter_amd import vecenv
    for module, names in MOVED.items():
        m = importlib.import_module("gym_copter_amd." + module)
        for n in names:
            assert getattr(gym_copter_amd, n) is getattr(m, n) is getattr(vecenv, n), (module, n)
    mppi, ppo = importlib.import_module("gym_copter_amd.mppi"), importlib.import_module("gym_copter_amd.ppo")
    assert vecenv.PPO_STATS is ppo.PPO_STATS and vecenv.MPPI_MAX_KNOT is mppi.MPPI_MAX_KNOT
    assert vecenv._torch is _wire._torch and callable(vecenv._torch)
    # (gym_copter_amd.mppi, .ilqr, .es, .ppo, .ekf, .pf, .lqg, .ukf name the DRIVER functions in the package namespace)
    assert gym_copter_amd.mppi is mppi.mppi and gym_copter_amd.ppo is ppo.ppo


def test_every_wrapper_is_bound_in_the_class_body_from_its_module():
    import importlib
    homes = {"rollout": ("step_jacobian", "_rollout_io", "rollout_states", "rollout_vjp", "rollout_vjp_params"),
             "mlp_rollout": ("_mlp_io", "rollout_mlp_states", "rollout_mlp_vjp", "mlp_param_grad"),
             "ilqr": ("rollout_lqr", "rollout_feedback_states"),
             "mppi": ("rollout_mppi_costs", "rollout_mppi_update", "rollout_mppi_temperature"),
             "es": ("rollout_mlp_population", "es_perturb", "es_gradient"),
             "ppo": ("rollout_actor_critic", "gae", "ppo_grad"), "ekf": ("rollout_ekf", "rollout_rts"),
             "pf": ("rollout_pf",), "lqg": ("rollout_lqg",), "ukf": ("rollout_ukf",)}
    for module, names in homes.items():
        m = importlib.import_module("gym_copter_amd." + module)
        for n in names:
            assert vars(gym_copter_amd.CopterVecEnv)[n] is getattr(m, n), (module, n)


def test_sharded_forwards_by_table():
    from gym_copter_amd.sharded import _LOCAL_ROLLOUTS, ShardedCopterVecEnv
    calls = []

    class Local:
        def __getattr__(self, name):
            return lambda *a, **kw: calls.append((name, a, kw)) or name
    sh = object.__new__(ShardedCopterVecEnv)
    sh.local, sh.n_local, sh.total_envs, sh.first_row = Local(), 2, 6, 2
    acts = torch.arange(3 * 6 * 4, dtype=torch.float32).view(3, 6, 4)
    for name in _LOCAL_ROLLOUTS + ("rollout_mppi_temperature", "rollout_mlp_states", "rollout_mlp_vjp", "step_jacobian"):
        assert hasattr(ShardedCopterVecEnv, name), name
    for name in _LOCAL_ROLLOUTS:
        method = getattr(ShardedCopterVecEnv, name)
        assert method.__name__ == name and ("CopterVecEnv.%s of this rank's envs" % name) in method.__doc__
        assert getattr(sh, name)(acts, "second", key="word") == name                 # the global tape: sliced
        assert getattr(sh, name)(actions=acts[:, 2:4], key="word") == name            # by keyword, already local
        (n1, a1, k1), (n2, a2, k2) = calls[-2:]
        assert n1 == n2 == name and a1[1:] == ("second",) and k1 == k2 == {"key": "word"} and len(a2) == 1
        assert torch.equal(a1[0], acts[:, 2:4]) and torch.equal(a2[0], acts[:, 2:4])
        with pytest.raises(TypeError, match="actions"):                               # a missing tape says so
            getattr(sh, name)(key="word")
    with pytest.raises(ValueError, match=r"actions must have 2 \(local\) or 6 \(global\) envs in dimension 1, got 5"):
        sh.rollout_states(acts[:, :5])
