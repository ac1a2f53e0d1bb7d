"""CPU-side checks of cs_ppo_grad: the entry point declared, exported and bound, the ctypes struct
mirroring the header; bad argument blocks refused without touching a device; ppo() refusing an unknown `update` before
it touches its env; and the reference of tests/ppo_update_ref.py: its autograd gradient against central differences of
its own loss and the conditions of the GPU cases (self-checks that need no library: they pass without the feature); and
that the instantiation matrix of tests/test_gpu_ppo_grad_matrix.py reaches all 40 instantiations of the kernel's template."""
import ctypes as C
import os
import re

import pytest

import ppo_update_ref
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()


# ---------------------------------------------------------------------------------------------------------------------
# 1. layout and errors
# ---------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    assert re.search(r"int cs_ppo_grad\s*\(cs_ctx\* ctx, const cs_ppo_grad_io\* \w+,\s*void\* stream\);", HEADER)
    assert hasattr(lib, "cs_ppo_grad") and "cs_ppo_grad" in _lib.SYMBOLS
    assert lib.cs_ppo_grad.argtypes[1] is C.POINTER(_lib.PpoGradIO)
    assert lib.cs_version() == 5 == _lib.ABI_VERSION and re.search(r"#define CS_ABI_VERSION 5\b", HEADER)
    import gym_copter_amd
    assert callable(gym_copter_amd.ppo_loss) and gym_copter_amd.PpoGrad._fields == ("grad", "stats")
    assert hasattr(gym_copter_amd.CopterVecEnv, "ppo_grad")
    from gym_copter_amd import vecenv
    assert vecenv.PPO_STATS == ppo_update_ref.STATS and len(vecenv.PPO_STATS) == 8


def test_struct_mirrors_the_header_field_by_field():
    body = re.search(r"typedef struct cs_ppo_grad_io \{(.*?)\} cs_ppo_grad_io;", HEADER, re.S).group(1)
    decls = re.findall(r"([\w \*]+?)\b(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    mirror = _lib.PpoGradIO
    assert [f for _, f in decls] == [f for f, _ in mirror._fields_]
    size = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "float": 4, "double": 8}
    at = 0
    for (ctype, field), (name, _) in zip(decls, mirror._fields_):
        w = 8 if "*" in ctype else size[ctype.replace("const", "").strip()]
        at = (at + w - 1) // w * w
        assert getattr(mirror, name).offset == at and getattr(mirror, name).size == w, field
        at += w
    assert C.sizeof(mirror) == (at + 7) // 8 * 8 == 16 + 3 * 8 + 3 * 8 + 12 * 8
    assert decls[0][1] == "struct_size"


def _pio(**kw):
    pio = _lib.PpoGradIO()
    pio.struct_size = C.sizeof(pio)
    pio.hidden, pio.critic_hidden, pio.normalize = 8, 16, 1
    pio.num_rows, pio.num_samples, pio.row_base = 1000, 100, 0
    pio.clip, pio.vf_coef, pio.ent_coef = 0.2, 0.5, 0.01
    pio.actor_dev, pio.critic_dev, pio.log_std_dev = 0x1000, 0x2000, 0x3000
    pio.obs_dev, pio.actions_dev, pio.logp_dev, pio.advantages_dev = 0x10000, 0x20000, 0x30000, 0x40000
    pio.returns_dev, pio.live_dev, pio.index_dev = 0x50000, 0x60001, 0x70000
    pio.grad_dev, pio.stats_dev = 0x80000, 0x90000
    for k, v in kw.items():
        setattr(pio, k, v)
    return pio


def test_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    fn = lib.cs_ppo_grad
    assert fn(None, None, None) == _lib.ERR_ARG and b"null pio" in lib.cs_last_error()
    for delta in (-8, 8):        # the layout first: a block of another size with everything else wrong too
        bad = _pio(struct_size=C.sizeof(_lib.PpoGradIO) + delta, hidden=-1, num_rows=0, actor_dev=None)
        assert fn(None, C.byref(bad), None) == _lib.ERR_ABI and b"struct_size" in lib.cs_last_error()
    for key in ("hidden", "critic_hidden"):
        for H in (-1, _lib.MLP_MAX_HIDDEN + 1):
            assert fn(None, C.byref(_pio(**{key: H})), None) == _lib.ERR_ARG
            assert key.encode() in lib.cs_last_error()
    assert fn(None, C.byref(_pio(normalize=2)), None) == _lib.ERR_ARG and b"normalize" in lib.cs_last_error()
    for key in ("num_rows", "num_samples"):
        for v in (0, -1):
            assert fn(None, C.byref(_pio(**{key: v})), None) == _lib.ERR_ARG and key.encode() in lib.cs_last_error()
    for v in (0.0, -0.2, float("inf"), float("nan")):
        assert fn(None, C.byref(_pio(clip=v)), None) == _lib.ERR_ARG and b"clip" in lib.cs_last_error()
    for key in ("vf_coef", "ent_coef"):
        for v in (float("inf"), float("nan")):
            assert fn(None, C.byref(_pio(**{key: v})), None) == _lib.ERR_ARG
            assert (key + " must be finite").encode() in lib.cs_last_error()
    for key in ("actor_dev", "log_std_dev", "obs_dev", "actions_dev", "logp_dev", "advantages_dev", "grad_dev",
                "stats_dev"):
        assert fn(None, C.byref(_pio(**{key: None})), None) == _lib.ERR_ARG
        assert (key + " is required").encode() in lib.cs_last_error()
    assert fn(None, C.byref(_pio(returns_dev=None)), None) == _lib.ERR_ARG
    assert b"returns_dev is required with critic_dev" in lib.cs_last_error()
    # a row range outside the tapes (an index, whose values the host cannot see, is checked by the kernel instead)
    for kw in (dict(row_base=-1), dict(row_base=901), dict(num_samples=1001), dict(row_base=1 << 62)):
        assert fn(None, C.byref(_pio(index_dev=None, **kw)), None) == _lib.ERR_ARG and b"row_base" in lib.cs_last_error()
    assert fn(None, C.byref(_pio(obs_dev=0x10008)), None) == _lib.ERR_ARG and b"16-byte" in lib.cs_last_error()
    for key in ("index_dev", "grad_dev", "stats_dev"):
        assert fn(None, C.byref(_pio(**{key: 0x70004})), None) == _lib.ERR_ARG and b"8-byte" in lib.cs_last_error()
    for key in ("actor_dev", "critic_dev", "log_std_dev", "actions_dev", "logp_dev", "advantages_dev", "returns_dev"):
        assert fn(None, C.byref(_pio(**{key: 0x1002})), None) == _lib.ERR_ARG and b"4-byte" in lib.cs_last_error()
    # ... as far as the context: no critic with or without returns, no live mask, a row range, more samples than rows
    for ok in (_pio(), _pio(critic_dev=None), _pio(critic_dev=None, returns_dev=None), _pio(live_dev=None),
               _pio(index_dev=None, row_base=900), _pio(num_samples=5000), _pio(hidden=0, critic_hidden=64, normalize=0),
               _pio(ent_coef=-1.0, vf_coef=0.0, clip=1e-9)):
        assert fn(None, C.byref(ok), None) == _lib.ERR_ARG and lib.cs_last_error() == b"null context"


def test_ppo_rejects_an_unknown_update_without_touching_the_env():
    import gym_copter_amd

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("ppo touched env.%s before it refused `update`" % name)
    for bad in ("host", "", None, "Device", 1):
        with pytest.raises(ValueError, match="update"):
            gym_copter_amd.ppo(Untouchable(), None, None, None, 16, 16, 8, 1, update=bad)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference (self-checks: they pass without the feature)
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_gradient_against_central_differences_of_its_own_loss():
    """50 rows, every parameter of both networks and log_std: autograd against (L(p + e) - L(p - e)) / 2e in float64 with
    e = 1e-6: the truncation error is e^2 L''' / 6 ~ 1e-12 x the third derivative and the rounding error 2^-53 |L| / e =
    1e-10 |L|; 1e-6 scaled is taken (third derivatives of exp((a - mu)^2 / sigma^2) at sigma = 0.05 are ~1e5).  A self-check
    that passes without the feature."""
    import torch
    for H, Hv, normalize in ((5, 3, True), (0, 0, False)):
        s = ppo_update_ref.synthetic("lander2d", H, Hv, 50, 8)
        idx = s["perm"][:40]
        kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, normalize=normalize)
        ref = ppo_update_ref.reference(s, idx, **kw)
        assert ref["edge"] > 1e-4 and 0 < ref["clip_fraction"] < 1
        grad = ref["grad"]
        P, Pv = s["actor"].shape[0], s["critic"].shape[0]
        e = 1e-6
        fd = torch.zeros_like(grad)
        for name, at, size in (("actor", 0, P), ("critic", P, Pv), ("log_std", P + Pv, grad.shape[0] - P - Pv)):
            for i in range(size):
                vals = []
                for sign in (1.0, -1.0):
                    t = dict(s)
                    p = s[name].double().clone()
                    p[i] += sign * e
                    t[name] = p                                  # (float64 parameters: evaluate() keeps them as they are)
                    vals.append(float(ppo_update_ref.evaluate(t, idx, **kw)["loss"]))
                fd[at + i] = (vals[0] - vals[1]) / (2 * e)
        err = ppo_update_ref.scaled(grad, fd)
        print("reference autograd against central differences, H = %d / %d: %.2e scaled" % (H, Hv, err))
        assert float(grad.abs().max()) > 1e-3 and err <= 1e-6, err


def test_the_gpu_cases_meet_their_conditions_on_the_reference():
    """For every case of the GPU test (both clips): at least 1 % of the live samples clipped, at least 50 % not, no ratio
    within 1e-8 of a clip edge, at least one dead row; the bar's constant covers the derived budget; and the float32
    autograd gradient differs from the float64 one (the kernel has something to beat).  A self-check of the test inputs
    that passes without the feature."""
    import torch
    for task, H, Hv, R, B, seed, opt in ppo_update_ref.CASES:
        if B > 5000:
            continue                                              # (the large case is checked where it runs)
        s = ppo_update_ref.synthetic(task, H, Hv, R, seed)
        rng = opt.get("range", False)
        idx = torch.arange(B) if rng else s["perm"][:B]
        for clip in (0.2, 0.1):
            kw = dict(clip=clip, vf_coef=0.5, ent_coef=0.01, normalize=opt.get("normalize", True), live=not rng)
            ref = ppo_update_ref.reference(s, idx, **kw)
            ppo_update_ref.check_conditions(ref, need_dead=not rng)
            assert ref["c_needed"] <= ppo_update_ref.BAR_C and ref["c_stats"] <= ppo_update_ref.BAR_C
            assert ppo_update_ref.float32_distance(s, idx, ref["grad"], **kw) > 1e-8


def test_the_matrix_reaches_every_instantiation_full_and_ragged():
    """ppo_update_ref.MATRIX against the kernel's dispatch, restated: the (OBS, A) shape of the task, HP =
    width_class(hidden), the head.  All 4 x 5 x 2 = 40 instantiations of <OBS, A, HP, head> occur; over the matrix every
    class H > 0 runs at its full width (H = HP: no idle lanes) and at a ragged one, for both heads; lander1d and hover2d,
    which share two of the shapes, occur by name; and B leaves a ragged last tile after more than one full one.  A later
    edit of the list cannot lose coverage silently."""
    pur = ppo_update_ref
    assert [pur.width_class(H) for H in (0, 1, 8, 9, 16, 17, 32, 33, 64)] == [0, 8, 8, 16, 16, 32, 32, 64, 64]
    shapes = {pur.TASK_SHAPE[t] for t in ("lander3d", "hover3d", "lander2d", "hover1d")}
    assert len(shapes) == 4 and pur.TASK_SHAPE["lander1d"] == pur.TASK_SHAPE["hover1d"]
    assert pur.TASK_SHAPE["hover2d"] == pur.TASK_SHAPE["lander2d"]
    from gym_copter_amd import vecenv
    for task, shape in pur.TASK_SHAPE.items():
        assert vecenv._TASK_SHAPES[task][1:] == shape, task
    triples, widths = set(), {"policy": set(), "value": set()}
    for task, H, Hv, R, B, seed in pur.MATRIX:
        assert (R, B) == (512, 300) and B // 64 > 1 and B % 64 != 0
        triples.add((pur.TASK_SHAPE[task], pur.width_class(H), "policy"))
        triples.add((pur.TASK_SHAPE[task], pur.width_class(Hv), "value"))
        widths["policy"].add(H)
        widths["value"].add(Hv)
    assert triples == {(shape, hp, head) for shape in shapes for hp in (0, 8, 16, 32, 64) for head in ("policy", "value")}
    assert len(triples) == 40
    for head, seen in widths.items():
        for hp in (8, 16, 32, 64):
            assert hp in seen, (head, hp)                                             # full
            assert any(pur.width_class(H) == hp and H != hp for H in seen), (head, hp)    # ragged
    assert {"lander1d", "hover2d"} <= {case[0] for case in pur.MATRIX}
    assert len(set(pur.MATRIX)) == len(pur.MATRIX) == 22


def test_the_matrix_and_degenerate_cases_meet_their_conditions_on_the_reference():
    """The conditions of the cases of tests/test_gpu_ppo_grad_matrix.py that are small enough to check here (the two of
    200 000 samples are checked where they run), on the reference alone: check_conditions() and the bar's constant over
    MATRIX, the equal-advantage cases without normalisation and the row range with a live mask; the bar's constant over
    the one-live-sample cases.  With normalisation the two degenerate set-ups have a deviation of exactly 0 in float64
    too.  A self-check of the test inputs that passes without the feature."""
    import torch
    pur = ppo_update_ref
    kw = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01)

    def holds(ref, conditions=True):
        if conditions:
            pur.check_conditions(ref)
        assert ref["c_needed"] <= pur.BAR_C and ref["c_stats"] <= pur.BAR_C, (ref["c_needed"], ref["c_stats"])
    for task, H, Hv, R, B, seed in pur.MATRIX:
        s = pur.synthetic(task, H, Hv, R, seed)
        holds(pur.reference(s, s["perm"][:B], **kw))
    for task, H, Hv, seed in pur.ONE_LIVE:
        s, idx = pur.one_live(task, H, Hv, seed)
        assert idx.shape[0] == 65 and int(s["live"][idx].sum()) == 1 == int(s["live"].sum())
        holds(pur.reference(s, idx, normalize=False, **kw), conditions=False)
    for task, H, Hv, seed in pur.EQUAL_ADV:
        s, idx = pur.equal_advantages(task, H, Hv, seed)
        ref = pur.reference(s, idx, normalize=False, **kw)
        holds(ref)
        w, a = s["live"][idx].double(), s["advantages"][idx].double()
        assert 1 < ref["count"] < idx.shape[0] == 256 and float((a * w).sum() / w.sum()) == 0.5
    task, H, Hv, seed = pur.RANGE_LIVE
    s = pur.synthetic(task, H, Hv, pur.DEGENERATE_R, seed)
    holds(pur.reference(s, torch.arange(pur.RANGE_BASE, pur.RANGE_BASE + pur.RANGE_B), **kw))
    for task, H, Hv, R, B, seed in pur.LARGE:
        tiles = -(-B // 64)
        assert -(-tiles // 1024) == 4 and tiles % 4 != 0 and B <= R
