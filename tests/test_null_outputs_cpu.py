"""CPU-side checks of tests/null_outputs.py (the table of optional, required and forbidden output pointers, and the
interposer that nulls them in a wrapper's call) and of the refusals the table promises, with ctx = NULL:

  - the table is complete: every non-const pointer member of every io block of every cs_rollout_*, cs_step_jacobian,
    cs_mlp_param_grad, cs_es_*, cs_gae and cs_ppo_grad declaration of include/copterstep.h has a class for that entry
    point, so that an output added later fails here until it is classified (and tests/test_gpu_null_outputs.py sweeps it);
  - the interposer nulls exactly the named members, restores the attribute after an exception, and fails when the
    function was never reached;
  - every `required`, `input` and `must_be_null` member is refused with CS_ERR_ARG and a message that names it (or says
    "must be NULL") before the context is looked at, from a block that is otherwise accepted as far as the context.
    cs_step_jacobian checks its block behind the context: its refusals need a device (tests/test_gpu_null_outputs.py)."""
import ctypes as C
import os
import types

import pytest

import null_outputs as NO
from gym_copter_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "copterstep.h")).read()
STRUCTS, FUNCTIONS = NO.parse_header(HEADER)


# ---------------------------------------------------------------------------------------------------------------------
# 1. completeness
# ---------------------------------------------------------------------------------------------------------------------
def test_every_tabled_declaration_has_a_row_and_every_row_a_declaration():
    declared = NO.tabled_functions(FUNCTIONS)
    assert len(declared) == 29 and declared[0] == "cs_es_gradient"
    assert sorted(NO.TABLE) == declared
    for name in declared:
        assert list(NO.TABLE[name].blocks) == FUNCTIONS[name], name      # the io blocks of the C signature, in order
        assert NO.TABLE[name].note, name


def test_every_output_member_of_every_block_is_classified():
    for name, row in NO.TABLE.items():
        want = {b + "." + m for b in row.blocks for m in NO.output_members(STRUCTS, b)}
        assert set(row.fields) == want, (name, sorted(set(row.fields) ^ want))
        assert set(row.fields.values()) <= set(NO.CLASSES)
    # the parser sees what it should: the filter's thirteen pointers, eight of them outputs
    assert len([t for t, _ in STRUCTS["cs_rollout_ekf_io"] if "*" in t]) == 13
    assert NO.output_members(STRUCTS, "cs_rollout_ekf_io") == ["x_pred_dev", "P_dev", "P_tape_dev", "var_dev", "nis_dev",
                                                               "loglik_dev", "branch_dev", "ok_dev"]
    assert NO.output_members(STRUCTS, "cs_rollout_mlp_ex_io") == []


def test_an_added_output_member_is_noticed():
    """the completeness check's own negative case: one more non-const pointer in cs_rollout_ekf_io"""
    grown = HEADER.replace("  uint8_t* ok_dev;             /* [N] */\n} cs_rollout_ekf_io;",
                           "  uint8_t* ok_dev;\n  double* gain_dev;\n} cs_rollout_ekf_io;")
    assert grown != HEADER
    structs, _ = NO.parse_header(grown)
    row = NO.TABLE["cs_rollout_ekf"]
    want = {b + "." + m for b in row.blocks for m in NO.output_members(structs, b)}
    assert want - set(row.fields) == {"cs_rollout_ekf_io.gain_dev"}


def test_the_mirrors_have_the_classified_members():
    for block, cls in NO.STRUCTS.items():
        names = [f for f, _ in getattr(_lib, cls)._fields_]
        assert names == [m for _, m in STRUCTS[block]], block
    for (entry, member), const in NO.CONDITIONAL.items():
        assert NO.TABLE[entry].fields[member] == NO.REQUIRED and const.split(".")[0] in NO.TABLE[entry].blocks


# ---------------------------------------------------------------------------------------------------------------------
# 2. the interposer, on a fake function object
# ---------------------------------------------------------------------------------------------------------------------
def _ekf_blocks():
    io, eio = _lib.RolloutIO(), _lib.RolloutEkfIO()
    for k, (f, t) in enumerate(io._fields_):
        setattr(io, f, 0x1000 * (k + 1) if t is C.c_void_p else k + 1)
    for k, (f, t) in enumerate(eio._fields_):
        setattr(eio, f, 0x100000 * (k + 1) if t is C.c_void_p else k + 1)
    return io, eio


def _fake():
    seen = []

    def cs_rollout_ekf(ctx, io, eio, stream):
        seen.append((ctx, bytes(io._obj), bytes(eio._obj), stream))
        return -7
    return types.SimpleNamespace(cs_rollout_ekf=cs_rollout_ekf), cs_rollout_ekf, seen


def test_interposer_nulls_exactly_the_named_members_and_no_others():
    lib, real, seen = _fake()
    io, eio = _ekf_blocks()
    before = bytes(io), bytes(eio)
    with NO.nulling(lib, "cs_rollout_ekf") as calls:
        assert lib.cs_rollout_ekf is not real
        assert lib.cs_rollout_ekf(11, C.byref(io), C.byref(eio), 22) == -7
    assert lib.cs_rollout_ekf is real
    assert seen[-1] == (11, before[0], before[1], 22) and len(calls) == 1 and calls[0].rc == -7
    assert calls[0].seen["cs_rollout_ekf_io.nis_dev"] == eio.nis_dev and calls[0].seen["cs_rollout_io.x_dev"] == io.x_dev
    assert set(calls[0].seen) == set(NO.TABLE["cs_rollout_ekf"].fields)
    with NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.nis_dev", "cs_rollout_io.x_dev"]) as calls:
        lib.cs_rollout_ekf(11, C.byref(io), C.byref(eio), 22)
    want_io, want_eio = _ekf_blocks()
    want_io.x_dev, want_eio.nis_dev = None, None
    assert seen[-1] == (11, bytes(want_io), bytes(want_eio), 22)              # less those pointers, and nothing else
    assert (bytes(io), bytes(eio)) == before                                  # the caller's blocks are put back
    assert calls[0].seen["cs_rollout_ekf_io.nis_dev"] == eio.nis_dev          # `seen` is what the wrapper had wired
    with pytest.raises(KeyError):
        NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.H_dev"])         # an input is no classified output
    with pytest.raises(KeyError):
        NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_lqg_io.z_dev"])


def test_interposer_restores_the_attribute_after_an_exception():
    lib, real, seen = _fake()
    io, eio = _ekf_blocks()
    with pytest.raises(RuntimeError, match="inside"):
        with NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.P_dev"]):
            lib.cs_rollout_ekf(None, C.byref(io), C.byref(eio), None)
            raise RuntimeError("inside")
    assert lib.cs_rollout_ekf is real and len(seen) == 1

    def boom(*a):
        raise ValueError("from the function")
    lib.cs_rollout_ekf = boom
    with pytest.raises(ValueError, match="from the function"):
        with NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.P_dev"]):
            lib.cs_rollout_ekf(None, C.byref(io), C.byref(eio), None)
    assert lib.cs_rollout_ekf is boom and eio.P_dev == _ekf_blocks()[1].P_dev  # attribute and member both restored


def test_interposer_fails_when_the_function_was_never_reached():
    lib, real, seen = _fake()
    with pytest.raises(AssertionError, match="never reached"):
        with NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.nis_dev"]):
            pass
    assert lib.cs_rollout_ekf is real and not seen
    io, _ = _ekf_blocks()
    with pytest.raises(AssertionError, match="passes no cs_rollout_ekf_io block"):
        with NO.nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.nis_dev"]):
            lib.cs_rollout_ekf(None, C.byref(io), None, None)
    assert lib.cs_rollout_ekf is real


def test_interposer_forwards_to_another_entry_point_without_the_null_block():
    seen = []
    lib = types.SimpleNamespace(cs_rollout_mlp_vjp_ex=lambda *a: seen.append(("ex",) + a) or 0,
                                cs_rollout_mlp_vjp=lambda *a: seen.append(("plain", len(a), bytes(a[1]._obj))) or 0)
    io, mio = _lib.RolloutIO(), _lib.RolloutMlpIO()
    io.g_actions_dev, io.g_x0_dev = 0x1000, 0x2000
    with NO.nulling(lib, "cs_rollout_mlp_vjp_ex", ["cs_rollout_io.g_x0_dev"], forward_to="cs_rollout_mlp_vjp") as calls:
        lib.cs_rollout_mlp_vjp_ex(None, C.byref(io), C.byref(mio), None, None)
    want = _lib.RolloutIO()
    want.g_actions_dev = 0x1000
    assert seen == [("plain", 4, bytes(want))] and calls[0].seen["cs_rollout_io.g_x0_dev"] == 0x2000


# ---------------------------------------------------------------------------------------------------------------------
# 3. the refusals, with ctx = NULL
# ---------------------------------------------------------------------------------------------------------------------
SCALARS = dict(num_steps=2, num_meas=1, num_particles=64, first_step=1, ess_frac=0.5, gamma=1.0, wm0=0.5, wc0=0.5, wi=0.02,
               members=2, envs_per_member=64, num_params=1, num_samples=1, lam=1.0, num_rows=1, clip=0.2, ess_target=1.0,
               lam_min=0.1, lam_max=1.0, flag_stride=1, sigma=0.1)
# const pointers a valid call leaves NULL (the outputs that must be NULL come from the table)
_NO_PENDING = ["cs_rollout_io.start_force_dev", "cs_rollout_io.start_prev_shaping_dev", "cs_rollout_io.gx_dev",
               "cs_rollout_io.gr_dev"]
_POLICY_ACTS = ["cs_rollout_io.actions_dev"]
INPUTS_NULL = {
    "cs_rollout_mlp_states": _POLICY_ACTS, "cs_rollout_mlp_vjp": _POLICY_ACTS, "cs_rollout_mlp_vjp_ex": _POLICY_ACTS,
    "cs_rollout_mlp_population": _POLICY_ACTS,
    "cs_rollout_ekf": _NO_PENDING, "cs_rollout_rts": _NO_PENDING, "cs_rollout_ukf": _NO_PENDING,
    "cs_rollout_pf": _NO_PENDING + ["cs_rollout_pf_io.part_in_dev", "cs_rollout_pf_io.pstatus_in_dev",
                                    "cs_rollout_pf_io.lw_in_dev"],
    "cs_rollout_lqg": ["cs_rollout_io.gx_dev", "cs_rollout_io.gr_dev"],
}
BEHIND_THE_CONTEXT = {"cs_step_jacobian"}
CASES = [(e, f) for e, row in sorted(NO.TABLE.items()) if e not in BEHIND_THE_CONTEXT
         for f, c in row.fields.items() if c in (NO.REQUIRED, NO.INPUT, NO.MUST_BE_NULL)]


def _valid(entry):
    """the blocks of a call of `entry` that is accepted as far as the context: fake, distinct, 256-B aligned pointers"""
    row = NO.TABLE[entry]
    blocks, at = {}, 0x10000
    for b in row.blocks:
        s = getattr(_lib, NO.STRUCTS[b])()
        s.struct_size = C.sizeof(s)
        for f, t in s._fields_:
            if t is C.c_void_p:
                setattr(s, f, at)
                at += 0x10000
            elif f in SCALARS:
                setattr(s, f, SCALARS[f])
        blocks[b] = s
    for f in NO.of_class(entry, NO.MUST_BE_NULL) + INPUTS_NULL.get(entry, []):
        setattr(blocks[f.split(".")[0]], f.split(".")[1], None)
    return blocks


def _call(entry, blocks):
    lib = _lib.load()
    rc = getattr(lib, entry)(None, *[C.byref(blocks[b]) for b in NO.TABLE[entry].blocks], None)
    return rc, lib.cs_last_error().decode()


@pytest.mark.parametrize("entry", sorted(e for e, row in NO.TABLE.items() if row.blocks))
def test_the_valid_block_is_accepted_as_far_as_the_context(entry):
    """... with every optional output present, and with every optional and unused output NULL"""
    blocks = _valid(entry)
    assert _call(entry, blocks) == (_lib.ERR_ARG, "null context")
    for f in NO.of_class(entry, NO.OPTIONAL) + NO.of_class(entry, NO.UNUSED):
        setattr(blocks[f.split(".")[0]], f.split(".")[1], None)
    assert _call(entry, blocks) == (_lib.ERR_ARG, "null context")


@pytest.mark.parametrize("entry,field", CASES)
def test_required_and_forbidden_members_are_refused_before_the_context(entry, field):
    blocks = _valid(entry)
    b, m = field.split(".")
    cls = NO.TABLE[entry].fields[field]
    if cls == NO.MUST_BE_NULL:
        setattr(blocks[b], m, 0x7f0000)
        rc, msg = _call(entry, blocks)
        assert rc == _lib.ERR_ARG and "must be NULL" in msg and msg.startswith(entry + ":"), msg
        return
    setattr(blocks[b], m, None)
    rc, msg = _call(entry, blocks)
    assert rc == _lib.ERR_ARG and m in msg and "required" in msg and msg.startswith(entry + ":"), msg
    const = NO.CONDITIONAL.get((entry, field))
    if const is not None:                        # ... and without the input that asks for it, it must be NULL
        blocks = _valid(entry)
        setattr(blocks[const.split(".")[0]], const.split(".")[1], None)
        rc, msg = _call(entry, blocks)
        assert rc == _lib.ERR_ARG and m in msg and "must be NULL" in msg, msg
        setattr(blocks[b], m, None)
        assert _call(entry, blocks) == (_lib.ERR_ARG, "null context")
