"""Optional outputs of the C entry points, NULL: the table of what include/copterstep.h says of every output pointer, and
the interposer that lets a test repeat a wrapper's call with some of them nulled (tests/test_null_outputs_cpu.py,
tests/test_gpu_null_outputs.py).  No GPU code of its own.

The wrappers of gym_copter_amd always wire every output, so the `!= nullptr` branches of the kernels run only for C
callers.  `with nulling(lib, "cs_rollout_ekf", ["cs_rollout_ekf_io.nis_dev"]) as calls:` replaces that one function
attribute of the loaded library object (the one the env calls through) with a Python callable that sets the named pointer
members of the byref'd io blocks to NULL, forwards every argument to the real function unchanged otherwise, puts the
members back and records the call; the attribute is restored on the way out, whatever happened inside.  Leaving the
block without the function having been reached is an error: a test cannot pass empty.

TABLE has one row per entry point from cs_step_jacobian to cs_ppo_grad -- the cs_rollout_*, cs_step_jacobian,
cs_mlp_param_grad, cs_es_*, cs_gae and cs_ppo_grad declarations of the header -- and classifies, for that entry point,
every non-const pointer member of every io block it takes:

  optional      the header says it may be NULL (not written)
  required      NULL is refused with CS_ERR_ARG before any launch
  input         the call reads it (a backward's tape); NULL is refused as for `required`
  must_be_null  anything else is refused with CS_ERR_ARG
  unused        the header says the call does not use the member: any value is accepted, nothing is read or written.
                (A fifth class beside the four a pointer of the call's own can have: cs_rollout_io and cs_rollout_mppi_io
                serve several entry points, and each of them leaves the others' members alone.)

The header's text is the source; where it is silent the launcher's check decided and the row's comment says so."""
import collections
import ctypes as C
import re

OPTIONAL, REQUIRED, INPUT, MUST_BE_NULL, UNUSED = "optional", "required", "input", "must_be_null", "unused"
CLASSES = (OPTIONAL, REQUIRED, INPUT, MUST_BE_NULL, UNUSED)

# header struct -> its ctypes mirror in gym_copter_amd._lib
STRUCTS = {
    "cs_jacobian_io": "JacobianIO", "cs_rollout_io": "RolloutIO", "cs_rollout_param_io": "RolloutParamIO",
    "cs_rollout_mlp_io": "RolloutMlpIO", "cs_rollout_mlp_ex_io": "RolloutMlpExIO", "cs_mlp_grad_io": "MlpGradIO",
    "cs_rollout_lqr_io": "RolloutLqrIO", "cs_rollout_feedback_io": "RolloutFeedbackIO",
    "cs_rollout_ekf_io": "RolloutEkfIO", "cs_rollout_rts_io": "RolloutRtsIO", "cs_rollout_pf_io": "RolloutPfIO",
    "cs_rollout_lqg_io": "RolloutLqgIO", "cs_rollout_ukf_io": "RolloutUkfIO", "cs_rollout_mppi_io": "RolloutMppiIO",
    "cs_rollout_mppi_ext": "RolloutMppiExt", "cs_rollout_population_io": "RolloutPopulationIO", "cs_es_io": "EsIO",
    "cs_rollout_ac_io": "RolloutAcIO", "cs_gae_io": "GaeIO", "cs_ppo_grad_io": "PpoGradIO",
}

Row = collections.namedtuple("Row", "blocks fields note")


def _row(note, **blocks):
    """blocks: header struct -> {class: "member member ..."} in the order of the C signature"""
    fields = {}
    for block, classes in blocks.items():
        assert block in STRUCTS, block
        for cls, members in classes.items():
            assert cls in CLASSES, cls
            for m in members.split():
                assert block + "." + m not in fields, m
                fields[block + "." + m] = cls
    return Row(tuple(blocks), fields, note)


_FWD_IO = dict(optional="x_dev reward_dev terminated_dev truncated_dev status_dev", unused="g_actions_dev g_x0_dev")
_BWD_IO = dict(input="x_dev status_dev", optional="g_actions_dev g_x0_dev", unused="reward_dev terminated_dev truncated_dev")
_NO_IO_OUT = dict(unused="x_dev reward_dev terminated_dev truncated_dev status_dev g_actions_dev g_x0_dev")
_FILTER_IO = dict(optional="x_dev status_dev", must_be_null="reward_dev terminated_dev truncated_dev g_actions_dev g_x0_dev")
_KALMAN = "x_pred_dev P_dev P_tape_dev var_dev nis_dev loglik_dev"
_MPPI_COSTS = dict(required="costs_dev", optional="best_dev", unused="actions_out_dev ess_dev cost_min_dev")
_MPPI_UPDATE = dict(input="costs_dev", required="actions_out_dev", optional="ess_dev cost_min_dev", unused="best_dev")
_EXT_UNUSED = dict(unused="lam_out_dev ess_out_dev")

TABLE = {
    "cs_rollout_pid": _row(
        "bare pointers, no io block: the step family, covered by tests/test_gpu_served.py (out of this table's scope)"),
    "cs_rollout_random": _row(
        "bare pointers, no io block: the step family, covered by tests/test_gpu_served.py (out of this table's scope)"),
    "cs_step_jacobian": _row(
        "'Every output pointer may be NULL (not written)'.  One kernel per <TASK, MODE>; the float32 / float64 stores are "
        "a run-time branch.  Its argument checks follow the context, so its refusals need a device.",
        cs_jacobian_io=dict(optional="dx_dev du_dev reward_dx_dev reward_du_dev branch_dev")),
    "cs_rollout_states": _row(
        "'Each of them may be NULL (not written)' of x, reward, the flags and status.  The header is silent on the "
        "gradient outputs in a forward call; the launcher never looks at them: unused.  One kernel per <TASK, MODE>.",
        cs_rollout_io=_FWD_IO),
    "cs_rollout_states_ex": _row(
        "as cs_rollout_states; 'cs_rollout_states_ex reads vehicle_dev only' of the parameter block",
        cs_rollout_io=_FWD_IO, cs_rollout_param_io=dict(unused="g_vehicle_dev g_force_dev")),
    "cs_rollout_vjp": _row(
        "'either may be NULL' of g_actions and g_x0; 'x_dev and status_dev are READ (both required)'.  The forward's "
        "reward and flags are not mentioned and not looked at: unused.  Kernels: <TASK, MODE, GYRO> by the context.",
        cs_rollout_io=_BWD_IO),
    "cs_rollout_vjp_ex": _row(
        "'NULL = not wanted' of g_vehicle and g_force.  The launcher picks by them: both NULL launches cs_rollout_vjp's "
        "kernel, either present the parameter sweep (SweepParam), g_vehicle present the unfold kernel behind it -- the "
        "subsets 'each nulled alone', 'each present alone' and 'all nulled' reach all three.",
        cs_rollout_io=_BWD_IO, cs_rollout_param_io=dict(optional="g_vehicle_dev g_force_dev")),
    "cs_rollout_mlp_states": _row(
        "io's outputs 'as cs_rollout_states does'; actions_out_dev 'required: it is the backward's tape'; obs_out_dev "
        "'or NULL (not written)'.  Kernels: <TASK, MODE, HIDDEN class> by mio->hidden.",
        cs_rollout_io=_FWD_IO, cs_rollout_mlp_io=dict(required="actions_out_dev", optional="obs_out_dev")),
    "cs_rollout_mlp_vjp": _row(
        "'reads the tape (io x_dev, status_dev and actions_out_dev ...; offsets_dev and obs_out_dev are not read)'.  "
        "The header says of g_actions_dev and g_x0_dev only what cs_rollout_vjp says ('the derivative rules are "
        "cs_rollout_vjp's'); the sweep is the same code and guards both: optional.",
        cs_rollout_io=_BWD_IO, cs_rollout_mlp_io=dict(input="actions_out_dev", unused="obs_out_dev")),
    "cs_rollout_mlp_vjp_ex": _row(
        "as cs_rollout_mlp_vjp (cs_rollout_mlp_ex_io has no output).  The launcher picks the kernel with the action "
        "cotangent by g_actions_in_dev, an input.",
        cs_rollout_io=_BWD_IO, cs_rollout_mlp_io=dict(input="actions_out_dev", unused="obs_out_dev"),
        cs_rollout_mlp_ex_io={}),
    "cs_mlp_param_grad": _row("'g_params_dev is WRITTEN': the call's only output, required by the launcher",
                              cs_mlp_grad_io=dict(required="g_params_dev")),
    "cs_rollout_lqr": _row(
        "'Outputs, each may be NULL'; io is 'cs_rollout_vjp's block -- the tape x_dev / status_dev ...; its cotangents "
        "and gradient outputs are not used'.  Kernels: <TASK, MODE, GYRO> by the context.",
        cs_rollout_io=dict(input="x_dev status_dev", unused="reward_dev terminated_dev truncated_dev g_actions_dev g_x0_dev"),
        cs_rollout_lqr_io=dict(optional="K_dev d_dev dV_dev S0_dev s0_dev ok_dev")),
    "cs_rollout_feedback_states": _row(
        "'Outputs are cs_rollout_states'' plus actions_out_dev (required)",
        cs_rollout_io=_FWD_IO, cs_rollout_feedback_io=dict(required="actions_out_dev")),
    "cs_rollout_ekf": _row(
        "'x_dev (or NULL) ... status_dev (or NULL)'; 'the reward, flag, cotangent and gradient pointers must be NULL'; "
        "'Outputs, each may be NULL'.  Kernels: <TASK, MODE, GYRO> by the context's rotor_gyro; P / P_tape present or "
        "absent changes the wave_sync() sequence of filter_store_row inside one kernel.",
        cs_rollout_io=_FILTER_IO, cs_rollout_ekf_io=dict(optional=_KALMAN + " branch_dev ok_dev")),
    "cs_rollout_rts": _row(
        "'x_dev (or NULL) receives the smoothed means; every other pointer of io must be NULL' (status_dev included); "
        "'Outputs, each may be NULL'.  Kernels: <TASK, MODE, GYRO>; end_x / end_P is a run-time branch.",
        cs_rollout_io=dict(optional="x_dev",
                           must_be_null="reward_dev terminated_dev truncated_dev status_dev g_actions_dev g_x0_dev"),
        cs_rollout_rts_io=dict(optional="P_tape_dev var_dev x0_dev P0_s_dev ok_dev")),
    "cs_rollout_pf": _row(
        "'the reward, flag, cotangent and gradient pointers ... must be NULL'; 'Outputs, each may be NULL', the tapes "
        "among them.  Kernels: <TASK, MODE, GYRO> and the workgroup size by num_particles; P_dev present adds two "
        "__syncthreads() on the last step.",
        cs_rollout_io=_FILTER_IO,
        cs_rollout_pf_io=dict(optional="var_dev ess_dev resampled_dev best_dev P_dev loglik_dev ok_dev part_out_dev "
                                       "pstatus_out_dev lw_out_dev part_tape_dev pstatus_tape_dev lw_tape_dev wq_tape_dev "
                                       "anc_tape_dev")),
    "cs_rollout_lqg": _row(
        "the truth's tapes 'each may be NULL'; the filter's outputs 'each may be NULL'; z 'is stored to z_dev (or NULL)'; "
        "actions_out_dev required; 'io's cotangent and gradient pointers must be NULL'",
        cs_rollout_io=dict(optional="x_dev reward_dev terminated_dev truncated_dev status_dev",
                           must_be_null="g_actions_dev g_x0_dev"),
        cs_rollout_lqg_io=dict(required="actions_out_dev",
                               optional="z_dev xhat_dev " + _KALMAN + " fstatus_dev branch_dev ok_dev")),
    "cs_rollout_ukf": _row(
        "io 'as cs_rollout_ekf'; 'Outputs, each may be NULL'.  filter_store_row syncs unconditionally here "
        "(STAGE_ALWAYS_REUSED); the point tapes are run-time branches.",
        cs_rollout_io=_FILTER_IO,
        cs_rollout_ukf_io=dict(optional=_KALMAN + " spread_dev ok_dev points_dev points_pred_dev point_status_dev")),
    "cs_rollout_mppi_costs": _row(
        "costs_dev 'required'; best_dev 'when best_dev != NULL' (a second kernel, launched only then); 'io's outputs, "
        "cotangents and gradients are not used'; the update's members are not looked at",
        cs_rollout_io=_NO_IO_OUT, cs_rollout_mppi_io=_MPPI_COSTS),
    "cs_rollout_mppi_update": _row(
        "actions_out_dev required; ess_dev and cost_min_dev 'each of the two may be NULL'; 'reads io->actions_dev and "
        "io->num_steps only'",
        cs_rollout_io=_NO_IO_OUT, cs_rollout_mppi_io=_MPPI_UPDATE),
    "cs_rollout_mppi_costs_ex": _row("'the same io and mio, the same outputs, the same rules'; the temperature's outputs "
                                     "belong to cs_rollout_mppi_temperature",
                                     cs_rollout_io=_NO_IO_OUT, cs_rollout_mppi_io=_MPPI_COSTS, cs_rollout_mppi_ext=_EXT_UNUSED),
    "cs_rollout_mppi_update_ex": _row("as cs_rollout_mppi_update",
                                      cs_rollout_io=_NO_IO_OUT, cs_rollout_mppi_io=_MPPI_UPDATE,
                                      cs_rollout_mppi_ext=_EXT_UNUSED),
    "cs_rollout_mppi_temperature": _row(
        "'reads mio->num_samples and mio->costs_dev [P,N] only'; 'writes lam_out_dev [N] (required) and, when not NULL, "
        "ess_out_dev'",
        cs_rollout_mppi_io=dict(input="costs_dev", unused="best_dev actions_out_dev ess_dev cost_min_dev"),
        cs_rollout_mppi_ext=dict(required="lam_out_dev", optional="ess_out_dev")),
    "cs_rollout_mlp_population": _row(
        "returns_dev '(required)'; 'each of the last three may be NULL'; member_returns_dev '[M] float64 or NULL' (a "
        "second kernel, launched only then); io's 'outputs, cotangents and gradients are not used'",
        cs_rollout_io=_NO_IO_OUT,
        cs_rollout_population_io=dict(required="returns_dev",
                                      optional="lengths_dev end_flags_dev end_status_dev member_returns_dev")),
    "cs_es_perturb": _row("table_dev 'perturb: [M,P], required'; grad_dev is cs_es_gradient's",
                          cs_es_io=dict(required="table_dev", unused="grad_dev")),
    "cs_es_gradient": _row("grad_dev 'gradient: [P], required'; 'neither the table nor theta is read'",
                           cs_es_io=dict(required="grad_dev", unused="table_dev")),
    "cs_rollout_actor_critic": _row(
        "every tape '(required)' but means_dev ('or NULL'); values_dev 'required with critic_dev, else must be NULL' "
        "(CONDITIONAL below).  Kernels by the critic's presence, `deterministic` and the configuration; means_dev is a "
        "run-time branch.",
        cs_rollout_ac_io=dict(required="obs_dev actions_dev logp_dev values_dev reward_dev flags_dev live_dev",
                              optional="means_dev")),
    "cs_gae": _row("both outputs required", cs_gae_io=dict(required="advantages_dev returns_dev")),
    "cs_ppo_grad": _row("both outputs required", cs_ppo_grad_io=dict(required="grad_dev stats_dev")),
}

# (entry, member) -> the const pointer whose presence decides: required with it, must_be_null without
CONDITIONAL = {("cs_rollout_actor_critic", "cs_rollout_ac_io.values_dev"): "cs_rollout_ac_io.critic_dev"}


def of_class(entry, cls):
    return [f for f, c in TABLE[entry].fields.items() if c == cls]


# ---------------------------------------------------------------------------------------------------------------------
# the header, parsed the way tests/test_abi_cpu.py parses it
# ---------------------------------------------------------------------------------------------------------------------
def parse_header(text):
    """(structs, functions): structs[name] = [(C type, member)] of every `typedef struct name {...} name;`;
    functions[name] = the io block struct names among the parameters of every function declared from cs_version on, in
    order."""
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    structs = {}
    for name, body in re.findall(r"typedef struct (\w+) \{(.*?)\} \1;", plain, re.S):
        structs[name] = [(t.strip(), m) for t, m in re.findall(r"([\w \*]+?)\b(\w+);", body)]
    rest = plain[plain.index("int cs_version(void);"):]
    functions = {}
    for name, params in re.findall(r"\b(cs_[a-z_]+)\s*\(([^)]*)\)\s*;", rest):
        functions[name] = [m.group(1) for m in re.finditer(r"const (cs_\w+)\*", params)]
    return structs, functions


def output_members(structs, block):
    """the non-const pointer members of a struct"""
    return [m for t, m in structs[block] if "*" in t and not t.startswith("const ")]


def tabled_functions(functions):
    """the declarations the table covers: cs_rollout_*, cs_step_jacobian, cs_mlp_param_grad, cs_es_*, cs_gae, cs_ppo_grad"""
    return sorted(f for f in functions if re.match(r"cs_(rollout_\w+|step_jacobian|mlp_param_grad|es_\w+|gae|ppo_grad)$", f))


# ---------------------------------------------------------------------------------------------------------------------
# the interposer
# ---------------------------------------------------------------------------------------------------------------------
Call = collections.namedtuple("Call", "seen rc message")


def _blocks(entry, args):
    """header struct name -> the ctypes structure behind the byref() arguments of one call"""
    from gym_copter_amd import _lib
    mirror = {getattr(_lib, cls): name for name, cls in STRUCTS.items()}
    found = {}
    for a in args:
        obj = getattr(a, "_obj", None)          # (byref()'s argument)
        if isinstance(obj, C.Structure) and type(obj) in mirror:
            found[mirror[type(obj)]] = obj
    return found


class nulling:
    """The context manager of the module's docstring.  fields: "struct.member" names of `entry`'s row to pass as NULL
    (none: the call is only recorded).  forward_to: the entry point to call instead of the replaced attribute, with the
    NULL blocks dropped (cs_rollout_mlp_vjp, which the wrappers reach through cs_rollout_mlp_vjp_ex with xio = NULL);
    the row is then forward_to's.  Yields the list of Call(seen, rc, message): seen = the pointer value of every classified
    member as the wrapper set it (0 for NULL), rc and cs_last_error() as the real function left them."""

    def __init__(self, lib, entry, fields=(), forward_to=None):
        self.lib, self.entry, self.target = lib, entry, forward_to or entry
        self.row = TABLE[self.target]
        self.fields = tuple(fields)
        for f in self.fields:
            if f not in self.row.fields:
                raise KeyError("%s has no classified member %s" % (self.target, f))
        self.calls = []

    def _forward(self, *args):
        real = self.real if self.target == self.entry else getattr(self.lib, self.target)
        if self.target != self.entry:
            args = tuple(a for i, a in enumerate(args) if a is not None or i == 0 or i == len(args) - 1)
        blocks = _blocks(self.target, args)
        split = lambda f: (blocks.get(f.split(".")[0]), f.split(".")[1])          # noqa: E731
        seen = {}
        for f in self.row.fields:
            b, m = split(f)
            seen[f] = 0 if b is None else (getattr(b, m) or 0)
        saved = []
        for f in self.fields:
            b, m = split(f)
            if b is None:
                raise AssertionError("%s: the call passes no %s block to null %s in" % (self.target, f.split(".")[0], f))
            saved.append((b, m, getattr(b, m)))
        try:
            for b, m, _ in saved:
                setattr(b, m, None)
            rc = real(*args)
        finally:
            for b, m, v in saved:
                setattr(b, m, v)
        err = getattr(self.lib, "cs_last_error", None)
        self.calls.append(Call(seen, rc, err().decode("utf-8", "replace") if err is not None and rc != 0 else ""))
        return rc

    def __enter__(self):
        self.real = getattr(self.lib, self.entry)
        setattr(self.lib, self.entry, self._forward)
        return self.calls

    def __exit__(self, exc_type, exc, tb):
        setattr(self.lib, self.entry, self.real)
        if exc_type is None and not self.calls:
            raise AssertionError("%s was never reached inside the block: nothing was tested" % self.entry)
        return False
