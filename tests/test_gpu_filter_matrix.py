"""Every instantiation of the three filter kernels (tests/filter_cases.py: six tasks x three storage modes x the
rotor-gyro term off or on, 36 kernels per entry point), each launched once and held to the step-by-step checkers of
tests/test_gpu_rollout_ekf.py (_check_steps), tests/test_gpu_rollout_rts.py (_check_rows) and
tests/test_gpu_rollout_pf.py (_check_steps), at their bars: 100 x the float64 reference's distance from its longdouble
twin, floored at 1e-12 scaled.  In the float32 modes the predicted mean and the prior particles are held to rollout_states
within 2^-23 max(1, |value|) (rollout_states rounds its stored words once, the filters' values are not rounded); in
float64 bit for bit.

EKF and RTS: 72 lanes (one whole wavefront and 8 lanes; nine lanes per group of test_gpu_rollout_ekf._points), K = 10,
M = 6 dense measurements; rollout_ekf(tape=True), its check, rollout_rts on those tapes, its check.  PF: the problem of
pf_ref.test_problem (N = 5, K = 12) at P = 64 with the particle env in the same mode and model.

The checkers compare the device with the device; _first_prior_against_the_oracle adds, per EKF case, one step of the
float64 CPU oracle, which tells a wrong action fan-out from the right one.

Measured on an MI355X, the worst ratio to the bar over the 36 cases (every case prints its own; each case runs in
under 0.2 s):
  EKF  x 0.042 (lander1d float32_rn), P_tape and var 0.00043, nis 0.120, loglik 0.0093; x_pred against rollout_states
       0.49 of 2^-23 scaled in float32_rn (half a unit of the float32 rounding) and 0.015 in float32 (5 more bits); the
       first x_pred against the oracle 0.0058 of its bar
  RTS  x_s 0.00065, P_s and var_s 0.00025
  PF   lw 0.050, x 0.0010, var 0.00033, P 0.00006, loglik 0.0071

Mutants this file fails for (an uncommitted build of the library): (a.y, a.x, a.x, a.y) in the A == 2 branch of
load_action_at fails the twelve lander2d and hover2d EKF cases, at the oracle comparison (the lander3d cases pass)."""
import zlib

import numpy as np
import pytest

import model_variants
import test_gpu_rollout_ekf as E
import test_gpu_rollout_pf as F
import test_gpu_rollout_rts as R
from filter_cases import CASES, case_id
from gpu_util import have_gpu, to_np

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

N, K, M = 72, 10, 6
OVERALL = {"ekf": {}, "rts": {}, "pf": {}}
FLYING = ("hover", "clip", "clip_hi", "soft_mid", "hard_mid")


def _overall(which, worst):
    o = OVERALL[which]
    for key, v in worst.items():
        o[key] = max(o.get(key, 0.0), v)
    print("%s, the worst over the cases so far: " % which + " ".join("%s %.5f" % kv for kv in o.items()))


def _model_kwargs(gyro):
    return model_variants.env_kwargs("gyro_only") if gyro else {}


def _first_prior_against_the_oracle(name, task, mode, p, filt):
    """The checkers compare the filters with rollout_states and step_jacobian of the same device, which read an action
    row through the same fan-out (load_action_at, csrc/dev_task.h) or one beside it: a wrong fan-out would pass them.  So
    the first prior mean -- one step from the given start, before any update -- is held to the float64 CPU oracle's step.
    The bar: float64 storage, the 1e-13 scaled of one step against the oracle (tests/test_gpu_numerics.py).  float32
    storage, 3 x 2^-23 max(1, |value|): x_pred is within 2^-23 of rollout_states' stored word (_check_steps), that word
    within one unit of its last place, 2^-23 |value|, of the oracle's rounded word (test_gpu_wide_attitudes.py, 1.), and
    the oracle's rounding is 2^-24 |value|.  For the 2-D tasks the oracle's step under the swapped row (b, a) is asserted
    to lie 1 000 bars away, so that the comparison does tell the two apart."""
    from rollout_fd import oracle_rollout
    x0, st0 = to_np(p["x0"]).astype(np.float64), to_np(p["st0"])
    a = to_np(p["acts"][:1]).astype(np.float64)
    want = oracle_rollout(task, x0, st0, a)[0][0]
    bar = 1e-13 if mode == "float64" else 3 * 2.0 ** -23
    err = float(np.max(np.abs(to_np(filt.x_pred[0]) - want) / np.maximum(1.0, np.abs(want))))
    print("%s: the first prior mean against the oracle %.2e (%.3f of the bar)" % (name, err, err / bar))
    assert err <= bar, (name, err, bar)
    if a.shape[2] == 2:
        swapped = oracle_rollout(task, x0, st0, a[:, :, ::-1])[0][0]
        apart = float(np.max(np.abs(swapped - want) / np.maximum(1.0, np.abs(want))))
        assert apart >= 1e3 * bar, (name, apart, bar)
    return err / bar


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_ekf_and_rts_in_every_instantiation(case):
    from gym_copter_amd import _lib
    task, mode, gyro = case
    name = "matrix " + case_id(case)
    rng = np.random.default_rng(zlib.crc32(repr(("ekf", task, mode, gyro)).encode()))
    env = E._env(task, N, mode, seed=3, **_model_kwargs(gyro))
    ref = E._env(task, N, mode, seed=3) if gyro else None
    try:
        assert bool(env.config.rotor_gyro) == gyro
        env.reset()
        p = E._problem(env, task, rng, M=M, steps=K)
        filt = E._clone(E._run(env, p, tape=True))
        bits, _ = E._check_steps(name, env, p, filt, exact_pred=mode == "float64")
        worst = dict(E.WORST[name])
        if not gyro or E.TASK_A[task] < 4:
            # (the oracle has no rotor-gyro term on the live thrust law, model_variants.oracle_model; for the 2-D and 1-D
            # tasks the term is an exact zero, see below, and the oracle's step is the gyro kernel's too)
            worst["first x_pred / oracle"] = _first_prior_against_the_oracle(name, task, mode, p, filt)
        _overall("ekf", worst)
        # every branch of the step in every case.  The physics and its status rules (plan_call, csrc/dev_physics.h) are
        # the same for the six tasks -- a task chooses the action fan-out (load_action_at, csrc/dev_task.h) and the
        # judging, which the filters do not run -- so no task makes one of the five impossible.
        for nm in ("INTEGRATED", "LANDED", "CONTACT", "CRASHED", "CLIPPED"):
            assert ((bits & getattr(_lib, "JAC_" + nm)) != 0).any(), (name, nm)
        assert not (bits & _lib.JAC_RESET).any()
        # ... and a touchdown inside the horizon: a lane that starts above the ground meets it after the first step
        mid = np.isin(p["grp"], ("soft_mid", "hard_mid"))
        assert mid.sum() == N // 4 and ((bits[1:, mid] & _lib.JAC_CONTACT) != 0).any(), name
        if gyro:
            ref.reset()
            mine, other = to_np(filt.x_pred), to_np(E._run(ref, p).x_pred)
            flies = np.isin(p["grp"], FLYING)
            assert flies.sum() >= N // 3
            if E.TASK_A[task] == 4:         # the term changes the prior mean of every lane that flies
                same = np.all(mine.view(np.uint64) == other.view(np.uint64), axis=(0, 2))
                assert not np.any(same & flies), np.flatnonzero(same & flies)[:8]
            else:
                # The 2-D and 1-D tasks never turn the rotors' net angular momentum on: their fan-outs (a, b, b, a) and
                # (a, a, a, a) make Omega = (m0 + m1) - (m2 + m3) an exact zero (torque_model, csrc/dev_physics.h), so
                # the gyro instantiation computes the values of the plain one (a zero's sign is free).
                assert np.array_equal(mine, other), name
        res = E._clone(R._rts(env, p, filt))
        R._check_rows(name, env, p, filt, res)
        _overall("rts", R.WORST[name])
    finally:
        env.close()
        if ref is not None:
            ref.close()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pf_in_every_instantiation(case):
    task, mode, gyro = case
    name = "matrix " + case_id(case)
    P = 64
    rng = np.random.default_rng(zlib.crc32(repr(("pf", task, mode, gyro)).encode()))
    env = F._env(task, F.N, mode, **_model_kwargs(gyro))
    penv = F._particle_env(task, P, 1, variant="gyro_only" if gyro else None, mode=mode)
    try:
        assert bool(env.config.rotor_gyro) == gyro and bool(penv.config.rotor_gyro) == gyro
        env.reset()
        p = F._problem(env, task, rng)
        res = F._clone(F._run(env, p, P))
        F._check_steps(name, env, penv, p, res, P, exact=mode == "float64")
        _overall("pf", F.WORST[name])
    finally:
        env.close()
        penv.close()
