"""The instantiation matrix of the filter kernels (cs_rollout_ekf, cs_rollout_rts, cs_rollout_pf): every task x every
storage mode (CS_DISPATCH, csrc/dev_launch.h) x the rotor-gyro term off or on (the launchers' c.gyro) -- 36 kernels per
entry point.  tests/test_gpu_filter_matrix.py launches each of them; tests/test_filter_matrix_cpu.py holds this table to
the tasks and modes CopterVecEnv offers, so that one added later fails there until it is listed here."""
import itertools

TASKS = ("lander3d", "hover3d", "lander2d", "hover2d", "lander1d", "hover1d")
MODES = ("float32", "float32_rn", "float64")
GYRO = (False, True)                      # True: model_variants.env_kwargs("gyro_only")
CASES = tuple(itertools.product(TASKS, MODES, GYRO))


def case_id(case):
    task, mode, gyro = case
    return "%s-%s-%s" % (task, mode, "gyro" if gyro else "plain")
