"""tests/filter_cases.py lists every instantiation of the filter kernels: the product of the distinct tasks and storage
modes CopterVecEnv offers (its aliases name the same kernels) with both settings of the rotor-gyro term."""
import itertools

import filter_cases
import model_variants


def test_the_case_table_is_every_task_mode_and_gyro_setting():
    from gym_copter_amd import vecenv
    got = [(vecenv._TASKS[task], vecenv._STATE_MODES[mode], bool(gyro)) for task, mode, gyro in filter_cases.CASES]
    want = set(itertools.product(set(vecenv._TASKS.values()), set(vecenv._STATE_MODES.values()), (False, True)))
    assert len(got) == len(set(got)), "a case is listed twice"
    assert set(got) == want, sorted(want.symmetric_difference(got))
    assert len({filter_cases.case_id(c) for c in filter_cases.CASES}) == len(filter_cases.CASES)
    # the table's tasks under their canonical names, each with an action width for the tests' problems
    assert {vecenv._TASK_NAMES[vecenv._TASKS[t]] for t in filter_cases.TASKS} == set(filter_cases.TASKS)
    assert set(filter_cases.TASKS) == set(vecenv._TASK_SHAPES)


def test_gyro_on_is_the_gyro_only_variant():
    assert model_variants.env_kwargs("gyro_only") == dict(rotor_gyro=True)
