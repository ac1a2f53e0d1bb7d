"""Every instantiation of the control-limited iLQR kernels (cs_ilqr_box_backward: six tasks x three storage modes x the
rotor-gyro term off or on, 36 kernels; cs_ilqr_box_forward: six tasks x three storage modes, 18 kernels;
tests/filter_cases.py), each launched once on 72 lanes (one whole wavefront and a partial one) for K = 10 and held to
what tests/test_gpu_ilqr_box.py holds the main cases to: the backward against tests/ilqr_box_ref.py on the chained
step_jacobian blocks with its exact statements, the forward bit for bit.  The `mars_gyro` and `vehicles` models of
tests/model_variants.py run the GYRO = true kernels under the lift law and the per-env coefficient load."""
import pytest

import test_gpu_ilqr_box as T
from filter_cases import CASES, MODES, TASKS, case_id
from gpu_util import have_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs a HIP device")]

VARIANT_CASES = [("lander3d", "float64", "mars_gyro"), ("hover3d", "float32", "mars_gyro"),
                 ("lander3d", "float32", "vehicles"), ("lander2d", "float64", "vehicles"),
                 ("hover3d", "float64", "vehicles_mars_gyro")]
FORWARD_VARIANTS = (None, "mars_gyro", "vehicles")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_backward_instantiation(case):
    task, mode, gyro = case
    T.gains_against_the_chain(task, mode, 1, 0.1, "gyro_only" if gyro else None, n=72, K=10, seed=7)


@pytest.mark.parametrize("task,mode,variant", VARIANT_CASES)
def test_backward_under_model_variants(task, mode, variant):
    T.gains_against_the_chain(task, mode, 1, 0.0, variant, n=72, K=10, seed=9)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("task", TASKS)
def test_forward_instantiation(task, mode):
    variant = FORWARD_VARIANTS[(TASKS.index(task) + MODES.index(mode)) % 3] if task in ("lander3d", "hover3d") else None
    T.forward_is_exact(task, mode, 1, variant, n=72, K=10)
