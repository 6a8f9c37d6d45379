"""vg_fe_lift with a Kannala-Brandt camera (model 3) point by point against the definition restated in NumPy double
(fe_kb_case.lift64_kb, held to the reference by tests/test_fe_kb_definition.py): identical float bit patterns for the five cameras of
the table and a camera without distortion, on every 8th pixel of each camera's frame, 512 random sub-pixel positions, the principal point
(the r < 1e-10 branch on the camera whose u0, v0 are floats), the four corners and a pixel with theta > pi / 2 on the tum camera (the
quadrant swap); CameraModel::liftProjective of the host class gives the same doubles.  The refusals: a non-finite parameter, a zero
p[0] / p[1], the models 2 and 4."""
import pytest

import fe_camera_case as cc
import fe_kb_case as kb


def test_lift_equals_the_definition_on_emulated_kernels():
    assert cc.run_emulated("fe_kb_case", "case.check_lift(H())") > 20000


def test_refusals_on_emulated_kernels():
    assert cc.run_emulated("fe_kb_case", "case.check_refusals(H())") is True


@pytest.mark.gpu
def test_lift_equals_the_definition_on_the_gpu(handle):
    assert kb.check_lift(handle) > 20000


@pytest.mark.gpu
def test_refusals_on_the_gpu(handle):
    assert kb.check_refusals(handle) is True
