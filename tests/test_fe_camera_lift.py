"""vg_fe_lift point by point against the reference's CataCamera::liftProjective (oracle/_ref/libvins_ref_fe.so, camera_model/src/
camera_models/CataCamera.cc compiled unchanged): identical float bit patterns of (float)(x / z), (float)(y / z) for the cameras A, B, C, D
of tests/fe_camera_case.py on every 8th pixel of 320 x 240 and 512 random sub-pixel positions; camera E (xi = 0.0) against
vg_fe_undistort."""
import pytest

import fe_camera_case as case
from oracle import ref_fe as RF

needs_ref = pytest.mark.skipif(not RF.available("ref"), reason="oracle/_ref front-end libraries are not built")


@needs_ref
def test_lift_equals_the_reference_cata_camera_on_emulated_kernels(tmp_path):
    assert case.run_emulated("fe_camera_case", "case.check_lift_against_reference(H(), %r)" % str(tmp_path)) > 1700


def test_lift_with_xi_zero_equals_undistort_on_emulated_kernels():
    assert case.run_emulated("fe_camera_case", "case.check_lift_xi_zero_is_the_pinhole(H())") > 1700


@needs_ref
@pytest.mark.gpu
def test_lift_equals_the_reference_cata_camera_on_the_gpu(handle, tmp_path):
    assert case.check_lift_against_reference(handle, str(tmp_path)) > 1700


@pytest.mark.gpu
def test_lift_with_xi_zero_equals_undistort_on_the_gpu(handle):
    assert case.check_lift_xi_zero_is_the_pinhole(handle) > 1700
