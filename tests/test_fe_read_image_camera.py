"""vg_fe_read_image with a MEI camera set on the stream against the step-by-step entry points: tests/fe_read_image_camera_case.py."""
import pytest

import fe_camera_case as cc


def test_one_call_frame_with_a_mei_camera_equals_the_step_by_step_calls_on_emulated_kernels():
    assert cc.run_emulated("fe_read_image_camera_case", "case.check(case.run(H(), H()))") is True


@pytest.mark.gpu
def test_one_call_frame_with_a_mei_camera_equals_the_step_by_step_calls_on_the_gpu(handle):
    import conftest
    import fe_read_image_camera_case as case
    other = conftest.new_handle()
    try:
        assert case.check(case.run(handle, other, W=752, H=480, n_frames=7, scale=2.35))
    finally:
        other.close()
