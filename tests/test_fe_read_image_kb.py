"""vg_fe_read_image on a stream with a Kannala-Brandt camera against the SAME frame composed from the step-by-step entry points on a second
handle (the construction of tests/fe_read_image_camera_case.py; fe_kb_case.lift64_kb supplies FOCAL * x / z + W / 2 for
vg_fe_reject_with_f): every field bit-identical on the streams normal, lmeds, few and unpublished, for a camera of degree 9 and one of
degree 7, 320 x 240, max_points 160, at most 5 frames."""
import pytest

import fe_camera_case as cc
import fe_kb_case as kb


def test_one_call_frame_with_a_kb_camera_equals_the_step_by_step_calls_on_emulated_kernels():
    assert cc.run_emulated("fe_kb_case", "case.check_read_image(case.run_read_image(H(), H()))") is True


@pytest.mark.gpu
def test_one_call_frame_with_a_kb_camera_equals_the_step_by_step_calls_on_the_gpu(handle):
    import conftest
    other = conftest.new_handle()
    try:
        assert kb.check_read_image(kb.run_read_image(handle, other))
    finally:
        other.close()
