"""Streams of different camera models in ONE vg_fe_read_image_batch call: stream 0 without a camera (the pinhole of intr), streams 1-3
with the MEI cameras A, B and D of tests/fe_camera_case.py; every output of every stream bit-identical to vg_fe_read_image on a
single-stream handle with the same camera (fe_camera_case.check_batch)."""
import pytest

import fe_camera_case as case


def test_batched_call_with_mixed_camera_models_equals_the_single_calls_on_emulated_kernels():
    assert case.run_emulated("fe_camera_case", "case.check_batch(H(), H())") is True


@pytest.mark.gpu
def test_batched_call_with_mixed_camera_models_equals_the_single_calls_on_the_gpu(handle):
    import conftest
    other = conftest.new_handle()
    try:
        assert case.check_batch(handle, other, W=752, H=480, scale=2.35)
    finally:
        other.close()
