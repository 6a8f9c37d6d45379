"""Kannala-Brandt streams among others in ONE call.  vg_fe_read_image_batch on a handle with four streams -- no camera, the MEI camera A,
KB of degree 9, KB of degree 3 -- against every stream alone (fe_camera_case.same_frame, bit-identical, published and unpublished steps
alternating); vg_fe_tracks_step on a handle with the streams (pinhole, KB) for four frames against vg_fe_read_image_batch on a second
handle with the same cameras that is fed the lists the steps return: counts and un_xy bit-identical, the KB stream's velocities non-zero
from the third frame on.  320 x 240, max_points 160."""
import pytest

import fe_camera_case as cc
import fe_kb_case as kb


def test_batched_call_with_kb_streams_equals_the_single_calls_on_emulated_kernels():
    assert cc.run_emulated("fe_kb_case", "case.check_batch(H(), H())") is True


def test_resident_track_lists_with_a_kb_stream_on_emulated_kernels():
    assert cc.run_emulated("fe_kb_case", "case.check_tracks(H(), H())") >= 20


@pytest.mark.gpu
def test_batched_call_with_kb_streams_equals_the_single_calls_on_the_gpu(handle):
    import conftest
    other = conftest.new_handle()
    try:
        assert kb.check_batch(handle, other)
    finally:
        other.close()


@pytest.mark.gpu
def test_resident_track_lists_with_a_kb_stream_on_the_gpu(handle):
    import conftest
    other = conftest.new_handle()
    try:
        assert kb.check_tracks(handle, other) >= 20
    finally:
        other.close()
