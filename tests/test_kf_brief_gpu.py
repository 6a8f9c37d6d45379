"""vg_kf_* on the MI355X: the check bodies of tests/kf_brief_ref.py (frames against the NumPy reference, blur border, window-point counts,
FAST cases, the keypoint cap, planted and rendered matches, batch and state, refusals) through the real library.  Every comparison is
for equality.  Reads nothing outside the repository."""
import os

import pytest

import conftest
import kf_brief_ref as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("size,cam", [((67, 41), "pinhole"), ((67, 41), "mei"), ((100, 70), "kb")])
def test_frames_against_the_reference(handle, size, cam):
    K.check_frame(handle, size, cam)


def test_full_size_frame(handle):
    """752 x 480: the row-major compaction across 5640 segments"""
    K.check_frame(handle, (752, 480), "pinhole", n_window=150)


def test_blur_border(handle):
    K.check_blur_border(handle)


def test_patterns_of_a_wider_reach(handle):
    K.check_wide_pattern(handle)


def test_window_point_counts(handle):
    K.check_window_counts(handle)


def test_fast_cases(handle):
    K.check_fast_cases(handle)


def test_keypoint_cap(handle):
    K.check_cap(handle)


def test_match_on_planted_records(handle):
    K.check_planted(handle)


def test_match_on_rendered_frames(handle):
    assert K.check_rendered(handle) == K.N_RENDERED


def test_batch_and_state(handle):
    K.check_batch_and_state(handle)


def test_refusals(handle):
    bare = conftest.new_handle()
    try:
        for name in K.REFUSALS:
            K.check_refusal(handle, name, bare)
    finally:
        bare.close()


def test_cpp_class_through_the_replay_tool(handle, tmp_path):
    """class KeyFrame, BriefExtractor and vg_pack_kf (host/keyframe.h, host/vg_pack.h) through `vins_replay kf`"""
    K.check_replay(os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path)
