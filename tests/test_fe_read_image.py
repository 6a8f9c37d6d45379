"""vg_fe_read_image (one call per frame) against the step-by-step entry points, and in turns with
vg_fe_read_image_batch(n_streams = 1) on one handle against itself alone: tests/fe_read_image_case.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(seen):
    assert seen["ransac_device"] >= 6 and seen["fb_lmeds"] >= 1 and seen["fb_collinear"] >= 1 and seen["no_ransac"] >= 3, seen
    assert all(0 <= v < 1000 for v in seen["niters"]) and any(v > 0 for v in seen["niters"]), seen      # the bookkeeping cut the iterations as OpenCV's loop does (0: every point an inlier)


_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import fe_read_image_case as case
seen = case.%(fn)s(conftest._simt_handle(), conftest._simt_handle())
print("SEEN", seen)
"""


def _child(fn):
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, fn=fn)], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "SEEN" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return eval(r.stdout[r.stdout.index("SEEN") + 4:].strip().splitlines()[0])


def test_one_call_frame_equals_the_step_by_step_calls_on_emulated_kernels():
    _check(_child("run"))


@pytest.mark.gpu
def test_one_call_frame_equals_the_step_by_step_calls_on_the_gpu(handle):
    import conftest
    import fe_read_image_case as case
    other = conftest.new_handle()
    try:
        _check(case.run(handle, other, W=752, H=480, n_frames=9))
    finally:
        other.close()


# (run_alternating asserts its own preconditions -- the device estimate ran under either entry point, an unpublished frame had points --
#  and does not come back without them)
def test_single_and_batch_of_one_in_turns_equal_the_single_call_alone_on_emulated_kernels():
    assert _child("run_alternating")["unpublished_tracked"] >= 1


@pytest.mark.gpu
def test_single_and_batch_of_one_in_turns_equal_the_single_call_alone_on_the_gpu(handle):
    import conftest
    import fe_read_image_case as case
    other = conftest.new_handle()
    try:
        assert case.run_alternating(handle, other)["unpublished_tracked"] >= 1
    finally:
        other.close()
