"""vg_fe_tracks_begin / _step / _get / _set -- the track lists of every stream resident on the device, a frame returning ids, counts,
positions, lifted points, velocities and the estimator's message -- held to vg_fe_read_image_batch plus FeatureTracker's bookkeeping
restated in NumPy, and to the reference's own class; bit by bit (tests/fe_tracks_case.py)."""
import os
import subprocess
import sys
import tempfile

import pytest

from oracle import ref_fe as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, tempfile
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import fe_tracks_case as case
print("RESULT", case.%(call)s)
"""

_REFUSALS = ["step without begin", "list without a previous frame", "wrong struct_size", "n_streams != n_cams", "mixed equalize",
             "mixed min_dist among publishing streams", "frames for some streams only", "max_cnt > max_points", "duplicate id", "n_id too small",
             "negative id", "callback failure"]

needs_ref = pytest.mark.skipif(not RF.available("ref"), reason="oracle/_ref front-end libraries are not built")


def _child(call):
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, call=call)], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "RESULT" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return eval(r.stdout[r.stdout.index("RESULT") + 6:].strip().splitlines()[0])


def _check_seven(seen):
    assert seen["nonzero_velocities"] >= 20 and seen["empty_messages"] >= 1 and seen["short_messages"] >= 1, seen


def _check_long(seen):
    assert len(seen["longest"]) == 4 and min(seen["longest"]) > 256 and seen["edge"] == [64, 65], seen


def test_commit_kernel_has_no_private_segment_and_no_spills():
    """the code object's metadata of the built library (no GPU needed): one workgroup per stream pays off only while it stays in registers"""
    import test_codegen_guard as G
    if not os.path.exists(G.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    md = G._kernel_metadata()
    assert "fe_tk_commit_kernel" in md, "kernel missing from the gfx950 code object"
    k = md["fe_tk_commit_kernel"]
    assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
    assert int(k["group_segment_fixed_size"]) <= 64 * 1024, k


# ---- the emulated kernels
def test_seven_resident_streams_equal_the_batch_call_plus_bookkeeping_on_emulated_kernels():
    """seven streams of different kinds at 320x240 over five frames: every field of every vg_fe_tracks_out"""
    _check_seven(_child("run_seven(conftest._simt_handle())"))


def test_long_lists_and_the_wavefront_edge_on_emulated_kernels():
    """lists of 257-300 entries (more than one pass of the compaction, a sort over 512 keys), one stream and three; lists of 64 and 65"""
    _check_long(_child("run_long(conftest._simt_handle())"))


@needs_ref
def test_resident_lists_equal_the_reference_class_on_emulated_kernels():
    """the reference's FeatureTracker::readImage + updateID at MAX_CNT 16: ids, track_cnt, cur_pts, cur_un_pts, pts_velocity, n_id"""
    seen = _child("run_reference(conftest._simt_handle(), tempfile.gettempdir())")
    assert seen["nonzero_velocities"] >= 20, seen


def test_export_reseed_and_refusals_on_emulated_kernels():
    assert _child("run_export_and_refusals(conftest._simt_handle(), conftest._simt_handle())") == _REFUSALS


# ---- the device
@pytest.mark.gpu
def test_seven_resident_streams_equal_the_batch_call_plus_bookkeeping_on_the_gpu(handle):
    import fe_tracks_case as case
    seen = case.run_seven(handle, W=752, H=480, n_frames=8)
    print("seven", seen)
    _check_seven(seen)


@pytest.mark.gpu
def test_long_lists_and_the_wavefront_edge_on_the_gpu(handle):
    import fe_tracks_case as case
    seen = case.run_long(handle)
    print("long", seen)
    _check_long(seen)


@needs_ref
@pytest.mark.gpu
def test_resident_lists_equal_the_reference_class_on_the_gpu(handle):
    import fe_tracks_case as case
    seen = case.run_reference(handle, tempfile.gettempdir())
    print("reference", seen)
    assert seen["nonzero_velocities"] >= 20, seen


@pytest.mark.gpu
def test_export_reseed_and_refusals_on_the_gpu(handle):
    import conftest
    import fe_tracks_case as case
    other = conftest.new_handle()
    try:
        assert case.run_export_and_refusals(handle, other) == _REFUSALS
    finally:
        other.close()
