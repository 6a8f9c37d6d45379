"""vg_vio_begin / _step_async / _get_frame / _end -- the front end's message goes to the resident sequences on the device, one call per
frame for N camera + IMU streams -- held exactly (bit patterns) to the path a caller had before: vg_fe_tracks_step, then
vg_ba_seq_step_imu_async fed from the pinned message, on a second handle from the same seeded state (tests/vio_bridge_case.py)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import vio_bridge_case as case
A, B = conftest._simt_handle(), conftest._simt_handle()
print("RESULT", %(call)s)
"""

# under the emulator: windows of K = 4 frames behind one frame of front-end warm-up, frames of 376x240
_EMU_DATA = "case.Data(4, 1, True)"


def _child(call):
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, call=call)], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "RESULT" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return eval(r.stdout[r.stdout.index("RESULT") + 6:].strip().splitlines()[0])


def test_bridge_kernel_has_no_private_segment_and_no_spills():
    """the code object's metadata of the built library (no GPU needed)"""
    import test_codegen_guard as G
    if not os.path.exists(G.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    md = G._kernel_metadata()
    assert "ba_seq_bridge_kernel" in md, "kernel missing from the gfx950 code object"
    k = md["ba_seq_bridge_kernel"]
    assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k


def test_header_and_library_agree_on_the_new_exports(pkg):
    import ctypes
    lib = ctypes.CDLL(pkg.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vinsgpu.h")).read()
    for name in ("vg_vio_begin", "vg_vio_step_async", "vg_vio_get_frame", "vg_vio_end"):
        assert ("int %s(vg_handle* h" % name) in header and hasattr(lib, name), name


# ---- the emulated kernels
def test_staged_frame_equals_the_message_on_emulated_kernels():
    """empty messages beside full ones, 64 and 65 rows, more than 256 rows, three streams with different counts in one call"""
    import vio_bridge_case as case
    case.check_staged(_child("case.run_staged(A, B)"))


def test_bridged_run_equals_the_hand_fed_run_on_emulated_kernels():
    import vio_bridge_case as case
    case.check_pair(_child("case.run_pair(A, B, %s, True, 'bridged')" % _EMU_DATA), True)


def test_counts_only_mode_on_emulated_kernels():
    import vio_bridge_case as case
    case.check_pair(_child("case.run_pair(A, B, %s, False, 'bridged')" % _EMU_DATA), False)


def test_interleaving_with_the_two_old_calls_on_emulated_kernels():
    import vio_bridge_case as case
    case.check_pair(_child("case.run_pair(A, B, %s, True, 'interleaved')" % _EMU_DATA), True)


def test_bridge_begun_again_after_a_larger_max_samples_on_emulated_kernels():
    """vg_vio_begin at max_samples 16, vg_ba_seq_imu_begin at 64, vg_vio_begin, a step with 33 rows; odd sample counts throughout"""
    assert _child("case.run_regrow(A, B, %s)" % _EMU_DATA) == dict(samples=[11, 33, 11])


def test_refusals_on_emulated_kernels():
    import vio_bridge_case as case
    assert _child("case.run_refusals(A, %s)" % _EMU_DATA) == case.REFUSALS


# ---- the device: K = 11, 752x480, 150 points
@pytest.fixture(scope="module")
def gpu_data():
    import vio_bridge_case as case
    return case.Data(11, 0, False)


@pytest.fixture(scope="module")
def second_handle():
    import conftest
    h = conftest.new_handle()
    yield h
    h.close()


@pytest.mark.gpu
def test_staged_frame_equals_the_message_on_the_gpu(handle, second_handle):
    import vio_bridge_case as case
    seen = case.run_staged(handle, second_handle)
    print("staged", seen)
    case.check_staged(seen)


@pytest.mark.gpu
def test_bridged_run_equals_the_hand_fed_run_on_the_gpu(handle, second_handle, gpu_data):
    import vio_bridge_case as case
    seen = case.run_pair(handle, second_handle, gpu_data, True, "bridged")
    print("bridged", seen)
    case.check_pair(seen, True)


@pytest.mark.gpu
def test_counts_only_mode_on_the_gpu(handle, second_handle, gpu_data):
    import vio_bridge_case as case
    seen = case.run_pair(handle, second_handle, gpu_data, False, "bridged")
    print("counts only", seen)
    case.check_pair(seen, False)


@pytest.mark.gpu
def test_interleaving_with_the_two_old_calls_on_the_gpu(handle, second_handle, gpu_data):
    import vio_bridge_case as case
    seen = case.run_pair(handle, second_handle, gpu_data, True, "interleaved")
    print("interleaved", seen)
    case.check_pair(seen, True)


@pytest.mark.gpu
def test_bridge_begun_again_after_a_larger_max_samples_on_the_gpu(handle, second_handle, gpu_data):
    import vio_bridge_case as case
    assert case.run_regrow(handle, second_handle, gpu_data) == dict(samples=[11, 33, 11])


@pytest.mark.gpu
def test_refusals_on_the_gpu(handle, gpu_data):
    import vio_bridge_case as case
    assert case.run_refusals(handle, gpu_data) == case.REFUSALS
