"""Relocalisation frames of a resident sequence (vg_ba_seq_relo_reserve / vg_ba_seq_set_relo / vg_ba_seq_get_relo; csrc/ba_seq.hip
ba_seq_build_kernel), kernel sources under the CPU fiber emulator.  The cases are in tests/seq_relo_case.py; tests/test_seq_relo_gpu.py
runs the same ones on the GPU."""
import pytest

import conftest
import seq_relo_case as R


@pytest.fixture(scope="module")
def two_handles():
    a, b = conftest._simt_handle(), conftest._simt_handle()
    yield a, b
    a.close(); b.close()


def _reference_built():
    from oracle import ref
    return ref.available()


def test_relocalisation_frame_equals_host_bookkeeping(two_handles):
    """Cases 1 and 6 (NumPy part): loop pose within 1e-9 of vg_ba_optimize with the walk's factors, by-products within 1e-12."""
    R.case_host_bookkeeping(*two_handles)


@pytest.mark.parametrize("K,estimate_td", [(12, 0), (11, 1)])
def test_relocalisation_frame_on_the_widest_block(two_handles, K, estimate_td):
    """Case 2: Kp = 13 = BA_MAX_K, and ProjectionTdFactor rows beside the (td-free) relocalisation factors."""
    R.case_host_bookkeeping(*two_handles, K=K, estimate_td=estimate_td)


@pytest.mark.parametrize("kind", ["not_ascending", "all_below", "all_above", "none"])
def test_relocalisation_walk(two_handles, kind):
    """Case 3."""
    R.case_walk(*two_handles, kind)


def test_idle_block_next_to_a_plain_sequence(two_handles):
    """Case 4."""
    R.case_idle(*two_handles, n_steps=2)


def test_relocalisation_by_products_against_the_reference(two_handles):
    """Case 6, against the reference's optimization() (oracle/_ref)."""
    if not _reference_built():
        pytest.skip("oracle/_ref is not built")
    R.case_host_bookkeeping(*two_handles, with_reference=True)


def test_relocalisation_frame_in_imu_mode(two_handles):
    """Case 7: the armed step through vg_ba_seq_step_imu_async."""
    R.case_imu_mode(*two_handles)


def test_refusals_and_lifetime(two_handles):
    """Case 8."""
    R.case_lifetime(*two_handles)
    R.case_no_reservation(*two_handles)
    R.case_overflow(*two_handles)


def test_relocalisation_frames_on_the_fused_factor_kernel(two_handles):
    """Case 5, emulated at the threshold itself: 32 windows."""
    R.case_fused(*two_handles)


def test_cpp_replay_with_a_relocalisation_frame(two_handles, tmp_path):
    """Case 9: `vins_replay seq` with VINS_REPLAY_RELO, linked against the emulated library."""
    import os
    conftest._build_simt()
    R.case_cpp(two_handles[0], os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path)


_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import seq_relo_case as R
import vio_bridge_case as case
A, B = conftest._simt_handle(), conftest._simt_handle()
print("RESULT", R.case_bridge(A, B, case.Data(4, 1, True, plan="PPP")))
"""


def test_relocalisation_frame_through_the_bridge():
    """Case 7, vg_vio_step_async on a small staged frame (windows of K = 4 frames, frames of 376x240, a process of its own like the
    cases of tests/test_vio_bridge.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=root)], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "RESULT" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    out = eval(r.stdout[r.stdout.index("RESULT") + 6:].strip().splitlines()[0])
    (armed0, n0), (armed1, n1), (after, n_req) = out
    assert armed0 == 1 and n0 >= 2 and armed1 == 0 and n1 == 0 and after == 0, out
