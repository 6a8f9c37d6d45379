"""GPU tests of the relocalisation frames of a resident sequence (vg_ba_seq_relo_reserve / vg_ba_seq_set_relo / vg_ba_seq_get_relo;
csrc/ba_seq.hip ba_seq_build_kernel): the cases of tests/seq_relo_case.py, which tests/test_seq_relo_simt.py runs on the emulated
kernels, at the same small shapes."""
import pytest

import conftest
import seq_relo_case as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two_handles():
    a, b = conftest.new_handle(), conftest.new_handle()
    yield a, b
    a.close(); b.close()


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
    R.case_idle(*two_handles, n_steps=3)


def test_relocalisation_frames_on_the_fused_factor_kernel(two_handles):
    """Case 5: 32 windows, the threshold from which the solve takes the fused factor kernel."""
    R.case_fused(*two_handles)


def test_relocalisation_by_products_against_the_reference(two_handles):
    """Case 6, against the reference's optimization() (oracle/_ref)."""
    from oracle import ref
    if not ref.available():
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


def test_cpp_replay_with_a_relocalisation_frame(two_handles, tmp_path):
    """Case 9: `vins_replay seq` with VINS_REPLAY_RELO on the GPU."""
    import os
    if os.environ.get("VINS_TEST_SIMT") == "1":
        pytest.skip("the emulated variant is tests/test_seq_relo_simt.py")
    R.case_cpp(two_handles[0], os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, timeout=300)
