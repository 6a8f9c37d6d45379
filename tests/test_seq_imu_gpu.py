"""GPU tests of the device-resident sequences that take raw IMU samples (vg_ba_seq_imu_begin / vg_ba_seq_step_imu_async:
Estimator::processIMU and the IMU part of slideWindow() on the device, csrc/ba_seq.hip + csrc/imu_step.h).  The drivers and what
they check are tests/seq_imu_model.py; small windows (K = 11, L = 70, 1-3 windows, 3-5 steps): the kernels under test do not see the
size of the problem."""
import os

import pytest

import conftest
import seq_imu_model as I
import seq_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two_handles():
    a, b = conftest.new_handle(), conftest.new_handle()
    yield a, b
    a.close(); b.close()


def _two_new_in_a_row(flags):
    return any(flags[s][w] == M.NEW and flags[s + 1][w] == M.NEW for s in range(len(flags) - 1) for w in range(len(flags[0])))


def test_record_and_guess_parity_over_both_slides(two_handles):
    """(seeds chosen under the emulator, tests/test_seq_imu_simt.py: window 1 drops three non-keyframes in a row)"""
    flags, worst = I.run_parity(two_handles[0], seeds=[22, 23], K=11, L=70, n_steps=4, min_parallax=0.25)
    flat = [f for fr in flags for f in fr]
    assert M.NEW in flat and M.OLD in flat and _two_new_in_a_row(flags)
    assert 'merged_record' in worst and 'record' in worst and 'guess' in worst


def test_ragged_sample_counts_in_one_call(two_handles):
    """1, 7 and max_samples samples in one call.  The covariance of a ONE-sample interval is singular in exact arithmetic (the
    position rows of V are dt / 2 times its velocity rows, integration_base.h:113-124), so whether the solve that uses it stays finite
    is a matter of rounding: that window may report VG_ERR_NUMERIC; its record and guess are held to the bound all the same."""
    I.run_parity(two_handles[0], seeds=[22, 23, 24], n_steps=1, counts=[1, 7, 20], max_samples=20, allow_numeric=(0,))
    flags, _ = I.run_parity(two_handles[0], seeds=[22, 23, 24], n_steps=3, counts=[2, 7, 20], max_samples=20)      # ragged merges too
    assert M.NEW in [f for fr in flags for f in fr]


def test_the_largest_sample_list(two_handles):
    """max_samples = 512, one window, 512 samples of 0.2 ms per frame"""
    I.run_parity(two_handles[0], seeds=[23], n_steps=2, counts=[512], dt=0.0002, max_samples=512)


@pytest.mark.parametrize("K,seed", [(4, 22), (12, 22)])
def test_other_window_sizes(two_handles, K, seed):
    flags, _ = I.run_parity(two_handles[0], seeds=[seed], K=K, L=70, n_steps=4, min_parallax=0.25)
    flat = [f for fr in flags for f in fr]
    assert M.NEW in flat and M.OLD in flat


def test_equivalence_with_the_host_fed_mode(two_handles):
    flags, worst = I.run_equivalence(two_handles[0], two_handles[1], seeds=[22, 23], n_steps=5)
    flat = [f for fr in flags for f in fr]
    assert M.NEW in flat and M.OLD in flat


def test_against_the_reference_loop(two_handles):
    from oracle import ref as R
    if not R.available():
        pytest.skip("oracle/_ref is not built")
    flags, worst, flips = I.run_against_reference(two_handles[0], 0.1, n_frames=24)
    assert 1 in flags and 0 in flags


def test_an_interval_longer_than_ten_seconds(two_handles):
    I.run_long_interval(two_handles[0])


def test_import_in_imu_mode(two_handles):
    I.run_import(two_handles[0], two_handles[1], seeds=[22, 23])


def test_refusals(two_handles):
    I.run_refusals(two_handles[0])


def test_kernel_timing_tap(two_handles):
    I.run_timing_tap(two_handles[0], positive=True)


def test_cpp_class_with_the_imu_on_the_device(tmp_path):
    if os.environ.get("VINS_TEST_SIMT") == "1":
        pytest.skip("the emulated variant is tests/test_seq_imu_simt.py")
    worst = I.run_cpp(os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, timeout=300)
    print("C++ ResidentEstimators, IMU on the device vs on the host: worst state difference", worst)
