"""vg_init_exrot on the MI355X: the case table, bound, split, batch-equals-single, neighbour, refusal, growing-table, stream-limit and
capacity checks of tests/init_exrot_ref.py through the real library.  Reads nothing outside the repository.

MEASURED, MI355X: every decision (branch, RANSAC inlier count / last and winning iteration / bound, front[4], picked, ok, first_ok, status,
used_fallback) equals the reference's on every step of the eight cases, the capacity step and the numeric window; worst value ratio 2.17 x
E64 (huber of a step of 'full64'; bound 4; the emulator: 2.01), the capacity window 1.00; `vins_replay exrot` equals the binding number
for number.  THE WHOLE FILE (14 tests, the chain, the separating-threshold scenes, the replay and cap tests included) takes 3.3 s in a run of the whole GPU
suite (sum of every setup, call and teardown; 0.8 s of it the case table with its 80-bit reference), where tests/test_init_relpose_gpu.py takes
1.9 s: 1.4 s MORE than that file in the same run, and under the 4.5 s that file records for itself run alone.  Alone, with the oracle's and
the library's first loads in it, the first eight checks took 4.4 s.

The chain (at ransac_threshold = 0.3 / 460; tests/init_exrot_ref.chain_window says why): calib_ric 3.3e-5 degrees from the scene's, the scale to
1.8e-5 (bound 1e-3); at the default threshold what it gives is asserted as recorded (6.262 degrees, scale 9.36e-3).  The noisy scenes at 0.3 / 460:
calib_ric 0.24 / 0.20 degrees from the scene's (perturbation bound 0.53 / 0.74)."""
import os

import pytest

import conftest
import init_exrot_ref as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(handle):
    return X.check_cases(handle, 'gpu')


def test_every_case_within_the_bound(table):
    assert set(table) == set(X.CASE_ARGS)


def test_split_run_equals_the_unsplit_one(handle):
    X.check_split(handle)


def test_batch_equals_single_windows(handle):
    X.check_batch_equals_single(handle, (1, 3, 33))


def test_numeric_window_leaves_its_neighbours(handle):
    X.check_numeric_neighbours(handle)


def test_refusals(handle):
    for name in X.REFUSALS:
        X.check_refusal(handle, name)


def test_growing_table():
    h = conftest.new_handle()
    try:
        X.check_growing_table(h)
    finally:
        h.close()


def test_stream_limit(handle):
    X.check_stream_limit(handle, run_limit=True)


def test_capacity_step(handle):
    X.check_capacity(handle, 'gpu')


@pytest.mark.parametrize("name", X.REPLAY_CASES)
def test_cpp_class_one_frame_at_a_time_through_the_replay_tool(handle, tmp_path, name):
    """Estimator::calibrateExtrinsicRotation / InitialEXRotation (host/estimator.cpp, vg_pack_exrot) through `vins_replay exrot`"""
    X.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)


def test_chain_into_sfm_and_alignment(handle):
    X.check_chain(handle)


def test_noisy_scenes_at_the_separating_threshold(handle):
    X.check_separating(handle)


def test_cpp_class_drops_its_oldest_record_at_the_cap(handle, tmp_path):
    X.check_replay_cap(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path)
