"""vg_init_relpose on the MI355X: the case table, bound, batch-equals-single, neighbour, refusal, growing-table, capacity and chain checks
of tests/init_relpose_ref.py through the real library.  Reads nothing outside the repository.

MEASURED, MI355X: every decision (n_corres, gate, RANSAC mask / count / last and winning iteration / bound, good[4], winner, inlier_cnt, l,
status, used_fallback) equals the reference's on the 13 cases and on all 15 candidates of the capacity window; worst value ratio over the table 1.00 x E64 (relative_R / relative_T of several cases: the device reproduces
the float64 Jacobi route; bound 4; the emulator: 1.00), the capacity window 0.63 / 0.29; the chain into vg_init_sfm and vg_init_align finds
the scene's scale to 2.5e-5 from l = 0; `vins_replay relpose` equals the binding number for number; the file takes 4.5 s."""
import os

import pytest

import conftest
import init_relpose_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(handle):
    return R.check_cases(handle, 'gpu')


def test_every_case_within_the_bound(table):
    assert set(table) == set(R.CASE_ARGS)


def test_batch_equals_single_windows(handle):
    R.check_batch_equals_single(handle, (1, 3, 33))


def test_none_window_leaves_its_neighbours(handle):
    R.check_none_neighbours(handle)


def test_refusals(handle):
    for name in R.REFUSALS:
        R.check_refusal(handle, name)


def test_growing_table():
    h = conftest.new_handle()
    try:
        R.check_growing_table(h)
    finally:
        h.close()


def test_stream_limit(handle):
    R.check_stream_limit(handle, run_limit=True)


def test_capacity_window(handle):
    R.check_capacity(handle, 'gpu')


def test_chain_into_sfm_and_alignment(handle):
    R.check_chain(handle)


@pytest.mark.parametrize("name", R.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(handle, tmp_path, name):
    """Estimator::relativePose / initialStructure() (host/estimator.cpp, vg_pack_relpose) through `vins_replay relpose`"""
    R.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)
