"""vg_init_sfm on the MI355X: the case table, bound, batch-equals-single, neighbour, refusal and chain checks of tests/init_sfm_ref.py
through the real library.  Reads nothing outside the repository.

MEASURED, MI355X: every decision equals the 80-bit route's; worst value ratio over the table 1.50 x E64 (position of F5_scaled; bound 4; the
emulator: 1.98); the capacity window (F = 16, 1024 features, the whole LDS of a CU) stays within 0.61 x the E64 floor of a float64 route;
the chain into vg_init_align finds the scene's scale to 2.4e-5; `vins_replay sfm` equals the binding number for number; the file takes
3.9 s."""
import os

import pytest

import conftest
import init_sfm_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(handle):
    return S.check_cases(handle, 'gpu')


def test_every_case_within_the_bound(table):
    assert set(table) == set(S.CASE_ARGS)


def test_batch_equals_single_windows(handle):
    S.check_batch_equals_single(handle, (1, 3, 33))


def test_numeric_window_leaves_its_neighbours(handle):
    S.check_numeric_neighbours(handle)


def test_refusals(handle):
    for name in S.REFUSALS:
        S.check_refusal(handle, name)


@pytest.mark.parametrize("name", S.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(handle, tmp_path, name):
    """Estimator::initialStructure (host/estimator.cpp, vg_pack_sfm) through `vins_replay sfm`"""
    S.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)


def test_capacity_window(handle):
    S.check_capacity(handle, 'gpu')


def test_chain_into_the_alignment(handle):
    S.check_chain(handle)
