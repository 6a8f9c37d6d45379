"""vg_init_align on the MI355X: the case table, bound, batch-equals-single and record checks of tests/init_align_ref.py through the real
library, and the stand-alone class through `vins_replay align`.  Reads nothing outside the repository.

MEASURED, MI355X: worst ratio over the table 0.52 x kappa 2^-53 (g_c0 of F5; bound 4; the emulator: 0.98, the float64 NumPy routes:
0.84); delta_bg against max|ref| instead of its own scale 4 .. 100; the records equal vg_imu_preintegrate's bit for bit (they come
from the same kernel); the file takes 2.3 s."""
import os

import pytest

import conftest
import init_align_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(handle):
    return A.check_cases(handle, 'gpu')


def test_every_case_within_the_bound(table):
    assert set(table) == set(A.CASE_ARGS)


def test_records_are_the_preintegration_kernels(handle, table):
    A.check_records(handle, table)


def test_batch_equals_single_windows(handle):
    A.check_batch_equals_single(handle, (1, 3, 70))


def test_numeric_window_leaves_its_neighbours(handle):
    A.check_numeric_neighbours(handle)


def test_refusals(handle):
    for name in ('in_struct_size', 'F_33', 'null_samples', 'interval_empty', 'key_is_F', 'sample_nan'):
        A.check_refusal(handle, name)


@pytest.mark.parametrize("name", A.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(handle, tmp_path, name):
    A.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)
