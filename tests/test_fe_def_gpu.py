"""The front end against its float64 DEFINITIONS (tests/fe_def_ref.py) on the MI355X: the check bodies of tests/test_fe_def_simt.py with the
product library.  256 x 160 frames at most, at most 64 tracks per LK call, 300 points for the gate table; nothing outside the repository
is read."""
import pytest

import fe_def_ref as D

pytestmark = pytest.mark.gpu


def test_pyramid_is_the_rounded_exact_filter_of_the_level_below(handle):
    D.check_pyramid(handle, 'gpu')


def test_min_eigenvalue_map_in_its_own_scale(handle):
    D.check_mineig(handle, 'gpu')


def test_corner_lists_have_the_stated_properties(handle):
    D.check_corners(handle, 'gpu')


def test_lk_position_and_err_against_the_float64_tracker(handle):
    D.check_lk_noisy(handle, 'gpu')


def test_lk_position_on_analytic_frames(handle):
    D.check_lk_analytic(handle, 'gpu')


def test_lk_minimum_eigenvalue_gate(handle):
    D.check_lk_gate(handle, 'gpu')


def test_lk_status_at_the_frames_edge(handle):
    D.check_lk_status(handle, 'gpu')


def test_reject_with_f_is_consistent_with_its_model(handle):
    D.check_reject_with_f(handle, 'gpu')
