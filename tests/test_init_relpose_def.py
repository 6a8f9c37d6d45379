"""The reference of vg_init_relpose against itself, on the CPU (tests/init_relpose_ref.py): every case of the table survives the
conditions of that module, does what it is listed for, and the float64 Jacobi route takes the 80-bit route's decisions."""
import numpy as np
import pytest

import init_relpose_ref as R


@pytest.mark.parametrize("name", list(R.CASE_ARGS))
def test_case_meets_the_conditions_and_its_purpose(name):
    ref = R.reference(name)
    assert R.conditions(ref, name in R.ALLOW_12_13) == []
    R.check_case_properties({name: R.as_result(ref, R.case(name))})
    for c in ref['cand']:
        if not c['gate']:
            continue
        assert c['replay_inliers'] == c['ransac_inliers'], "the NumPy replay ends on the oracle's model"
        r64 = R.pose(c['F'], c['ll'], c['rr'], c['ransac_mask'], np.float64, 'jacobi')
        assert (r64['good'], r64['winner']) == (c['good'], c['winner']) and np.array_equal(r64['mask'], c['mask'])
        s64 = R.pose(c['F'], c['ll'], c['rr'], c['ransac_mask'], np.float64, 'svd')
        assert sorted(s64['good']) == sorted(c['good']) and s64['inlier_cnt'] == c['inlier_cnt']
        assert np.abs(s64['R'] - c['R'].astype(np.float64)).max() < 1e-9 and np.abs(s64['T'] - c['T'].astype(np.float64)).max() < 1e-9


def test_recovered_pose_is_the_scene_s():
    """relative_R / relative_T of the noise-light reference shape against the generator's cameras"""
    win, ref = R.case('F11_first'), R.reference('F11_first')
    l, F = ref['l'], win['n_frames']
    Rw, pos = win['truth']['R'], win['truth']['pos']
    Rt = Rw[l].T @ Rw[F - 1]
    Tt = Rw[l].T @ (pos[F - 1] - pos[l])
    assert np.abs(ref['R'].astype(np.float64) - Rt).max() < 2e-3
    assert np.abs(ref['T'].astype(np.float64) - Tt / np.linalg.norm(Tt)).max() < 2e-2


def test_gate_sum_order_bound():
    """any order of the positive terms stays within n 2^-53 relative of the correctly rounded sum: the header's order included"""
    a, b = R.corres(R.capacity_scene(), 0)
    d = a - b
    t = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    s = np.zeros(256)
    for k in range(0, len(t), 256):
        s[:len(t[k:k + 256])] += t[k:k + 256]
    h = 128
    while h >= 1:
        s[:h] += s[h:2 * h]
        h //= 2
    n, avg, _, _ = R.gate(a, b)
    assert abs(s[0] / n - avg) / avg <= n * 2.0 ** -53


def test_capacity_window_meets_the_conditions():
    ref = R.capacity_reference()
    assert R.conditions(ref) == [] and ref['l'] == 0
    for c in ref['cand']:
        if c['gate']:
            assert c['replay_inliers'] == c['ransac_inliers']


def test_e64_stays_under_its_ceiling():
    """the two float64 routes against the 80-bit one on every gated candidate of the table: below E64_CEILING, the figure of the count
    in tests/init_relpose_ref.py"""
    for name in R.CASE_ARGS:
        for c in R.reference(name)['cand']:
            if c['gate']:
                R.pose_errors(c['R'], c['T'], c, c['F'])        # (asserts the ceiling)


def test_window_walk_with_a_numeric_candidate():
    """the pick over the candidates, restated: a gated candidate whose SVD did not converge ends the window with NUMERIC when the walk
    meets it before a success, and is never looked at behind one"""
    ok, fail, off = dict(gate=1, success=True, conv=True), dict(gate=1, success=False, conv=True), dict(gate=0)
    bad = dict(gate=1, success=True, conv=False)
    assert R.pick([off, fail, ok, bad]) == (R.OK, 2)
    assert R.pick([off, bad, ok]) == (R.NUMERIC, -1)
    assert R.pick([fail, off, fail]) == (R.NONE, -1)
    assert R.pick([dict(off, conv=False), ok]) == (R.OK, 1)
