"""vg_init_exrot's NumPy reference against itself (tests/init_exrot_ref.py), no device: a float64 run of every case stands in for the
device and goes through the very check body the emulator and the MI355X go through, so that the conditions the decision checks rest on
are asserted here -- the two float64 routes and the 80-bit route take the same decisions on every step of every case (no ratio1 ==
ratio2, no depth within 1e-4 of zero, sigma[2] not within 1e-6 of 0.25, no angular distance within 1e-6 degrees of 5) -- and each case
is about what its comment says.

RECOVERY of the scene's true ric (test_calibrated_ric_recovers_the_scene), at the default threshold 3.0 and at the separating one, 0.3 / 460
(the threshold solveRelativeRT passes, in the units of the points), on the noisy scenes 'success10' and 'ric90'.  Two bounds, both
written down before any figure was taken:
  RECORDS, from the noise, at the separating threshold only.  The points carry NOISE_PX = 0.05 pixels; the RANSAC accepts a model whose
    points lie within 0.3 pixels = 6 sigma of their epipolar lines.  A rotation error delta of the model moves a point by delta; the
    translation can take up at most all of it, and what it takes it takes as parallax, baseline / depth per unit of translation
    direction; so a point's line moves by at least delta baseline / depth, and delta <= 6 sigma depth_max / baseline_min = 6 * 1.09e-4 *
    8 / 0.12 = 4.3e-2 rad: RECORD_DEG = 2.5 degrees for every record.  (Loose: it is the worst direction of translation.  Measured: 0.31
    at most.)  At 3.0 nothing of the kind holds: every root of the first sample's cubic takes all points and records are 5 degrees off.
  CALIBRATION, from the records, at both thresholds: exact perturbation theory of the null vector.  With x the quaternion of the scene's
    ric, record k leaves the residual h_k |q(Rc_k) - q(Rc_k of the scene)| <= h_k delta_k / 2 in A x (h_k <= 1 its Huber weight,
    delta_k its rotation error), and the part of x outside the computed vector is stretched by at least sigma[2]; so the angle between
    calib_ric and the scene's ric is at most 2 asin(sqrt(sum (h_k delta_k)^2) / (2 sigma[2])).  No constant is chosen.  A wrong block,
    convention, inverse or singular vector breaks it.  Measured: 0.24 (bound about 0.5) and 0.20 (0.85) degrees at 0.3 / 460, 2.23 and
    2.23 at 3.0."""
import numpy as np
import pytest

import init_exrot_ref as X

SEPARATING = X.CHAIN_THRESHOLD
RECORD_DEG = float(np.degrees(6 * X.NOISE_PX * X.PX * 8.0 / 0.12))


@pytest.fixture(scope="module")
def runs():
    return {n: X.run(X.case(n), np.float64, 'jacobi', with_replay=True) for n in X.CASE_ARGS}


@pytest.mark.parametrize("name", list(X.CASE_ARGS))
def test_routes_take_the_same_decisions(runs, name):
    X.check_window(name, X.case(name), X.as_device(runs[name]), 'def')


def test_cases_are_about_what_they_say(runs):
    X.check_case_properties({n: X.as_device(r) for n, r in runs.items()})


def test_huber_branch_is_taken_at_ric90(runs):
    s = runs['ric90']['steps']
    assert s[0]['ang'] > X.HUBER_DEG and s[0]['huber'] < 1.0 and s[1]['huber'] < 1.0, [x['ang'] for x in s[:3]]


@pytest.mark.parametrize("thresh", [X.THRESH, SEPARATING])
@pytest.mark.parametrize("name", ['success10', 'ric90'])
def test_calibrated_ric_recovers_the_scene(runs, name, thresh):
    win = dict(X.case(name), ransac_threshold=thresh)
    r = runs[name] if thresh == X.THRESH else X.run(win, np.float64, 'jacobi', with_replay=True)
    truth = win['truth']
    m = r['first_ok']
    assert m == X.MIN_FRAMES
    delta = np.array([X._angle_deg(np.asarray(s['Rc'], np.float64) @ truth['Rc'][k].T) for k, s in enumerate(r['steps'][:m])])
    hub = np.array([float(s['huber']) for s in r['steps'][:m]])
    sigma2 = float(r['steps'][m - 1]['sigma'][2])
    arg = np.sqrt(np.sum(np.radians(hub * delta) ** 2)) / (2 * sigma2)
    bound = float(np.degrees(2 * np.arcsin(min(1.0, arg)))) + 1e-9
    err = X._angle_deg(r['calib_ric'] @ truth['ric'].T)
    print(f"init_exrot def {name} at {thresh:.3g}: records off by {delta.round(3)} degrees, sigma[2] {sigma2:.3f}: calib_ric {err:.3f} degrees from the "
          f"scene's (bound {bound:.3f})")
    assert err <= bound
    assert abs(np.linalg.det(r['calib_ric']) - 1) < 1e-9
    if thresh == SEPARATING:
        assert delta.max() <= RECORD_DEG, (delta, RECORD_DEG)
        X.check_window(name, win, X.as_device(r), 'def', quiet=True)      # the three routes decide alike at this threshold too


def test_numeric_and_capacity_scenes(runs):
    r = X.run(X.numeric_scene(), with_replay=True)
    assert r['status'] == X.NUMERIC and r['first_ok'] == -1 and [s['model'] for s in r['steps']] == [True, False, True]
    X.check_window('numeric', X.numeric_scene(), X.as_device(r), 'def', quiet=True)
    c = X.run(X.capacity_scene(), with_replay=True)
    X.check_window('capacity', X.capacity_scene(), X.as_device(c), 'def', quiet=True)


def test_split_run_equals_the_unsplit_one(runs):
    """the carried state is the whole state: the reference resumed through records / ric is the reference unsplit, bit for bit"""
    win, whole = X.case(X.SPLIT_CASE), X.as_device(runs[X.SPLIT_CASE])
    for cut in (1, 9, 11):
        a = X.as_device(X.run(X.resume(win, [], 0, cut), with_replay=True))
        b = X.as_device(X.run(X.resume(win, [a], cut, 12), with_replay=True))
        for k in X.TAPS:
            assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), (cut, k)


def test_chain_scene_reference_recovers_ric_at_the_chain_threshold():
    """the scene of the chain check, the reference alone: at CHAIN_THRESHOLD the calibration succeeds at step min_frames and returns the
    scene's ric within CHAIN_RIC_DEG (the bound's reasoning stands beside it), and the three routes take the same decisions"""
    ex = X.chain_window()
    r = X.run(ex, np.float64, 'jacobi', with_replay=True)
    err = X._angle_deg(r['calib_ric'] @ ex['truth']['ric'].T)
    print(f"init_exrot def chain scene: first_ok {r['first_ok']}  calib_ric {err:.2e} degrees from the scene's (bound {X.CHAIN_RIC_DEG})")
    assert r['status'] == X.OK and r['first_ok'] == X.MIN_FRAMES and err <= X.CHAIN_RIC_DEG
    X.check_window('chain', ex, X.as_device(r), 'def', quiet=True)
