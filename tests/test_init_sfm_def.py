"""The definition of vg_init_sfm, on the CPU: the three routes of tests/init_sfm_ref.sfm against each other on every case of the table,
the cases the table must contain, and the edits.  The device files (test_init_sfm_simt.py, test_init_sfm_gpu.py) hold the kernels to the
80-bit route within M x E64 with these E64.

MEASURED on the CPU (this file prints them; profiles/init_sfm.json keeps the same table): E64 per case and group, max|d| / max|ref| of
the worse float64 route against the 80-bit route:
    F3_10       q0 2.0e-17  T0 1.0e-15  position0 7.2e-15  q 4.4e-17  T 1.8e-16  position 2.8e-15  R_all 9.9e-17  T_all 1.8e-16  ba_cost 2.0e-12
    F3_14       q0 1.5e-16  T0 7.5e-16  position0 1.3e-14  q 5.8e-16  T 8.9e-16  position 2.8e-15  R_all 1.0e-16  T_all 8.9e-16  ba_cost 8.1e-13
    F5_12       q0 5.1e-17  T0 1.3e-15  position0 1.6e-15  q 1.8e-16  T 5.2e-16  position 7.4e-16  R_all 1.3e-16  T_all 5.2e-16  ba_cost 8.3e-12
    F5_nk6      q0 5.6e-17  T0 2.9e-16  position0 4.2e-15  q 1.7e-16  T 2.5e-16  position 5.6e-16  R_all 1.2e-16  T_all 4.7e-16  ba_cost 2.8e-12
    F5_nk5      q0 5.6e-17  T0 2.9e-16  position0 4.2e-15  q 1.7e-16  T 2.5e-16  position 5.6e-16  R_all 1.2e-16  T_all 3.9e-16  ba_cost 2.8e-12
    F5_scaled   q0 4.6e-17  T0 6.1e-16  position0 1.2e-14  q 2.7e-16  T 7.9e-16  position 3.2e-15  R_all 8.6e-17  T_all 7.9e-16  ba_cost 2.4e-13
    F11_l0      q0 1.7e-16  T0 1.7e-16  position0 1.3e-14  q 2.0e-16  T 1.5e-16  position 1.4e-15  R_all 1.2e-16  T_all 1.5e-16  ba_cost 1.1e-12
    F11_mid     q0 8.5e-17  T0 3.4e-16  position0 7.3e-15  q 2.9e-16  T 2.9e-16  position 2.2e-15  R_all 1.3e-16  T_all 2.9e-16  ba_cost 1.9e-12
    F11_last    q0 2.0e-16  T0 2.3e-16  position0 9.6e-15  q 2.7e-16  T 7.6e-16  position 2.4e-15  R_all 1.8e-16  T_all 7.6e-16  ba_cost 1.2e-12
    F5_50_ok    q0 8.3e-17  T0 1.0e-15  position0 1.1e-13  q 9.4e-16  T 8.1e-15  position 1.9e-10  R_all 1.5e-15  T_all 8.1e-15  ba_cost 1.8e-10
    F5_50_fail  q0 5.5e-17  T0 2.9e-16  position0 3.8e-14  ba_cost 3.0e-11
    F16         q0 6.5e-17  T0 3.0e-16  position0 4.2e-14  q 2.8e-16  T 2.6e-16  position 1.6e-15  R_all 1.2e-16  T_all 2.6e-16  ba_cost 5.7e-12
the floors (tests/init_sfm_ref.e64_floor), the largest over the cases whose BA converges:
    q0 2.0e-16  T0 1.3e-15  position0 4.2e-14  q 5.8e-16  T 8.9e-16  position 3.2e-15  R_all 1.8e-16  T_all 8.9e-16  ba_cost 8.3e-12
and over the two whose BA runs out of its 50 iterations (50 steps along a valley amplify the last bits of the start):
    q0 8.3e-17  T0 1.0e-15  position0 1.1e-13  q 9.4e-16  T 8.1e-15  position 1.9e-10  R_all 1.5e-15  T_all 8.1e-15  ba_cost 1.8e-10
Every edit exceeds M x E64 on the case named beside it in EDIT_CASE (or changes a decision there)."""
import numpy as np
import pytest

import init_sfm_ref as S

NAMES = list(S.CASE_ARGS)
# the case each edit is judged on
EDIT_CASE = {'no_float32': 'F11_mid', 'stage3_first': 'F11_l0', 'stage5_first_two': 'F11_mid', 'threshold_15': 'F3_10', 'T_last_free': 'F11_mid',
             'no_normalisation': 'F5_scaled', 'lm_unclamped': 'F5_50_fail', 'ric_dropped': 'F11_mid'}


@pytest.mark.parametrize("name", NAMES)
def test_float64_routes_decide_like_the_80_bit_route(name):
    """the precondition of the table: status, state[], pnp_iters / pnp_up, the accept flags, ba_iters, ba_termination"""
    ref = S.reference(name)
    for route in ('solve', 'ldlt'):
        got = S.route64(name, route)
        assert got['dec'] == ref['dec'], (name, route, got['dec'], ref['dec'])
    e = S.e64(name)
    print(f"init_sfm E64 {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert all(np.isfinite(v) for v in e.values())
    assert ref['pnp_margin'] >= S.PNP_MARGIN, (name, ref['pnp_margin'])


def test_e64_floor():
    fl, out = S.e64_floor(), S.e64_floor(True)
    print("init_sfm E64 floor, converging cases: " + "  ".join(f"{k} {v:.1e}" for k, v in fl.items()))
    print("init_sfm E64 floor, cases that run out of iterations: " + "  ".join(f"{k} {v:.1e}" for k, v in out.items()))
    assert set(fl) == set(S.VALUE_KEYS) and set(out) <= set(S.VALUE_KEYS)
    for n in S.CASE_ARGS:                                    # never looser than the floor over the whole table
        for k, v in S.bound(n).items():
            assert v <= S.M * max(max(fl[k], out.get(k, 0.0)), S.e64(n)[k])


def test_the_table_holds_the_cases_it_must():
    dec = {n: S.reference(n)['dec'] for n in NAMES}
    status = {n: d['status'] for n, d in dec.items()}
    assert status['F3_9'] == S.FAILED_PNP and status['F3_10'] == S.OK and status['F3_14'] == S.OK
    assert status['F5_nk5'] == S.FAILED_FRAME and status['F5_nk6'] == S.OK and status['F5_nan'] == S.NUMERIC
    assert dec['F5_50_ok']['ba_iters'] == 50 and status['F5_50_ok'] == S.OK and dec['F5_50_ok']['ba_termination'] == S.NO_CONVERGENCE
    assert dec['F5_50_fail']['ba_iters'] == 50 and status['F5_50_fail'] == S.FAILED_BA
    assert any(1 in d['flags'][:-1] for d in dec.values()), "a rejected LM step"
    assert any(S.reference(n)['function_tolerance'] for n in NAMES), "a BA that ends by function tolerance"
    assert {len(S.case(n)['start']) for n in NAMES} >= {12, 64, 65, 300}
    assert {(S.case(n)['n_frames'], S.case(n)['l']) for n in NAMES} >= {(3, 0), (11, 0), (11, 5), (11, 9), (16, 7)}
    # the exact point counts of frame 1 in the F = 3 cases
    for n, k in (('F3_10', 10), ('F3_14', 14), ('F3_9', 9)):
        w = S.case(n)
        assert int(np.sum((w['start'] == 0) & (w['nobs'] == 3))) == k
    w, d = S.case('F11_mid'), dec['F11_mid']
    l, F = w['l'], w['n_frames']
    one = w['nobs'] == 1
    assert one.any() and not any(d['state'][j] for j in np.nonzero(one)[0]), "features of length 1 stay out"
    # seen neither in l nor in F - 1, two observations or more: only stage 5 reaches them
    late = (w['nobs'] >= 2) & ((w['start'] + w['nobs'] <= l) | ((w['start'] > l) & (w['start'] + w['nobs'] < F)))
    assert late.any() and all(d['state'][j] for j in np.nonzero(late)[0])
    assert len(w['all_key']) == 2 * F - 1 and len(S.case('F16')['all_key']) == 16


@pytest.mark.parametrize("edit", S.EDITS)
def test_edit_exceeds_the_bound(edit):
    name = EDIT_CASE[edit]
    got = S.view(S.sfm(S.case(name), np.float64, 'ldlt', edit=edit))
    ref = S.reference(name)
    if got['dec'] != ref['dec']:
        print(f"init_sfm edit {edit} on {name}: the decisions change")
        return
    r = S.ratios(got, name)
    print(f"init_sfm edit {edit} on {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in r.items()))
    assert max(r.values()) > S.M, (edit, r)


def test_reference_recovers_the_scene():
    """noise-free, true relative pose: the 80-bit route returns the scene's camera positions and landmarks"""
    w = S.scene(5, F=7, l=3, n_feat=60, noise=0.0)
    o = S.sfm(w)
    assert o['status'] == S.OK
    T = np.array([c[1] for c in w['truth']['cam']])
    assert np.abs(np.asarray(o['T'], np.float64) - T).max() < 1e-6
    on = o['state']
    assert np.abs(np.asarray(o['position'], np.float64)[on] - w['truth']['X'][on]).max() < 1e-5
