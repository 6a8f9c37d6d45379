"""The reference, the case table, the metric and the edits of vg_init_align (tests/init_align_ref.py), checked on their own: no device
takes part.  The device tests are tests/test_init_align_simt.py (emulated kernels) and tests/test_init_align_gpu.py.

MEASURED (this file, NumPy only): kappa of the Jacobi-scaled systems over the table 1.0 (every 3x3 bias system), 5.1e2 .. 3.3e6
(LinearAlignment), 4.8e2 .. 2.2e6 (last pass of RefineGravity); worst ratio of the two float64 routes 0.84 (s_lin of F5_refine_fails);
delta_bg against max|ref| instead of its own scale (init_align_ref's docstring): 9 .. 120 for the same routes; every edit moves some
output of a noisy case by 2e9 .. 4e12 times kappa 2^-53 (bound: 4); truth on the noise-free scenes: scale 2e-5, gyro bias 4e-3 of
its norm at most (7e-5 rad/s), Q g 4e-5 relative."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import init_align_ref as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROUTES = ('solve', 'ldlt')


@pytest.mark.parametrize("name", list(A.CASE_ARGS))
def test_case_meets_the_tables_condition(name):
    """both float64 routes at or below 1 in every group, the reference's status, and no status decision on its threshold"""
    ref, win = A.reference(name), A.case(name)
    if name == 'F2':
        assert ref['status'] == A.NUMERIC and 'delta_bg' in ref and 'g_lin' not in ref
        return
    assert ref['status'] != A.NUMERIC
    gl = np.asarray(ref['g_lin'], np.float64)
    assert abs(abs(np.linalg.norm(gl) - win['g_norm']) - 1) > 1e-3 and abs(float(ref['s_lin'])) > 1e-6
    if 's' in ref:
        assert abs(float(ref['s'])) > 1e-6
    for route in ROUTES:
        got = A.align(win, np.float64, route)
        assert got['status'] == ref['status'], route
        e = A.errors(got, ref)
        print(f"{name} {route}: status {got['status']}  " + "  ".join(f"{k} {v:.3f}" for k, v in e.items())
              + f"  (delta_bg against max|ref|: {A.errors(got, ref, literal=True)['delta_bg']:.1f};"
              + " kappa " + " ".join(f"{k} {A.kappa(m):.1e}" for k, m in ref['systems'].items()) + ")")
        assert e and max(e.values()) <= 1.0, e


def test_table_covers_what_it_must():
    st = {n: A.reference(n)['status'] for n in A.CASE_ARGS}
    assert {A.OK, A.FAILED_LINEAR, A.FAILED_REFINE, A.NUMERIC} == set(st.values())
    # the gravity-norm failure, s_lin < 0, s < 0 only after the refinement
    r = A.reference('F11_gnorm')
    assert st['F11_gnorm'] == A.FAILED_LINEAR and r['s_lin'] > 0
    r = A.reference('F11_mirrored')
    assert st['F11_mirrored'] == A.FAILED_LINEAR and r['s_lin'] < 0 and abs(np.sqrt(r['g_lin'] @ r['g_lin']) - A.case('F11_mirrored')['g_norm']) < 1
    r = A.reference('F5_refine_fails')
    assert st['F5_refine_fails'] == A.FAILED_REFINE and r['s_lin'] > 0 and r['s'] < 0
    assert {len(A.case(n)['R']) for n in A.CASE_ARGS} >= {2, 4, 5, 11, 32}
    spi = {n: sorted({len(iv) - 1 for iv in A.case(n)['intervals']}) for n in A.CASE_ARGS}
    assert spi['F11_spi1'] == [1] and spi['F11'] == [20] and len(spi['F11_ragged']) > 3 and len(spi['F32_noisy']) > 3
    keys = {n: A.case(n)['key'] for n in A.CASE_ARGS}
    assert keys['F5'] is None and keys['F11'] == list(range(11)) and keys['F11_noisy_subset'][0] == 2 and st['F11_noisy_subset'] == A.OK
    assert all(A.CASE_ARGS[n].get('noise') for n in A.NOISY) and len(A.NOISY) >= 5


@pytest.mark.parametrize("edit", A.EDITS)
def test_each_edit_exceeds_the_bound(edit):
    """applied to the float64 route, on the cases with pose noise only"""
    worst = (0.0, None, None)
    for name in A.NOISY:
        ref = A.reference(name)
        e = A.errors(A.align(A.case(name), np.float64, 'solve', edit=edit), ref)
        k = max(e, key=e.get)
        if e[k] > worst[0]:
            worst = (e[k], name, k)
    print(f"edit {edit}: {worst[0]:.3g} x kappa 2^-53 ({worst[2]} of {worst[1]}); bound {A.M}")
    assert worst[0] > A.M, worst


@pytest.mark.parametrize("name", A.TRUTH_CASES)
def test_reference_recovers_the_truth(name):
    """noise-free scene: the 80-bit route finds the scale, the gyro bias and Q g the scene was made with (what is left is the
    mid-point integration at 200 Hz)"""
    ref, truth = A.reference(name), A.case(name)['truth']
    assert ref['status'] == A.OK
    s = abs(float(ref['s']) - truth['s']) / truth['s']
    g = np.abs(np.asarray(ref['g_c0'], np.float64) - truth['g']).max() / A.G_TRUE
    bg = np.abs(np.asarray(ref['bg'], np.float64) - truth['bg']).max()
    print(f"{name}: scale {s:.1e}  g {g:.1e}  gyro bias {bg:.1e} rad/s ({bg / np.abs(truth['bg']).max():.1e} of its largest component)")
    assert s < 1e-3 and g < 1e-3 and bg < 1e-3 * max(1.0, np.abs(truth['bg']).max())


def test_window_stage_properties():
    """what :376-435 promise, in the 80-bit route: gravity along +z in the world, the first window frame at the origin without yaw"""
    for name in ('F11', 'F11_noisy_subset', 'F32'):
        ref, win = A.reference(name), A.case(name)
        gw = np.asarray(ref['g_w'], np.float64)
        assert np.abs(gw - [0, 0, win['g_norm']]).max() < 1e-9
        assert not np.asarray(ref['Ps'][0], np.float64).any()
        R0s = np.asarray(ref['Rs'][0], np.float64)
        assert abs(np.arctan2(R0s[1, 0], R0s[0, 0])) < 1e-12
        R0 = np.asarray(ref['R0'], np.float64)
        assert np.abs(R0 @ R0.T - np.eye(3)).max() < 1e-12


def test_lds_carve(tmp_path):
    """csrc/init_align_carve.h through its stand-alone checker: every F fits, F = 32 is what the header says"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "init_align_carve_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "init_align_carve_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 31
    last = dict(zip(lines[-1].split()[::2], map(int, lines[-1].split()[1::2])))
    assert last['F'] == 32 and last['n'] == 100 and last['bytes'] == 8 * last['end'] <= 160 * 1024
    assert last['fac'] - last['acc'] == 5050 and last['bytes'] < 100 * 1024
