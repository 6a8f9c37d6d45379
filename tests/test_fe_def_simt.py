"""The front end against its float64 DEFINITIONS (tests/fe_def_ref.py), per pixel and per track, on the EMULATED library (the kernel sources
under the CPU fiber emulator, tests/simt), plus the device-free checks: the recorded figures re-derived from oracle/fe_numpy.py, the
conditions the case tables must meet (band caps, the masked threshold ratio, the Sobel count of the gate table) and the mutation test.
The same check bodies run on the MI355X in tests/test_fe_def_gpu.py.

`python tests/test_fe_def_simt.py` prints every recorded figure and the mutation table (tests/simt/README.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conftest  # noqa: F401  (loads the package)

import fe_def_ref as D  # noqa: E402
from oracle import fe_numpy as N  # noqa: E402


# ---------------------------------------------------------------------------------------------- the restatement on the tables
_CACHE = {}


def _once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def restated_eig():
    """name -> (fe_numpy map, lambda_64, S)"""
    return _once('eig', lambda: {k: (N.mineig(img),) + D.mineig64(img) for k, img in D.eig_cases().items()})


def restated_lk_noisy():
    """name -> (levels_i, levels_j, pts, (xy, st, err) of fe_numpy.lk, LK64)"""
    def run():
        out = {}
        for name, (a, b, pts) in D.lk_noisy_tables().items():
            li, lj = N.pyramid(a), N.pyramid(b)
            out[name] = (li, lj, pts, N.lk(a, b, pts), D.lk64(li, lj, pts))
        return out
    return _once('lk', run)


def restated_lk_analytic():
    """shift -> (largest distance of LK64 to the truth, of fe_numpy.lk to the truth)"""
    def run():
        a, pts = D.analytic_points()
        out = {}
        for shift in D.ANALYTIC_SHIFTS:
            b = D.analytic_frame(shift)
            ref = D.lk64(N.pyramid(a), N.pyramid(b), pts)
            xy, st, _ = N.lk(a, b, pts)
            truth = pts.astype(np.float64) + np.array(shift)
            assert ref['status'].all() and ref['converged'].all() and st.all(), shift
            out[shift] = (float(np.linalg.norm(ref['xy'] - truth, axis=1).max()), float(np.linalg.norm(xy - truth, axis=1).max()))
        return out
    return _once('analytic', run)


def restated_gate():
    def run():
        img, pts = D.gate_table()
        st = np.concatenate([N.lk(img, img, pts[k:k + 60])[1] for k in range(0, len(pts), 60)])
        return img, pts, st, D.gate64(img, pts)
    return _once('gate', run)


# ---------------------------------------------------------------------------------------------- device-free checks
def test_recorded_figures_are_the_restatements():
    """Every recorded constant of fe_def_ref is what oracle/fe_numpy shows on the same table (to the digits recorded), and no bound exceeds
    the ceiling the issue set for it."""
    e32 = max(float(D.eig_error(g, lam, S).max()) for g, lam, S in restated_eig().values())
    assert 0.98 * D.E32 <= e32 <= D.E32, (e32, D.E32)
    for name, (li, lj, pts, (xy, st, err), ref) in restated_lk_noisy().items():
        f = D.lk_figures(ref, xy, st, err)
        assert 0.98 * D.LK_MAX_REC[name] <= f['max'] <= D.LK_MAX_REC[name], (name, f)
        assert 0.98 * D.LK_MED_REC[name] <= f['median'] <= D.LK_MED_REC[name], (name, f)
        assert 0.98 * D.LK_ERR_REC[name] <= f['err'] <= D.LK_ERR_REC[name], (name, f)
        D.lk_bounds(name)                                                  # (asserts the ceilings)
    worst = max(v[0] for v in restated_lk_analytic().values())
    assert 0.98 * D.LK_TRUTH_REC <= worst <= D.LK_TRUTH_REC, worst
    assert D.lk_truth_bound() <= D.LK_TRUTH_CEIL
    assert D.M_EIG == 2


def test_caps_on_left_out_cases_are_met_by_the_restatement():
    for name, (li, lj, pts, (xy, st, err), ref) in restated_lk_noisy().items():
        f = D.lk_figures(ref, xy, st, err)
        assert 40 <= f['n'] <= 64 and f['left_out'] <= D.LEFT_OUT_CAP * f['n'] and f['lost'] == 0, (name, f)
    img, pts, st, q = restated_gate()
    want, judged = D.gate_judgement(q)
    assert len(pts) == 300 and (~judged).sum() <= D.GATE_BAND_CAP * 300
    assert want[judged].sum() >= 60 and (1 - want[judged]).sum() >= 60          # the ramp crosses the threshold
    assert np.array_equal(st[judged], want[judged]), np.nonzero(judged & (st != want))[0]
    from oracle import fe_cpu as C
    for seed in (3, 4, 5, 6, 7):
        p1, p2, out = D.two_view(seed)
        st_f, Fm = C.reject_with_f(p1, p2, 1.0)
        bad, band = D.f_consistency(st_f, int(st_f.sum()), Fm, p1, p2, 1.0)
        assert not bad and band <= D.F_BAND_CAP * len(p1), (seed, bad, band)


def test_masked_threshold_differs_twofold():
    assert D.masked_threshold_ratio() >= 2.0
    img, mask, n, md = D.corner_cases()['masked_max_md12']
    eig = N.mineig(img)
    ys, xs, thr = D.candidates(eig, mask)
    # candidates exist between the two thresholds: a threshold taken from the unmasked maximum would lose them
    assert ((eig[ys, xs] > thr) & (eig[ys, xs] <= np.float32(float(eig.max()) * D.QUALITY))).sum() >= 5


def test_gate_table_tells_sobel_from_scharr():
    """4c is the F2 test: the Sobel form of the gate (scaled to the same gain on a ramp) must disagree with the Scharr form on at least
    five judged points of the table -- a table of smooth texture gives none."""
    img, pts, st, q = restated_gate()
    want, judged = D.gate_judgement(q)
    for edit in ('sobel_for_scharr', 'central_for_scharr'):
        other = (D.gate64(img, pts, edit) >= D.GATE).astype(np.uint8)
        assert (judged & (other != want)).sum() >= D.SOBEL_MIN_DISAGREE, edit


def test_corner_properties_hold_for_the_restatement_and_the_definition():
    for name, (img, mask, n, md) in D.corner_cases().items():
        eig = N.mineig(img)
        lst = N.gftt(img, n, D.QUALITY, md, mask)
        assert not D.corner_violations(eig, mask, lst, n, D.QUALITY, md), name
        assert np.array_equal(lst, D.greedy_corners(eig, mask, n, D.QUALITY, md)), name


def test_reject_with_f_checks_hold_for_the_restatement():
    from oracle import fe_cpu as C

    def run(p1, p2, thr):
        st, Fm = C.reject_with_f(p1, p2, thr)
        return st, int(st.sum()), Fm
    D.check_reject_with_f(None, 'restated', run)


def mutation_table():
    """edit -> (table, figure, twice the bound in force there) for the table that tells the edit apart best."""
    def run():
        rows = {}
        # pyramid / min-eigenvalue edits: against the restated levels and maps
        img = D.eig_cases()['256x160']
        levels = N.pyramid(img)
        rows['border_replicate'] = ('pyramid 256x160: largest |level - exact|', max(w for _, w in D.pyramid_errors(levels, 'border_replicate')), 2 * 0.5)
        for edit in ('border_replicate', 'scale_255x8', 'normalised_box'):
            worst = max((float(D.eig_error(g, *D.mineig64(D.eig_cases()[k], edit)).max()), k) for k, (g, _, _) in restated_eig().items() if k != 'flat')
            if edit != 'border_replicate' or rows[edit][1] < rows[edit][2]:
                rows[edit] = ('min-eig %s: own-scale error' % worst[1], worst[0], 2 * D.M_EIG * D.E32)
        # LK edits: the restated tracker against the EDITED float64 tracker on the 4a tables (max and median), and on the gate table
        gimg, gpts, gst, q = restated_gate()
        want, judged = D.gate_judgement(q)
        for edit in ('sobel_for_scharr', 'central_for_scharr', 'window_19', 'window_23', 'origin_10p5', 'guess_not_doubled'):
            best = None
            for name, (li, lj, pts, (xy, st, err), _) in restated_lk_noisy().items():
                f = D.lk_figures(D.lk64(li, lj, pts, edit), xy, st, err)
                bmax, bmed, berr = D.lk_bounds(name)
                for kind, fig, b in (('max', f['max'], bmax), ('median', f['median'], bmed), ('err', f['err'], berr)):
                    if best is None or fig / b > best[1] / (best[2] / 2):
                        best = ('LK %s %s' % (name, kind), fig, 2 * b)
            ge, gj = D.gate_judgement(D.gate64(gimg, gpts, edit))
            ndis = int((gj & (ge != gst)).sum())
            if best[1] < best[2] and ndis >= D.SOBEL_MIN_DISAGREE:
                best = ('LK gate: judged points whose status disagrees', ndis, D.SOBEL_MIN_DISAGREE)
            rows[edit] = best
        # corner edits: the list the EDITED definition implies, judged by the unedited properties on the restated map
        for edit in ('thr_unmasked_max', 'localmax_unmasked_only', 'dist_le', 'ties_smaller_first'):
            best = ('no case', 0, 1)
            for name, (cimg, mask, n, md) in D.corner_cases().items():
                eig = N.mineig(cimg)
                nbad = len(D.corner_violations(eig, mask, D.greedy_corners(eig, mask, n, D.QUALITY, md, edit), n, D.QUALITY, md))
                if nbad > best[1]:
                    best = ('corners %s: violated properties' % name, nbad, 1)
            rows[edit] = best
        return rows
    return _once('mutations', run)


# edits that no table can tell from the unedited definition, with the reason (none: every edit is caught)
INDISTINGUISHABLE = {}


def test_each_edit_is_told_apart():
    rows = mutation_table()
    assert set(rows) == set(D.EDITS)
    for edit, (table, figure, twice_bound) in rows.items():
        if edit in INDISTINGUISHABLE:
            continue
        assert figure >= twice_bound, "%s (%s) is not told apart: %s = %.3e, twice the bound %.3e" % (edit, D.EDITS[edit], table, figure, twice_bound)


# ---------------------------------------------------------------------------------------------- the emulated library
def test_emulated_pyramid(simt_handle):
    D.check_pyramid(simt_handle, 'emulated')


def test_emulated_mineig(simt_handle):
    D.check_mineig(simt_handle, 'emulated')


def test_emulated_corners(simt_handle):
    D.check_corners(simt_handle, 'emulated')


_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import fe_def_ref as D
h = conftest._simt_handle()
print(D.check_lk_noisy(h, 'emulated'))
h.close()
print("OK")
"""


@pytest.mark.parametrize("order", ["forward", "reverse", "shuffle"])
def test_emulated_lk_position_in_every_fiber_order(order):
    """4a / 4d under the emulator with the fibers of a wavefront scheduled forward, in reverse and shuffled (a child process: the order is
    read when the emulated library is loaded)."""
    env = dict(os.environ, SIMT_ORDER=order)
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_emulated_lk_analytic(simt_handle):
    D.check_lk_analytic(simt_handle, 'emulated')


def test_emulated_lk_gate(simt_handle):
    D.check_lk_gate(simt_handle, 'emulated')


def test_emulated_lk_status(simt_handle):
    D.check_lk_status(simt_handle, 'emulated')


def test_emulated_reject_with_f(simt_handle):
    D.check_reject_with_f(simt_handle, 'emulated')


if __name__ == "__main__":
    np.set_printoptions(precision=4, linewidth=200)
    print("E32 per table:", {k: float(D.eig_error(g, lam, S).max()) for k, (g, lam, S) in restated_eig().items()})
    for name, (li, lj, pts, (xy, st, err), ref) in restated_lk_noisy().items():
        print("LK", name, D.lk_figures(ref, xy, st, err))
    print("LK analytic (LK64 to truth, fe_numpy to truth):", restated_lk_analytic())
    img, pts, st, q = restated_gate()
    want, judged = D.gate_judgement(q)
    print("gate: judged %d, passing %d, nearest %.4f %%, wrong %d" % (judged.sum(), want.sum(), 100 * np.abs(q / D.GATE - 1).min(), (judged & (st != want)).sum()))
    print("masked threshold ratio:", D.masked_threshold_ratio())
    for edit, row in mutation_table().items():
        print("| %s | %s | %.3g | %.3g |" % (D.EDITS[edit], row[0], row[1], row[2]))
