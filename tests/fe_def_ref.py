"""tests/fe_def_ref.py -- float64 DEFINITIONS of the front-end kernels (TEST INFRASTRUCTURE), the case tables and the check bodies of
tests/test_fe_def_simt.py (emulated library, device-free checks) and tests/test_fe_def_gpu.py (MI355X).

Every other front-end test is bit-exact against oracle/fe_cpu.cpp, which is bit-exact against oracle/fe_numpy.py: two restatements of the
same fixed-point procedure by the same hand.  This module states what the procedure is FOR, from the mathematical rows F1-F5 / F9 of
oracle/ASSUMPTIONS.md, in float64 NumPy and without the fixed-point detail (no 14-bit weights, no 5-bit patches, no `>> 8`, no float32
intermediates), imports nothing from oracle/, and holds the device to it per pixel and per track:

  1  pyramid      level k+1 == round-half-up of the exact [1 4 6 4 1]^2 / 256 reflect-101 filter of the device's own level k (256 x the
                  exact value is an integer: an equality), the number of levels == the depth rule
  2  min-eig map  the smaller eigenvalue of the 3 x 3 box sum of Sobel/3060 outer products, per pixel in the OWN SCALE S (below)
  3  corner list  properties of the device's list on the device's own map (threshold, local maximum, order, distance, maximality)
  4  LK           a float64 Gauss-Newton pyramidal tracker run to convergence on the device's own levels: position (max and median),
                  the min-eigenvalue gate, err, status
  5  rejectWithF  status consistent with the returned F, F33 == 1, det F == 0, scenes with a known answer

OWN SCALE OF THE MIN-EIGENVALUE MAP.  With s = 1/3060 the float32 pipeline forms dx = 2s r(y) + s (r(y-1) + r(y+1)) from exact integer
row differences r = I(x+1) - I(x-1): two rounded products and a rounded sum, an error of a few u rho_x with u = 2^-24 and
rho_x = s (2 |r(y)| + |r(y-1)| + |r(y+1)|) >= |dx|.  dy is different: it DIFFERENCES two smoothed rows rr = s (2 I(x) + I(x-1) + I(x+1)),
each of size ~ I / 765 and each rounded to u rr, so dy carries an ABSOLUTE error u rho_y, rho_y = rr(y+1) + rr(y-1), however small dy
itself is (the cancellation: on a bright, nearly flat patch rho_y / |dy| is in the hundreds).  A product dx dy is then off by
|dx| u rho_y + |dy| u rho_x, the squares by 2 |d| u rho; the 3 x 3 box adds them up (in double: nothing further), and the smaller
eigenvalue of a symmetric matrix moves by at most the norm of the perturbation.  The last float32 steps ((a + c), the square, the
square root, the difference) each round something of the size of the trace T = box(dx^2 + dy^2).  Hence

      S(x, y) = T + box( 2 (|dx| + |dy|) (rho_x + rho_y) ),        error(x, y) = |map - lambda_64| / S,

u taken out: a correct float32 pipeline sits at a few u = 6e-8 everywhere, flat regions included (S = 0 there and the map must be
exactly 0).  The bound is M_EIG x E32, E32 = what oracle/fe_numpy.mineig loses in this measure over the same table, M_EIG = 2.

RECORDED FIGURES.  Every bound below is a named constant = 2 x a figure of the restatement (oracle/fe_numpy) on the same table, produced
by `python tests/test_fe_def_simt.py` (prints them) and re-derived by test_fe_def_simt.py::test_recorded_figures_are_the_restatements.

EDITS are mutations of THESE definitions (never of a kernel): test_fe_def_simt.py::test_each_edit_is_told_apart shows that each one
moves at least one table to at least twice the bound in force there.
"""
import numpy as np

WIN, HALF = 21, 10
GATE = 1e-4
FLT_EPS = 2.0 ** -23
QUALITY = 0.01

# ---- recorded figures of the restatement (oracle/fe_numpy.py) on the tables of this module: `python tests/test_fe_def_simt.py`
E32 = 2.87e-8                    # min-eigenvalue map, largest |fe_numpy.mineig - lambda_64| / S over EIG_CASES
M_EIG = 2
LK_MAX_REC = {'pair_11_12': 4.34e-4, 'pair_21_22': 6.51e-4}                 # 4a: largest |fe_numpy.lk - LK64| per table, px
LK_MED_REC = {'pair_11_12': 1.015e-4, 'pair_21_22': 1.30e-4}                 # 4a: median of the same
LK_ERR_REC = {'pair_11_12': 1.495e-3, 'pair_21_22': 1.289e-3}                 # 4d: largest |err - err_64| per table, grey levels
LK_TRUTH_REC = 0.0287           # 4b: LK64's own worst distance to p + shift over the four shifts, px
LK_MAX_CEIL, LK_MED_CEIL, LK_TRUTH_CEIL = 0.03, 1e-3, 0.1
LEFT_OUT_CAP = 0.10             # 4a: tracks left out because LK64 did not converge or left the frame
GATE_BAND, GATE_BAND_CAP = 5e-3, 0.05
SOBEL_MIN_DISAGREE = 5
F_BAND, F_BAND_CAP = 1e-3, 0.02


def lk_bounds(name):
    """(max, median, err) bounds of 4a / 4d on table `name`: 2 x the recorded figure, never above the ceilings."""
    bmax, bmed = 2 * LK_MAX_REC[name], 2 * LK_MED_REC[name]
    assert bmax <= LK_MAX_CEIL and bmed <= LK_MED_CEIL, (name, bmax, bmed)
    return bmax, bmed, 2 * LK_ERR_REC[name]


def lk_truth_bound():
    assert 2 * LK_TRUTH_REC <= LK_TRUTH_CEIL
    return 2 * LK_TRUTH_REC


EDITS = {
    'border_replicate': "replicate border for reflect-101 (pyramid, Sobel, box)",
    'sobel_for_scharr': "LK derivative: Sobel x 4 for Scharr (same gain on a ramp)",
    'central_for_scharr': "LK derivative: plain central difference for Scharr",
    'window_19': "LK window 19 x 19",
    'window_23': "LK window 23 x 23",
    'origin_10p5': "LK window origin p - 10.5",
    'guess_not_doubled': "LK guess carried to the next level without doubling",
    'scale_255x8': "Sobel scale 1 / (255 * 8) for 1 / 3060",
    'normalised_box': "3 x 3 box normalised",
    'thr_unmasked_max': "corner threshold from the maximum over ALL pixels",
    'localmax_unmasked_only': "local maximum taken over unmasked neighbours only",
    'dist_le': "`<=` for `<` in the distance test",
    'ties_smaller_first': "ties in order of smaller linear index first",
}


def _fe():
    from vins_mono_amd import fe
    return fe


def _synth():
    from vins_mono_amd import synth
    return synth


def _border(img, p, edit=None):
    return np.pad(np.asarray(img, np.float64), p, mode='edge' if edit == 'border_replicate' else 'reflect')


# ================================================================================================ 1 pyramid (F1)
PYR_SIZES = ((256, 160), (190, 122), (128, 94), (64, 47))       # levels 95 x 61 (of 190 x 122) and 64 x 47 (of 128 x 94, and as a frame)


def pyrdown64(img, edit=None):
    """The exact value of [1 4 6 4 1] x [1 4 6 4 1] / 256, reflect-101, at the even pixels."""
    h, w = np.asarray(img).shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    p = _border(img, 2, edit)
    k = (1.0, 4.0, 6.0, 4.0, 1.0)
    rows, cols = 2 * np.arange(dh), 2 * np.arange(dw)
    acc = np.zeros((dh, dw))
    for a in range(5):
        for b in range(5):
            acc += k[a] * k[b] * p[rows + a][:, cols + b]
    return acc / 256.0


def n_levels(w, h, max_level=3):
    """Images of the pyramid: a further level while both of its dimensions stay larger than the window, at most max_level + 1."""
    n = 1
    while n <= max_level and (w + 1) // 2 > WIN and (h + 1) // 2 > WIN:
        w, h, n = (w + 1) // 2, (h + 1) // 2, n + 1
    return n


def pyramid_errors(levels, edit=None):
    """[(pixels that differ from round-half-up of the exact filter, largest |level - exact|)] for each level k + 1 of `levels`."""
    out = []
    for k in range(len(levels) - 1):
        ex = pyrdown64(levels[k], edit)
        got = levels[k + 1].astype(np.float64)
        assert got.shape == ex.shape, (got.shape, ex.shape)
        out.append((int((got != np.floor(ex + 0.5)).sum()), float(np.abs(got - ex).max())))
    return out


def check_pyramid(h, tag):
    fe, synth = _fe(), _synth()
    rows = []
    for (W, H) in PYR_SIZES:
        tr = fe.FrontEnd(h, W, H, 1, 8)
        img = synth.synth_frame(100 + W, W, H)
        tr.push_frames([img])
        nl = n_levels(W, H)
        levels = [tr.get_level(0, l) for l in range(nl)]
        assert np.array_equal(levels[0], img), (tag, W, H)
        try:
            tr.get_level(0, nl)
            raise AssertionError("%s %dx%d: a level beyond the depth rule (%d images)" % (tag, W, H, nl))
        except RuntimeError:
            pass
        w, hh = W, H
        for l in range(nl):
            assert levels[l].shape == (hh, w), (tag, W, H, l, levels[l].shape)
            w, hh = (w + 1) // 2, (hh + 1) // 2
        for l, (nbad, worst) in enumerate(pyramid_errors(levels)):
            rows.append((W, H, l + 1, nbad, worst))
            assert nbad == 0 and worst <= 0.5, "%s pyramid %dx%d level %d: %d pixels off, |level - exact| = %.3f" % (tag, W, H, l + 1, nbad, worst)
    return rows


# ================================================================================================ 2 min-eigenvalue map (F4)
def _box3(f, edit=None):
    p = _border(f, 1, edit)
    h, w = f.shape
    acc = np.zeros((h, w))
    for a in range(3):
        for b in range(3):
            acc += p[a:a + h, b:b + w]
    return acc / 9.0 if edit == 'normalised_box' else acc


def mineig64(img, edit=None):
    """(lambda, S): the smaller eigenvalue of [[box dx^2, box dx dy], [box dx dy, box dy^2]], Sobel 3 x 3 scaled by 1 / 3060, reflect-101
    everywhere; S = its own scale (module docstring)."""
    s = 1.0 / (255.0 * 8.0) if edit == 'scale_255x8' else 1.0 / 3060.0
    p = _border(img, 1, edit)
    r = p[:, 2:] - p[:, :-2]
    dx = s * (2 * r[1:-1] + r[:-2] + r[2:])
    rho_x = s * (2 * np.abs(r[1:-1]) + np.abs(r[:-2]) + np.abs(r[2:]))
    rr = s * (2 * p[:, 1:-1] + p[:, :-2] + p[:, 2:])
    dy = rr[2:] - rr[:-2]
    rho_y = rr[2:] + rr[:-2]
    a, b, c = _box3(dx * dx, edit), _box3(dx * dy, edit), _box3(dy * dy, edit)
    lam = 0.5 * (a + c) - np.sqrt(0.25 * (a - c) ** 2 + b * b)
    S = (a + c) + _box3(2 * (np.abs(dx) + np.abs(dy)) * (rho_x + rho_y))
    return lam, S


def eig_error(got, lam, S):
    """|got - lambda| / S per pixel; where S == 0 (exactly flat neighbourhood) the map must be exactly lambda (= 0)."""
    d = np.abs(np.asarray(got, np.float64) - lam)
    return np.where(S > 0, d / np.where(S > 0, S, 1.0), np.where(d == 0, 0.0, np.inf))


def tie_image():
    """Identical 4 x 4 squares: two of them exactly 12 px apart (the corresponding corners tie in value AND sit at min_dist = 12 exactly:
    `<` against `<=`), one far away (ties: larger linear index first)."""
    t = np.zeros((60, 80), np.uint8)
    for (x, y) in ((10, 10), (22, 10), (50, 40)):
        t[y:y + 4, x:x + 4] = 200
    return t


def saturated_image():
    img = _synth().synth_frame(71, 128, 96).copy()
    img[10:40, 20:70] = 255
    img[50:90, 60:120] = 0
    img[60:70, 70:80] = 255
    img[0:6, 100:128] = 255              # a saturated block on the border
    return img


def eig_cases():
    synth = _synth()
    return {
        '256x160': synth.synth_frame(11, 256, 160),
        '95x60': synth.synth_frame(12, 95, 60),          # (95 x 61 cannot be a FRAME: vg_fe_configure asks for width * height % 4 == 0)
        '64x47': synth.synth_frame(13, 64, 47),
        'flat': np.full((48, 64), 77, np.uint8),
        'tie': tie_image(),
        'saturated': saturated_image(),
    }


def device_eig(h, img, max_pts=8):
    fe = _fe()
    H, W = img.shape
    tr = fe.FrontEnd(h, W, H, 1, max_pts)
    tr.push_frames([img])
    tr.keep_eig()
    tr.detect(0, 1, QUALITY, 12.0)
    return tr, tr.get_eig(0)


def check_mineig(h, tag):
    fe = _fe()
    try:                                                   # the size the table cannot carry is refused, not mis-computed
        fe.FrontEnd(h, 95, 61, 1, 8)
        raise AssertionError("95 x 61 accepted: put it into eig_cases()")
    except RuntimeError:
        pass
    bound = M_EIG * E32
    rows = {}
    for name, img in eig_cases().items():
        _, got = device_eig(h, img)
        lam, S = mineig64(img)
        e = eig_error(got, lam, S)
        rows[name] = float(e.max())
        y, x = np.unravel_index(int(np.argmax(e)), e.shape)
        assert e.max() <= bound, "%s min-eig %s: error %.3e of the own scale at (%d, %d), bound %.3e (map %.9g, lambda %.9g, S %.3g)" % (
            tag, name, e.max(), x, y, bound, got[y, x], lam[y, x], S[y, x])
    return rows


# ================================================================================================ 3 corner lists (F5)
def candidates(eig, mask, quality=QUALITY, edit=None):
    """(ys, xs) of the pixels goodFeaturesToTrack may return: unmasked, interior, strictly above (float)(max over unmasked x quality),
    >= their eight neighbours (masked ones included, -inf outside the image)."""
    eig = np.asarray(eig, np.float32)
    h, w = eig.shape
    m = np.ones((h, w), bool) if mask is None else (np.asarray(mask) != 0)
    if not m.any():
        return np.zeros(0, int), np.zeros(0, int), np.float32(0)
    top = float(eig.max()) if edit == 'thr_unmasked_max' else float(eig[m].max())
    thr = np.float32(top * quality)
    src = np.where(m, eig, -np.inf) if edit == 'localmax_unmasked_only' else eig
    p = np.pad(src.astype(np.float64), 1, mode='constant', constant_values=-np.inf)
    nb = np.full((h, w), -np.inf)
    for a in range(3):
        for b in range(3):
            if (a, b) != (1, 1):
                nb = np.maximum(nb, p[a:a + h, b:b + w])
    c = m & (eig > thr) & (eig.astype(np.float64) >= nb)
    c[0, :] = c[-1, :] = False
    c[:, 0] = c[:, -1] = False
    ys, xs = np.nonzero(c)
    return ys, xs, thr


def _order(eig, ys, xs, edit=None):
    lin = ys * eig.shape[1] + xs
    return np.lexsort((lin if edit == 'ties_smaller_first' else -lin, -eig[ys, xs].astype(np.float64)))


def greedy_corners(eig, mask, max_corners, quality=QUALITY, min_dist=12.0, edit=None):
    """The list the definition implies (used for the LK tables and to produce the EDITED lists of the mutation test; the device's list is
    never compared with it, only judged by corner_violations)."""
    ys, xs, _ = candidates(eig, mask, quality, edit)
    order = _order(np.asarray(eig, np.float32), ys, xs, edit)
    out = []
    for k in order:
        x, y = int(xs[k]), int(ys[k])
        if min_dist >= 1 and out:
            d2 = (np.array(out)[:, 0] - x) ** 2 + (np.array(out)[:, 1] - y) ** 2
            if (d2 <= min_dist * min_dist).any() if edit == 'dist_le' else (d2 < min_dist * min_dist).any():
                continue
        out.append((x, y))
        if len(out) >= max_corners:
            break
    return np.array(out, np.float32).reshape(-1, 2)


def corner_violations(eig, mask, corners, max_corners, quality=QUALITY, min_dist=12.0):
    """What is wrong with `corners` as the goodFeaturesToTrack list of the map `eig`: a list of sentences, empty for a correct list."""
    eig = np.asarray(eig, np.float32)
    h, w = eig.shape
    bad = []
    c = np.asarray(corners)
    if len(c) > max_corners:
        bad.append("%d corners for max_corners %d" % (len(c), max_corners))
    if np.any(c != np.rint(c)):
        bad.append("non-integer coordinates")
    cx, cy = c[:, 0].astype(int), c[:, 1].astype(int)
    ys, xs, thr = candidates(eig, mask, quality)
    cand = set(zip(xs.tolist(), ys.tolist()))
    for x, y in zip(cx.tolist(), cy.tolist()):
        if (x, y) not in cand:
            bad.append("(%d, %d) is masked, on the border, not above the threshold %.6g or below a neighbour" % (x, y, thr))
    if len(set(zip(cx.tolist(), cy.tolist()))) != len(c):
        bad.append("a corner is listed twice")
    if bad:
        return bad
    v = eig[cy, cx].astype(np.float64)
    lin = cy * w + cx
    for i in range(len(c) - 1):
        if v[i] < v[i + 1] or (v[i] == v[i + 1] and lin[i] < lin[i + 1]):
            bad.append("order: corner %d (value %.9g, index %d) before corner %d (%.9g, %d)" % (i, v[i], lin[i], i + 1, v[i + 1], lin[i + 1]))
    md2 = float(min_dist) ** 2
    if min_dist >= 1 and len(c) > 1:
        d2 = (cx[:, None] - cx[None, :]) ** 2 + (cy[:, None] - cy[None, :]) ** 2
        d2 = d2 + np.eye(len(c)) * 1e18
        if (d2 < md2).any():
            i, j = np.unravel_index(int(np.argmin(d2)), d2.shape)
            bad.append("corners %d and %d are %.3f apart, min_dist %.3f" % (i, j, np.sqrt(d2[i, j]), min_dist))
    # maximality: every unselected candidate (of those that precede the last selected one, when the list is full) is blocked by a selected
    # corner that precedes it in the order (value descending, larger index first)
    sel = {(x, y): i for i, (x, y) in enumerate(zip(cx.tolist(), cy.tolist()))}
    full = len(c) >= max_corners
    order = _order(eig, ys, xs)
    n_before = 0
    for k in order:
        x, y = int(xs[k]), int(ys[k])
        if (x, y) in sel:
            n_before = sel[(x, y)] + 1
            if full and n_before == len(c):
                break
            continue
        blocked = min_dist >= 1 and n_before > 0 and bool((((cx[:n_before] - x) ** 2 + (cy[:n_before] - y) ** 2) < md2).any())
        if not blocked:
            bad.append("not maximal: candidate (%d, %d) value %.9g is unselected and no earlier corner lies within min_dist" % (x, y, eig[y, x]))
            if len(bad) > 5:
                break
    return bad


def _disc_mask_over_maximum(eig, radius):
    h, w = eig.shape
    y, x = np.unravel_index(int(np.argmax(eig)), eig.shape)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.full((h, w), 255, np.uint8)
    m[(xx - x) ** 2 + (yy - y) ** 2 <= radius * radius] = 0
    return m


def corner_cases():
    """name -> (image, mask builder or None, max_corners, min_dist).  The mask of 'masked_max' is built from the float64 map, so the case is
    the same on every library."""
    synth = _synth()
    a = (synth.synth_frame(11, 256, 160) // 2 + 64).astype(np.uint8)      # (half contrast: the texture's corners at a quarter)
    a[70:78, 120:128] = 255                 # one corner far above the rest of the texture: masking it moves the threshold
    a[78:86, 120:128] = 0
    a[70:78, 128:136] = 0
    a[78:86, 128:136] = 255
    mask_a = _disc_mask_over_maximum(mineig64(a)[0], 9)
    small = synth.synth_frame(14, 32, 32)
    return {
        'masked_max_md12': (a, mask_a, 400, 12.0),
        'masked_max_md7.5': (a, mask_a, 400, 7.5),
        'unmasked_md7.5_n7': (a, None, 7, 7.5),
        'unmasked_md12_n1': (a, None, 1, 12.0),
        'no_distance_md0.5': (small, None, 400, 0.5),
        'no_distance_md0.5_n7': (small, None, 7, 0.5),
        'tie_md12': (tie_image(), None, 400, 12.0),
        'tie_md3': (tie_image(), None, 400, 3.0),
        'empty_mask': (a, np.zeros(a.shape, np.uint8), 400, 12.0),
    }


def masked_threshold_ratio():
    img, mask, _, _ = corner_cases()['masked_max_md12']
    lam = mineig64(img)[0]
    return float(lam.max() / lam[mask != 0].max())


def check_corners(h, tag):
    fe = _fe()
    rows = {}
    for name, (img, mask, n, md) in corner_cases().items():
        H, W = img.shape
        tr = fe.FrontEnd(h, W, H, 1, 400)
        tr.push_frames([img])
        tr.keep_eig()
        got = tr.detect(0, n, QUALITY, md, mask)
        eig = tr.get_eig(0)
        bad = corner_violations(eig, mask, got, n, QUALITY, md)
        assert not bad, "%s corners %s: %s" % (tag, name, "; ".join(bad[:4]))
        ncand = len(candidates(eig, mask)[0])
        rows[name] = (len(got), ncand)
        if name == 'empty_mask':
            assert len(got) == 0
        elif name.endswith('_n7') or name.endswith('_n1'):
            assert len(got) == n < ncand, (tag, name, len(got), ncand)
        else:
            assert 0 < len(got) < n and ncand < n, (tag, name, len(got), ncand)            # more asked for than there are candidates
    return rows


# ================================================================================================ 4 LK (F2, F3)
def scharr64(img, edit=None):
    """(dx, dy) in grey levels per pixel: Scharr [3 10 3] x [-1 0 1] / 32, reflect-101 at the image edge."""
    p = _border(img, 1, edit)
    a, b, g = (1.0, 2.0, 8.0) if edit == 'sobel_for_scharr' else (0.0, 1.0, 2.0) if edit == 'central_for_scharr' else (3.0, 10.0, 32.0)
    up, mid, dn = p[:-2], p[1:-1], p[2:]
    sm = a * (up + dn) + b * mid
    df = dn - up
    return (sm[:, 2:] - sm[:, :-2]) / g, (a * (df[:, :-2] + df[:, 2:]) + b * df[:, 1:-1]) / g


class _Level:
    def __init__(self, I, J, win, edit):
        self.pad = win + 3
        self.H, self.W = I.shape
        self.I = _border(I, self.pad)                                    # the pyramid images carry a reflect-101 border ...
        self.J = _border(J, self.pad)
        dx, dy = scharr64(I, edit)
        self.dx, self.dy = np.pad(dx, self.pad), np.pad(dy, self.pad)    # ... the derivative a border of zeros


def _sample(P, pad, ox, oy, win):
    """win x win exact bilinear samples of the padded plane P at (ox + i, oy + j)."""
    ix, iy = int(np.floor(ox)), int(np.floor(oy))
    fx, fy = ox - ix, oy - iy
    q = P[iy + pad:iy + pad + win + 1, ix + pad:ix + pad + win + 1]
    return (q[:-1, :-1] * (1 - fx) + q[:-1, 1:] * fx) * (1 - fy) + (q[1:, :-1] * (1 - fx) + q[1:, 1:] * fx) * fy


def _gate(dIx, dIy, win):
    """(gate quantity, det, A): A = sum of outer products of the UN-NORMALISED (gain 32) derivative x 2^-20 (ASSUMPTIONS F3)."""
    a11, a12, a22 = (dIx * dIx).sum() / 1024.0, (dIx * dIy).sum() / 1024.0, (dIy * dIy).sum() / 1024.0
    q = (a11 + a22 - np.sqrt((a11 - a22) ** 2 + 4 * a12 * a12)) / (2.0 * win * win)
    return q, a11 * a22 - a12 * a12, (a11, a12, a22)


def _window(edit):
    win = 19 if edit == 'window_19' else 23 if edit == 'window_23' else WIN
    off = 10.5 if edit == 'origin_10p5' else (win - 1) / 2.0
    return win, off


def lk64(levels_i, levels_j, pts, edit=None, max_iter=200, tol=1e-9):
    """Pyramidal Lucas-Kanade in float64 on the given pyramid levels: window 21 x 21 with its origin at p - 10, exact bilinear sampling,
    Gauss-Newton with the template's Scharr gradient to |delta| < tol at EVERY level, the guess doubled from level to level; a level whose
    window origin lies outside [-21, W) x [-21, H) or whose gate fails is passed over (status 0 at level 0).
    Returns dict(xy, status, err, converged, gate): gate = the level-0 gate quantity (nan where the window was outside)."""
    win, off = _window(edit)
    nl = len(levels_i) - 1
    lv = [_Level(levels_i[l], levels_j[l], win, edit) for l in range(nl + 1)]
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    n = len(pts)
    xy, st, err = np.zeros((n, 2)), np.ones(n, np.uint8), np.zeros(n)
    conv, gate = np.ones(n, bool), np.full(n, np.nan)

    def outside(o, L):
        ix, iy = np.floor(o[0]), np.floor(o[1])
        return ix < -WIN or ix >= L.W or iy < -WIN or iy >= L.H

    for i in range(n):
        g = None
        for l in range(nl, -1, -1):
            L = lv[l]
            p = pts[i] / 2.0 ** l
            g = p.copy() if l == nl else (g if edit == 'guess_not_doubled' else 2.0 * g)
            o = p - off
            if outside(o, L):
                if l == 0:
                    st[i], err[i] = 0, 0
                continue
            Ip = _sample(L.I, L.pad, o[0], o[1], win)
            dIx, dIy = _sample(L.dx, L.pad, o[0], o[1], win), _sample(L.dy, L.pad, o[0], o[1], win)
            q, det, (a11, a12, a22) = _gate(dIx, dIy, win)
            if l == 0:
                gate[i] = q
            if q < GATE or det < FLT_EPS:
                if l == 0:
                    st[i] = 0
                continue
            for it in range(max_iter):
                og = g - off
                if outside(og, L):
                    if l == 0:
                        st[i] = 0
                    break
                diff = _sample(L.J, L.pad, og[0], og[1], win) - Ip
                b1, b2 = (diff * dIx).sum() / 1024.0, (diff * dIy).sum() / 1024.0
                d = np.array([(a12 * b2 - a22 * b1) / det, (a12 * b1 - a11 * b2) / det])
                g = g + d
                if d[0] * d[0] + d[1] * d[1] < tol * tol:
                    break
            else:
                conv[i] = False
            if l == 0 and st[i]:
                og = g - off
                if outside(og, L):
                    st[i] = 0
                else:
                    err[i] = np.abs(_sample(L.J, L.pad, og[0], og[1], win) - Ip).mean()
        xy[i] = g
    return dict(xy=xy, status=st, err=err, converged=conv, gate=gate)


def gate64(level0, pts, edit=None):
    """The level-0 gate quantity of every point (the frame tracked onto itself: status == (gate >= 1e-4))."""
    win, off = _window(edit)
    L = _Level(level0, level0, win, edit)
    out = np.zeros(len(pts))
    for i, p in enumerate(np.asarray(pts, np.float64)):
        o = p - off
        out[i] = _gate(_sample(L.dx, L.pad, o[0], o[1], win), _sample(L.dy, L.pad, o[0], o[1], win), win)[0]
    return out


# ---- 4a / 4d: noisy frames
def lk_noisy_tables():
    synth = _synth()
    out = {}
    for name, (s0, s1, shift, ang) in (('pair_11_12', (11, 12, (3.7, -2.2), 0.5)), ('pair_21_22', (21, 22, (-5.1, 4.4), -0.8))):
        a = synth.synth_frame(s0, 256, 160)
        b = synth.warp_frame(a, s1, shift=shift, angle_deg=ang)
        pts = greedy_corners(mineig64(a)[0].astype(np.float32), None, 64, QUALITY, 12.0)
        pts = pts[(pts[:, 0] > 14) & (pts[:, 0] < 241) & (pts[:, 1] > 14) & (pts[:, 1] < 145)]
        rng = np.random.default_rng(s0)
        pts = (pts + rng.uniform(-0.5, 0.5, pts.shape)).astype(np.float32)
        out[name] = (a, b, pts)
    return out


def lk_figures(ref, xy, st, err):
    """The 4a / 4d / 4e figures of a tracker's output against LK64's on the same levels."""
    judged = ref['converged'] & (ref['status'] == 1)
    both = judged & (st == 1)
    d = np.linalg.norm(np.asarray(xy, np.float64) - ref['xy'], axis=1)
    return dict(n=len(st), left_out=int((~judged).sum()), kept=int(both.sum()), lost=int((judged & (st == 0)).sum()),
                max=float(d[both].max()), median=float(np.median(d[both])), argmax=int(np.argmax(np.where(both, d, -1))),
                err=float(np.abs(np.asarray(err, np.float64) - ref['err'])[both].max()))


def device_levels(tr, w, h):
    nl = n_levels(w, h)
    return [tr.get_level(0, l, previous=True) for l in range(nl)], [tr.get_level(0, l) for l in range(nl)]


def check_lk_noisy(h, tag):
    fe = _fe()
    rows = {}
    for name, (a, b, pts) in lk_noisy_tables().items():
        assert len(pts) <= 64
        tr = fe.FrontEnd(h, 256, 160, 1, 64)
        tr.push_frames([a])
        tr.push_frames([b])
        li, lj = device_levels(tr, 256, 160)
        xy, st, err = tr.track(0, pts)
        ref = lk64(li, lj, pts)
        f = lk_figures(ref, xy, st, err)
        rows[name] = f
        bmax, bmed, berr = lk_bounds(name)
        assert f['left_out'] <= LEFT_OUT_CAP * f['n'], (tag, name, f)
        assert f['lost'] == 0, "%s LK %s: %d tracks lost that pass the gate and stay in the frame in float64" % (tag, name, f['lost'])
        i = f['argmax']
        assert f['max'] <= bmax, "%s LK %s: track %d at %s is %.5f px from LK64 %s, bound %.5f" % (tag, name, i, xy[i], f['max'], ref['xy'][i], bmax)
        assert f['median'] <= bmed, "%s LK %s: median distance to LK64 %.3e px, bound %.3e" % (tag, name, f['median'], bmed)
        assert f['err'] <= berr, "%s LK %s: err off by %.4f grey levels, bound %.4f" % (tag, name, f['err'], berr)
    return rows


# ---- 4b: analytic frames
ANALYTIC_SHIFTS = ((2.37, -1.61), (7.3, 5.2), (-11.45, 3.9), (0.0, 0.0))


def analytic_frame(shift=(0.0, 0.0), w=256, h=160):
    """Gaussian blobs + low-frequency sinusoids sampled at x - shift, rounded to u8 (no noise: the truth of the track is p + shift)."""
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xx, yy = xx - shift[0], yy - shift[1]
    f = 128.0 + 9.0 * np.sin(2 * np.pi * (xx / 83.0 + yy / 131.0)) + 7.0 * np.cos(2 * np.pi * (xx / 57.0 - yy / 71.0))
    for _ in range(90):
        cx, cy = rng.uniform(-10, w + 10), rng.uniform(-10, h + 10)
        sx, sy, th = rng.uniform(1.5, 4.5), rng.uniform(1.5, 4.5), rng.uniform(0, np.pi)
        amp = rng.uniform(25, 60) * rng.choice([-1.0, 1.0])
        u = np.cos(th) * (xx - cx) + np.sin(th) * (yy - cy)
        v = -np.sin(th) * (xx - cx) + np.cos(th) * (yy - cy)
        f += amp * np.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def analytic_points():
    a = analytic_frame()
    pts = greedy_corners(mineig64(a)[0].astype(np.float32), None, 64, QUALITY, 10.0)
    pts = pts[(pts[:, 0] > 25.5) & (pts[:, 0] < 256 - 26.5) & (pts[:, 1] > 25.5) & (pts[:, 1] < 160 - 26.5)]
    rng = np.random.default_rng(6)
    return a, (pts + rng.uniform(-0.5, 0.5, pts.shape)).astype(np.float32)


def check_lk_analytic(h, tag):
    fe = _fe()
    a, pts = analytic_points()
    assert 24 <= len(pts) <= 64
    bound = lk_truth_bound()
    rows = {}
    for shift in ANALYTIC_SHIFTS:
        b = analytic_frame(shift)
        tr = fe.FrontEnd(h, 256, 160, 1, 64)
        tr.push_frames([a])
        tr.push_frames([b])
        xy, st, err = tr.track(0, pts)
        assert st.all(), (tag, shift, st)
        if shift == (0.0, 0.0):
            assert np.array_equal(xy.view(np.uint32), pts.view(np.uint32)), "%s LK zero shift moved a point" % tag
            assert np.all(err == 0)
        d = np.linalg.norm(xy.astype(np.float64) - (pts.astype(np.float64) + np.array(shift)), axis=1)
        rows[shift] = float(d.max())
        assert d.max() <= bound, "%s LK analytic shift %s: track %d is %.4f px from the truth, bound %.4f" % (tag, shift, int(d.argmax()), d.max(), bound)
    return rows


# ---- 4c: the minimum-eigenvalue gate (the F2 test)
def gate_table():
    """A 256 x 160 frame of FINE texture (independent pixels: the band where [3 10 3] / 16 and [1 2 1] / 4 differ most) whose contrast
    ramps from nothing to a few grey levels, and 300 points on a 30 x 10 lattice (integer, half and odd fractions)."""
    rng = np.random.default_rng(17)
    h, w = 160, 256
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    contrast = 0.15 + 2.6 * (xx / w) + 0.5 * (yy / h)
    img = np.clip(np.rint(128.0 + contrast * rng.uniform(-1, 1, (h, w))), 0, 255).astype(np.uint8)
    gx, gy = np.meshgrid(12.0 + 8.0 * np.arange(30), 14.0 + 14.0 * np.arange(10))
    pts = np.c_[gx.ravel(), gy.ravel()]
    frac = rng.choice([0.0, 0.0, 0.5, 0.25, 0.37, 0.81], pts.shape)
    return img, (pts + frac).astype(np.float32)


def gate_judgement(q):
    """(expected status, judged): judged = farther than GATE_BAND (relative) from the threshold."""
    return (q >= GATE).astype(np.uint8), np.abs(q - GATE) > GATE_BAND * GATE


def check_lk_gate(h, tag):
    fe = _fe()
    img, pts = gate_table()
    tr = fe.FrontEnd(h, 256, 160, 1, 64)
    tr.push_frames([img])
    tr.push_frames([img])
    assert np.array_equal(tr.get_level(0, 0, previous=True), img)
    st = np.concatenate([tr.track(0, pts[k:k + 60])[1] for k in range(0, len(pts), 60)])
    q = gate64(img, pts)
    want, judged = gate_judgement(q)
    assert (~judged).sum() <= GATE_BAND_CAP * len(pts), (tag, int((~judged).sum()))
    wrong = judged & (st != want)
    assert not wrong.any(), "%s LK gate: %d of %d judged points disagree, e.g. point %d gate %.6e status %d" % (
        tag, wrong.sum(), judged.sum(), int(np.argmax(wrong)), q[np.argmax(wrong)], st[np.argmax(wrong)])
    return dict(judged=int(judged.sum()), passing=int(want.sum()), nearest=float(np.abs(q / GATE - 1).min()))


# ---- 4e: status at the frame's edge
def check_lk_status(h, tag):
    fe = _fe()
    a, b, _ = lk_noisy_tables()['pair_11_12']
    W, H = 256, 160
    outside = np.array([[-11.5, 80.0], [-40.0, 50.0], [W + 10.2, 80.0], [100.0, -11.25], [100.0, H + 10.5], [W + 30.0, H + 30.0]], np.float32)
    # origin still inside [-21, W) x [-21, H): windows that hang over the frame's edge (reflect-101 image, zero derivative out there)
    inside = np.array([[-10.9, 80.0], [W + 9.9, 80.0], [100.0, -10.75], [100.0, H + 9.75], [2.0, 3.0], [253.5, 157.2], [128.0, 1.0], [5.5, 150.0],
                       [0.0, 0.0], [255.0, 159.0], [120.25, 80.75]], np.float32)
    tr = fe.FrontEnd(h, W, H, 1, 64)
    tr.push_frames([a])
    tr.push_frames([b])
    li, lj = device_levels(tr, W, H)
    xy, st, err = tr.track(0, np.concatenate([outside, inside]))
    assert not st[:len(outside)].any() and np.all(err[:len(outside)] == 0), (tag, st, err)
    ref = lk64(li, lj, np.concatenate([outside, inside]))
    assert not ref['status'][:len(outside)].any()
    k = len(outside)
    sure = ref['converged'][k:] & (np.abs(ref['gate'][k:] - GATE) > GATE_BAND * GATE)
    stays = (ref['status'][k:] == 1) | (ref['gate'][k:] < GATE)               # (status 0 in float64 for another reason: it left the frame)
    assert np.array_equal(st[k:][sure & stays], ref['status'][k:][sure & stays]), (tag, st[k:], ref['status'][k:])
    assert st[k:][sure & stays].sum() >= 4 and (sure & stays).sum() >= 8, (tag, st[k:], sure, stays)
    return dict(status=st.tolist(), judged=int((sure & stays).sum()))


# ================================================================================================ 5 rejectWithF (F9)
def reject_with_f(h, p1, p2, threshold=1.0):
    """vg_fe_reject_with_f with every output: (status, n_inliers, F)."""
    import ctypes as C
    _fe().FrontEnd                                            # (argtypes are set by FrontEnd.__init__; set the one call used here)
    p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 2)
    p2 = np.ascontiguousarray(p2, np.float32).reshape(-1, 2)
    n = len(p1)
    st, Fm, ni = np.zeros(n, np.uint8), np.zeros(9), C.c_int(-1)
    f4, u8 = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    h.lib.vg_fe_reject_with_f.argtypes = [C.c_void_p, f4, f4, C.c_int, C.c_double, u8, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    h._chk(h.lib.vg_fe_reject_with_f(h.h, p1.ctypes.data_as(f4), p2.ctypes.data_as(f4), n, float(threshold), st.ctypes.data_as(u8),
                                     C.byref(ni), Fm.ctypes.data_as(C.POINTER(C.c_double))), "vg_fe_reject_with_f")
    return st, ni.value, Fm.reshape(3, 3)


def epipolar_d2(Fm, p1, p2):
    """max(d1^2, d2^2): squared distances of p2 to the line F p1 and of p1 to the line F^T p2, float64."""
    h1 = np.c_[np.asarray(p1, np.float64), np.ones(len(p1))]
    h2 = np.c_[np.asarray(p2, np.float64), np.ones(len(p2))]
    l2, l1 = h1 @ Fm.T, h2 @ Fm
    with np.errstate(divide='ignore', invalid='ignore'):
        d2 = (h2 * l2).sum(1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2)
        d1 = (h1 * l1).sum(1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2)
    return np.maximum(d1, d2)


def f_consistency(st, ni, Fm, p1, p2, threshold):
    """Sentences about what is inconsistent between (status, n_inliers, F); the number of points inside the band."""
    bad = []
    if ni != int(st.sum()):
        bad.append("n_inliers %d != sum(status) %d" % (ni, st.sum()))
    if Fm[2, 2] != 1.0:
        bad.append("F33 = %r" % Fm[2, 2])
    if not abs(np.linalg.det(Fm)) <= 1e-9 * np.abs(Fm).max() ** 3:
        bad.append("det F = %.3e, max|F| = %.3e" % (np.linalg.det(Fm), np.abs(Fm).max()))
    e, t2 = epipolar_d2(Fm, p1, p2), threshold * threshold
    judged = np.abs(e - t2) > F_BAND * t2
    wrong = judged & (st.astype(bool) != (e <= t2))
    if wrong.any():
        bad.append("%d points whose status contradicts F (e.g. point %d: error^2 %.6f, status %d)" % (wrong.sum(), int(np.argmax(wrong)), e[np.argmax(wrong)], st[np.argmax(wrong)]))
    return bad, int((~judged).sum())


def two_view(seed, n=120, n_out=25):
    """The scenes of tests/test_fe_oracle.py::_two_view: (p1, p2, is_outlier)."""
    from test_fe_oracle import _two_view
    return _two_view(seed, n=n, n_out=n_out)


def collinear_scene(n=40):
    """Every point of both views on one line: no admissible 7-point sample."""
    t = np.linspace(0.0, 1.0, n)
    p1 = np.c_[100 + 500 * t, 80 + 300 * t]
    p2 = np.c_[110 + 480 * t, 95 + 288 * t]
    return p1.astype(np.float32), p2.astype(np.float32)


def check_reject_with_f(h, tag, run=None):
    run = run or (lambda p1, p2, thr: reject_with_f(h, p1, p2, thr))
    rows = {}
    for seed in (3, 4, 5, 6, 7):
        p1, p2, out = two_view(seed, 120, 25)
        st, ni, Fm = run(p1, p2, 1.0)
        bad, band = f_consistency(st, ni, Fm, p1, p2, 1.0)
        assert not bad, "%s rejectWithF seed %d: %s" % (tag, seed, "; ".join(bad))
        assert band <= F_BAND_CAP * len(p1), (tag, seed, band)
        l = np.c_[p1[~out].astype(np.float64), np.ones((~out).sum())] @ Fm.T
        d = np.abs((np.c_[p2[~out].astype(np.float64), np.ones((~out).sum())] * l).sum(1)) / np.hypot(l[:, 0], l[:, 1])
        rows[seed] = (int(st[out].sum()), float(st[~out].mean()), float(np.median(d)))
        assert st[out].sum() <= 1, (tag, seed, rows[seed])
        assert st[~out].mean() > 0.9, (tag, seed, rows[seed])
        assert np.median(d) < 0.5, (tag, seed, rows[seed])
    for seed in (8, 9, 13):                                    # 14 points: LMedS (its inlier band is sigma, not the threshold)
        p1, p2, out = two_view(seed, 14, 2)
        st, ni, Fm = run(p1, p2, 1.0)
        assert ni == st.sum() and 7 <= st.sum() < 14 and Fm[2, 2] == 1.0, (tag, seed, st)
        assert abs(np.linalg.det(Fm)) <= 1e-9 * np.abs(Fm).max() ** 3, (tag, seed)
    p1, p2, out = two_view(12, 100, 0)
    st, ni, Fm = run(p1, p2, 1.0)
    bad, band = f_consistency(st, ni, Fm, p1, p2, 1.0)
    assert not bad and band <= F_BAND_CAP * 100, (tag, 'clean', bad, band)
    assert st.mean() > 0.85, (tag, 'clean', st.mean())
    rows['clean'] = float(st.mean())
    p1, p2 = collinear_scene()
    st, ni, Fm = run(p1, p2, 1.0)
    if st.all():
        assert ni == len(st)
        rows['collinear'] = 'no model: all ones'
    else:
        bad, band = f_consistency(st, ni, Fm, p1, p2, 1.0)
        assert not bad, "%s rejectWithF collinear: %s" % (tag, "; ".join(bad))
        rows['collinear'] = int(st.sum())
    return rows
