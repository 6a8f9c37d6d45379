"""vg_init_relpose (include/vinsgpu.h): scenes, reference, metric and the check bodies that tests/test_init_relpose_simt.py (emulated
kernels) and tests/test_init_relpose_gpu.py (MI355X) both run; tests/test_init_relpose_def.py runs the reference against itself.

REFERENCE
  correspondences and gate   a NumPy restatement of FeatureManager::getCorresponding and the gate of Estimator::relativePose; the
                             parallax sum by math.fsum (correctly rounded: any order of the positive terms lies within n 2^-53 of it)
  RANSAC                     oracle.fe_cpu.reject_with_f(ll, rr, 0.3 / 460) for the mask and the model; the oracle does not return the
                             winning iteration and the bound, so `ransac_replay` replays them: the sample schedule of cv::RNG((uint64)-1)
                             with OpenCV's redraws, run7Point with numpy.linalg.svd for the null space, the bookkeeping
  pose stage                 `pose()`, a restatement of decomposeEssentialMat / recoverPose as the header defines them, taking THE DEVICE'S
                             OWN F TAP: route 'ld' (numpy.longdouble, the Jacobi SVDs of the header), 'jac64' (the same in float64) and
                             'svd64' (numpy.linalg.svd for the 3x3 matrix and for the 6x4 design matrices).  The disagreement of the two
                             float64 routes with 'ld' is the floor E64; relative_R / relative_T are held to M = 4 x E64.
A LAPACK SVD may name R1 what the header's convention names R2: the svd64 route is compared by the winner's pose, not by its index.

CONDITIONS the table's scenes meet (`conditions`, asserted by test_init_relpose_def.py and again on the device's taps): no correspondence
of a gated candidate has an epipolar error within 1e-6 relative of the threshold; no gate value within 1e-9 relative of 30; the winner's
count strictly exceeds the other three; inlier_cnt is not 12 or 13 unless the case is about that."""
import ctypes as C
import functools
import math
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import fe_cpu  # noqa: E402

LD = np.longdouble
M = 4.0
OK, NONE, NUMERIC = 0, 1, 2
THRESH = 0.3 / 460
FOCAL, GATE, MIN_CORRES, MIN_INLIERS, DIST = 460.0, 30.0, 20, 12, 50.0
MAXIT = 1000
RP_CHUNK0 = 63                  # csrc/init_relpose.h: the iterations of the first part of the chunked launch
PX = 1.0 / 460.0


# --------------------------------------------------------------------------------------------------- correspondences and gate
def corres(win, i):
    """getCorresponding(i, F - 1): [(x y at i), (x y at F-1)] in feature order, in double"""
    F = int(win['n_frames'])
    start, nobs = np.asarray(win['start']), np.asarray(win['nobs'])
    off = np.concatenate([[0], np.cumsum(nobs)[:-1]]) if win.get('obs_off') is None else np.asarray(win['obs_off'])
    pts = np.asarray(win['points'], np.float64).reshape(-1, 3)
    a, b = [], []
    for j in range(len(start)):
        if start[j] <= i and start[j] + nobs[j] - 1 >= F - 1:
            a.append(pts[off[j] + i - start[j], :2])
            b.append(pts[off[j] + F - 1 - start[j], :2])
    return np.array(a, np.float64).reshape(-1, 2), np.array(b, np.float64).reshape(-1, 2)


def gate(a, b):
    """(n_corres, average_parallax, gate value, gate)"""
    n = len(a)
    if n == 0:
        return 0, 0.0, 0.0, False
    d = a - b
    avg = math.fsum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])) / n
    return n, avg, avg * FOCAL, n > MIN_CORRES and avg * FOCAL > GATE


# --------------------------------------------------------------------------------------------------- the RANSAC replay
class CvRng:
    def __init__(self, s):
        self.state = s if s else 0xffffffff

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + (self.state >> 32)) & 0xffffffffffffffff
        return self.state & 0xffffffff

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


def _last_collinear(p, idx):
    """haveCollinearPoints: the last point of the sample against every pair of earlier ones (double, as written)"""
    q = p[idx].astype(np.float64)
    d = q[:-1] - q[-1]
    for j in range(len(d)):
        for k in range(j):
            if abs(d[k, 0] * d[j, 1] - d[k, 1] * d[j, 0]) <= 1.1920928955078125e-07 * (abs(d[j, 0]) + abs(d[j, 1]) + abs(d[k, 0]) + abs(d[k, 1])):
                return True
    return False


def _get_subset(rng, p1, p2, n, max_attempts=10000):
    """PointSetRegistrator::getSubset; p1 is None: the part of the schedule that depends on n alone"""
    iters = 0
    while iters < max_attempts:
        idx = []
        while len(idx) < 7:
            c = rng.uniform(0, n)
            if c not in idx:
                idx.append(c)
        if p1 is not None and (_last_collinear(p1, idx) or _last_collinear(p2, idx)):
            iters += 1
            continue
        return idx
    return None


def schedule_needs_fallback(p1, p2):
    """does any of the 1000 samples of the n-only schedule hold a last point collinear with two earlier ones (all samples at once)"""
    S = np.array(n_only_schedule(len(p1), MAXIT))
    for p in (p1, p2):
        q = np.asarray(p, np.float64)[S]                        # [MAXIT, 7, 2]
        d = q[:, :6] - q[:, 6:7]
        for j in range(6):
            for k in range(j):
                cross = np.abs(d[:, k, 0] * d[:, j, 1] - d[:, k, 1] * d[:, j, 0])
                if np.any(cross <= 1.1920928955078125e-07 * (np.abs(d[:, j, 0]) + np.abs(d[:, j, 1]) + np.abs(d[:, k, 0]) + np.abs(d[:, k, 1]))):
                    return True
    return False


def n_only_schedule(n, count):
    rng = CvRng(0xffffffffffffffff)
    return [_get_subset(rng, None, None, n) for _ in range(count)]


def _update_num_iters(p, ep, model_points, max_iters):
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num, denom = max(1.0 - p, sys.float_info.min), 1.0 - (1.0 - ep) ** model_points
    if denom < sys.float_info.min:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(round(num / denom))


def _solve_cubic(cf):
    a0, a1, a2, a3 = cf
    if a0 == 0:
        if a1 == 0:
            return [] if a2 == 0 else [-a3 / a2]
        d = a2 * a2 - 4 * a1 * a3
        if d < 0:
            return []
        d = math.sqrt(d)
        q1, q2 = (-a2 + d) * 0.5, (a2 + d) * -0.5
        r = [q1 / a1, a3 / q1] if abs(q1) > abs(q2) else [q2 / a1, a3 / q2]
        return r if d > 0 else r[:1]
    a0 = 1.0 / a0
    a1, a2, a3 = a1 * a0, a2 * a0, a3 * a0
    Q, R = (a1 * a1 - 3 * a2) / 9, (2 * a1 * a1 * a1 - 9 * a1 * a2 + 27 * a3) / 54
    Qc = Q * Q * Q
    d = Qc - R * R
    if d >= 0:
        th, sq = math.acos(max(-1.0, min(1.0, R / math.sqrt(Qc)))) if Qc > 0 else 0.0, math.sqrt(Q)
        return [-2 * sq * math.cos((th + k * 2 * math.pi) / 3) - a1 / 3 for k in range(3)]
    d = math.sqrt(-d)
    e = (d + abs(R)) ** (1.0 / 3)
    if R > 0:
        e = -e
    return [(e + Q / e) - a1 / 3]


def _det3(m):
    return float(np.linalg.det(m.reshape(3, 3)))


def _seven_point(p1, p2, idx):
    """run7Point: the up-to-three models of the sample, F33 = 1"""
    a, b = p1[idx].astype(np.float64), p2[idx].astype(np.float64)
    A = np.stack([b[:, 0] * a[:, 0], b[:, 0] * a[:, 1], b[:, 0], b[:, 1] * a[:, 0], b[:, 1] * a[:, 1], b[:, 1], a[:, 0], a[:, 1], np.ones(7)], 1)
    vt = np.linalg.svd(A)[2]
    f2, f1 = vt[8], vt[7] - vt[8]
    # det(lambda f1 + f2) as a cubic in lambda, by interpolation-free expansion: coefficients from four determinants
    c3 = _det3(f2)
    c0 = _det3(f1)
    dp, dm = _det3(f1 + f2), _det3(f2 - f1)
    c2s = (dp + dm) / 2 - c3                                    # coefficient of lambda^2
    c1s = (dp - dm) / 2 - c0                                    # coefficient of lambda
    out = []
    for r in _solve_cubic([c0, c2s, c1s, c3]):
        sc = f1[8] * r + f2[8]
        lam, mu, f33 = r, 1.0, 0.0
        if abs(sc) > 2.220446049250313e-16:
            mu = 1.0 / sc
            lam, f33 = lam * mu, 1.0
        Fm = f1 * lam + f2 * mu
        Fm[8] = f33
        if np.all(np.isfinite(Fm)):
            out.append(Fm)
    return out


def epipolar_error(Fm, p1, p2):
    """FMEstimatorCallback::computeError, float32 as OpenCV stores it"""
    f = np.asarray(Fm, np.float64).reshape(-1)
    x1, y1, x2, y2 = (p1[:, 0].astype(np.float64), p1[:, 1].astype(np.float64), p2[:, 0].astype(np.float64), p2[:, 1].astype(np.float64))
    a, b, c = f[0] * x1 + f[1] * y1 + f[2], f[3] * x1 + f[4] * y1 + f[5], f[6] * x1 + f[7] * y1 + f[8]
    s2, d2 = 1.0 / (a * a + b * b), x2 * a + y2 * b + c
    a, b, c = f[0] * x2 + f[3] * y2 + f[6], f[1] * x2 + f[4] * y2 + f[7], f[2] * x2 + f[5] * y2 + f[8]
    s1, d1 = 1.0 / (a * a + b * b), x1 * a + y1 * b + c
    return np.maximum(d1 * d1 * s1, d2 * d2 * s2)


def _model_before(Fa, Fb):
    va, vb = Fa / Fa[np.argmax(np.abs(Fa))], Fb / Fb[np.argmax(np.abs(Fb))]
    for x, y in zip(va, vb):
        if abs(x - y) > 1e-6:
            return x < y
    return False


def ransac_replay(p1, p2, thresh=THRESH):
    """(winning iteration, final bound, inliers, F, the last iteration the loop looked at) of the registrator's loop over the EXACT schedule"""
    n, t2 = len(p1), np.float32(thresh * thresh)
    rng = CvRng(0xffffffffffffffff)
    niters, max_good, best, bestF, it = MAXIT, 0, -1, None, 0
    while it < niters:
        idx = _get_subset(rng, p1, p2, n)
        if idx is None:
            break
        top = None
        for Fm in _seven_point(p1, p2, idx):
            good = int(np.count_nonzero(epipolar_error(Fm, p1, p2).astype(np.float32) <= t2))
            if top is None or good > top[0] or (good == top[0] and _model_before(Fm, top[1])):
                top = (good, Fm)
        if top is not None and top[0] > max(max_good, 6):
            best, max_good, bestF = it, top[0], top[1]
            niters = _update_num_iters(0.99, (n - top[0]) / n, 7, niters)
        it += 1
    return best, niters, max_good, bestF, it - 1


# --------------------------------------------------------------------------------------------------- the pose stage
def _jacobi_cols(A, V, tol, signal_rule, sweeps=40):
    """one-sided Jacobi over the columns of a batch A [N, m, k], V [N, k, k] in place; returns the per-item convergence flags"""
    N, m, k = A.shape
    dt = A.dtype.type
    signal = dt(1e-26) * (A * A).reshape(N, -1).sum(1) if signal_rule else None
    conv = np.zeros(N, bool)
    for _ in range(sweeps):
        rotated = np.zeros(N, bool)
        for p in range(k - 1):
            for q in range(p + 1, k):
                al, be, ga = np.zeros(N, A.dtype), np.zeros(N, A.dtype), np.zeros(N, A.dtype)
                for r in range(m):
                    x, y = A[:, r, p], A[:, r, q]
                    al, be, ga = al + x * x, be + y * y, ga + x * y
                rot = (np.abs(ga) > dt(tol) * np.sqrt(al * be)) & (ga != 0) & ~conv
                if not rot.any():
                    continue
                rotated |= rot & ((al > signal) & (be > signal) if signal_rule else True)
                g = np.where(rot, ga, dt(1))
                zeta = (be - al) / (dt(2) * g)
                tn = np.where(zeta >= 0, dt(1), dt(-1)) / (np.abs(zeta) + np.sqrt(dt(1) + zeta * zeta))
                cs = dt(1) / np.sqrt(dt(1) + tn * tn)
                sn = cs * tn
                cs, sn = np.where(rot, cs, dt(1)), np.where(rot, sn, dt(0))
                for Mx in (A, V):
                    x, y = Mx[:, :, p].copy(), Mx[:, :, q].copy()
                    Mx[:, :, p] = cs[:, None] * x - sn[:, None] * y
                    Mx[:, :, q] = sn[:, None] * x + cs[:, None] * y
        conv |= ~rotated
        if conv.all():
            break
    return conv


def decompose(E, dtype, route):
    """(R1, R2, t, converged) of decomposeEssentialMat"""
    E = np.asarray(E, dtype).reshape(3, 3)
    if route == 'svd':
        U, _, Vt = np.linalg.svd(E.astype(np.float64))
        if np.linalg.det(U) < 0:
            U = -U
        if np.linalg.det(Vt) < 0:
            Vt = -Vt
        Wm = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float64)
        return U @ Wm @ Vt, U @ Wm.T @ Vt, U[:, 2].copy(), True
    A, V = E.copy()[None], np.eye(3, dtype=dtype)[None]
    conv = bool(_jacobi_cols(A, V, 1e-15, True)[0])
    A, V = A[0], V[0]
    s = [A[0, c] * A[0, c] + A[1, c] * A[1, c] + A[2, c] * A[2, c] for c in range(3)]
    order = [0, 1, 2]
    for a in (0, 1, 0):                                         # descending, stable: three compare-exchanges
        if s[order[a + 1]] > s[order[a]]:
            order[a], order[a + 1] = order[a + 1], order[a]
    o0, o1, o2 = order
    u0, u1 = A[:, o0] / np.sqrt(s[o0]), A[:, o1] / np.sqrt(s[o1])
    u2 = np.array([u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]], dtype)
    v0, v1, v2 = V[:, o0], V[:, o1], V[:, o2]
    det = v0[0] * (v1[1] * v2[2] - v1[2] * v2[1]) + v0[1] * (v1[2] * v2[0] - v1[0] * v2[2]) + v0[2] * (v1[0] * v2[1] - v1[1] * v2[0])
    if det < 0:
        v0, v1, v2 = -v0, -v1, -v2
    R1, R2 = np.zeros((3, 3), dtype), np.zeros((3, 3), dtype)
    for r in range(3):
        for c in range(3):
            R1[r, c] = -u1[r] * v0[c] + u0[r] * v1[c] + u2[r] * v2[c]
            R2[r, c] = u1[r] * v0[c] - u0[r] * v1[c] + u2[r] * v2[c]
    return R1, R2, u2, conv


def _triangulate(R, t, ll, rr, dtype, route):
    """Q [n, 4]: per point the right singular vector of the smallest singular value of the 6x4 design matrix"""
    n = len(ll)
    x0, y0, x1, y1 = (ll[:, 0].astype(dtype), ll[:, 1].astype(dtype), rr[:, 0].astype(dtype), rr[:, 1].astype(dtype))
    P = np.concatenate([np.asarray(R, dtype), np.asarray(t, dtype).reshape(3, 1)], 1)
    A = np.zeros((n, 6, 4), dtype)
    A[:, 0, 0], A[:, 0, 2] = -1, x0
    A[:, 1, 1], A[:, 1, 2] = -1, y0
    A[:, 2, 0], A[:, 2, 1] = -y0, x0
    for c in range(4):
        A[:, 3, c] = x1 * P[2, c] - P[0, c]
        A[:, 4, c] = y1 * P[2, c] - P[1, c]
        A[:, 5, c] = x1 * P[1, c] - y1 * P[0, c]
    if route == 'svd':
        return np.linalg.svd(A.astype(np.float64))[2][:, 3, :]
    V = np.tile(np.eye(4, dtype=dtype), (n, 1, 1))
    _jacobi_cols(A, V, 1e-16, False)
    s2 = np.zeros((n, 4), dtype)
    for r in range(6):
        s2 = s2 + A[:, r, :] * A[:, r, :]
    bi = np.zeros(n, int)
    best = s2[:, 0].copy()
    for c in range(1, 4):
        less = s2[:, c] < best
        bi[less], best[less] = c, s2[less, c]
    return V[np.arange(n), :, bi]


def pose(Fm, ll, rr, rmask, dtype=LD, route='jacobi', dist=DIST):
    """recoverPose + the tail of solveRelativeRT: dict(good [4], winner, inlier_cnt, mask, R, T, conv)"""
    R1, R2, t, conv = decompose(Fm, dtype, route)
    cands = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    masks = []
    with np.errstate(all='ignore'):
        for R, tt in cands:
            Q = _triangulate(R, tt, ll, rr, dtype, route).astype(dtype)
            m = Q[:, 2] * Q[:, 3] > 0
            X, Y, Z, Wq = Q[:, 0] / Q[:, 3], Q[:, 1] / Q[:, 3], Q[:, 2] / Q[:, 3], Q[:, 3] / Q[:, 3]
            m = (Z < dist) & m
            z1 = R[2, 0] * X + R[2, 1] * Y + R[2, 2] * Z + tt[2] * Wq
            m = (z1 > 0) & m
            m = (z1 < dist) & m
            masks.append(m & (np.asarray(rmask) != 0))
    good = [int(np.count_nonzero(m)) for m in masks]
    if good[0] >= good[1] and good[0] >= good[2] and good[0] >= good[3]:
        win = 0
    elif good[1] >= good[0] and good[1] >= good[2] and good[1] >= good[3]:
        win = 1
    elif good[2] >= good[0] and good[2] >= good[1] and good[2] >= good[3]:
        win = 2
    else:
        win = 3
    R, tt = cands[win]
    R, tt = np.asarray(R, dtype), np.asarray(tt, dtype)
    return dict(good=good, winner=win, inlier_cnt=good[win], mask=masks[win].astype(np.uint8), R=R.T.copy(), T=-(R.T @ tt), conv=conv)


# --------------------------------------------------------------------------------------------------- the whole call, sequentially
def candidate(win, i, F_tap=None, with_replay=True):
    """every tap of candidate i; F_tap: the model to run the pose stage on (None: the oracle's)"""
    a, b = corres(win, i)
    n, avg, gv, g = gate(a, b)
    out = dict(n_corres=n, avg_parallax=avg, gate_value=gv, gate=int(g))
    if not g:
        return out
    ll, rr = a.astype(np.float32), b.astype(np.float32)
    st, Fm = fe_cpu.reject_with_f(ll, rr, THRESH)
    out.update(ll=ll, rr=rr, ransac_mask=st, ransac_inliers=int(st.sum()), F=Fm)
    if with_replay:
        best, bound, cnt, _, last = ransac_replay(ll, rr)
        out.update(ransac_iter=last, ransac_best=best, ransac_bound=bound, replay_inliers=cnt)
    out['err'] = epipolar_error(Fm, ll, rr)
    p = pose(Fm if F_tap is None else F_tap, ll, rr, st)
    out.update(good=p['good'], winner=p['winner'], inlier_cnt=p['inlier_cnt'], mask=p['mask'], R=p['R'], T=p['T'], conv=p['conv'],
               success=p['inlier_cnt'] > MIN_INLIERS)
    return out


def pick(cand):
    """(status, l) of the walk over the candidates in ascending order: the first gated one that succeeded; a gated candidate whose 3x3 SVD
    did not converge, met before a success, ends the window with NUMERIC"""
    for i, c in enumerate(cand):
        if not c['gate']:
            continue
        if not c.get('conv', True):
            return NUMERIC, -1
        if c['success']:
            return OK, i
    return NONE, -1


def relative_pose(win, F_taps=None, with_replay=True):
    """Estimator::relativePose with every gated candidate computed: dict(status, l, R, T, cand [F-1])"""
    F = int(win['n_frames'])
    cand = [candidate(win, i, None if F_taps is None else F_taps[i], with_replay) for i in range(F - 1)]
    status, l = pick(cand)
    return dict(status=status, l=l, R=cand[l]['R'] if l >= 0 else np.zeros((3, 3)), T=cand[l]['T'] if l >= 0 else np.zeros(3), cand=cand)


def conditions(ref, allow_12_13=False):
    """the conditions of the module docstring on a result of relative_pose(); returns the list of violations"""
    bad = []
    for i, c in enumerate(ref['cand']):
        if c['n_corres'] and abs(c['gate_value'] - GATE) <= 1e-9 * GATE:
            bad.append(f"candidate {i}: gate value {c['gate_value']!r} at the gate")
        if not c['gate']:
            continue
        t2 = THRESH * THRESH
        if np.any(np.abs(c['err'] - t2) <= 1e-6 * t2):
            bad.append(f"candidate {i}: an epipolar error at the threshold")
        g = sorted(c['good'])
        if g[3] == g[2] and g[3] > 0:
            bad.append(f"candidate {i}: the winner's count {g[3]} is not strictly the largest")
        if c['inlier_cnt'] in (12, 13) and not allow_12_13:
            bad.append(f"candidate {i}: inlier_cnt {c['inlier_cnt']}")
    return bad


# --------------------------------------------------------------------------------------------------- the scenes
def _rot(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def scene(seed, F=11, tracks=None, n_feat=150, xs=None, depth=(4.0, 8.0), noise=0.05, outlier=0.0, deep=0, deep_z=(60.0, 90.0), spoil=None,
          collinear=None):
    """The window dict of ba.Handle.init_relpose.  xs: the camera's x position per frame (default 0.12 per frame); noise: pixels; outlier:
    share of the features whose observation in F-1 is displaced by 20 .. 60 pixels; deep: that many features (the first ones) lie at
    deep_z; spoil: (frame, count): the observation in that frame of the first `count` features that live through the window is displaced;
    collinear: (candidate, iteration): the last point of that sample of the candidate's n-only schedule is put on the line of its
    first two, in the candidate's frame, on a grid that float32 holds exactly."""
    rng = np.random.default_rng(seed)
    xs = [0.12 * i for i in range(F)] if xs is None else list(xs)
    pos = [np.array([xs[i], 0.03 * math.sin(0.9 * i + seed), 0.02 * math.cos(0.7 * i)]) for i in range(F)]
    Rw = [_rot(rng.normal(0, 0.008, 3)) for _ in range(F)]
    if tracks is None:
        tracks = []
        for _ in range(n_feat):
            u = rng.random()
            if u < 0.08:
                tracks.append((int(rng.integers(0, F)), 1))
            elif u < 0.5 or F < 4:
                tracks.append((0, F))
            elif u < 0.8:
                s0 = int(rng.integers(1, F - 1))
                tracks.append((s0, F - s0))
            else:
                tracks.append((0, int(rng.integers(2, F))))
    tracks = list(tracks)
    n = len(tracks)
    points, Xs = [], []
    mid = pos[F // 2]
    for j, (s0, k) in enumerate(tracks):
        z = rng.uniform(*(deep_z if j < deep else depth))
        X = mid + np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z])
        Xs.append(X)
        out = rng.random() < outlier
        for f in range(s0, s0 + k):
            p = Rw[f].T @ (X - pos[f])
            x, y = p[0] / p[2] + rng.normal(0, noise) * PX, p[1] / p[2] + rng.normal(0, noise) * PX
            if out and f == F - 1:
                ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(20, 60) * PX
                x, y = x + r * math.cos(ang), y + r * math.sin(ang)
            points.append([x, y, 1.0])
    points = np.array(points).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum([k for _, k in tracks])[:-1]]).astype(int)
    if spoil is not None:
        fr, cnt = spoil
        whole = [j for j, (s0, k) in enumerate(tracks) if s0 == 0 and k == F][:cnt]
        assert len(whole) == cnt
        for j in whole:
            ang, r = rng.uniform(0, 2 * np.pi), rng.uniform(25, 70) * PX
            points[off[j] + fr, 0] += r * math.cos(ang)
            points[off[j] + fr, 1] += r * math.sin(ang)
    win = dict(n_frames=F, start=np.array([t[0] for t in tracks]), nobs=np.array([t[1] for t in tracks]), points=points,
               feature_id=np.arange(100, 100 + n), truth=dict(pos=pos, R=Rw))
    if collinear is not None:
        i, it = collinear
        members = [j for j, (s0, k) in enumerate(tracks) if s0 <= i and s0 + k - 1 >= F - 1]
        idx = n_only_schedule(len(members), it + 1)[it]
        g = 4096.0                                              # the grid: 1/4096 (0.11 pixels), coordinates below 1 keep 12 more bits in float32
        ja, jb, jc = members[idx[0]], members[idx[1]], members[idx[6]]
        ra, rb, rc = (off[j] + i - tracks[j][0] for j in (ja, jb, jc))
        points[ra, :2] = np.round(points[ra, :2] * g) / g
        points[rb, :2] = np.round(points[rb, :2] * g) / g
        points[rc, :2] = 2 * points[rb, :2] - points[ra, :2]
    return win


def _whole(n, F):
    return [(0, F)] * n


# name -> scene arguments (the issue's list; the comment names what the case is about)
CASE_ARGS = {
    'F3_two': dict(seed=1, F=3, n_feat=60, xs=[0.0, 0.5, 1.0]),                                  # F = 3: two candidates, the first wins
    'F11_first': dict(seed=2, F=11, n_feat=150),                                                 # the reference's shape; candidate 0 wins
    'F16': dict(seed=3, F=16, n_feat=200, xs=[0.1 * i for i in range(16)]),                      # the capacity in frames
    'n20_refused': dict(seed=4, F=4, tracks=_whole(20, 4) + [(1, 3)] * 10, xs=[0.0, 0.4, 0.8, 1.2]),   # 20 pairs: candidate 0 is not gated, 1 wins with 30
    'n21_runs': dict(seed=5, F=4, tracks=_whole(21, 4), xs=[0.0, 0.4, 0.8, 1.2]),                # 21: the smallest that runs
    'n64': dict(seed=6, F=4, tracks=_whole(64, 4), xs=[0.0, 0.4, 0.8, 1.2]),                     # one full ballot word
    'n65': dict(seed=7, F=4, tracks=_whole(65, 4), xs=[0.0, 0.4, 0.8, 1.2]),                     # one bit into the second word
    'late_gate': dict(seed=8, F=8, n_feat=120, xs=[1.30, 1.31, 1.29, 1.30, 0.0, 0.3, 0.6, 1.3]),  # 0 .. 3 fail the parallax gate, 4 wins
    'few_inliers': dict(seed=9, F=5, tracks=_whole(21, 5) + [(1, 4)] * 40 + [(2, 1), (0, 3), (3, 2)], xs=[0.0, 0.3, 0.6, 0.9, 1.2], spoil=(0, 9)),
    #                ^ candidate 0: 21 pairs of which 12 are consistent -> inlier_cnt <= 12, candidate 1 wins; and features that start
    #                  after i, end before F-1 or have one observation
    'none': dict(seed=10, F=5, n_feat=80, xs=[0.0, 0.01, 0.02, 0.03, 0.04]),                     # no candidate passes: VG_RELPOSE_NONE
    'deep': dict(seed=11, F=5, tracks=_whole(70, 5), xs=[0.0, 0.25, 0.5, 0.75, 1.0], deep=15, depth=(3.0, 6.0)),   # deeper than 50 baselines: dropped
    'outliers30': dict(seed=12, F=4, n_feat=150, xs=[0.0, 0.4, 0.8, 1.2], outlier=0.3),          # the bound stays in the hundreds: part 2 runs
    'collinear': dict(seed=13, F=4, tracks=_whole(48, 4), xs=[0.0, 0.4, 0.8, 1.2], collinear=(0, 0)),   # the exact schedule from the host
}
ALLOW_12_13 = ('few_inliers',)


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(**CASE_ARGS[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    return relative_pose(case(name))


@functools.lru_cache(maxsize=None)
def capacity_scene():
    """F = 16 with VG_SFM_MAX_FEATURES features that all live through the window: 1024 correspondences for every candidate"""
    return scene(20, F=16, tracks=_whole(1024, 16), xs=[0.1 * i for i in range(16)])


# --------------------------------------------------------------------------------------------------- the metric
def pose_errors(got_R, got_T, cand, F_tap):
    """(error of relative_R, of relative_T against the 80-bit route on F_tap, E64 of both): max |d| (both are of unit scale)"""
    ld = pose(F_tap, cand['ll'], cand['rr'], cand['ransac_mask'], LD, 'jacobi')
    e64 = [0.0, 0.0]
    for route in ('jacobi', 'svd'):
        r = pose(F_tap, cand['ll'], cand['rr'], cand['ransac_mask'], np.float64, route)
        assert r['inlier_cnt'] == ld['inlier_cnt'], "the float64 routes agree with the 80-bit one on the count"
        e64[0] = max(e64[0], float(np.abs(r['R'].astype(LD) - ld['R']).max()))
        e64[1] = max(e64[1], float(np.abs(r['T'].astype(LD) - ld['T']).max()))
    assert max(e64) <= E64_CEILING, ("E64 above its ceiling", e64)
    eR = float(np.abs(np.asarray(got_R, LD) - ld['R']).max())
    eT = float(np.abs(np.asarray(got_T, LD) - ld['T']).max())
    return eR, eT, e64[0], e64[1], ld


E64_FLOOR = 2.0 ** -52          # one rounding of a unit-scale number: the least two float64 evaluations of R or T may differ by
# What E64 itself may reach, so that a degraded Jacobi cannot hide behind its own float64 restatement.  R and T are of unit scale; an entry
# of R = U W Vt is a sum of three products of entries that each carry the roundings of the rotations that touched their column (two per
# sweep, under ten sweeps on a 3x3 matrix: ~20 x 2^-53 each, two factors per product) plus the sum's own three: ~45 x 2^-53, taken as 32 x
# 2^-52 = 7.1e-15.  It comes from this count, not from what the routes were seen to give (they give 1e-16 .. 6e-16).
E64_CEILING = 32 * 2.0 ** -52


# --------------------------------------------------------------------------------------------------- the device checks
# one body for the emulator (tests/test_init_relpose_simt.py) and the MI355X (tests/test_init_relpose_gpu.py); h: a ba.Handle
TAPS = ('n_corres', 'avg_parallax', 'gate', 'ransac_iter', 'ransac_bound', 'ransac_inliers', 'ransac_best', 'F', 'good', 'winner', 'inlier_cnt', 'used_fallback')


def same_output(a, b):
    """two results of Handle.init_relpose, bit for bit"""
    return (a['status'] == b['status'] and a['l'] == b['l'] and
            all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in TAPS + ('relative_R', 'relative_T', 'mask', 'ransac_mask')))


def check_window(name, win, g, ref, tag, allow_12_13=False):
    """one window's result against the reference; returns the worst value ratio (0 when there is no pose)"""
    F = int(win['n_frames'])
    assert (g['status'], g['l']) == (ref['status'], ref['l']), (name, g['status'], g['l'], ref['status'], ref['l'])
    worst = 0.0
    for i in range(F - 1):
        c = ref['cand'][i]
        assert g['n_corres'][i] == c['n_corres'] and g['gate'][i] == c['gate'], (name, i)
        if c['n_corres']:
            rel = abs(g['avg_parallax'][i] - c['avg_parallax']) / c['avg_parallax']
            assert rel <= c['n_corres'] * 2.0 ** -53, (name, i, rel)
        if not c['gate']:
            for k in TAPS[3:]:
                assert not np.asarray(g[k][i]).any(), (name, i, k)
            continue
        assert g['ransac_inliers'][i] == c['ransac_inliers'], (name, i, g['ransac_inliers'][i], c['ransac_inliers'])
        got_it, ref_it = (g['ransac_iter'][i], g['ransac_best'][i], g['ransac_bound'][i]), (c['ransac_iter'], c['ransac_best'], c['ransac_bound'])
        assert got_it == ref_it, (name, i, got_it, ref_it)
        assert c['replay_inliers'] == c['ransac_inliers'], (name, i)
        Fd = np.asarray(g['F'][i], np.float64)
        assert np.abs(Fd - c['F']).max() <= 1e-6 * np.abs(c['F']).max(), (name, i, np.abs(Fd - c['F']).max())
        ld = pose(Fd, c['ll'], c['rr'], c['ransac_mask'], LD, 'jacobi')
        assert list(g['good'][i]) == ld['good'] and g['winner'][i] == ld['winner'] and g['inlier_cnt'][i] == ld['inlier_cnt'], \
            (name, i, list(g['good'][i]), ld['good'], g['winner'][i], ld['winner'])
        assert ld['conv'], (name, i)
        assert g['used_fallback'][i] == int(schedule_needs_fallback(c['ll'], c['rr'])), (name, i, g['used_fallback'][i])
        gs = sorted(ld['good'])
        assert gs[3] > gs[2] or gs[3] == 0, (name, i, "the winner's count is strictly the largest on the device's F too")
        assert allow_12_13 or ld['inlier_cnt'] not in (12, 13), (name, i)
        if i == g['l']:
            assert np.array_equal(g['ransac_mask'], c['ransac_mask']), (name, i)
            assert np.array_equal(g['mask'], ld['mask']), (name, i)
            eR, eT, e64R, e64T, _ = pose_errors(g['relative_R'], g['relative_T'], c, Fd)
            rR, rT = eR / max(e64R, E64_FLOOR), eT / max(e64T, E64_FLOOR)
            print(f"init_relpose {tag} {name}: l {i}  n {c['n_corres']}  iter {c['ransac_iter']} best {c['ransac_best']} bound {c['ransac_bound']} inliers {c['ransac_inliers']}  "
                  f"good {ld['good']}  relative_R {rR:.2f}  relative_T {rT:.2f}  (E64 {e64R:.1e} {e64T:.1e})")
            assert rR <= M and rT <= M, (name, rR, rT)
            worst = max(worst, rR, rT)
    if g['l'] < 0:
        assert not g['relative_R'].any() and not g['relative_T'].any() and len(g['mask']) == 0, name
    return worst


def check_cases(h, tag, names=None):
    """the cases in ONE call"""
    names = list(names or CASE_ARGS)
    got = dict(zip(names, h.init_relpose([case(n) for n in names])))
    worst = (0.0, None)
    for n in names:
        worst = max(worst, (check_window(n, case(n), got[n], reference(n), tag, n in ALLOW_12_13), n))
    print(f"init_relpose {tag}: worst ratio {worst[0]:.3f} ({worst[1]}; bound {M})")
    check_case_properties(got)
    return got


def check_case_properties(got):
    """what each case is about, on results keyed by case name (the device's, or `as_result(reference)`)"""
    g = got
    if 'F3_two' in g:
        assert g['F3_two']['l'] == 0 and list(g['F3_two']['gate']) == [1, 1]
    if 'F11_first' in g:
        assert g['F11_first']['l'] == 0
    if 'n20_refused' in g:
        assert g['n20_refused']['n_corres'][0] == 20 and g['n20_refused']['gate'][0] == 0 and g['n20_refused']['l'] == 1
    if 'n21_runs' in g:
        assert g['n21_runs']['n_corres'][0] == 21 and g['n21_runs']['l'] == 0
    for k, n in (('n64', 64), ('n65', 65)):
        if k in g:
            assert g[k]['n_corres'][0] == n and g[k]['l'] == 0
    if 'late_gate' in g:
        assert list(g['late_gate']['gate'][:4]) == [0, 0, 0, 0] and g['late_gate']['l'] == 4
    if 'few_inliers' in g:
        f = g['few_inliers']
        assert f['n_corres'][0] == 21 and f['gate'][0] == 1 and f['inlier_cnt'][0] <= 12 and f['l'] == 1
    if 'none' in g:
        assert g['none']['status'] == NONE and g['none']['l'] == -1
    if 'deep' in g:
        d = g['deep']
        assert d['l'] == 0 and d['inlier_cnt'][0] <= d['ransac_inliers'][0] - 10, "the deep points are inliers of the model and fail z < 50"
    if 'outliers30' in g:
        o = g['outliers30']
        assert 100 <= o['ransac_bound'][o['l']] < 1000 and o['ransac_best'][o['l']] >= 0 and o['ransac_iter'][o['l']] >= RP_CHUNK0, "the second part of the chunked launch runs"
    if 'collinear' in g:
        assert g['collinear']['used_fallback'][0] == 1 and g['collinear']['l'] == 0
    for k, v in g.items():
        if k != 'collinear':
            assert not np.asarray(v['used_fallback']).any(), k


def as_result(ref, win):
    """a result of relative_pose() in the shape of Handle.init_relpose (for check_case_properties)"""
    F = int(win['n_frames'])
    z = lambda k, d=0: np.array([c.get(k, d) for c in ref['cand']])
    return dict(status=ref['status'], l=ref['l'], n_corres=z('n_corres'), gate=z('gate'), inlier_cnt=z('inlier_cnt'), ransac_inliers=z('ransac_inliers'),
                ransac_bound=z('ransac_bound'), ransac_iter=z('ransac_iter'), ransac_best=z('ransac_best'),
                used_fallback=np.array([int(bool(c['gate']) and schedule_needs_fallback(c['ll'], c['rr'])) for c in ref['cand']]))


def batch(n, seed=500):
    """n small windows of mixed F and statuses for the batch-equals-single checks"""
    rng = np.random.default_rng(seed)
    fixed = [case('none'), case('n21_runs'), case('F3_two'), case('few_inliers')]
    out = []
    for i in range(n):
        if i % 4 == 1:
            out.append(fixed[(i // 4) % len(fixed)])
            continue
        F = int(rng.choice([3, 4, 5]))
        out.append(scene(seed + i, F=F, n_feat=int(rng.integers(30, 70)), xs=[1.0 * k / (F - 1) for k in range(F)]))
    return out


def check_batch_equals_single(h, sizes=(1, 3, 33)):
    wins = batch(max(sizes))
    single = [h.init_relpose([w])[0] for w in wins]
    assert {s['status'] for s in single} == {OK, NONE}, "the batch mixes statuses"
    assert len({w['n_frames'] for w in wins}) >= 3, "the batch mixes F"
    for n in sizes:
        for k, g in enumerate(h.init_relpose(wins[:n])):
            assert same_output(g, single[k]), (n, k)


def check_none_neighbours(h):
    """a window that ends with VG_RELPOSE_NONE between two good ones: they are what they are alone, and it returns zeros"""
    wins = [case('n64'), case('none'), case('F3_two')]
    alone = [h.init_relpose([w])[0] for w in wins]
    together = h.init_relpose(wins)
    assert [a['status'] for a in alone] == [OK, NONE, OK]
    for a, b in zip(alone, together):
        assert same_output(a, b)
    t = together[1]
    assert t['l'] == -1 and not t['relative_R'].any() and not t['relative_T'].any() and len(t['mask']) == 0
    for k in TAPS[3:]:
        assert not np.asarray(t[k]).any(), k


def check_growing_table(h_new):
    """a call at n_feat 40 followed by one at 300 on the same (fresh) handle: the resident tables grow, both calls are what a handle that
    saw the large call first returns"""
    small, large = scene(31, F=4, n_feat=40, xs=[0.0, 0.4, 0.8, 1.2]), scene(32, F=4, n_feat=300, xs=[0.0, 0.4, 0.8, 1.2])
    a1 = h_new.init_relpose([small])[0]
    b1 = h_new.init_relpose([large])[0]
    a2 = h_new.init_relpose([small])[0]
    assert a1['status'] == OK and b1['status'] == OK and b1['n_corres'].max() > 100
    assert same_output(a1, a2)
    check_window('grow_small', small, a1, relative_pose(small), 'grow')
    check_window('grow_large', large, b1, relative_pose(large), 'grow')


def _refusals():
    """name -> a function that spoils window 1 of the packed call (ins, outs, keep) and returns the n_windows to pass"""
    nan = float('nan')

    def setter(fn, n=2):
        def f(ins, outs, keep):
            fn(ins, outs, keep)
            return n
        return f

    def arr(name, idx, val):
        return setter(lambda ins, outs, keep: keep[1][name].reshape(-1).__setitem__(idx, val))

    def null(field):
        return setter(lambda ins, outs, keep: setattr(ins[1], field, C.cast(None, type(getattr(ins[1], field)))))

    def field(obj, name, val):
        return setter(lambda ins, outs, keep: setattr((ins if obj == 'in' else outs)[1], name, val))

    r = {'n_windows_0': setter(lambda *a: None, 0), 'in_struct_size': field('in', 'struct_size', 8), 'out_struct_size': field('out', 'struct_size', 0),
         'F_2': field('in', 'n_frames', 2), 'F_17': field('in', 'n_frames', 17), 'n_feat_0': field('in', 'n_feat', 0), 'n_feat_above': field('in', 'n_feat', 1025),
         'span_leaves_F': arr('start', 0, 3), 'nobs_0': arr('nobs', 3, 0), 'obs_off_descends': arr('off', 5, 2), 'obs_off_negative': arr('off', 0, -1), 'point_nan': arr('points', 3 * 11 + 1, nan),
         'point_inf': arr('points', 3 * 7, float('inf')), 'threshold_0': field('in', 'ransac_threshold', 0.0), 'threshold_negative': field('in', 'ransac_threshold', -1e-3),
         'threshold_nan': field('in', 'ransac_threshold', nan), 'confidence_0999': field('in', 'confidence', 0.999), 'confidence_0': field('in', 'confidence', 0.0),
         'gate_0': field('in', 'parallax_gate', 0.0), 'focal_negative': field('in', 'focal', -460.0), 'dist_0': field('in', 'cheirality_dist', 0.0),
         'min_corres_13': field('in', 'min_corres', 13), 'min_inliers_negative': field('in', 'min_inliers', -1)}
    for t in ('start', 'nobs', 'obs_off', 'points'):
        r['null_' + t] = null(t)
    return r


REFUSALS = tuple(_refusals())


_REFUSAL_GOOD = {}


@functools.lru_cache(maxsize=None)
def _refusal_windows():
    """two windows of F = 3 and 24 features each (the smallest that still run every stage)"""
    return [scene(41 + k, F=3, tracks=_whole(22, 3) + [(1, 2), (0, 2)], xs=[0.0, 0.5, 1.0]) for k in range(2)]


def check_refusal(h, name):
    """the spoiled call returns VG_ERR_BAD_ARG with a message, writes nothing, and the handle goes on working"""
    wins = _refusal_windows()
    if id(h) not in _REFUSAL_GOOD:
        _REFUSAL_GOOD[id(h)] = h.init_relpose(wins)
    good = _REFUSAL_GOOD[id(h)]
    ins, outs, keep = h.init_relpose_pack(wins)
    for o, b in zip(outs, keep):
        o.status, o.l, o.n_mask = 77, 55, -3
        o.relative_R[0], o.relative_T[2] = 3.25, 3.25
        for k in TAPS + ('mask', 'ransac_mask'):
            b[k][...] = 9
    n = _refusals()[name](ins, outs, keep)
    rc = h.lib.vg_init_relpose(h.h, n, ins, outs)
    assert rc == -1, (name, rc)                              # VG_ERR_BAD_ARG
    assert b"vg_init_relpose" in h.lib.vg_last_error(h.h), name
    for o, b in zip(outs, keep):
        assert (o.status, o.l, o.n_mask, o.relative_R[0], o.relative_T[2]) == (77, 55, -3, 3.25, 3.25), name
        assert all(np.all(b[k] == 9) for k in TAPS + ('mask', 'ransac_mask')), name
    assert same_output(good[1], h.init_relpose(wins[1:])[0]), name


@functools.lru_cache(maxsize=None)
def capacity_reference():
    return relative_pose(capacity_scene())


def check_stream_limit(h, run_limit=False):
    """more than VG_RELPOSE_MAX_STREAMS (window, candidate) pairs in one call: refused, nothing written, the handle goes on"""
    w = _refusal_windows()[0]
    few = h.init_relpose([w])[0]
    wins = [w] * 2049                                           # F = 3: 4098 streams
    ins, outs, keep = h.init_relpose_pack(wins)
    for o in outs:
        o.status, o.l = 77, 55
    rc = h.lib.vg_init_relpose(h.h, len(wins), ins, outs)
    assert rc == -1 and b"VG_RELPOSE_MAX_STREAMS" in h.lib.vg_last_error(h.h), rc
    assert all((o.status, o.l) == (77, 55) for o in outs)
    if run_limit:                                               # exactly the limit runs (the emulator would take minutes over 4096 streams)
        assert h.lib.vg_init_relpose(h.h, 2048, ins, outs) == 0
        assert all(o.status == OK and o.l == few['l'] for o in list(outs)[:2048]) and (outs[2048].status, outs[2048].l) == (77, 55)
    assert same_output(few, h.init_relpose([w])[0])


def check_capacity(h, tag):
    """F = 16 with 1024 correspondences per candidate (four terms per thread in the parallax sum, 16 ballot words): held like every case
    of the table by check_window -- every tap of all 15 candidates, the RANSAC replay included, the pose within M x E64"""
    win, ref = capacity_scene(), capacity_reference()
    g = h.init_relpose([win])[0]
    assert list(g['n_corres']) == [1024] * 15 and g['l'] == 0 and sum(c['gate'] for c in ref['cand']) >= 8
    worst = check_window('capacity', win, g, ref, tag)
    print(f"init_relpose {tag} capacity: worst ratio {worst:.2f}")
    return worst


def check_chain(h):
    """vg_init_relpose -> vg_init_sfm -> vg_init_align on the chain scene of tests/init_sfm_ref.py, no pose handed in from the generator"""
    import init_sfm_ref as S
    A = S.A
    win, al, s_true = S.chain_scene()
    rp = h.init_relpose([win])[0]
    ref = relative_pose(win, with_replay=False)
    assert rp['status'] == OK and rp['l'] == ref['l'], (rp['status'], rp['l'], ref['l'])
    g = h.init_sfm([dict(win, l=rp['l'], relative_R=rp['relative_R'], relative_T=rp['relative_T'])])[0]
    assert g['status'] == S.OK, g['status']
    res = h.init_align([dict(al, R=g['R_all'], T=g['T_all'])])[0]
    # relative_T has unit length where the generator's has the scene's: the scale the alignment finds is in units of THIS baseline
    base_l = np.linalg.norm(win['truth']['cam'][-1][1] - win['truth']['cam'][rp['l']][1]) * win['truth']['base']
    s_here = al['truth']['s'] * base_l
    err = abs(res['s'] - s_here) / s_here
    print(f"init_relpose chain: l {rp['l']}  sfm status {g['status']}  align status {res['status']}  scale {res['s']:.9g} (scene {s_here:.9g}, relative error {err:.1e})")
    assert res['status'] == A.OK and err < S.SCALE_BOUND
    return rp['l']


REPLAY_CASES = ('F11_first', 'few_inliers', 'none')          # the reference's shape / a gated candidate that fails / no frame passes


def check_replay(h, exe, tmp_dir, name):
    """Estimator::relativePose (host/estimator.cpp, vg_pack_relpose) through `vins_replay relpose`: number for number the binding's"""
    win = case(name)
    path, out = os.path.join(str(tmp_dir), name + ".bin"), os.path.join(str(tmp_dir), name + ".txt")
    write_file(path, win)
    r = subprocess.run([exe, "relpose", path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = {ln.split()[0]: ln.split()[1:] for ln in open(out).read().splitlines()}
    g = h.init_relpose([win])[0]
    assert [int(x) for x in rows['result']] == [int(g['status'] == OK), g['status'], g['l']], (rows['result'], g['status'], g['l'])
    assert np.array_equal(np.array([float(x) for x in rows['R']]), g['relative_R'].reshape(-1)), name
    assert np.array_equal(np.array([float(x) for x in rows['T']]), g['relative_T']), name
    if g['status'] != OK:
        assert [int(x) for x in rows['structure']] == [0, 1], "initialStructure() returns false and leaves marginalization_flag (MARGIN_SECOND_NEW) alone"
    else:
        assert 'structure' not in rows


# --------------------------------------------------------------------------------------------------- files for the stand-alone programs
def write_file(path, win):
    """VRP1: int32 magic, F, n_feat, rows; start, nobs, obs_off (int32 each); points (float64 x y z rows)"""
    start, nobs = np.asarray(win['start'], np.int32), np.asarray(win['nobs'], np.int32)
    off = np.concatenate([[0], np.cumsum(nobs)[:-1]]).astype(np.int32)
    pts = np.asarray(win['points'], np.float64).reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", 0x31505256, int(win['n_frames']), len(start), len(pts)))
        f.write(start.tobytes()); f.write(nobs.tobytes()); f.write(off.tobytes()); f.write(pts.tobytes())
