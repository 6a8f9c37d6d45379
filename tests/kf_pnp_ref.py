"""vg_kf_pnp (include/vinsgpu.h): a NumPy statement of the definition that takes none of the kernel's shortcuts (one sample at a time,
plain loops, no chunks, no lane groups), the scenes, the conditions the scenes must meet and the check bodies shared by
tests/test_kf_pnp_def.py (the reference alone, on the CPU), tests/test_kf_pnp_simt.py (the emulated kernels) and tests/test_kf_pnp_gpu.py
(the MI355X).

Three routes, as the initialisation tests have them:
  ld     numpy.longdouble with the header's Jacobi routines,
  jac64  the same in float64,
  svd64  float64 with numpy.linalg.eigh / svd for the three eigenproblems, followed by the same canonical basis step.
E64 is the disagreement of the two float64 routes with `ld`; values are held to M = 4 x E64 (the project's standing bound), each stage
started from the device's own taps where it feeds the next: the sample's model is compared with the reference's EPnP of the same sample,
the returned pose with the reference's refit over the DEVICE's mask, the pose algebra with the reference's on the DEVICE's rvec / tvec.
Decisions (status, mask, n_inliers, the RANSAC taps, has_loop, the compacted lists, refit_iters / refit_up) are compared for equality."""
import functools
import os
import struct
import sys

import numpy as np

import init_sfm_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
M = 4.0
OK, SKIPPED, NO_MODEL, NUMERIC = 0, 1, 2, 3
ROUTES = {'ld': (LD, 'jacobi', 'ld'), 'jac64': (np.float64, 'jacobi', 'ldlt'), 'svd64': (np.float64, 'linalg', 'solve')}
DEFAULTS = dict(min_loop_num=25, max_iters=100, refine=0, reproj_threshold=10.0 / 460.0, confidence=0.99, max_yaw_deg=30.0, max_dist=20.0)


# --------------------------------------------------------------------------------------------------- the registrator's schedule and bound
class CvRng:
    def __init__(self, s):
        self.state = s if s else 0xffffffff

    def next(self):
        self.state = ((self.state & 0xffffffff) * 4164903690 + (self.state >> 32)) & 0xffffffffffffffff
        return self.state & 0xffffffff

    def uniform(self, a, b):
        return a if a == b else self.next() % (b - a) + a


@functools.lru_cache(maxsize=None)
def schedule(n, iters):
    rng, out = CvRng(0xffffffffffffffff), []
    for _ in range(iters):
        idx = []
        while len(idx) < 5:
            c = rng.uniform(0, n)
            if c not in idx:
                idx.append(c)
        out.append(tuple(idx))
    return tuple(out)


def update_num_iters(p, ep, model_points, max_iters):
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num, denom = max(1.0 - p, sys.float_info.min), 1.0 - (1.0 - ep) ** model_points
    if denom < sys.float_info.min:
        return 0
    num, denom = np.log(num), np.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(np.rint(num / denom))


# --------------------------------------------------------------------------------------------------- the header's Jacobi
def _pairs(n):
    if n == 3:
        return [[(0, 1)], [(0, 2)], [(1, 2)]]
    return [[(i, (r - i) % n) for i in range(n) if i < (r - i) % n] for r in range(n)]


def jacobi_cols(A, tol=1e-15, sweeps=40):
    """one-sided Jacobi on the columns of A: (A V, V); only rotations between two columns above the noise keep the sweeps going"""
    A = A.copy()
    n = A.shape[1]
    V = np.eye(n, dtype=A.dtype)
    signal = A.dtype.type(1e-26) * (A * A).sum()
    rounds = _pairs(n)
    for _ in range(sweeps):
        rotated = False
        for rd in rounds:
            for p, q in rd:
                a, b = A[:, p].copy(), A[:, q].copy()
                al, be, ga = a @ a, b @ b, a @ b
                if ga != 0 and abs(ga) > tol * np.sqrt(al * be):
                    rotated = rotated or (al > signal and be > signal)
                    zeta = (be - al) / (2 * ga)
                    t = (1 if zeta >= 0 else -1) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    A[:, p], A[:, q] = c * a - s * b, s * a + c * b
                    va, vb = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * va - s * vb, s * va + c * vb
        if not rotated:
            break
    return A, V


def _positive(v):
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def eig3(C, how):
    """eigenpairs of the symmetric 3x3 C, descending: (lambda [3], columns)"""
    if how == 'linalg':
        w, V = np.linalg.eigh(C)
        return w[::-1].copy(), V[:, ::-1].copy()
    A, V = jacobi_cols(C)
    nn = (A * A).sum(axis=0)
    o = np.argsort(-nn, kind='stable')
    return np.sqrt(nn[o]), V[:, o]


def svd3(Mx, how):
    """(U, V) of Arun's 3x3 matrix, singular values descending"""
    if how == 'linalg':
        U, _, Vt = np.linalg.svd(Mx)
        return U, Vt.T
    A, V = jacobi_cols(Mx)
    nn = (A * A).sum(axis=0)
    o = np.argsort(-nn, kind='stable')
    return A[:, o] / np.sqrt(nn[o]), V[:, o]


def null4(Mx, how):
    """the eigenvectors of M^T M for its four smallest eigenvalues, ascending, as rows; and the row margin of the canonical step"""
    if how == 'linalg':
        w, V = np.linalg.eigh(Mx.T @ Mx)
        v = V[:, :4].T.copy()
    else:
        A, V = jacobi_cols(Mx)
        nn = (A * A).sum(axis=0)
        o = np.argsort(nn, kind='stable')[:4]
        v = V[:, o].T.copy()
    a, b = v[0].copy(), v[1].copy()
    s = a * a + b * b
    k = int(np.argmax(s))
    r = np.sqrt(s[k])
    v[0], v[1] = (b[k] * a - a[k] * b) / r, (a[k] * a + b[k] * b) / r
    v[0][k] = 0
    ss = np.sort(s)
    margin = float((ss[-1] - ss[-2]) / ss[-1])
    return np.array([_positive(x) for x in v]), margin


def qr_solve(A, b):
    """qr_solve of epnp.cpp; None: a column that is all zero"""
    A, b = A.copy(), b.copy()
    nr, nc = A.shape
    A1, A2 = np.zeros(nc, A.dtype), np.zeros(nc, A.dtype)
    for k in range(nc):
        mx = np.abs(A[k:, k]).max()
        if mx == 0:
            return None
        A[k:, k] *= 1 / mx
        sigma = np.sqrt(A[k:, k] @ A[k:, k])
        if A[k, k] < 0:
            sigma = -sigma
        A[k, k] += sigma
        A1[k], A2[k] = sigma * A[k, k], -mx * sigma
        for j in range(k + 1, nc):
            tau = (A[k:, k] @ A[k:, j]) / A1[k]
            A[k:, j] -= tau * A[k:, k]
    for j in range(nc):
        tau = (A[j:, j] @ b[j:]) / A1[j]
        b[j:] -= tau * A[j:, j]
    X = np.zeros(nc, A.dtype)
    for i in range(nc - 1, -1, -1):
        X[i] = (b[i] - A[i, i + 1:] @ X[i + 1:]) / A2[i]
    return X


# --------------------------------------------------------------------------------------------------- EPnP of one sample
def _inv3(C):
    k = np.array([[C[1, 1] * C[2, 2] - C[1, 2] * C[2, 1], C[0, 2] * C[2, 1] - C[0, 1] * C[2, 2], C[0, 1] * C[1, 2] - C[0, 2] * C[1, 1]],
                  [C[1, 2] * C[2, 0] - C[1, 0] * C[2, 2], C[0, 0] * C[2, 2] - C[0, 2] * C[2, 0], C[0, 2] * C[1, 0] - C[0, 0] * C[1, 2]],
                  [C[1, 0] * C[2, 1] - C[1, 1] * C[2, 0], C[0, 1] * C[2, 0] - C[0, 0] * C[2, 1], C[0, 0] * C[1, 1] - C[0, 1] * C[1, 0]]])
    det = C[0, 0] * k[0, 0] + C[0, 1] * k[1, 0] + C[0, 2] * k[2, 0]
    return k, det


def epnp(P3, p2, route):
    """solvePnP(SOLVEPNP_EPNP) on five points -> (rvec, tvec, row margin) or None (no model)"""
    dt, how, _ = ROUTES[route]
    pw, us = P3.astype(np.float32).astype(dt), p2.astype(np.float32).astype(dt)
    with np.errstate(all='ignore'):
        c0 = pw.sum(axis=0) / 5
        d = pw - c0
        lam, E = eig3(d.T @ d, how)
        cw = np.array([c0] + [c0 + np.sqrt(lam[i] / 5) * _positive(E[:, i]) for i in range(3)])
        k, det = _inv3((cw[1:] - cw[0]).T)
        if det == 0 or not np.isfinite(np.float64(det)):
            return None
        al3 = (pw - cw[0]) @ (k / det).T
        al = np.concatenate([(1 - al3[:, 0] - al3[:, 1] - al3[:, 2])[:, None], al3], axis=1)
        Mx = np.zeros((10, 12), dt)
        for i in range(5):
            for j in range(4):
                Mx[2 * i, 3 * j], Mx[2 * i, 3 * j + 2] = al[i, j], al[i, j] * (0 - us[i, 0])
                Mx[2 * i + 1, 3 * j + 1], Mx[2 * i + 1, 3 * j + 2] = al[i, j], al[i, j] * (0 - us[i, 1])
        v, margin = null4(Mx, how)
        L, rho = np.zeros((6, 10), dt), np.zeros(6, dt)
        for pr, (a, b) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))):
            dv = v[:, 3 * a:3 * a + 3] - v[:, 3 * b:3 * b + 3]
            g = dv @ dv.T
            L[pr] = [g[0, 0], 2 * g[0, 1], g[1, 1], 2 * g[0, 2], 2 * g[1, 2], g[2, 2], 2 * g[0, 3], 2 * g[1, 3], 2 * g[2, 3], g[3, 3]]
            rho[pr] = (cw[a] - cw[b]) @ (cw[a] - cw[b])

        def gauss_newton(bt):
            for _ in range(5):
                b0, b1, b2, b3 = bt
                A = np.stack([2 * L[:, 0] * b0 + L[:, 1] * b1 + L[:, 3] * b2 + L[:, 6] * b3, L[:, 1] * b0 + 2 * L[:, 2] * b1 + L[:, 4] * b2 + L[:, 7] * b3,
                              L[:, 3] * b0 + L[:, 4] * b1 + 2 * L[:, 5] * b2 + L[:, 8] * b3, L[:, 6] * b0 + L[:, 7] * b1 + L[:, 8] * b2 + 2 * L[:, 9] * b3], axis=1)
                r = rho - (L[:, 0] * b0 * b0 + L[:, 1] * b0 * b1 + L[:, 2] * b1 * b1 + L[:, 3] * b0 * b2 + L[:, 4] * b1 * b2 + L[:, 5] * b2 * b2 +
                           L[:, 6] * b0 * b3 + L[:, 7] * b1 * b3 + L[:, 8] * b2 * b3 + L[:, 9] * b3 * b3)
                x = qr_solve(A, r)
                if x is None:
                    return None
                bt = bt + x
            return bt

        def R_and_t(bt):
            ccs = (bt[:, None] * v).sum(axis=0).reshape(4, 3)
            pcs = al @ ccs
            if pcs[0, 2] < 0:
                pcs = -pcs
            pc0, pw0 = pcs.sum(axis=0) / 5, pw.sum(axis=0) / 5
            U, V = svd3((pcs - pc0).T @ (pw - pw0), how)
            R = U @ V.T
            if np.linalg.det(R.astype(np.float64)) < 0:
                R[2] = -R[2]
            t = pc0 - R @ pw0
            X = pw @ R.T + t
            iz = 1 / X[:, 2]
            return R, t, np.sqrt((us[:, 0] - X[:, 0] * iz) ** 2 + (us[:, 1] - X[:, 1] * iz) ** 2).sum() / 5

        cands = []
        for cols in ((0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4)):
            x = qr_solve(L[:, cols], rho)
            if x is None:
                return None
            bt = np.zeros(4, dt)
            if len(cols) == 4:
                sg = -1 if x[0] < 0 else 1
                bt[0] = np.sqrt(sg * x[0])
                bt[1:] = sg * x[1:] / bt[0]
            else:
                if x[0] < 0:
                    bt[0], bt[1] = np.sqrt(-x[0]), (np.sqrt(-x[2]) if x[2] < 0 else 0)
                else:
                    bt[0], bt[1] = np.sqrt(x[0]), (np.sqrt(x[2]) if x[2] > 0 else 0)
                if x[1] < 0:
                    bt[0] = -bt[0]
                if len(cols) == 5:
                    bt[2] = x[3] / bt[0]
            bt = gauss_newton(bt)
            if bt is None:
                return None
            cands.append(R_and_t(bt))
        N = 0
        if cands[1][2] < cands[0][2]:
            N = 1
        if cands[2][2] < cands[N][2]:
            N = 2
        R, t, _ = cands[N]
        rv = S._rodrigues_R2r(R, dt)
        vals = [c[2] for c in cands] + list(t) + ([] if rv is None else list(rv))
        if rv is None or not np.all(np.isfinite(np.array(vals, np.float64))):
            return None
    return rv, t, margin


def errors(rv, tv, P3, p2, dt):
    """step 3: float32 errors of every point"""
    R = S._rodrigues_r2R(np.asarray(rv, dt), dt)[0]
    X = P3.astype(dt) @ R.T + np.asarray(tv, dt)
    with np.errstate(all='ignore'):
        z = np.where(X[:, 2] != 0, 1 / np.where(X[:, 2] != 0, X[:, 2], 1), 1)
        px, py = (X[:, 0] * z).astype(np.float32), (X[:, 1] * z).astype(np.float32)
    dx, dy = (px - p2[:, 0]).astype(np.float64), (py - p2[:, 1]).astype(np.float64)
    return (dx * dx + dy * dy).astype(np.float32)


# --------------------------------------------------------------------------------------------------- the call for one pair
def full(pair):
    p = dict(DEFAULTS)
    p.update(origin_vio_T=np.zeros(3), origin_vio_R=np.eye(3), tic=np.zeros(3), qic=np.eye(3))
    p.update(pair)
    p['point_3d'] = np.ascontiguousarray(p['point_3d'], np.float32).reshape(-1, 3)
    p['old_norm'] = np.ascontiguousarray(p['old_norm'], np.float32).reshape(-1, 2)
    return p


def guess(p, dt):
    """R_inital, P_inital"""
    oR, qic = np.asarray(p['origin_vio_R'], np.float64).reshape(3, 3).astype(dt), np.asarray(p['qic'], np.float64).reshape(3, 3).astype(dt)
    Rwc = oR @ qic
    Twc = np.asarray(p['origin_vio_T'], np.float64).astype(dt) + oR @ np.asarray(p['tic'], np.float64).astype(dt)
    k, det = _inv3(Rwc)
    Rg = k * (1 / det)
    return Rg, -(Rg @ Twc)


def ransac(p, route):
    """the registrator: the bookkeeping trace [(iteration, count, model or None)], best, bound, and the scene conditions' margins"""
    dt = ROUTES[route][0]
    P3, p2 = p['point_3d'], p['old_norm']
    n = len(P3)
    thr2 = np.float32(p['reproj_threshold'] * p['reproj_threshold'])
    niters, best, good, trace, it = p['max_iters'], -1, 0, [], 0
    err_margin, row_margin = np.inf, np.inf
    sched = schedule(n, p['max_iters'])
    while it < niters:
        idx = list(sched[it])
        m = epnp(P3[idx], p2[idx], route)
        cnt = -1
        if m is not None:
            e = errors(m[0], m[1], P3, p2, dt)
            cnt = int((e <= thr2).sum())
            err_margin = min(err_margin, float(np.abs(e.astype(np.float64) - float(thr2)).min() / float(thr2)))
            row_margin = min(row_margin, m[2])
        trace.append((it, cnt))
        if cnt > max(good, 4):
            best, good, model = it, cnt, m
            niters = update_num_iters(0.99, (n - cnt) / n, 5, niters)
        it += 1
    out = dict(trace=trace, best=best, bound=niters, iter=max(best, min(niters, p['max_iters']) - 1), err_margin=err_margin, row_margin=row_margin)
    if best >= 0:
        out.update(sample_rvec=model[0], sample_tvec=model[1], mask=(errors(model[0], model[1], P3, p2, dt) <= thr2).astype(np.uint8))
    return out


def returned_pose(p, route, sample, mask):
    """step 5 from a sample model (rvec, tvec) or None and a mask -> (status, rvec, tvec, refit_iters, refit_up)"""
    dt, _, pr = ROUTES[route]
    Rg, tg = guess(p, dt)
    if sample is None or p['refine'] == 1:
        rv0 = S._rodrigues_R2r(Rg, dt)
        if rv0 is None or not np.all(np.isfinite(np.concatenate([rv0, tg]).astype(np.float64))):
            return NUMERIC, None, None, 0, 0
        if sample is None:
            return NO_MODEL, rv0, tg, 0, 0
        sel = np.asarray(mask) != 0
        r = S.pnp(Rg, tg, p['point_3d'][sel].astype(dt), p['old_norm'][sel].astype(dt), dt, pr)
        rv = None if r is None else S._rodrigues_R2r(r[0], dt)
        if rv is None:
            return NUMERIC, None, None, 0, 0
        return OK, rv, r[1], r[2], r[3]
    return OK, np.asarray(sample[0], dt), np.asarray(sample[1], dt), 0, 0


def _yaw(R):
    return np.arctan2(R[1, 0], R[0, 0]) / np.pi * 180


def tail(p, rv, tv, n_in, status, dt):
    """step 6 from a returned pose -> PnP_R_old, PnP_T_old, loop_info, has_loop, the gates' margins"""
    oR, qic = np.asarray(p['origin_vio_R'], np.float64).reshape(3, 3).astype(dt), np.asarray(p['qic'], np.float64).reshape(3, 3).astype(dt)
    oT, tic = np.asarray(p['origin_vio_T'], np.float64).astype(dt), np.asarray(p['tic'], np.float64).astype(dt)
    r = S._rodrigues_r2R(np.asarray(rv, dt), dt)[0]
    Rold = r.T
    Told = Rold @ (-np.asarray(tv, dt))
    PR = Rold @ qic.T
    PT = Told - PR @ tic
    info, has, gm = np.zeros(8, dt), 0, np.inf
    if status == OK and n_in > p['min_loop_num']:
        rt = PR.T @ (oT - PT)
        q = S._q_from_R(PR.T @ oR, dt)
        if q[0] < 0:
            q = -q
        a = _yaw(oR) - _yaw(PR)
        yaw = a - 360 * np.floor((a + 180) / 360) if a > 0 else a + 360 * np.floor((-a + 180) / 360)
        info = np.concatenate([rt, q, [yaw]])
        dist = np.sqrt(rt @ rt)
        has = int(abs(yaw) < p['max_yaw_deg'] and dist < p['max_dist'])
        gm = float(min(abs(abs(yaw) - p['max_yaw_deg']) / p['max_yaw_deg'], abs(dist - p['max_dist']) / p['max_dist']))
    return dict(PnP_R_old=PR, PnP_T_old=PT, loop_info=info, has_loop=has, gate_margin=gm)


def reference(pair, route='ld'):
    """the whole call for one pair"""
    p = full(pair)
    dt = ROUTES[route][0]
    n = len(p['point_3d'])
    out = dict(status=SKIPPED, n_inliers=0, mask=np.zeros(n, np.uint8), ransac_best=0, ransac_iter=0, ransac_bound=0, has_loop=0, refit_iters=0,
               refit_up=0, matched_index=np.zeros(0, np.int32))
    if n <= p['min_loop_num']:
        return out
    rs = ransac(p, route)
    sample = (rs['sample_rvec'], rs['sample_tvec']) if rs['best'] >= 0 else None
    mask = rs.get('mask', np.zeros(n, np.uint8))
    st, rv, tv, rit, rup = returned_pose(p, route, sample, mask)
    out.update(status=st, n_inliers=int(mask.sum()), mask=mask, ransac_best=rs['best'], ransac_iter=rs['iter'], ransac_bound=rs['bound'],
               refit_iters=rit, refit_up=rup, matched_index=np.flatnonzero(mask).astype(np.int32), ransac=rs, sample=sample)
    if st != NUMERIC:
        out.update(rvec=rv, tvec=tv, **tail(p, rv, tv, out['n_inliers'], st, dt))
    return out


# --------------------------------------------------------------------------------------------------- scenes
def _rot(v):
    return S._rodrigues_r2R(np.asarray(v, np.float64), np.float64)[0]


def scene(seed, n=150, outlier=0.0, noise=0.0005, yaw_deg=5.0, dist=1.0, refine=0, n_good=None, coplanar=False, **over):
    """An old keyframe looking at n landmarks; the current frame's VIO pose (origin_vio_*) differs from the old camera's body pose by a yaw of
    yaw_deg and a translation of length dist.  Outliers get a wrong observation."""
    rng = np.random.default_rng(seed)
    qic = _rot([0.02, -0.01, 0.03])
    tic = np.array([0.05, -0.02, 0.01])
    R_old = _rot([0.0, 0.0, 0.3])                                  # body pose of the old keyframe in the world
    T_old = np.array([1.0, 2.0, 0.5])
    Rc, Tc = R_old @ qic, T_old + R_old @ tic                       # its camera
    pc = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(3.0, 9.0, n)], axis=1)
    P3 = (pc @ Rc.T + Tc).astype(np.float32)
    if coplanar:                                                    # 30 landmarks of exactly one world z: a sample of five of them has no model
        P3[:30, 2] = np.float32(5.0)
    pcf = (P3.astype(np.float64) - Tc) @ Rc
    obs = pcf[:, :2] / pcf[:, 2:3] + rng.normal(0, noise, (n, 2))
    n_out = int(round(outlier * n)) if n_good is None else n - n_good
    bad = rng.permutation(n)[:n_out]
    obs[bad] += rng.uniform(0.15, 0.6, (n_out, 2)) * rng.choice([-1.0, 1.0], (n_out, 2))
    d = rng.normal(size=3)
    d[2] *= 0.2
    oR = _rot([0.0, 0.0, np.deg2rad(yaw_deg)]) @ R_old
    oT = T_old + dist * d / np.linalg.norm(d)
    pair = dict(point_3d=P3, old_norm=obs.astype(np.float32), point_id=(np.cumsum(rng.integers(1, 4, n)) + 10).astype(np.int32),
                origin_vio_T=oT, origin_vio_R=oR, tic=tic, qic=qic, refine=refine)
    pair.update(over)
    return pair


CASE_ARGS = {
    'n6': dict(seed=1, n=6, min_loop_num=3),
    'n26': dict(seed=2, n=26),
    'n27': dict(seed=3, n=27),
    'n64': dict(seed=4, n=64, outlier=0.3),
    'n65': dict(seed=5, n=65, outlier=0.3, refine=1),
    'n150': dict(seed=6, n=150, outlier=0.3),
    'n150_clean': dict(seed=7, n=150, outlier=0.0, refine=1),
    'n150_out60': dict(seed=8, n=150, outlier=0.6),
    'no_model': dict(seed=9, n=40, outlier=1.0),
    'skipped': dict(seed=10, n=25),
    'exactly_min': dict(seed=11, n=36, n_good=25, noise=0.0),
    'yaw_beyond': dict(seed=12, n=80, yaw_deg=30.5),
    'dist_beyond': dict(seed=13, n=80, dist=20.5),
    'coplanar': dict(seed=14, n=40, outlier=0.3, coplanar=True),
    'refine_out30': dict(seed=15, n=150, outlier=0.3, refine=1),
}
EDGE_CASES = ('exactly_min', 'no_model', 'n26')                   # where n_inliers may be min_loop_num or min_loop_num + 1


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(**CASE_ARGS[name])


@functools.lru_cache(maxsize=None)
def case_reference(name, route='ld'):
    return reference(case(name), route)


@functools.lru_cache(maxsize=None)
def capacity_scene():
    return scene(seed=20, n=1024, outlier=0.3, refine=1)


def conditions(name, pair, refs):
    """what a scene must meet, on the reference's three routes (refs: route -> reference())"""
    ld = refs['ld']
    if ld['status'] == SKIPPED:
        return
    for r in ('jac64', 'svd64'):
        assert refs[r]['ransac']['trace'] == ld['ransac']['trace'], (name, r, "the routes give the same bookkeeping trace")
        assert np.array_equal(refs[r]['mask'], ld['mask']), (name, r, "and the same mask")
        assert (refs[r]['status'], refs[r]['has_loop'], refs[r]['refit_iters'], refs[r]['refit_up']) == \
            (ld['status'], ld['has_loop'], ld['refit_iters'], ld['refit_up']), (name, r)
    for r in refs.values():
        assert r['ransac']['err_margin'] >= 1e-6, (name, "an error of a model of the trace within 1e-6 of the squared threshold", r['ransac']['err_margin'])
        assert r['ransac']['row_margin'] >= 1e-6, (name, "the canonical row leads by less than 1e-6", r['ransac']['row_margin'])
    p = full(pair)
    if name not in EDGE_CASES:
        assert ld['n_inliers'] not in (p['min_loop_num'], p['min_loop_num'] + 1), (name, ld['n_inliers'])
    if ld['status'] == OK:
        assert ld['gate_margin'] >= 1e-9, (name, ld['gate_margin'])


def case_properties():
    """the cases are what their names say (on the `ld` reference)"""
    r = {n: case_reference(n) for n in CASE_ARGS}
    assert r['skipped']['status'] == SKIPPED and r['no_model']['status'] == NO_MODEL and r['no_model']['ransac_best'] == -1
    assert r['n150_out60']['ransac_bound'] == 100 and r['n150_clean']['ransac_bound'] < 30 < r['n150_out60']['ransac_iter']
    assert r['exactly_min']['n_inliers'] == 25 and r['exactly_min']['status'] == OK and not r['exactly_min']['loop_info'].any()
    for n, k in (('yaw_beyond', 7), ('dist_beyond', None)):
        assert r[n]['status'] == OK and r[n]['n_inliers'] > 25 and r[n]['has_loop'] == 0 and r[n]['loop_info'].any(), n
    assert 30.0 < abs(r['yaw_beyond']['loop_info'][7]) < 31.5 and 20.0 < np.linalg.norm(r['dist_beyond']['loop_info'][:3].astype(float)) < 21.0
    assert any(c == -1 for _, c in r['coplanar']['ransac']['trace']) and r['coplanar']['status'] == OK
    for n in ('n6', 'n26', 'n27', 'n64', 'n65', 'n150', 'n150_clean', 'n150_out60', 'refine_out30'):
        assert r[n]['status'] == OK and r[n]['has_loop'] == 1, (n, r[n]['status'])
    assert r['n65']['refit_iters'] > 0 and r['refine_out30']['refit_iters'] > 0


# --------------------------------------------------------------------------------------------------- the device checks
# one body for the emulator and the MI355X; h: a ba.Handle
def _fe():
    import __graft_entry__ as graft
    graft.load_package()
    from vins_mono_amd import fe
    return fe


DECISIONS = ('status', 'n_inliers', 'ransac_best', 'ransac_iter', 'ransac_bound', 'has_loop', 'refit_iters', 'refit_up')
E64_FLOOR = 2.0 ** -52
VALUES = ('sample_rvec', 'sample_tvec', 'rvec', 'tvec', 'PnP_R_old', 'PnP_T_old', 'loop_info')


def same_output(a, b):
    return all(a[k] == b[k] for k in DECISIONS) and all(np.array_equal(a[k], b[k]) for k in VALUES + ('mask', 'matched_index', 'match_id', 'match_xy'))


def _ratio(got, ld, others, scale=1.0):
    """max |got - ld| over max(E64, floor), E64 = the float64 routes' disagreement with ld; the quantities are of the scale given"""
    ld = np.asarray(ld, LD).reshape(-1)
    e64 = max([float(np.abs(np.asarray(o, LD).reshape(-1) - ld).max()) for o in others] + [E64_FLOOR * scale])
    return float(np.abs(np.asarray(got, LD).reshape(-1) - ld).max()) / e64


def check_pair(name, pair, g, tag):
    """one pair's device result g against the reference; returns the worst value ratio"""
    p = full(pair)
    n = len(p['point_3d'])
    ref = reference(pair, 'ld')
    for k in DECISIONS:
        assert g[k] == ref[k], (name, k, g[k], ref[k])
    assert np.array_equal(g['mask'], ref['mask']), name
    assert np.array_equal(g['matched_index'], ref['matched_index']), name
    ids = p.get('point_id')
    assert np.array_equal(g['match_id'], ref['matched_index'] if ids is None else np.asarray(ids)[ref['matched_index']]), name
    assert np.array_equal(g['match_xy'], p['old_norm'][ref['matched_index']].astype(np.float64)), name
    if ref['status'] == SKIPPED:
        assert not any(np.asarray(g[k]).any() for k in VALUES), name
        return 0.0
    worst = 0.0
    # the winning sample's model against the reference's EPnP of that sample
    if ref['ransac_best'] >= 0:
        idx = list(schedule(n, p['max_iters'])[g['ransac_best']])
        m = {r: epnp(p['point_3d'][idx], p['old_norm'][idx], r) for r in ROUTES}
        assert min(x[2] for x in m.values()) >= 1e-6, (name, "the canonical row of the winning sample leads by less than 1e-6", [x[2] for x in m.values()])
        worst = max(worst, _ratio(g['sample_rvec'], m['ld'][0], [m['jac64'][0], m['svd64'][0]]), _ratio(g['sample_tvec'], m['ld'][1], [m['jac64'][1], m['svd64'][1]], 8.0))
        # on the device's model: the mask and the conditions
        e = errors(g['sample_rvec'], g['sample_tvec'], p['point_3d'], p['old_norm'], LD)
        thr2 = np.float32(p['reproj_threshold'] ** 2)
        assert np.array_equal((e <= thr2).astype(np.uint8), g['mask']), (name, "the mask of the device's own model")
        assert float(np.abs(e.astype(np.float64) - float(thr2)).min() / float(thr2)) >= 1e-6, name
    else:
        assert not g['sample_rvec'].any() and not g['sample_tvec'].any(), name
    if ref['status'] == NUMERIC:
        return worst
    # the returned pose: the reference's step 5 from the device's sample model and mask
    sample = (g['sample_rvec'], g['sample_tvec']) if ref['ransac_best'] >= 0 else None
    ps = {r: returned_pose(p, r, sample, g['mask']) for r in ROUTES}
    assert all(x[0] == g['status'] and x[3:] == (g['refit_iters'], g['refit_up']) for x in ps.values()), (name, [x[0:1] + x[3:] for x in ps.values()])
    worst = max(worst, _ratio(g['rvec'], ps['ld'][1], [ps['jac64'][1], ps['svd64'][1]]), _ratio(g['tvec'], ps['ld'][2], [ps['jac64'][2], ps['svd64'][2]], 8.0))
    # the pose algebra: the reference's step 6 on the device's rvec / tvec
    ts = {r: tail(p, g['rvec'], g['tvec'], g['n_inliers'], g['status'], ROUTES[r][0]) for r in ('ld', 'jac64')}
    assert ts['ld']['has_loop'] == g['has_loop'] and ts['ld']['gate_margin'] >= 1e-9, name
    scale = {'PnP_R_old': 1.0, 'PnP_T_old': 8.0, 'loop_info': 64.0}
    for k in scale:
        worst = max(worst, _ratio(g[k], ts['ld'][k], [ts['jac64'][k]], scale[k]))
    print(f"kf_pnp {tag} {name}: n {n} status {g['status']} inliers {g['n_inliers']} best {g['ransac_best']} iter {g['ransac_iter']} bound {g['ransac_bound']} "
          f"refit {g['refit_iters']}/{g['refit_up']} has_loop {g['has_loop']}  worst ratio {worst:.2f}")
    assert worst <= M, (name, worst)
    return worst


def check_cases(h, tag, names=None):
    """the cases in ONE call"""
    names = list(names or CASE_ARGS)
    got = dict(zip(names, _fe().kf_pnp(h, [case(n) for n in names])))
    worst = max((check_pair(n, case(n), got[n], tag), n) for n in names)
    print(f"kf_pnp {tag}: worst ratio {worst[0]:.3f} ({worst[1]}; bound {M})")
    return got


def check_capacity(h, tag):
    g = _fe().kf_pnp(h, [capacity_scene()])[0]
    check_pair('capacity', capacity_scene(), g, tag)


def batch(n, seed=300):
    """n pairs, sizes and statuses mixed"""
    names = ('n27', 'skipped', 'n65', 'no_model', 'n6', 'exactly_min', 'n150_out60', 'yaw_beyond', 'n150_clean')
    return [case(names[i % len(names)]) if i % 4 else scene(seed + i, n=30 + 7 * (i % 13), outlier=0.1 * (i % 5), refine=i % 2) for i in range(n)]


def check_batch_equals_single(h, sizes=(1, 3, 33)):
    fe = _fe()
    for n in sizes:
        prs = batch(n)
        together = fe.kf_pnp(h, prs)
        for i, pr in enumerate(prs):
            assert same_output(together[i], fe.kf_pnp(h, [pr])[0]), (n, i)
        assert len({g['status'] for g in together}) >= min(n, 2) or n == 1


def check_failed_neighbours(h):
    """a pair without a model between two good ones: the good ones are what they are alone"""
    fe = _fe()
    prs = [case('n150'), case('no_model'), case('n65')]
    g = fe.kf_pnp(h, prs)
    assert [x['status'] for x in g] == [OK, NO_MODEL, OK]
    assert same_output(g[0], fe.kf_pnp(h, [prs[0]])[0]) and same_output(g[2], fe.kf_pnp(h, [prs[2]])[0])


def _refusals():
    nan3 = case('n27')['point_3d'].copy()
    nan3[5, 1] = np.nan
    inf2 = case('n27')['old_norm'].copy()
    inf2[3, 0] = np.inf
    return {
        'struct_size': dict(struct_size=8), 'out_struct_size': dict(out_struct_size=8), 'n_5': dict(n=5), 'n_1025': dict(n=1025),
        'null_point_3d': dict(point_3d=None, n=27), 'null_old_norm': dict(old_norm=None, n=27), 'nan_point': dict(point_3d=nan3),
        'inf_obs': dict(old_norm=inf2), 'nan_T': dict(origin_vio_T=[0.0, np.nan, 0.0]), 'inf_qic': dict(qic=np.full(9, np.inf)),
        'threshold_0': dict(reproj_threshold=0.0), 'yaw_gate_negative': dict(max_yaw_deg=-1.0), 'dist_gate_0': dict(max_dist=0.0),
        'max_iters_0': dict(max_iters=0), 'max_iters_1001': dict(max_iters=1001), 'confidence_0.999': dict(confidence=0.999),
        'refine_2': dict(refine=2), 'refine_-1': dict(refine=-1),
    }


REFUSALS = tuple(_refusals())


def check_refusal(h, name):
    """refused with VG_ERR_BAD_ARG, nothing moved (the good neighbour's outputs too), the handle usable"""
    fe = _fe()
    good = case('n27')
    bad = dict(good)
    bad.update(_refusals()[name])
    want = fe.kf_pnp(h, [good])[0]
    L = h.lib
    ins, outs = (fe.KfPnpIn * 2)(), (fe.KfPnpOut * 2)()
    keep = []
    for i, p in enumerate((good, bad)):
        L.vg_kf_pnp_defaults(fe.C.byref(ins[i]))
        p3 = None if p.get('point_3d') is None else np.ascontiguousarray(p['point_3d'], np.float32)
        p2 = None if p.get('old_norm') is None else np.ascontiguousarray(p['old_norm'], np.float32)
        ins[i].n = int(p.get('n', 27))
        ins[i].point_3d = None if p3 is None else p3.ctypes.data_as(fe._f4)
        ins[i].old_norm = None if p2 is None else p2.ctypes.data_as(fe._f4)
        for k, cnt in (('origin_vio_T', 3), ('origin_vio_R', 9), ('tic', 3), ('qic', 9)):
            setattr(ins[i], k, (fe.C.c_double * cnt)(*np.asarray(p[k], np.float64).reshape(-1)))
        for k in fe._KF_PNP_SCALARS:
            if k in p:
                setattr(ins[i], k, p[k])
        if 'struct_size' in p:
            ins[i].struct_size = p['struct_size']
        mask = np.full(1024, 7, np.uint8)
        outs[i].struct_size = p.get('out_struct_size', fe.C.sizeof(fe.KfPnpOut))
        outs[i].status, outs[i].n_inliers, outs[i].has_loop = -5, -6, -7
        outs[i].mask = mask.ctypes.data_as(fe._u8)
        keep.append((p3, p2, mask))
    rc = L.vg_kf_pnp(h.h, 2, ins, outs)
    assert rc == -1, (name, rc)                            # VG_ERR_BAD_ARG
    for i in range(2):
        assert (outs[i].status, outs[i].n_inliers, outs[i].has_loop) == (-5, -6, -7) and (keep[i][2] == 7).all(), (name, i)
    assert same_output(fe.kf_pnp(h, [good])[0], want), name


# --------------------------------------------------------------------------------------------------- the chain into the relocalisation frame
def chain_pair(m, ids, seed=40):
    """The caller's side of findConnection for a match result m (kf_brief_ref.match / KeyFrames.match): point_3d such that the matched old
    points are their projections in an old camera (30 % of them spoiled), point_id = ids, the VIO pose 5 degrees of yaw and 0.8 away."""
    rng = np.random.default_rng(seed)
    n = int(m['n_matched'])
    on = np.asarray(m['matched_old_norm'], np.float32)[:n]
    Rc, Tc = _rot([0.1, -0.05, 0.2]), np.array([0.5, -0.3, 0.2])
    z = rng.uniform(3.0, 9.0, n)
    pc = np.stack([on[:, 0] * z, on[:, 1] * z, z], axis=1)
    P3 = pc @ Rc.T + Tc
    bad = rng.permutation(n)[:int(round(0.3 * n))]
    P3[bad] += rng.uniform(0.5, 1.5, (len(bad), 3)) * rng.choice([-1.0, 1.0], (len(bad), 3))
    return dict(point_3d=P3.astype(np.float32), old_norm=on, point_id=np.asarray(ids, np.int32)[:n], origin_vio_R=_rot([0.0, 0.0, np.deg2rad(5.0)]) @ Rc,
                origin_vio_T=Tc + np.array([0.6, -0.5, 0.1]), tic=np.zeros(3), qic=np.eye(3))


def check_chain(h_seq, h_ref, size=(100, 70)):
    """vg_kf_add -> vg_kf_match -> vg_kf_pnp -> vg_ba_seq_set_relo -> a step -> vg_ba_seq_get_relo on the rendered frames of kf_brief_ref.py and
    the scene of seq_relo_case.py: the armed step equals, bit for bit, the one whose relocalisation frame is built from the reference's
    lists (NumPy match, NumPy PnPRANSAC).  The lists are decisions and pass-through float32, so equality is the bar."""
    import kf_brief_ref as KB
    import seq_relo_case as R
    fe = _fe()
    w, _, mref = KB.rendered_pair(size)
    kf = fe.KeyFrames(h_seq, size[0], size[1], 150, 150, 2, KB.pattern())
    kf.add([0, 1], KB.frames(size), [KB.camera_struct(KB.cameras(size[0])["pinhole"])] * 2, [w, np.zeros((0, 2), np.float32)], arrays=False)
    mdev = kf.match([(0, 1)])[0]
    assert mdev['n_matched'] == mref['n_matched'] == KB.N_RENDERED > DEFAULTS['min_loop_num']
    seen = {}

    def ids_of(win):
        ids = sorted({int(ft['id']) for ft in win.features})[:KB.N_RENDERED]
        while len(ids) < KB.N_RENDERED:
            ids.append(ids[-1] + 3)
        return ids

    def request(route, win, prob):
        if route == 'device':
            pair = chain_pair(mdev, ids_of(win))
            g = fe.kf_pnp(h_seq, [pair])[0]
            check_pair('chain', pair, g, 'chain')
            assert g['status'] == OK and g['has_loop'] == 1 and g['n_inliers'] > DEFAULTS['min_loop_num']
            lists = (g['match_id'], g['match_xy'])
        else:
            pair = chain_pair(mref, ids_of(win))
            r = reference(pair)
            assert r['status'] == OK and r['has_loop'] == 1
            lists = (pair['point_id'][r['matched_index']], pair['old_norm'][r['matched_index']].astype(np.float64))
        seen[route] = lists
        base = R.standard_request(win, prob, frame=3)
        return dict(frame=3, pose=base['pose'], match_id=lists[0], match_xy=lists[1], prev_t=base['prev_t'], prev_r=base['prev_r'])

    out = {}
    for route in ('device', 'reference'):
        armed = {}

        def check(step, w_, host, flag, dev, armed=armed):
            if host.last['relo'] is not None:
                armed[(step, w_)] = dev
        R.run(h_seq, h_ref, [22, 23], {(1, 0): lambda win, prob, route=route: request(route, win, prob)}, K=11, L=40, n_steps=2, max_match=128, check=check,
              prepare=R.ascending)
        assert list(armed) == [(1, 0)]
        out[route] = armed[(1, 0)]
    assert np.array_equal(seen['device'][0], seen['reference'][0]) and np.array_equal(seen['device'][1], seen['reference'][1])
    a, b = out['device'], out['reference']
    assert a['relo']['armed'] == 1 and a['relo']['n_factors'] > 0, a['relo']
    for k in a['relo']:
        assert np.array_equal(np.asarray(a['relo'][k]), np.asarray(b['relo'][k])), ('relo', k)
    for k in a['state']:
        assert np.array_equal(np.asarray(a['state'][k]), np.asarray(b['state'][k])), ('state', k)
    assert a['info'] == b['info']
    print(f"kf_pnp chain: {KB.N_RENDERED} matches -> {len(seen['device'][0])} survivors -> {a['relo']['n_factors']} relocalisation factors; the armed step is bit-identical")


# --------------------------------------------------------------------------------------------------- the stand-alone program's files
def write_file(path, pair):
    """KPN1: magic, n, min_loop_num, max_iters, refine | reproj_threshold, max_yaw_deg, max_dist, T 3, R 9, tic 3, qic 9 | point_3d | old_norm | ids"""
    p = full(pair)
    n = len(p['point_3d'])
    with open(path, 'wb') as f:
        f.write(struct.pack('<5i', 0x314E504B, n, p['min_loop_num'], p['max_iters'], p['refine']))
        f.write(np.concatenate([[p['reproj_threshold'], p['max_yaw_deg'], p['max_dist']], np.asarray(p['origin_vio_T'], float).reshape(-1),
                                np.asarray(p['origin_vio_R'], float).reshape(-1), np.asarray(p['tic'], float).reshape(-1),
                                np.asarray(p['qic'], float).reshape(-1)]).astype('<f8').tobytes())
        f.write(p['point_3d'].astype('<f4').tobytes())
        f.write(p['old_norm'].astype('<f4').tobytes())
        f.write(np.asarray(p['point_id'], '<i4').tobytes())


# --------------------------------------------------------------------------------------------------- the C++ class through the replay tool
REPLAY_CASES = ('n150', 'refine_out30', 'yaw_beyond', 'no_model', 'exactly_min', 'skipped')


def check_replay(h, exe, tmp_dir, name):
    """`vins_replay kfpnp` (KeyFrame::PnPRANSAC, findConnection's second half, vg_pack_kf_pnp) against the binding, number for number"""
    import subprocess
    fe = _fe()
    pair = case(name)
    n = len(pair['point_3d'])
    src, dst = os.path.join(str(tmp_dir), name + '.bin'), os.path.join(str(tmp_dir), name + '.txt')
    write_file(src, pair)
    r = subprocess.run([exe, 'kfpnp', src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in open(dst).read().splitlines()]
    by = {}
    for row in rows:
        by.setdefault(row[0], []).append(row[1:])
    alone = dict(pair, min_loop_num=min(25, n - 1))
    del alone['point_id']
    a, g = fe.kf_pnp(h, [alone])[0], fe.kf_pnp(h, [pair])[0]
    num = lambda xs: np.array([float(x) for x in xs])
    assert [int(x) for x in by['pnp'][0]] == [a['status'], a['n_inliers']], name
    assert np.array_equal(np.array(by['status'][0], int), a['mask']), name
    assert np.array_equal(num(by['R'][0]), a['PnP_R_old'].reshape(-1)) and np.array_equal(num(by['T'][0]), a['PnP_T_old']), name
    skipped = g['status'] == SKIPPED
    last = a if skipped else g
    assert [int(x) for x in by['connection'][0]] == [g['has_loop'], g['status'], g['has_loop'], 3 if g['has_loop'] else -1, n if skipped else g['n_inliers']], (name, by['connection'])
    assert np.array_equal(num(by['loop_info'][0]), g['loop_info'] if g['has_loop'] else np.zeros(8)), name
    assert [int(x) for x in by['taps'][0]] == [last[k] for k in ('ransac_best', 'ransac_iter', 'ransac_bound', 'refit_iters', 'refit_up')], name
    assert np.array_equal(num(by['pose'][0]), np.concatenate([last['rvec'], last['tvec']])), name
    ms = by.get('m', [])
    if g['has_loop']:
        assert [int(m[0]) for m in ms] == list(g['match_id']) and np.array_equal(np.array([[float(m[1]), float(m[2])] for m in ms]), g['match_xy']), name
        assert np.array_equal(num(by['tq'][0]), np.array([0.1, 0.2, 0.3, 1.0, 0.0, 0.0, 0.0, 7.0])), name
    else:
        assert not ms, name
