"""Reference, scene generator, case table, metric and edits for vg_init_sfm (helper module of tests/test_init_sfm_def.py,
test_init_sfm_simt.py and test_init_sfm_gpu.py; no tests in here).

`sfm(win, dtype, route)` restates what include/vinsgpu.h defines for vg_init_sfm: GlobalSFM::construct (initial/initial_sfm.cpp), the
chain and per-frame PnP (OpenCV's guess branch, restated), the full BA (Ceres' trust-region loop with the LEVENBERG_MARQUARDT strategy)
and the frame stage of Estimator::initialStructure (estimator.cpp:286-353).  The inputs are the float64 inputs, widened.
    dtype = np.longdouble, route 'ld'     the 80-bit reference (one-sided Jacobi SVD, pivoted Gaussian elimination, in 80 bits)
    dtype = np.float64,    route 'solve'  numpy.linalg (svd, solve, cholesky), sums ascending
    dtype = np.float64,    route 'ldlt'   one-sided Jacobi SVD, unpivoted LDL^T / Cholesky written out, sums descending
`edit` (one of EDITS) changes one documented item; each must exceed the device's bound on some case.

The scene (`scene`): cameras on an analytic trajectory looking at random landmarks in front of them, tracks over consecutive frames
(some born late, some dying early, some of length 1), observation noise in units of 1 / 460, relative_R / T from the true poses of l
and F - 1 (optionally perturbed), optional non-key frames between the key frames.

A PnP compares the error norm of a step with the one before (`grew`).  Once a PnP has converged below float64's resolution a further
iteration compares two norms that differ by less than their rounding, and the outcome belongs to no definition.  Every residual is a
projected coordinate minus an observed one, so it carries an absolute error of about 2^-53 max|p|, and so does, at worst, the norm.  The
80-bit route records the smallest difference it compared in that unit, `pnp_margin`; the table holds only scenes whose margin is at
least PNP_MARGIN = 8.

The metric: decisions (status, state[], pnp_iters / pnp_up, the BA accept flags, ba_iters, ba_termination) must EQUAL the 80-bit
route's; values are measured per group as max|d| / max|ref| against the 80-bit route and held to M x E64, E64 = the larger error of
the two float64 routes in that group on that case, floored by the group's largest E64 over the table's cases of the same kind:
those whose BA converges, and those whose BA runs out of iterations (`e64_floor`; never looser than the floor over the whole table)."""
import functools

import numpy as np

import imu_ref
import init_align_ref as A

LD = np.longdouble
M = imu_ref.M
OK, FAILED_PNP, FAILED_BA, FAILED_FRAME, NUMERIC = 0, 1, 2, 3, 4
NO_CONVERGENCE, CONVERGENCE, FAILURE = 0, 1, 2
MAX_ITERS = 50
EDITS = ('no_float32', 'stage3_first', 'stage5_first_two', 'threshold_15', 'T_last_free', 'no_normalisation', 'lm_unclamped', 'ric_dropped')
FLT_EPSILON = 2.0 ** -23
PNP_MARGIN = 8.0


# --------------------------------------------------------------------------------------------------- small math, any dtype
def _q_from_R(m, dtype):
    """Eigen's Quaterniond(Matrix3d), (w x y z)"""
    x, y, z, w = A._R2q(m, dtype)
    return np.array([w, x, y, z])


def _q2R(q):
    """Eigen's toRotationMatrix (no normalisation) of (w x y z)"""
    return A._q2R(np.array([q[1], q[2], q[3], q[0]]))


def _q_inverse(q):
    """Eigen's inverse(): the conjugate over the squared norm"""
    return np.array([q[0], -q[1], -q[2], -q[3]]) / (q @ q)


def _qmul(a, b):
    """(w x y z)"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx])


def _jacobi_vmin(D, tol):
    """the right singular vector of the smallest singular value by a one-sided (Hestenes) Jacobi SVD on the columns"""
    D = D.copy()
    n = D.shape[1]
    V = np.eye(n, dtype=D.dtype)
    for _ in range(60):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                a, b = D[:, p].copy(), D[:, q].copy()
                alpha, beta, gamma = a @ a, b @ b, a @ b
                if gamma != 0 and abs(gamma) > tol * np.sqrt(alpha * beta):
                    rotated = True
                    zeta = (beta - alpha) / (2 * gamma)
                    t = (1 if zeta >= 0 else -1) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + t * t)
                    s = c * t
                    D[:, p], D[:, q] = c * a - s * b, s * a + c * b
                    va, vb = V[:, p].copy(), V[:, q].copy()
                    V[:, p], V[:, q] = c * va - s * vb, s * va + c * vb
        if not rotated:
            break
    return V[:, int(np.argmin((D * D).sum(axis=0)))]


def _sum0(a, route):
    """the sum over axis 0, ascending or (route 'ldlt') descending"""
    return (a[::-1] if route == 'ldlt' else a).sum(axis=0)


def _cholesky_solve(S, b, route):
    """x = S^-1 b for a symmetric positive definite S; None when it is not"""
    if route == 'solve':
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return None
        return np.linalg.solve(L.T, np.linalg.solve(L, b))
    n = len(b)
    L = np.zeros_like(S)
    for j in range(n):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not (d > 0 and np.isfinite(np.float64(d))):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros_like(b)
    for j in range(n):
        y[j] = (b[j] - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros_like(b)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


# --------------------------------------------------------------------------------------------------- Rodrigues, regular branch
def _rodrigues_R2r(R, dtype):
    """rotation matrix -> rvec; None in the near-pi branch"""
    r = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((r @ r) * dtype(0.25))
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) * dtype(0.5)
    c = min(max(c, dtype(-1)), dtype(1))
    theta = np.arccos(c)
    if s < 1e-5:
        if c > 0:
            return np.zeros(3, dtype)
        return None
    return r * (theta / (2 * s))


_DRX = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0], [0, 0, 1, 0, 0, 0, -1, 0, 0], [0, -1, 0, 1, 0, 0, 0, 0, 0]], float)  # d[r]x / d r_i


def _rodrigues_r2R(rv, dtype):
    """rvec -> (R, dR/dr [3][3][3]: dR[i] = dR / d r_i)"""
    theta = np.sqrt(rv @ rv)
    I = np.eye(3, dtype=dtype)
    if theta < 2.0 ** -52:
        return I, np.array([_DRX[i].reshape(3, 3).astype(dtype) for i in range(3)])
    c, s, it = np.cos(theta), np.sin(theta), 1 / theta
    c1 = 1 - c
    r = rv * it
    rrt = np.outer(r, r)
    rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    R = c * I + c1 * rrt + s * rx
    dR = []
    for i in range(3):
        ri = r[i]
        a0, a1, a2, a3, a4 = -s * ri, (s - 2 * c1 * it) * ri, c1 * it, (c - s * it) * ri, s * it
        e = np.zeros(3, dtype)
        e[i] = 1
        drrt = np.outer(e, r) + np.outer(r, e)
        dR.append(a0 * I + a1 * rrt + a2 * drrt + a3 * rx + a4 * _DRX[i].reshape(3, 3).astype(dtype))
    return R, np.array(dR)


def _pow10(k, dtype):
    return dtype(10) ** k if k >= 0 else 1 / dtype(10) ** (-k)


def _solve6(Am, b, route):
    if route == 'ld':
        x = A._solve_pivoted_plain(Am, b)
        d = np.diag(Am)
        return x if np.all(np.isfinite(x.astype(np.float64))) and np.all(d > 0) else None
    if route == 'solve':
        try:
            x = np.linalg.solve(Am, b)
        except np.linalg.LinAlgError:
            return None
        return x if np.all(np.isfinite(x)) else None
    return A._solve_ldlt(Am, b)


def pnp(R0, t0, P3, p2, dtype, route, edit=None):
    """cv::solvePnP(..., useExtrinsicGuess, SOLVEPNP_ITERATIVE) as the header restates it.  Returns (R, t, iters, ups) or None
    (the near-pi branch, or a pivot that is not positive and finite)."""
    if edit != 'no_float32':
        P3 = P3.astype(np.float32).astype(dtype)
        p2 = p2.astype(np.float32).astype(dtype)
    rv = _rodrigues_R2r(R0, dtype)
    if rv is None:
        return None
    par = np.concatenate([rv, t0])

    def project(par, jac):
        R, dR = _rodrigues_r2R(par[:3], dtype)
        X = P3 @ R.T + par[3:]
        z = 1 / X[:, 2]
        x, y = X[:, 0] * z, X[:, 1] * z
        err = np.stack([x - p2[:, 0], y - p2[:, 1]], axis=1)
        if not jac:
            return err, None
        J = np.zeros((len(P3), 2, 6), dtype)
        for i in range(3):
            dX = P3 @ dR[i].T
            J[:, 0, i] = z * (dX[:, 0] - x * dX[:, 2])
            J[:, 1, i] = z * (dX[:, 1] - y * dX[:, 2])
        J[:, 0, 3], J[:, 0, 5] = z, -x * z
        J[:, 1, 4], J[:, 1, 5] = z, -y * z
        return err, J

    def norm2(err):
        return _sum0((err * err).sum(axis=1), route)

    k, iters, ups = -3, 0, 0
    prev_norm, margin, pmax = None, np.inf, float(np.abs(p2).max())
    while True:
        err, J = project(par, True)
        JtJ = _sum0(np.einsum('nra,nrb->nab', J, J), route)
        Jte = _sum0(np.einsum('nra,nr->na', J, err), route)
        if iters == 0:
            prev_norm = np.sqrt(norm2(err))
        prev = par.copy()

        def step():
            lam = _pow10(k, dtype)
            An = JtJ.copy()
            An[np.diag_indices(6)] *= 1 + lam
            d = _solve6(An, Jte, route)
            return None if d is None else prev - d
        par = step()
        if par is None:
            return None
        while True:
            nrm = np.sqrt(norm2(project(par, False)[0]))
            if not np.isfinite(np.float64(nrm)):
                return None
            margin = min(margin, float(abs(nrm - prev_norm) / (2.0 ** -53 * pmax)))
            if nrm > prev_norm and k + 1 <= 16:
                k += 1
                ups += 1
                par = step()
                if par is None:
                    return None
                continue
            if nrm > prev_norm:
                k += 1
            break
        k = max(k - 1, -16)
        iters += 1
        d = par - prev
        if iters >= 20 or np.sqrt(d @ d) / (np.sqrt(prev @ prev) + dtype(2.0 ** -52)) < FLT_EPSILON:
            break
        prev_norm = nrm
    if not np.all(np.isfinite(par.astype(np.float64))):
        return None
    return _rodrigues_r2R(par[:3], dtype)[0], par[3:], iters, ups, margin


# --------------------------------------------------------------------------------------------------- the BA
def _rotate(q, X, normalise=True):
    """ceres::QuaternionRotatePoint of (w x y z): (p [n][3], dp/dq [n][3][4], R(u))"""
    s = 1 / np.sqrt(q @ q) if normalise else q.dtype.type(1)
    a, b, c, d = q * s
    t2, t3, t4, t5, t6, t7, t8, t9, t1 = a * b, a * c, a * d, -b * b, b * c, b * d, -c * c, c * d, -d * d
    Mx = np.array([[t8 + t1, t6 - t4, t3 + t7], [t4 + t6, t5 + t1, t9 - t2], [t7 - t3, t2 + t9, t5 + t8]])
    p = 2 * (X @ Mx.T) + X
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    G = np.zeros((len(X), 3, 4), q.dtype)
    G[:, :, 0] = 2 * np.stack([c * X2 - d * X1, d * X0 - b * X2, b * X1 - c * X0], axis=1)
    G[:, :, 1] = 2 * np.stack([c * X1 + d * X2, c * X0 - 2 * b * X1 - a * X2, d * X0 + a * X1 - 2 * b * X2], axis=1)
    G[:, :, 2] = 2 * np.stack([-2 * c * X0 + b * X1 + a * X2, b * X0 + d * X2, -a * X0 + d * X1 - 2 * c * X2], axis=1)
    G[:, :, 3] = 2 * np.stack([-2 * d * X0 - a * X1 + b * X2, a * X0 - 2 * d * X1 + c * X2, b * X0 + c * X1], axis=1)
    if normalise:
        u = np.array([a, b, c, d])
        G = s * (G - np.einsum('nr,k->nrk', G @ u, u))
    return p, G, 2 * Mx + np.eye(3, dtype=q.dtype)


def _plus_jacobian(q):
    """ceres::QuaternionParameterization::ComputeJacobian, 4 x 3"""
    w, x, y, z = q
    return np.array([[-x, -y, -z], [w, z, -y], [-z, w, x], [y, -x, w]])


def _quat_plus(q, d):
    n = np.sqrt(d @ d)
    if n > 0:
        s = np.sin(n) / n
        return _qmul(np.array([np.cos(n), s * d[0], s * d[1], s * d[2]]), q)
    return q.copy()


class _Problem:
    """the observations of the triangulated features, frame by frame, and the free columns"""

    def __init__(self, F, l, feats, state, dtype, route, edit):
        self.F, self.l, self.dtype, self.route, self.edit = F, l, dtype, route, edit
        self.idx = [j for j in range(len(feats)) if state[j]]
        fr, ft, uv = [], [], []
        for k, j in enumerate(self.idx):
            s0, xy = feats[j]
            for o in range(len(xy)):
                fr.append(s0 + o)
                ft.append(k)
                uv.append(xy[o])
        self.fr, self.ft, self.uv = np.array(fr, int), np.array(ft, int), np.array(uv, dtype).reshape(-1, 2)
        free = np.ones((F, 6), bool)
        free[l, :] = False
        if edit != 'T_last_free':
            free[F - 1, 3:] = False
        self.free = free.reshape(-1)

    def evaluate(self, cq, ct, X, jac):
        """cost, r [n][2], and Jc [n][2][6] (rotation tangent | translation), Jp [n][2][3]"""
        n, dt = len(self.fr), self.dtype
        r, Jc, Jp = np.zeros((n, 2), dt), np.zeros((n, 2, 6), dt), np.zeros((n, 2, 3), dt)
        for f in range(self.F):
            m = self.fr == f
            if not m.any():
                continue
            p, G, Ru = _rotate(cq[f], X[self.ft[m]], self.edit != 'no_normalisation')
            p = p + ct[f]
            iz = 1 / p[:, 2]
            xp, yp = p[:, 0] * iz, p[:, 1] * iz
            r[m] = np.stack([xp - self.uv[m, 0], yp - self.uv[m, 1]], axis=1)
            if jac:
                dr = np.zeros((int(m.sum()), 2, 3), dt)
                dr[:, 0, 0], dr[:, 0, 2] = iz, -xp * iz
                dr[:, 1, 1], dr[:, 1, 2] = iz, -yp * iz
                Jc[m, :, :3] = dr @ (G @ _plus_jacobian(cq[f]))
                Jc[m, :, 3:] = dr
                Jp[m] = dr @ Ru
        cost = _sum0((r * r).sum(axis=1), self.route) / 2
        return cost, r, Jc, Jp

    def by_frame(self, v):
        """sum of v [n][...] per frame -> [F][...]"""
        out = np.zeros((self.F,) + v.shape[1:], self.dtype)
        for f in range(self.F):
            m = self.fr == f
            if m.any():
                out[f] = _sum0(v[m], self.route)
        return out

    def by_feature(self, v):
        out = np.zeros((len(self.idx),) + v.shape[1:], self.dtype)
        order = range(len(self.fr) - 1, -1, -1) if self.route == 'ldlt' else range(len(self.fr))
        for o in order:
            out[self.ft[o]] += v[o]
        return out


def _ba(F, l, feats, state, cq, ct, pos, dtype, route, edit):
    """Ceres' TrustRegionMinimizer with the LEVENBERG_MARQUARDT strategy, as the header restates it.  Returns the summary dict;
    cq, ct, pos are updated in place."""
    P = _Problem(F, l, feats, state, dtype, route, edit)
    nk = len(P.idx)
    X = np.array([pos[j] for j in P.idx], dtype).reshape(nk, 3)
    free = P.free
    one = dtype(1)

    def linearise(cq, ct, X):
        cost, r, Jc, Jp = P.evaluate(cq, ct, X, True)
        return cost, r, Jc, Jp

    def ambient(cq, ct, X):
        parts = []
        for f in range(F):
            if free[6 * f]:
                parts.append(cq[f])
            if free[6 * f + 3]:
                parts.append(ct[f])
        parts.append(X.reshape(-1))
        return np.concatenate(parts)

    cost, r, Jc, Jp = linearise(cq, ct, X)
    sc = one / (one + np.sqrt(P.by_frame((Jc * Jc).sum(axis=1)).reshape(-1)))
    sp = one / (one + np.sqrt(P.by_feature((Jp * Jp).sum(axis=1))))
    summ = dict(trace=[], termination=NO_CONVERGENCE, initial_cost=cost)

    def gradient_max(r, Jc, Jp):
        gc = P.by_frame(np.einsum('nra,nr->na', Jc, r)).reshape(-1)
        gp = P.by_feature(np.einsum('nra,nr->na', Jp, r))
        return max(np.abs(gc[free]).max(initial=0), np.abs(gp).max(initial=0))

    radius, dec, invalid, it = dtype(1e4), dtype(2), 0, 0
    x_norm = np.sqrt((ambient(cq, ct, X) ** 2).sum())
    if gradient_max(r, Jc, Jp) <= 1e-10:
        summ['termination'] = CONVERGENCE
    else:
        while it < MAX_ITERS:
            it += 1
            Jcs, Jps = Jc * sc.reshape(F, 6)[P.fr][:, None, :], Jp * sp[P.ft][:, None, :]
            dc = P.by_frame((Jcs * Jcs).sum(axis=1)).reshape(-1)
            dp = P.by_feature((Jps * Jps).sum(axis=1))
            if edit != 'lm_unclamped':
                dc, dp = np.clip(dc, dtype(1e-6), dtype(1e32)), np.clip(dp, dtype(1e-6), dtype(1e32))
            Dc, Dp = np.sqrt(dc / radius), np.sqrt(dp / radius)
            # ---- DENSE_SCHUR: the points first
            U = P.by_frame(np.einsum('nra,nrb->nab', Jcs, Jcs))                    # [F][6][6]
            V = P.by_feature(np.einsum('nra,nrb->nab', Jps, Jps))                  # [nk][3][3]
            gc = P.by_frame(np.einsum('nra,nr->na', Jcs, r)).reshape(-1)
            gp = P.by_feature(np.einsum('nra,nr->na', Jps, r))
            V[:, [0, 1, 2], [0, 1, 2]] += Dp * Dp
            W = np.zeros((nk, 6 * F, 3), dtype)
            Wo = np.einsum('nra,nrb->nab', Jcs, Jps)
            for o in range(len(P.fr)):
                W[P.ft[o], 6 * P.fr[o]:6 * P.fr[o] + 6] = Wo[o]
            rec = dict(cost=cost, radius=radius, valid=False, accepted=False, cost_cand=dtype(0), model=dtype(0))
            y = None
            Vi = _inv3(V)
            if Vi is not None:
                S = np.zeros((6 * F, 6 * F), dtype)
                for f in range(F):
                    S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = U[f]
                S[np.diag_indices(6 * F)] += Dc * Dc
                Y = np.einsum('jak,jkm->jam', W, Vi)
                S = S - _sum0(np.einsum('jam,jbm->jab', Y, W), route)
                rhs = gc - _sum0(np.einsum('jam,jm->ja', Y, gp), route)
                yc = np.zeros(6 * F, dtype)
                sol = _cholesky_solve(S[np.ix_(free, free)], rhs[free], route) if route != 'ld' else _ld_spd_solve(S[np.ix_(free, free)], rhs[free])
                if sol is not None:
                    yc[free] = sol
                    yp = np.einsum('jkm,jm->jk', Vi, gp - np.einsum('jam,a->jm', W, yc))
                    if np.all(np.isfinite(yc.astype(np.float64))) and np.all(np.isfinite(yp.astype(np.float64))):
                        y = (-yc, -yp)
            if y is not None:
                stc, stp = y
                Js = np.einsum('nra,na->nr', Jcs, stc.reshape(F, 6)[P.fr]) + np.einsum('nra,na->nr', Jps, stp[P.ft])
                model = -_sum0((Js * (r + Js / 2)).sum(axis=1), route)
                rec['model'] = model
            if y is None or not (model > 0):
                summ['trace'].append(rec)
                invalid += 1
                if invalid >= 5:
                    summ['termination'] = FAILURE
                    break
                radius, dec = radius / dec, dec * 2
                continue
            invalid = 0
            rec['valid'] = True
            dcam, dpt = (stc * sc).reshape(F, 6), stp * sp
            cq2 = [(_quat_plus(cq[f], dcam[f, :3]) if free[6 * f] else cq[f].copy()) for f in range(F)]
            ct2 = [(ct[f] + dcam[f, 3:] if free[6 * f + 3] else ct[f].copy()) for f in range(F)]
            X2 = X + dpt
            cost2 = P.evaluate(cq2, ct2, X2, False)[0]
            rec['cost_cand'] = cost2
            dx = ambient(cq, ct, X) - ambient(cq2, ct2, X2)
            if np.sqrt((dx * dx).sum()) <= 1e-8 * (x_norm + 1e-8):
                summ['trace'].append(rec)
                summ['termination'] = CONVERGENCE
                break
            if abs(cost - cost2) <= 1e-6 * cost:
                summ['trace'].append(rec)
                summ['termination'] = CONVERGENCE
                summ['function_tolerance'] = True
                break
            rho = (cost - cost2) / model
            if rho > 1e-3:
                rec['accepted'] = True
                summ['trace'].append(rec)
                for f in range(F):
                    cq[f], ct[f] = cq2[f], ct2[f]
                X = X2
                x_norm = np.sqrt((ambient(cq, ct, X) ** 2).sum())
                cost, r, Jc, Jp = linearise(cq, ct, X)
                t = 2 * rho - 1
                radius = min(radius / max(one / 3, 1 - t * t * t), dtype(1e16))
                dec = dtype(2)
                if gradient_max(r, Jc, Jp) <= 1e-10:
                    summ['termination'] = CONVERGENCE
                    break
            else:
                summ['trace'].append(rec)
                radius, dec = radius / dec, dec * 2
                if radius < 1e-32:
                    summ['termination'] = CONVERGENCE
                    break
    for k, j in enumerate(P.idx):
        pos[j] = X[k]
    summ.update(final_cost=cost, iters=it)
    return summ


def _inv3(V):
    """the inverses of symmetric 3x3 blocks by the adjugate; None when a determinant is not positive and finite"""
    a, b, c, d, e, f = V[:, 0, 0], V[:, 1, 0], V[:, 1, 1], V[:, 2, 0], V[:, 2, 1], V[:, 2, 2]
    c00, c10, c20 = c * f - e * e, d * e - b * f, b * e - c * d
    det = a * c00 + b * c10 + d * c20
    if not np.all((det > 0) & np.isfinite(det.astype(np.float64))):
        return None
    c11, c21, c22 = a * f - d * d, b * d - a * e, a * c - b * b
    inv = np.empty_like(V)
    inv[:, 0, 0], inv[:, 1, 1], inv[:, 2, 2] = c00 / det, c11 / det, c22 / det
    inv[:, 1, 0] = inv[:, 0, 1] = c10 / det
    inv[:, 2, 0] = inv[:, 0, 2] = c20 / det
    inv[:, 2, 1] = inv[:, 1, 2] = c21 / det
    return inv


def _ld_spd_solve(S, b):
    d = np.diag(S)
    if not np.all(d > 0):
        return None
    x = A._solve_pivoted(S, b)
    return x if np.all(np.isfinite(x.astype(np.float64))) else None


# --------------------------------------------------------------------------------------------------- the restatement
def _pose(R, t):
    return np.concatenate([R, t.reshape(3, 1)], axis=1)


def _triangulate_point(P0, P1, p0, p1, dtype, route):
    D = np.stack([p0[0] * P0[2] - P0[0], p0[1] * P0[2] - P0[1], p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1]])
    if route == 'solve':
        v = np.linalg.svd(D)[2][3]
    else:
        v = _jacobi_vmin(D, 1e-19 if dtype is LD else 1e-16)
    with np.errstate(all='ignore'):
        return v[:3] / v[3]


def sfm(win, dtype=LD, route='ld', edit=None):
    """One window.  Returns status and the outputs of vg_sfm_out the status reaches (the rest absent)."""
    w = lambda v: np.asarray(v, np.float64).astype(dtype)
    F, l = int(win['n_frames']), int(win['l'])
    start, nobs = np.asarray(win['start'], int), np.asarray(win['nobs'], int)
    pts = w(win['points']).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum(nobs)])
    n = len(start)
    feats = [(int(start[j]), pts[off[j]:off[j + 1], :2]) for j in range(n)]
    ric = np.eye(3, dtype=dtype) if edit == 'ric_dropped' else w(win['ric']).reshape(3, 3)
    out = dict(status=NUMERIC, pnp_iters=np.zeros(F, int), pnp_up=np.zeros(F, int), pnp_margin=np.inf)
    state, pos = np.zeros(n, bool), np.zeros((n, 3), dtype)
    thr = 15 if edit == 'threshold_15' else 10
    # ---- construct
    q = [None] * F
    T = [None] * F
    q[l] = np.array([1, 0, 0, 0], dtype)
    T[l] = np.zeros(3, dtype)
    q[F - 1] = _qmul(q[l], _q_from_R(w(win['relative_R']).reshape(3, 3), dtype))
    T[F - 1] = w(win['relative_T'])
    cQ, cR, cT, Pose = [None] * F, [None] * F, [None] * F, [None] * F
    for i in (l, F - 1):
        cQ[i] = _q_inverse(q[i])
        cR[i] = _q2R(cQ[i])
        cT[i] = -(cR[i] @ T[i])
        Pose[i] = _pose(cR[i], cT[i])

    def obs_in(j, f):
        s0, xy = feats[j]
        return xy[f - s0] if s0 <= f < s0 + len(xy) else None

    def two_frames(f0, f1):
        for j in range(n):
            if state[j]:
                continue
            a, b = obs_in(j, f0), obs_in(j, f1)
            if a is not None and b is not None:
                X = _triangulate_point(Pose[f0], Pose[f1], a, b, dtype, route)
                if not np.all(np.isfinite(X.astype(np.float64))):
                    return False
                state[j], pos[j] = True, X
        return True

    def frame_pnp(i, guess):
        sel = [j for j in range(n) if state[j] and obs_in(j, i) is not None]
        if len(sel) < thr:
            return FAILED_PNP
        res = pnp(cR[guess], cT[guess], pos[sel], np.array([obs_in(j, i) for j in sel]), dtype, route, edit)
        if res is None:
            return NUMERIC
        cR[i], cT[i], out['pnp_iters'][i], out['pnp_up'][i] = res[:4]
        out['pnp_margin'] = min(out['pnp_margin'], res[4])
        cQ[i] = _q_from_R(cR[i], dtype)
        Pose[i] = _pose(cR[i], cT[i])
        return OK

    def stage3():
        for i in range(l + 1, F - 1):
            if not two_frames(l, i):
                return False
        return True

    for i in range(l, F - 1):
        if i > l:
            st = frame_pnp(i, i - 1)
            if st != OK:
                out['status'] = st
                return out
            if edit == 'stage3_first' and not two_frames(l, i):     # the edit: l with i as soon as i has a pose, before i with F - 1
                return out
        if not two_frames(i, F - 1):
            return out
    if not stage3():
        return out
    for i in range(l - 1, -1, -1):
        st = frame_pnp(i, i + 1)
        if st != OK:
            out['status'] = st
            return out
        if not two_frames(i, l):
            return out
    for j in range(n):
        s0, xy = feats[j]
        if state[j] or len(xy) < 2:
            continue
        k1 = 1 if edit == 'stage5_first_two' else len(xy) - 1
        X = _triangulate_point(Pose[s0], Pose[s0 + k1], xy[0], xy[k1], dtype, route)
        if not np.all(np.isfinite(X.astype(np.float64))):
            return out
        state[j], pos[j] = True, X
    out.update(state=state.copy(), q0=np.array(cQ), T0=np.array(cT), position0=pos.copy())
    # ---- full BA
    cq, ct = [x.copy() for x in cQ], [x.copy() for x in cT]
    summ = _ba(F, l, feats, state, cq, ct, pos, dtype, route, edit)
    out.update(ba_iters=summ['iters'], ba_termination=summ['termination'], final_cost=summ['final_cost'], trace=summ['trace'],
               function_tolerance=summ.get('function_tolerance', False))
    if summ['termination'] != CONVERGENCE and not (summ['final_cost'] < 5e-3):
        out['status'] = FAILED_BA
        return out
    Q, Tw = [], []
    for i in range(F):
        qi = _q_inverse(cq[i])
        Q.append(qi)
        Tw.append(-(_q2R(qi) @ ct[i]))
    out.update(q=np.array(Q), T=np.array(Tw), position=pos * state[:, None])
    # ---- the frames
    ids = {int(fid): j for j, fid in enumerate(win['feature_id'])}
    n_all = len(win['all_key'])
    R_all, T_all, is_key = np.zeros((n_all, 3, 3), dtype), np.zeros((n_all, 3), dtype), np.zeros(n_all, int)
    status = OK
    for a in range(n_all):
        i = int(win['all_key'][a])
        if i >= 0:
            is_key[a], R_all[a], T_all[a] = 1, _q2R(Q[i]) @ ric.T, Tw[i]
            continue
        g = int(win['all_guess'][a])
        Rg = _q2R(_q_inverse(Q[g]))
        fid, xy = win['all_pts'][a]
        sel = [(ids[int(f)], k) for k, f in enumerate(fid) if int(f) in ids and state[ids[int(f)]]]
        if len(sel) < 6:
            status = FAILED_FRAME if status == OK else status
            continue
        res = pnp(Rg, -(Rg @ Tw[g]), pos[[j for j, _ in sel]], w(xy).reshape(-1, 2)[[k for _, k in sel]], dtype, route, edit)
        if res is None:
            status = NUMERIC if status == OK else status
            continue
        out['pnp_margin'] = min(out['pnp_margin'], res[4])
        Rp = res[0].T
        R_all[a], T_all[a] = Rp @ ric.T, Rp @ (-res[1])
    out.update(status=status, R_all=R_all, T_all=T_all, is_key=is_key)
    return out


# --------------------------------------------------------------------------------------------------- the scene
PX = 1.0 / 460.0


def _tracks(rng, F, n_feat, len1):
    """(start, nobs) per feature: consecutive frames; about 40 % live through the window, the others are born late or die early,
    a share `len1` has one observation"""
    out = []
    for _ in range(n_feat):
        u = rng.random()
        if u < len1:
            out.append((int(rng.integers(0, F)), 1))
        elif u < len1 + 0.4 or F < 4:
            out.append((0, F))
        elif u < len1 + 0.7:
            s0 = int(rng.integers(1, F - 1))
            out.append((s0, F - s0))
        else:
            out.append((0, int(rng.integers(2, F))))
    return out


def scene(seed, F=11, n_feat=150, l=None, noise=0.005, tracks=None, nonkey=False, nonkey_matches=None, rel_noise=0.0, rel_scale=1.0,
          step=0.25, poses=None, depth=(3.0, 8.0), origin_feature=False, identity_rel=False):
    """The window dict of ba.Handle.init_sfm, with `truth`.  noise: pixels (1 / 460); tracks: an explicit (start, nobs) list;
    nonkey: one non-key frame inside every interval; nonkey_matches: {interval: number of ids of tracked features it sees};
    rel_noise: a rotation (rad) and a relative translation error put on relative_R / T; rel_scale: relative_R multiplied by it (a
    matrix that is no rotation); poses: (R [F], T [F], mid (R, T) [F - 1]) camera poses in a world frame instead of the built-in
    trajectory; origin_feature / identity_rel: the NaN-producing triangulation (a feature seen at (0, 0) in l and F - 1 with
    relative_R = I)."""
    rng = np.random.default_rng(seed)
    l = F // 2 if l is None else l
    if poses is None:
        amp, om, ph = rng.uniform(0.6, 1.2, 3) * step * 4, rng.uniform(0.6, 1.4, 3), rng.uniform(0, 2 * np.pi, 3)
        aamp, aom, aph = rng.uniform(0.03, 0.1, 3), rng.uniform(0.8, 2.0, 3), rng.uniform(0, 2 * np.pi, 3)
        pos = lambda t: amp * np.sin(om * t + ph)
        rot = lambda t: A._Rzyx(*(aamp * np.sin(aom * t + aph)))
        Rw, Tw = [rot(0.25 * i) for i in range(F)], [pos(0.25 * i) for i in range(F)]
        mid = [(rot(0.25 * i + 0.11), pos(0.25 * i + 0.11)) for i in range(F - 1)]
    else:
        Rw, Tw, mid = poses
    rel = lambda R, T: (Rw[l].T @ R, Rw[l].T @ (T - Tw[l]))
    cam = [rel(Rw[i], Tw[i]) for i in range(F)]
    base = np.linalg.norm(cam[F - 1][1])
    cam = [(R, T / base) for R, T in cam]
    mid = [(lambda RT: (RT[0], RT[1] / base))(rel(R, T)) for R, T in (mid or [])]
    tracks = list(tracks) if tracks is not None else _tracks(rng, F, n_feat, 0.1)
    n = len(tracks)
    ids = rng.permutation(np.arange(100, 100 + 3 * n))[:n]
    X, points = [], []
    dscale = 1.0 / base
    for j, (s0, k) in enumerate(tracks):
        c = int(rng.integers(s0, s0 + k))
        z = rng.uniform(*depth) * dscale * step * 4
        Xj = cam[c][1] + cam[c][0] @ np.array([rng.uniform(-0.45, 0.45) * z, rng.uniform(-0.35, 0.35) * z, z])
        X.append(Xj)
        for f in range(s0, s0 + k):
            p = cam[f][0].T @ (Xj - cam[f][1])
            points.append([p[0] / p[2] + rng.normal(0, noise) * PX, p[1] / p[2] + rng.normal(0, noise) * PX, 1.0])
    X, points = np.array(X).reshape(n, 3), np.array(points).reshape(-1, 3)
    relR, relT = cam[F - 1][0].copy(), cam[F - 1][1].copy()
    if rel_noise:
        relR = relR @ A._small_rotation(rng.normal(0, rel_noise, 3))
        relT = relT * (1 + rng.normal(0, rel_noise, 3))
    relR = relR * rel_scale
    if identity_rel:
        relR = np.eye(3)
    if origin_feature:
        j = next(j for j, (s0, k) in enumerate(tracks) if s0 <= l and s0 + k == F)
        o = int(np.sum([k for _, k in tracks[:j]]))
        points[o + l - tracks[j][0], :2] = 0.0
        points[o + F - 1 - tracks[j][0], :2] = 0.0
    ric = A._small_rotation(rng.normal(0, 0.2, 3))
    all_key, all_guess, all_pts = [], [], []
    for i in range(F):
        all_key.append(i); all_guess.append(i); all_pts.append(None)
        if nonkey and i < F - 1:
            Rm, Tm = mid[i]
            seen = [j for j, (s0, k) in enumerate(tracks) if s0 <= i and i + 1 < s0 + k]
            if nonkey_matches is not None and i in nonkey_matches:
                seen = seen[:nonkey_matches[i]]
            fid = [int(ids[j]) for j in seen] + [int(x) for x in rng.integers(5000, 6000, 3)]       # three ids the table does not hold
            xy = []
            for j in seen:
                p = Rm.T @ (X[j] - Tm)
                xy.append([p[0] / p[2] + rng.normal(0, noise) * PX, p[1] / p[2] + rng.normal(0, noise) * PX])
            xy += [[0.1, -0.2], [0.3, 0.1], [-0.2, 0.2]]
            order = np.argsort(fid)
            all_key.append(-1); all_guess.append(i + 1); all_pts.append((np.array(fid)[order], np.array(xy)[order]))
    return dict(n_frames=F, l=l, relative_R=relR, relative_T=relT, ric=ric, feature_id=ids, start=np.array([t[0] for t in tracks]),
                nobs=np.array([t[1] for t in tracks]), points=points, all_key=all_key, all_guess=all_guess, all_pts=all_pts,
                truth=dict(cam=cam, X=X, base=base))


# --------------------------------------------------------------------------------------------------- the cases
def _f3(full):
    """F = 3, l = 0: frame 1 is solved from exactly `full` points (the features seen in all three frames)"""
    return [(0, 3)] * full + [(1, 2)] * 8 + [(0, 2)] * 8 + [(2, 1)] * 2


# name -> scene arguments
CASE_ARGS = {
    'F3_10': dict(seed=1, F=3, l=0, tracks=_f3(10)),                                  # exactly 10 points: the chain goes on
    'F3_14': dict(seed=2, F=3, l=0, tracks=_f3(14)),                                  # 14: the reference only prints a warning
    'F3_9': dict(seed=5, F=3, l=0, tracks=_f3(9)),                                    # 9: VG_SFM_FAILED_PNP
    'F5_12': dict(seed=1, F=5, l=2, tracks=[(0, 5)] * 12),                            # 12 features, one partly filled wavefront
    'F5_nk6': dict(seed=8, F=5, l=1, n_feat=64, nonkey=True, nonkey_matches={1: 6}),  # a non-key frame with 6 matches
    'F5_nk5': dict(seed=8, F=5, l=1, n_feat=64, nonkey=True, nonkey_matches={1: 5}),  # 5: VG_SFM_FAILED_FRAME
    'F5_scaled': dict(seed=1, F=5, l=2, n_feat=65, rel_scale=1.02),                   # relative_R is no rotation: quaternions off the unit sphere
    'F5_nan': dict(seed=10, F=5, l=2, n_feat=40, identity_rel=True, origin_feature=True),     # w = 0 in a triangulation: VG_SFM_NUMERIC
    'F11_l0': dict(seed=2, F=11, l=0, n_feat=64),                                    # no backward chain
    'F11_mid': dict(seed=4, F=11, l=5, n_feat=150, nonkey=True),                      # the reference's shape, a non-key frame in every interval
    'F11_last': dict(seed=4, F=11, l=9, n_feat=65),                                  # l = F - 2: no forward PnP
    'F5_50_ok': dict(seed=28, F=5, l=2, n_feat=40, rel_noise=0.06),                   # a perturbed relative pose: 50 iterations, final_cost < 5e-3
    'F5_50_fail': dict(seed=50, F=5, l=2, n_feat=40, rel_noise=0.1),                  # 50 iterations with rejected steps, VG_SFM_FAILED_BA
    'F16': dict(seed=5, F=16, l=7, n_feat=300),                                      # the capacity in frames, more than one pass of features
}


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(**CASE_ARGS[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    return view(sfm(case(name)))


@functools.lru_cache(maxsize=None)
def route64(name, route):
    return view(sfm(case(name), np.float64, route))


# --------------------------------------------------------------------------------------------------- the metric
VALUE_KEYS = ('q0', 'T0', 'position0', 'ba_cost', 'q', 'T', 'position', 'R_all', 'T_all')


def view(o):
    """decisions and value groups of a result of sfm() or of Handle.init_sfm, in one shape"""
    if 'trace' in o or 'it_flags' not in o:                 # sfm()
        tr = o.get('trace', [])
        flags = [int(r['valid']) + 2 * int(r['accepted']) for r in tr]
        costs = [r['cost'] for r in tr] + [r['cost_cand'] for r in tr if r['valid']] + ([o['final_cost']] if 'final_cost' in o else [])
    else:
        flags = [int(x) for x in o['it_flags']]
        costs = list(o['it_cost']) + [c for c, f in zip(o['it_cost_cand'], flags) if f & 1] + ([o['final_cost']] if o['ba_iters'] or o['ba_termination'] else [])
    st = o.get('state')
    dec = dict(status=int(o['status']), state=tuple(int(x) for x in st) if st is not None else None, pnp_iters=tuple(int(x) for x in o['pnp_iters']),
               pnp_up=tuple(int(x) for x in o['pnp_up']), flags=tuple(flags), ba_iters=int(o.get('ba_iters', 0)), ba_termination=int(o.get('ba_termination', 0)))
    if dec['state'] is not None and not any(dec['state']):
        dec['state'] = None
    val = {k: np.asarray(o[k], LD).reshape(-1) for k in VALUE_KEYS if k != 'ba_cost' and k in o and np.asarray(o[k]).size and np.asarray(o[k], np.float64).any()}
    if costs:
        val['ba_cost'] = np.asarray(costs, LD)
    return dict(dec=dec, val=val, function_tolerance=bool(o.get('function_tolerance', False)), pnp_margin=float(o.get('pnp_margin', np.inf)))


def errors(got, ref):
    """{group: max|d| / max|ref|} for every group the reference has; inf for one `got` lacks, has in another shape or non-finite"""
    out = {}
    for k, r in ref['val'].items():
        g = got['val'].get(k)
        if g is None or g.shape != r.shape or not np.all(np.isfinite(g.astype(np.float64))):
            out[k] = np.inf
            continue
        out[k] = float(np.abs(g - r).max() / np.abs(r).max())
    return out


def e64(name):
    """{group: the larger error of the two float64 routes} on one case"""
    ref = reference(name)
    a, b = errors(route64(name, 'solve'), ref), errors(route64(name, 'ldlt'), ref)
    return {k: max(a[k], b[k]) for k in ref['val']}


def runs_out(name):
    """the BA of the case uses up its 50 iterations: 50 steps along a valley amplify the last bits of the start a thousandfold, and
    E64 of `position` and `ba_cost` is 1e-10 there against 1e-15 on the cases that converge"""
    return reference(name)['dec']['ba_iters'] >= MAX_ITERS


@functools.lru_cache(maxsize=None)
def e64_floor(run_out=False):
    """{group: the largest E64 over the cases of the table whose BA converges (or, run_out, over those whose BA runs out)}.  The floor
    over the WHOLE table, which is the least the metric asks for, is the larger of the two; holding the converging cases to their own
    keeps the device's `position` and `ba_cost` within five more digits."""
    out = {}
    for n in CASE_ARGS:
        if runs_out(n) != run_out:
            continue
        for k, v in e64(n).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def bound(name):
    """{group: M x E64}: the case's own, floored by the group's largest over the cases of its kind (`e64_floor`)"""
    fl = e64_floor(runs_out(name))
    return {k: M * max(v, fl[k]) for k, v in e64(name).items()}


def ratios(got, name):
    """{group: error / E64 (floored)}: the device may reach M"""
    e, b = errors(got, reference(name)), bound(name)
    return {k: e[k] / (b[k] / M) for k in e}


# --------------------------------------------------------------------------------------------------- the device checks
# one body for the emulator (tests/test_init_sfm_simt.py) and the MI355X (tests/test_init_sfm_gpu.py); h: a ba.Handle
OUT_KEYS = ('q', 'T', 'state', 'position', 'R_all', 'T_all', 'is_key', 'q0', 'T0', 'position0', 'pnp_iters', 'pnp_up', 'it_cost', 'it_cost_cand',
            'it_model', 'it_radius', 'it_flags')


def same_output(a, b):
    """two results of Handle.init_sfm, bit for bit"""
    return (a['status'] == b['status'] and a['ba_iters'] == b['ba_iters'] and a['ba_termination'] == b['ba_termination'] and
            np.array_equal(a['final_cost'], b['final_cost']) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in OUT_KEYS))


def check_cases(h, tag, names=None):
    """the cases in ONE call: the 80-bit route's decisions, every value group within M x E64, the rest zero"""
    names = list(names or CASE_ARGS)
    got = dict(zip(names, h.init_sfm([case(n) for n in names])))
    worst = (0.0, None)
    for n in names:
        ref, g = reference(n), view(got[n])
        assert g['dec'] == ref['dec'], (n, g['dec'], ref['dec'])
        r = ratios(g, n)
        print(f"init_sfm {tag} {n}: status {g['dec']['status']}  " + "  ".join(f"{k} {v:.2f}" for k, v in r.items()))
        for k, v in r.items():
            assert v <= M, f"{n} {k}: {v:.3f} x E64 > {M}"
            worst = max(worst, (v, f"{k} of {n}"))
        for k in VALUE_KEYS:
            if k not in ref['val'] and k != 'ba_cost':
                assert not np.asarray(got[n][k]).any(), (n, k)
    print(f"init_sfm {tag}: worst ratio {worst[0]:.3f} ({worst[1]}; bound {M})")
    return got


def batch(n, seed=77):
    """n small windows of mixed F, l and statuses for the batch-equals-single checks"""
    rng = np.random.default_rng(seed)
    fixed = [case('F3_9'), case('F5_nan'), case('F5_nk5'), case('F3_10'), case('F5_12')]
    out = []
    for i in range(n):
        if i == 0:                                          # n_all = 0: construct only, no all_* table at all
            out.append(dict(scene(2999, F=5, l=2, n_feat=30), all_key=[], all_guess=[], all_pts=[]))
            continue
        if i % 4 == 1:
            out.append(fixed[(i // 4) % len(fixed)])
            continue
        F = int(rng.choice([3, 4, 5, 7, 16 if i == 2 else 6]))
        out.append(scene(3000 + i, F=F, l=int(rng.integers(0, F - 1)), n_feat=int(rng.integers(24, 48)), nonkey=bool(i % 2)))
    return out


def check_batch_equals_single(h, sizes=(1, 3, 33)):
    wins = batch(max(sizes))
    single = [h.init_sfm([w])[0] for w in wins]
    assert len({s['status'] for s in single}) >= 4, "the batch mixes statuses"
    assert len({w['n_frames'] for w in wins}) >= 4, "the batch mixes F"
    assert len(wins[0]['all_key']) == 0 and single[0]['status'] == OK and single[0]['q'].any() and single[0]['R_all'].size == 0, "construct only"
    for n in sizes:
        for k, g in enumerate(h.init_sfm(wins[:n])):
            assert same_output(g, single[k]), (n, k)
    return single


def check_numeric_neighbours(h):
    """a window that ends with VG_SFM_NUMERIC (a NaN-producing triangulation) between two good ones: they are what they are alone"""
    wins = [case('F5_12'), case('F5_nan'), case('F11_l0')]
    alone = [h.init_sfm([w])[0] for w in wins]
    together = h.init_sfm(wins)
    assert [a['status'] for a in alone] == [OK, NUMERIC, OK]
    for a, b in zip(alone, together):
        assert same_output(a, b)
    for k in OUT_KEYS:
        assert not np.asarray(together[1][k]).any(), k


def _refusals():
    """name -> a function that spoils window 1 of the packed call (ins, outs, keep) and returns the n_windows to pass"""
    import ctypes as C
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

    def vec(name, idx, val):
        return setter(lambda ins, outs, keep: getattr(ins[1], name).__setitem__(idx, val))

    r = {'n_windows_0': setter(lambda *a: None, 0), 'in_struct_size': field('in', 'struct_size', 8), 'out_struct_size': field('out', 'struct_size', 0),
         'F_2': field('in', 'n_frames', 2), 'F_17': field('in', 'n_frames', 17), 'l_negative': field('in', 'l', -1), 'l_is_F_minus_1': field('in', 'l', 4),
         'n_feat_0': field('in', 'n_feat', 0), 'n_feat_above': field('in', 'n_feat', 1025), 'span_leaves_F': arr('start', 0, 4), 'nobs_0': arr('nobs', 3, 0),
         'obs_off_descends': arr('off', 5, 2), 'id_repeats': setter(lambda ins, outs, keep: keep[1]['fid'].__setitem__(7, keep[1]['fid'][2])),
         'all_key_descends': arr('all_key', 2, 0), 'all_key_skips': arr('all_key', 8, -1), 'all_guess_is_F': arr('all_guess', 1, 5),
         'all_guess_negative': arr('all_guess', 3, -1), 'all_off_descends': arr('all_off', 1, 100), 'relative_R_nan': vec('relative_R', 4, nan),
         'relative_T_inf': vec('relative_T', 0, float('inf')), 'ric_nan': vec('ric', 8, nan), 'point_nan': arr('points', 3 * 11 + 1, nan),
         'all_xy_inf': arr('xy', 5, float('-inf'))}
    for t in ('feature_id', 'start', 'nobs', 'obs_off', 'points', 'all_key', 'all_guess', 'all_off', 'all_id', 'all_xy'):
        r['null_' + t] = null(t)
    return r


REFUSALS = tuple(_refusals())


def check_refusal(h, name):
    """the spoiled call returns VG_ERR_BAD_ARG with a message, writes nothing, and the handle goes on working"""
    wins = [case('F5_12'), case('F5_nk6')]
    good = h.init_sfm(wins)
    ins, outs, keep = h.init_sfm_pack(wins)
    marked = ('q', 'T', 'position', 'R_all', 'T_all', 'q0', 'T0', 'position0')
    for o, b in zip(outs, keep):
        o.status, o.final_cost = 77, -5.0
        o.it_cost[0] = -1.0
        for k in marked:
            b[k][...] = 3.25
        b['state'][...] = 9
    n = _refusals()[name](ins, outs, keep)
    rc = h.lib.vg_init_sfm(h.h, n, ins, outs)
    assert rc == -1, (name, rc)                              # VG_ERR_BAD_ARG
    assert b"vg_init_sfm" in h.lib.vg_last_error(h.h), name
    for o, b in zip(outs, keep):
        assert o.status == 77 and o.final_cost == -5.0 and o.it_cost[0] == -1.0
        assert all(np.all(b[k] == 3.25) for k in marked) and np.all(b['state'] == 9), name
    for a, b in zip(good, h.init_sfm(wins)):
        assert same_output(a, b), name


@functools.lru_cache(maxsize=None)
def capacity_scene():
    """F = 16 with VG_SFM_MAX_FEATURES features: the whole LDS of a CU, one feature staged at a time"""
    return scene(8, F=16, l=7, n_feat=1024)


def check_capacity(h, tag):
    """the capacity window against the float64 route 'ldlt' (the 80-bit route takes a minute at this size): equal decisions, and every
    group within M x the table's E64 floor, which is what two float64 evaluations may differ by"""
    ref = view(sfm(capacity_scene(), np.float64, 'ldlt'))
    assert ref['pnp_margin'] >= PNP_MARGIN and ref['dec']['status'] == OK
    g = view(h.init_sfm([capacity_scene()])[0])
    assert g['dec'] == ref['dec']
    e, fl = errors(g, ref), e64_floor()
    print(f"init_sfm {tag} capacity: " + "  ".join(f"{k} {e[k] / fl[k]:.2f}" for k in e))
    for k in e:
        assert e[k] <= M * fl[k], (k, e[k], fl[k])


def chain_scene(name='F11'):
    """(the window of vg_init_sfm, the window of vg_init_align it feeds, the scale the alignment must find): the IMU scene of
    tests/init_align_ref.py, its cameras looking at landmarks, noise-free"""
    al = A.case(name)
    F = len(al['R'])
    ric = A._small_rotation(np.array([0.1, -0.2, 0.15]))
    win = scene(21, F=F, l=F // 2, n_feat=120, noise=0.0, poses=([R @ ric for R in al['R']], list(al['T']), None))
    win['ric'] = ric
    return win, al, al['truth']['s'] * win['truth']['base']


# The scale bound of the alignment's own tests: tests/test_init_align_def.py holds the 80-bit alignment's `s` to the scene's scale within
# this figure on noise-free scenes (its kappa 2^-53 bound measures `s` against the 80-bit alignment of the SAME R / T; here R / T come
# out of another stage, the SfM's BA with its 1e-6 function tolerance, so only the bound against the scene's truth carries over).
SCALE_BOUND = 1e-3


def check_chain(h):
    """R_all / T_all handed to vg_init_align with the scene's IMU rows: VG_ALIGN_OK and the scene's scale within SCALE_BOUND"""
    win, al, s_true = chain_scene()
    g = h.init_sfm([win])[0]
    assert g['status'] == OK
    res = h.init_align([dict(al, R=g['R_all'], T=g['T_all'])])[0]
    err = abs(res['s'] - s_true) / s_true
    print(f"init_sfm chain: align status {res['status']}  scale {res['s']:.9g} (scene {s_true:.9g}, relative error {err:.1e})")
    assert res['status'] == A.OK and err < SCALE_BOUND


def write_file(path, win):
    """a window as a VSF1 file (tests/init_sfm_san_main.cpp reads it)"""
    import struct
    from vins_mono_amd import ba
    _, _, keep = ba.Handle.init_sfm_pack([win])
    b = keep[0]
    na, npt = len(b['all_key']), int(b['all_off'][-1]) if len(b['all_key']) else 0
    with open(path, 'wb') as f:
        f.write(struct.pack('<7i', 0x31465356, int(win['n_frames']), int(win['l']), len(b['start']), len(b['points']), na, npt))
        d = lambda a: f.write(np.ascontiguousarray(a, '<f8').tobytes())
        i = lambda a: f.write(np.ascontiguousarray(a, '<i4').tobytes())
        d(win['relative_R']); d(win['relative_T']); d(win['ric'])
        i(b['fid']); i(b['start']); i(b['nobs']); i(b['off']); d(b['points'])
        i(b['all_key']); i(b['all_guess']); i(b['all_off'] if na else [0]); i(b['ids'][:npt]); d(b['xy'][:npt])


# --------------------------------------------------------------------------------------------------- the stand-alone class
REPLAY_CASES = ('ok', 'failed_pnp')         # initialStructure goes through to visualInitialAlign / construct fails in the chain
INIT_DEPTH = 5.0


@functools.lru_cache(maxsize=None)
def replay_scene(name):
    """(the window of vg_init_sfm, the IMU window of tests/init_align_ref.py it belongs to): 11 entries of all_image_frame, the even ones
    the 6 window frames, the odd ones non-key frames between them; 'failed_pnp' has too few features for the chain"""
    al = A.scene(31, 11, 20, key=[0, 2, 4, 6, 8, 10])
    ric = A._small_rotation(np.array([0.1, -0.2, 0.15]))
    cam = [(R @ ric, T) for R, T in zip(al['R'], al['T'])]
    poses = ([cam[k][0] for k in al['key']], [cam[k][1] for k in al['key']], [cam[k] for k in range(1, 11, 2)])
    win = scene(22, F=6, l=3, n_feat=80 if name == 'ok' else 8, noise=0.0, nonkey=True, poses=poses)
    win['ric'] = ric
    return win, al


def write_replay(path, win, al):
    """the VSR1 file `vins_replay sfm` reads (host/replay_main.cpp: replay_sfm)"""
    import struct
    na, key = len(win['all_key']), [a for a, k in enumerate(win['all_key']) if k >= 0]
    with open(path, 'wb') as f:
        f.write(struct.pack('<5i', 0x31525356, na, len(key), len(win['start']), int(win['l'])))
        d = lambda a: f.write(np.ascontiguousarray(a, '<f8').tobytes())
        d(al['ba0']); d(al['bg0']); d(al['noise']); d(al['tic']); d(win['ric']); d([al['g_norm'], INIT_DEPTH]); d(win['relative_R']); d(win['relative_T'])
        for a in range(na):
            pts = win['all_pts'][a]
            d([0.05 * a + 100.0])
            f.write(struct.pack('<i', 0 if pts is None else len(pts[0])))
            if pts is not None:
                for fid, xy in zip(*pts):
                    f.write(struct.pack('<i', int(fid)))
                    d(xy)
        for iv in al['intervals']:
            f.write(struct.pack('<i', len(iv) - 1))
            d(np.concatenate([iv[0][1], iv[0][2]]))
            d([[dt, *a, *g] for dt, a, g in iv[1:]])
        f.write(np.asarray(key, '<i4').tobytes())
        o = 0
        for fid, s0, n in zip(win['feature_id'], win['start'], win['nobs']):
            f.write(struct.pack('<3i', int(fid), int(s0), int(n)))
            d(win['points'][o:o + n])
            o += n


def check_replay(h, exe, tmp_dir, name):
    """`vins_replay sfm` (Estimator::initialStructure of host/estimator.cpp with vg_pack_sfm's walk over all_image_frame) against the
    binding fed the hand-built all_key / all_guess, number for number"""
    import os
    import subprocess
    win, al = replay_scene(name)
    src, dst = os.path.join(str(tmp_dir), name + '.bin'), os.path.join(str(tmp_dir), name + '.txt')
    write_replay(src, win, al)
    r = subprocess.run([exe, 'sfm', src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in open(dst)]
    num = lambda row: np.array([float(x) for x in row[1:]])
    g = h.init_sfm([win])[0]
    entries = [num(r_) for r_ in rows if r_[0] == 'entry']
    frames = [num(r_) for r_ in rows if r_[0] == 'frame']
    depth = np.array([float(r_[1]) for r_ in rows if r_[0] == 'depth'])
    if name == 'failed_pnp':
        assert g['status'] == FAILED_PNP
        assert rows[0] == ['result', '0', str(FAILED_PNP), '0', '0']         # MARGIN_OLD = 0 (the harness starts from MARGIN_SECOND_NEW)
        assert not frames and np.all(depth == -1.0) and all(e[0] == 0 for e in entries)
        return
    assert g['status'] == OK
    key = [a for a, k in enumerate(win['all_key']) if k >= 0]
    res = h.init_align([dict(al, R=g['R_all'], T=g['T_all'], key=key)])[0]
    assert res['status'] == A.OK
    assert rows[0] == ['result', '1', str(OK), str(A.OK), '1']                # (marginalization_flag untouched)
    assert len(entries) == len(win['all_key'])
    for a, e in enumerate(entries):
        assert e[0] == g['is_key'][a] and np.array_equal(e[1:10], g['R_all'][a].ravel()) and np.array_equal(e[10:], g['T_all'][a]), a
    assert np.array_equal(num(rows[1 + len(entries)]), res['bg']) and np.array_equal(num(rows[2 + len(entries)]), res['g_w'])
    assert len(frames) == len(key)
    for k, fr in enumerate(frames):
        assert np.array_equal(fr[:3], res['Ps'][k]) and np.array_equal(fr[3:12], res['Rs'][k].ravel()) and np.array_equal(fr[12:], res['Vs'][k]), k
    two = np.asarray(win['nobs']) >= 2
    off = np.concatenate([[0], np.cumsum(win['nobs'])[:-1]])
    want = h.triangulate(g['T_all'][key], g['R_all'][key], np.zeros(3), win['ric'], np.asarray(win['start'])[two], np.asarray(win['nobs'])[two], off[two],
                         win['points'], INIT_DEPTH) * res['s']
    assert np.array_equal(depth[two], want) and np.all(depth[~two] == -1.0)
    s_true = al['truth']['s'] * win['truth']['base']
    assert abs(res['s'] - s_true) / s_true < SCALE_BOUND
