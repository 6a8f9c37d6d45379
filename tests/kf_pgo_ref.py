"""vg_pg_optimize (include/vinsgpu.h, the "4-DoF pose-graph optimisation" block): the float64 / long-double restatement, the cases, the
metric and the check bodies shared by tests/test_kf_pgo_simt.py (emulated kernels) and tests/test_kf_pgo_gpu.py (the MI355X).

Three routes through the same definition:
  ld       numpy.longdouble, the LM system assembled dense and solved by a dense Cholesky
  dense64  float64, numpy.linalg.solve on the dense system
  pcg64    float64, the header's banded Cholesky inside conjugate gradients, with its summation orders
The bound is the project's standing one: a device value may differ from `ld` by at most M = 4 times E64, the larger disagreement of the
two float64 routes with `ld`, per quantity in its own scale (KINDS: positions by the graph's extent, angles in degrees, costs by the
initial cost; rotation entries and the radius are quantities of their own), floored at 2^-52 of the scale.  A quantity's E64 runs over all
outputs of that quantity: the two float64 routes share everything but the solver, so on a single trace row their distance from `ld` is at
times a fraction of the rounding noise that row carries (the model change of in_band_loop's first row: 3e-18 for both, 6e-17 for the same
row of `wrap`).  Decisions (status, termination, iterations, the flags of every trace row) must be EQUAL: a case
qualifies only when the three routes agree on them and every accept and tolerance test of the `ld` route has a relative margin of 1e-6."""
import functools
import math

import numpy as np

LD = np.longdouble
M = 4.0
E64_FLOOR = 2.0 ** -52
OK, NO_EDGES, NUMERIC = 0, 1, 2
NO_CONVERGENCE, CONVERGENCE, FAILURE = 0, 1, 2
MAX_KEYFRAMES, MAX_ITERS, MAX_CG, NT, KD = 2048, 8, 128, 256, 19
ROUTES = {'ld': LD, 'dense64': np.float64, 'pcg64': np.float64}
ALL_ROUTES = dict(ROUTES, sparse64=np.float64)     # the capacity pair's second float64 route: scipy's sparse LU on the same system
MARGIN = 1e-6
# what a mutated restatement gets wrong (check_mutations: the case table must tell each from the definition, but for the one that is equivalent)
EDITS = ('no_huber', 'no_yaw_weight', 'chain_yaw_normalised', 'no_pi_180', 'rescale_every_iteration', 'cg_1e-3', 'no_tail_drift', 'seq0_free',
         'candidate_residuals_kept')
EQUIVALENT_EDITS = ('chain_yaw_normalised',)     # NormalizeAngle's one wrap takes the 360 degrees back: the same residual to rounding


# --------------------------------------------------------------------------------------------------- small pieces
def tree_sum(v):
    """the header's SUM OVER A LIST"""
    p = np.zeros(NT, v.dtype)
    for s in range(0, len(v), NT):
        c = v[s:s + NT]
        p[:len(c)] += c
    h = NT // 2
    while h:
        p[:h] += p[h:2 * h]
        h //= 2
    return p[0]


def normalize(a):
    return np.where(a > 180, a - 360, np.where(a < -180, a + 360, a))


def R2ypr(R, dt):
    """Utility::R2ypr over [n, 3, 3], degrees"""
    pi = dt(np.pi)
    y = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    p = np.arctan2(-R[:, 2, 0], R[:, 0, 0] * np.cos(y) + R[:, 1, 0] * np.sin(y))
    r = np.arctan2(R[:, 0, 2] * np.sin(y) - R[:, 1, 2] * np.cos(y), -R[:, 0, 1] * np.sin(y) + R[:, 1, 1] * np.cos(y))
    return np.stack([y / pi * 180, p / pi * 180, r / pi * 180], 1)


def _mm(A, B):
    """[n, 3, 3] products, the inner index ascending from the first term"""
    t = A[:, :, 0, None] * B[:, None, 0, :]
    for k in (1, 2):
        t = t + A[:, :, k, None] * B[:, None, k, :]
    return t


def ypr2R(yaw, pitch, roll, dt):
    """Utility::ypr2R over [n]: (Rz Ry) Rx"""
    pi = dt(np.pi)
    y, p, r = yaw / 180 * pi, pitch / 180 * pi, roll / 180 * pi
    z, o = np.zeros_like(y), np.ones_like(y)
    Rz = np.stack([np.cos(y), -np.sin(y), z, np.sin(y), np.cos(y), z, z, z, o], 1).reshape(-1, 3, 3)
    Ry = np.stack([np.cos(p), z, np.sin(p), z, o, z, -np.sin(p), z, np.cos(p)], 1).reshape(-1, 3, 3)
    Rx = np.stack([o, z, z, z, np.cos(r), -np.sin(r), z, np.sin(r), np.cos(r)], 1).reshape(-1, 3, 3)
    return _mm(_mm(Rz, Ry), Rx)


def _mv3(R, v):
    t = R[..., 0] * v[..., None, 0]
    for k in (1, 2):
        t = t + R[..., k] * v[..., None, k]
    return t


def _AtB(A, B):
    """[e, 4, 4]: A^T B over the residual index, ascending from the first term"""
    t = A[:, 0, :, None] * B[:, 0, None, :]
    for r in (1, 2, 3):
        t = t + A[:, r, :, None] * B[:, r, None, :]
    return t


def _Atr(A, r):
    t = A[:, 0, :] * r[:, 0, None]
    for k in (1, 2, 3):
        t = t + A[:, k, :] * r[:, k, None]
    return t


def _Jv(J, v):
    t = J[:, :, 0] * v[:, None, 0]
    for k in (1, 2, 3):
        t = t + J[:, :, k] * v[:, None, k]
    return t


# --------------------------------------------------------------------------------------------------- the graph
class Graph:
    """the topology the host builds (fidx, nof, ea, the arriving loops) and the inputs in the route's number format"""

    def __init__(self, g, dt, edit=None):
        self.dt, self.edit = dt, edit
        self.index = np.asarray(g['index'], np.int64)
        self.NKF = len(self.index)
        self.N = N = int(g.get('n_opt', self.NKF))
        seq, first = np.asarray(g['sequence'], np.int64), int(g['first_looped_index'])
        self.vT = np.asarray(g['vio_T'], np.float64).astype(dt).reshape(-1, 3)
        self.vR = np.asarray(g['vio_R'], np.float64).astype(dt).reshape(-1, 3, 3)
        self.delta = dt(g.get('huber_delta', 0.1))
        self.max_iters = int(g.get('max_iters', 5))
        const = (self.index[:N] == first) | ((seq[:N] == 0) if edit != 'seq0_free' else False)
        self.fidx = np.where(const, -1, np.cumsum(~const) - 1)
        self.nof = np.nonzero(~const)[0]
        self.NF = len(self.nof)
        self.ea = np.full(5 * N, -1, np.int64)
        self.meas_loop = np.zeros((N, 4), dt)
        arriving = [[] for _ in range(N)]
        info = np.asarray(g['loop_info'], np.float64).reshape(-1, 8)
        for i in range(N):
            for j in range(1, 5):
                if i - j >= 0 and seq[i] == seq[i - j]:
                    self.ea[5 * i + j - 1] = i - j
            if g['has_loop'][i]:
                la = int(np.searchsorted(self.index, g['loop_index'][i]))
                assert self.index[la] == g['loop_index'][i] and la < i
                self.ea[5 * i + 4] = la
                arriving[la].append(i)
                self.meas_loop[i] = info[i, [0, 1, 2, 7]].astype(dt)
        self.arriving = arriving
        self.valid = self.ea >= 0
        self.a = np.where(self.valid, self.ea, 0)
        self.b = np.arange(5 * N) // 5
        self.loop = (np.arange(5 * N) % 5 == 4)
        self.n_edges, self.n_loop_edges = int(self.valid.sum()), int((self.valid & self.loop).sum())
        ypr = R2ypr(self.vR[:N], dt)
        self.yaw0, self.pitch, self.roll, self.t0 = ypr[:, 0].copy(), ypr[:, 1], ypr[:, 2], self.vT[:N].copy()
        # the measurements: chain edges from the VIO poses (the matrix used directly), loop edges from loop_info
        d = self.t0[self.b] - self.t0[self.a]
        Ra = self.vR[self.a]
        mt = _mv3(np.swapaxes(Ra, 1, 2), d)
        dy = self.yaw0[self.b] - self.yaw0[self.a]
        if edit == 'chain_yaw_normalised':
            dy = normalize(dy)
        self.meas = np.concatenate([mt, dy[:, None]], 1)
        self.meas[self.loop] = self.meas_loop
        self.meas[~self.valid] = 0

    def gather(self, Pb, Pa):
        """per node: its own slots 0 .. 4 (as b), the chain edges leaving it to i+1 .. i+4 (as a), the arriving loops in ascending source"""
        N = self.N
        acc = np.zeros((N,) + Pb.shape[1:], self.dt)
        n = np.arange(N)
        for k in range(5):
            acc = acc + Pb[5 * n + k]
        for j in range(1, 5):
            e = np.minimum(5 * (n + j) + j - 1, 5 * N - 1)
            ok = (n + j < N)
            ok = ok & self.valid[e]
            acc = acc + np.where(ok.reshape((-1,) + (1,) * (Pb.ndim - 1)), Pa[e], 0)
        for i in range(N):
            for s in self.arriving[i]:
                acc[i] = acc[i] + Pa[5 * s + 4]
        return acc

    def evaluate(self, yaw, t, jac, marg=None):
        """rho per slot, the corrected residuals and (jac) Jacobians; the cost"""
        dt, edit = self.dt, self.edit
        pi = dt(np.pi)
        a, b = self.a, self.b
        y, p, r = yaw[a] / 180 * pi, self.pitch[a] / 180 * pi, self.roll[a] / 180 * pi
        cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
        R = np.stack([cy * cp, -sy * cr + cy * sp * sr, sy * sr + cy * sp * cr, sy * cp, cy * cr + sy * sp * sr, -cy * sr + sy * sp * cr, -sp,
                      cp * sr, cp * cr], 1)
        d = t[b] - t[a]
        e = np.zeros((len(a), 4), dt)
        for c in range(3):
            e[:, c] = (R[:, c] * d[:, 0] + R[:, 3 + c] * d[:, 1] + R[:, 6 + c] * d[:, 2]) - self.meas[:, c]
        ang = normalize(yaw[b] - yaw[a] - self.meas[:, 3])
        wdiv = edit != 'no_yaw_weight'
        e[:, 3] = np.where(self.loop & wdiv, ang / 10, ang)
        s = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2] + e[:, 3] * e[:, 3]
        d2 = self.delta * self.delta
        hub = self.loop & self.valid & (s > d2) & (edit != 'no_huber')
        if marg is not None:
            lv = self.loop & self.valid
            if lv.any():
                marg.append(float(np.abs(s[lv] - d2).min() / d2))
        with np.errstate(all='ignore'):
            rt = np.sqrt(np.where(hub, s, 1))
            rho = np.where(hub, 2 * self.delta * rt - d2, s)
            sc = np.where(hub, np.sqrt(np.maximum(dt(np.finfo(np.float64).tiny), self.delta / rt)), dt(1))
        rho = np.where(self.valid, rho, 0)
        res = np.where(self.valid[:, None], sc[:, None] * e, 0)
        cost = tree_sum(rho) / 2
        if not jac:
            return cost, res, None, None, hub
        w = np.where(self.loop & wdiv, dt(1) / 10, dt(1))
        k180 = pi / 180 if edit != 'no_pi_180' else dt(1)
        Ja, Jb = np.zeros((len(a), 4, 4), dt), np.zeros((len(a), 4, 4), dt)
        for c in range(3):
            dy = (R[:, c] * d[:, 1] - R[:, 3 + c] * d[:, 0]) * k180
            Ja[:, c, 0] = sc * dy
            for k in range(3):
                Ja[:, c, 1 + k] = sc * -R[:, 3 * k + c]
                Jb[:, c, 1 + k] = sc * R[:, 3 * k + c]
        Ja[:, 3, 0], Jb[:, 3, 0] = sc * -w, sc * w
        Ja[~self.valid], Jb[~self.valid] = 0, 0
        return cost, res, Ja, Jb, hub


class System:
    """the blocks of JtJ over the free nodes (unscaled, then scaled in place), the gradient"""

    def __init__(self, G, res, Ja, Jb):
        self.G = G
        NF, nof, fidx, ea, dt = G.NF, G.nof, G.fidx, G.ea, G.dt
        D = G.gather(_AtB(Jb, Jb), _AtB(Ja, Ja))[nof]
        self.g = G.gather(_Atr(Jb, res), _Atr(Ja, res))[nof].reshape(-1)
        BA = _AtB(Jb, Ja)
        self.Ab = np.zeros((NF, 5, 4, 4), dt)
        self.Ab[:, 0] = D
        for d in range(1, 5):
            f = np.arange(d, NF)
            nd, q = nof[f], nof[f - d]
            dist = nd - q
            e = 5 * nd + np.clip(dist - 1, 0, 3)
            chain = (dist <= 4) & (ea[e] >= 0)
            blk = np.where(chain[:, None, None], BA[e], 0)
            blk = blk + np.where((ea[5 * nd + 4] == q)[:, None, None], BA[5 * nd + 4], 0)
            self.Ab[d:, d] = blk
        la = ea[5 * nof + 4]
        fa = np.where(la >= 0, fidx[np.maximum(la, 0)], -1)
        self.oob = (la >= 0) & (fa >= 0) & (np.arange(NF) - fa > 4)        # per free node: its own loop edge lies outside the band
        self.fa = fa
        self.LB = np.where(self.oob[:, None, None], BA[5 * nof + 4], 0)

    def scale(self, s):
        s = s.reshape(-1, 4)
        NF = len(s)
        D = self.Ab[:, 0]
        low = s[:, :, None] * (D * s[:, None, :])
        tri = np.tril(np.ones((4, 4), bool))
        self.Ab[:, 0] = np.where(tri, low, np.swapaxes(low, 1, 2))
        for d in range(1, 5):
            self.Ab[d:, d] = s[d:, :, None] * (self.Ab[d:, d] * s[:NF - d, None, :])
        f = np.nonzero(self.oob)[0]
        self.LB[f] = s[f][:, :, None] * (self.LB[f] * s[self.fa[f]][:, None, :])
        self.gs = self.g * s.reshape(-1)

    def dense(self, dd):
        NF = len(self.Ab)
        A = np.zeros((4 * NF, 4 * NF), self.G.dt)
        for f in range(NF):
            A[4 * f:4 * f + 4, 4 * f:4 * f + 4] = self.Ab[f, 0]
            for d in range(1, 5):
                if f - d >= 0:
                    A[4 * f:4 * f + 4, 4 * (f - d):4 * (f - d) + 4] = self.Ab[f, d]
                    A[4 * (f - d):4 * (f - d) + 4, 4 * f:4 * f + 4] = self.Ab[f, d].T
            if self.oob[f]:
                a = self.fa[f]
                A[4 * f:4 * f + 4, 4 * a:4 * a + 4] = self.LB[f]
                A[4 * a:4 * a + 4, 4 * f:4 * f + 4] = self.LB[f].T
        A[np.diag_indices(4 * NF)] += dd
        return A

    def sparse_solve(self, dd, b):
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        NF = len(self.Ab)
        rows, cols, vals = [], [], []
        pq = np.arange(16)

        def put(fr, fc, B):
            rows.append((4 * fr[:, None] + pq // 4).reshape(-1)); cols.append((4 * fc[:, None] + pq % 4).reshape(-1)); vals.append(B.reshape(-1))
        f = np.arange(NF)
        put(f, f, self.Ab[:, 0])
        for d in range(1, 5):
            put(f[d:], f[d:] - d, self.Ab[d:, d])
            put(f[d:] - d, f[d:], np.swapaxes(self.Ab[d:, d], 1, 2))
        o = np.nonzero(self.oob)[0]
        put(o, self.fa[o], self.LB[o])
        put(self.fa[o], o, np.swapaxes(self.LB[o], 1, 2))
        A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(4 * NF, 4 * NF)) + sp.diags(dd)
        return spl.spsolve(A.tocsc(), b)

    def matvec(self, p, dd):
        """q = A p by rows in the header's order"""
        NF = len(self.Ab)
        P = p.reshape(NF, 4)
        acc = np.zeros((NF, 4), p.dtype)

        def bv(B, v, tr):
            t = (B[:, 0, :] if tr else B[:, :, 0]) * v[:, None, 0]
            for k in (1, 2, 3):
                t = t + (B[:, k, :] if tr else B[:, :, k]) * v[:, None, k]
            return t
        for d in (4, 3, 2, 1):
            if NF > d:
                acc[d:] = acc[d:] + bv(self.Ab[d:, d], P[:NF - d], False)
        acc = acc + bv(self.Ab[:, 0], P, False)
        for d in (1, 2, 3, 4):
            if NF > d:
                acc[:NF - d] = acc[:NF - d] + bv(self.Ab[d:, d], P[d:], True)
        f = np.nonzero(self.oob)[0]
        acc[f] = acc[f] + bv(self.LB[f], P[self.fa[f]], False)
        for ff in f:                                            # (ascending source: the free index ascends with the node)
            a = self.fa[ff]
            acc[a] = acc[a] + bv(self.LB[ff:ff + 1], P[ff:ff + 1], True)[0]
        return acc.reshape(-1) + dd * p


_TRI = np.tril_indices(KD)


def band_cholesky(S, dd):
    """the header's scalar band Cholesky of M -> (Lcol [n, 20]: [j, l] = L(j + l, j), l >= 1; Lrow [n, 20]: [i, o] = L(i, i - o); Linv) or None"""
    NF = len(S.Ab)
    n = 4 * NF
    B = np.zeros((n + KD + 1, KD + 1), np.float64)
    for f in range(NF):
        for pp in range(4):
            i = 4 * f + pp
            for d in range(0, 5):
                if f - d < 0:
                    continue
                for qq in range(4):
                    o = i - (4 * (f - d) + qq)
                    if 0 <= o <= KD:
                        B[i, o] = S.Ab[f, d, pp, qq]
    B[np.arange(n), 0] += dd
    Linv = np.zeros(n)
    ls = np.arange(1, KD + 1)
    li, lk = _TRI[0] + 1, _TRI[1] + 1
    for j in range(n):
        piv = B[j, 0]
        if not (piv > 0 and np.isfinite(piv)):
            return None
        inv = 1.0 / np.sqrt(piv)
        Linv[j] = inv
        col = B[j + ls, ls] * inv
        B[j + ls, ls] = col
        B[j + li, li - lk] -= col[li - 1] * col[lk - 1]
    Lrow = B[:n]
    Lcol = np.zeros((n, KD + 1))
    for l in range(1, KD + 1):
        Lcol[:n - l, l] = Lrow[l:, l]
    return Lcol, Lrow, Linv


def band_solve(F, rhs):
    Lcol, Lrow, Linv = F
    n = len(rhs)
    acc = np.concatenate([rhs, np.zeros(KD)])
    z = np.zeros(n)
    for j in range(n):
        zj = acc[j] * Linv[j]
        z[j] = zj
        acc[j + 1:j + 1 + KD] -= Lcol[j, 1:] * zj
    acc = np.concatenate([np.zeros(KD), z])
    y = np.zeros(n)
    for j in range(n - 1, -1, -1):
        yj = acc[j + KD] * Linv[j]
        y[j] = yj
        acc[j:j + KD] -= Lrow[j, KD:0:-1] * yj
    return y


def pcg(S, dd, b, tol2=1e-24):
    """the header's preconditioned conjugate gradients -> (y or None, iterations)"""
    F = band_cholesky(S, dd)
    if F is None:
        return None, 0
    x, r = np.zeros_like(b), b.copy()
    z = band_solve(F, r)
    p = z.copy()
    rz = tree_sum(r * z)
    rz0 = rz
    if not (rz0 > 0 and np.isfinite(rz0)):
        return None, 0
    for k in range(1, MAX_CG + 1):
        q = S.matvec(p, dd)
        pq = tree_sum(p * q)
        if not (pq > 0 and np.isfinite(pq)):
            return None, k
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = band_solve(F, r)
        rzn = tree_sum(r * z)
        if not np.isfinite(rzn):
            return None, k
        if rzn <= tol2 * rz0:
            return x, k
        p = z + (rzn / rz) * p
        rz = rzn
    return None, MAX_CG


def _dense_cholesky_solve(A, b):
    L = A.copy()
    n = len(b)
    for j in range(n):
        d = L[j, j]
        if not (d > 0 and np.isfinite(np.float64(d))):
            return None
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] /= L[j, j]
        c = L[j + 1:, j]
        nz = np.nonzero(c)[0]                                   # (the factor of a banded system plus a few loops: mostly zeros)
        if len(nz):
            L[np.ix_(j + 1 + nz, j + 1 + nz)] -= np.outer(c[nz], c[nz])
    y = b.copy()
    for j in range(n):
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


# --------------------------------------------------------------------------------------------------- the call for one graph
def solve(g, route='ld', edit=None, steps=None):
    """the header's definition; the dict fe.pg_optimize returns, plus 'margin' (the smallest relative margin of a decision), 'huber'
    (loop edges with s > delta^2 at the first point), 'wrapped' (Plus wrapped an angle) and, with `steps` a list, the (A, b, y) of every row"""
    dt = ALL_ROUTES[route]
    G = Graph(g, dt, edit)
    N, NF, nof = G.N, G.NF, G.nof
    yaw, t = G.yaw0.copy(), G.t0.copy()
    marg, wrapped = [], False
    trace = []
    with np.errstate(all='ignore'):
        cost, res, Ja, Jb, hub = G.evaluate(yaw, t, True, marg)
    out = dict(n_edges=G.n_edges, n_loop_edges=G.n_loop_edges, n_free=NF, initial_cost=cost, huber=int(hub.sum()))
    term, it = NO_CONVERGENCE, 0
    finite0 = bool(np.isfinite(np.float64(cost)))
    if NF == 0 and finite0:
        term = CONVERGENCE
    if NF > 0 and finite0:
        one = dt(1)
        radius, dec, invalid = dt(1e4), dt(2), 0
        relin, first, scale = True, True, None

        def ambient(yaw, t):
            return np.concatenate([yaw[nof, None], t[nof]], 1).reshape(-1)
        while True:
            if relin:
                S = System(G, res, Ja, Jb)
                if first or edit == 'rescale_every_iteration':
                    scale = one / (one + np.sqrt(S.Ab[:, 0][:, [0, 1, 2, 3], [0, 1, 2, 3]].reshape(-1)))
                x_norm = np.sqrt(tree_sum(ambient(yaw, t) ** 2))
                gmax = np.abs(S.g).max()
                marg.append(abs(float(gmax) - 1e-10) / 1e-10)
                if gmax <= 1e-10:
                    term = CONVERGENCE
                    break
                S.scale(scale)
                dcl = np.clip(S.Ab[:, 0][:, [0, 1, 2, 3], [0, 1, 2, 3]].reshape(-1), dt(1e-6), dt(1e32))
                relin, first = False, False
            if it >= G.max_iters:
                break
            it += 1
            D = np.sqrt(dcl / radius)
            dd = D * D
            rec = dict(cost=cost, radius=radius, cand=dt(0), model=dt(0), flags=0, cg=0)
            trace.append(rec)
            b = -S.gs
            if route == 'pcg64':
                y, rec['cg'] = pcg(S, dd, b, 1e-6 if edit == 'cg_1e-3' else 1e-24)
            elif route == 'sparse64':
                y = S.sparse_solve(dd, b)
            elif route == 'dense64':
                try:
                    y = np.linalg.solve(S.dense(dd), b)
                except np.linalg.LinAlgError:
                    y = None
            else:
                y = _dense_cholesky_solve(S.dense(dd), b)
            if y is not None and not np.all(np.isfinite(y.astype(np.float64))):
                y = None
            model = dt(0)
            if y is not None:
                if steps is not None:
                    steps.append((S.dense(dd), b, y))
                w = np.zeros((NF + 1, 4), dt)
                w[:NF] = (scale * y).reshape(NF, 4)
                fa, fb = G.fidx[G.a], G.fidx[G.b]
                u = _Jv(Ja, w[fa]) + _Jv(Jb, w[fb])              # (a constant node reads the zero row)
                m = u[:, 0] * (res[:, 0] + u[:, 0] / 2)
                for k in (1, 2, 3):
                    m = m + u[:, k] * (res[:, k] + u[:, k] / 2)
                model = -tree_sum(np.where(G.valid, m, 0))
                rec['model'] = model
            if y is None or not (model > 0):
                invalid += 1
                if invalid >= 5:
                    term = FAILURE
                    break
                radius, dec = radius / dec, dec * 2
                continue
            invalid = 0
            yaw2, t2 = yaw.copy(), t.copy()
            raw = yaw[nof] + w[:NF, 0]
            wrapped = wrapped or bool((np.abs(raw) > 180).any())
            yaw2[nof], t2[nof] = normalize(raw), t[nof] + w[:NF, 1:]
            with np.errstate(all='ignore'):
                cost2 = G.evaluate(yaw2, t2, False)[0]
            rec['cand'], rec['flags'] = cost2, 1
            if edit == 'candidate_residuals_kept':              # (a rejected step then meets the candidate's residuals with the old Jacobians)
                res = G.evaluate(yaw2, t2, False)[1]
            dx = ambient(yaw, t) - ambient(yaw2, t2)
            dxn, ptol = np.sqrt(tree_sum(dx * dx)), 1e-8 * (x_norm + 1e-8)
            marg.append(abs(float(dxn - ptol)) / float(ptol))
            if dxn <= ptol:
                term = CONVERGENCE
                break
            marg.append(abs(float(abs(cost - cost2) - 1e-6 * cost)) / float(1e-6 * cost))
            if abs(cost - cost2) <= 1e-6 * cost:
                term = CONVERGENCE
                break
            rho = (cost - cost2) / model
            marg.append(abs(float(rho) - 1e-3) / 1e-3)
            if rho > 1e-3:
                rec['flags'] = 3
                yaw, t = yaw2, t2
                with np.errstate(all='ignore'):
                    cost, res, Ja, Jb, _ = G.evaluate(yaw, t, True)
                t3 = 2 * rho - 1
                radius = min(radius / max(one / 3, 1 - t3 * t3 * t3), dt(1e16))
                dec = dt(2)
                relin = True
            else:
                radius, dec = radius / dec, dec * 2
                if radius < 1e-32:
                    term = CONVERGENCE
                    break
    # ---- updatePose, the drift, the keyframes behind cur_index
    NKF = G.NKF
    T, R = np.zeros((NKF, 3), dt), np.zeros((NKF, 3, 3), dt)
    with np.errstate(all='ignore'):
        T[:N], R[:N] = t, ypr2R(yaw, G.pitch, G.roll, dt)
        yd = R2ypr(R[N - 1:N], dt)[0, 0] - R2ypr(G.vR[N - 1:N], dt)[0, 0]
        rd = ypr2R(np.array([yd], dt), np.zeros(1, dt), np.zeros(1, dt), dt)[0]
        td = T[N - 1] - _mv3(rd, G.vT[N - 1])
        if edit == 'no_tail_drift':
            T[N:], R[N:] = G.vT[N:], G.vR[N:]
        else:
            T[N:] = _mv3(rd[None], G.vT[N:]) + td
            R[N:] = _mm(np.broadcast_to(rd, (NKF - N, 3, 3)), G.vR[N:])
    fin = lambda v: bool(np.all(np.isfinite(np.asarray(v, np.float64))))
    numeric = not (finite0 and fin(T) and fin(R) and fin(cost) and fin(yd) and fin(td))
    if numeric:
        T, R, yd, rd, td = np.zeros((NKF, 3), dt), np.zeros((NKF, 3, 3), dt), dt(0), np.zeros((3, 3), dt), np.zeros(3, dt)
    out.update(status=NUMERIC if numeric else (OK if NF > 0 else NO_EDGES), termination=term, iterations=it, final_cost=cost, T=T, R=R,
               yaw_drift=yd, r_drift=rd, t_drift=td, it_cost=np.array([r['cost'] for r in trace], dt), it_radius=np.array([r['radius'] for r in trace], dt),
               it_cost_cand=np.array([r['cand'] for r in trace], dt), it_model=np.array([r['model'] for r in trace], dt),
               it_flags=np.array([r['flags'] for r in trace], np.int32), it_cg=np.array([r['cg'] for r in trace], np.int32),
               margin=min(marg) if marg else 1.0, wrapped=wrapped)
    return out


# --------------------------------------------------------------------------------------------------- the cases
def scene(seed, n, loops, n_tail=0, split=None, seq0=0, outliers=(), wrap_node=None, first=100, stride=1, all_seq0=False, noise=1.0,
          split_yaw=20.0, huber_delta=None):
    """VIO poses drifting along a loop of about two turns (radius 5 m, pitch and roll about 2 degrees), loop measurements with noise.
    loops: (i, a) pairs of local indices; split: the second sequence starts there (its VIO frame is turned by split_yaw degrees and shifted); seq0: that many leading
    keyframes are of sequence 0; outliers: positions in `loops` whose measurement is off by a metre; wrap_node: that keyframe's VIO yaw
    lies 0.001 degrees inside -180, on the side the correction pushes it over."""
    rng = np.random.default_rng(seed)
    nk = n + n_tail
    pr = rng.normal(0, 2.0, (nk, 2))
    # the drift of the odometry: yaw grows to a few degrees, the position to a few decimetres
    dyaw = np.cumsum(rng.normal(0.04, 0.02, nk)) * noise
    dpos = np.cumsum(rng.normal(0.004, 0.004, (nk, 3)), 0) * noise
    s = np.arange(nk) / max(n - 1, 1)
    ang = 4 * np.pi * s * 0.97
    if wrap_node is not None:
        ang = ang + np.radians(180.001 - (np.degrees(ang[wrap_node]) + 90 + dyaw[wrap_node]))
    true_t = np.stack([5 * np.cos(ang), 5 * np.sin(ang), 0.3 * np.sin(3 * ang)], 1)
    true_yaw = np.degrees(ang) + 90
    R_true = ypr2R(true_yaw, pr[:, 0], pr[:, 1], np.float64)
    vio_R = ypr2R(true_yaw + dyaw, pr[:, 0], pr[:, 1], np.float64)
    vio_T = true_t + dpos
    seq = np.ones(nk, np.int32)
    if split is not None:
        seq[split:] = 2
        off = ypr2R(np.array([split_yaw]), np.zeros(1), np.zeros(1), np.float64)[0]
        vio_T[split:] = vio_T[split:] @ off.T + np.array([1.0, -2.0, 0.3])
        vio_R[split:] = off @ vio_R[split:]
    if seq0:
        seq[:seq0] = 0
    if all_seq0:
        seq[:] = 0
    index = first + stride * np.arange(nk)
    has_loop, loop_index, info = np.zeros(nk, np.int32), np.full(nk, -1, np.int32), np.zeros((nk, 8))
    for k, (i, a) in enumerate(loops):
        rel_t = R_true[a].T @ (true_t[i] - true_t[a]) + rng.normal(0, 0.02, 3) * noise
        rel_yaw = float(normalize(np.float64(true_yaw[i] - true_yaw[a]) % 360.0)) + rng.normal(0, 0.3) * noise
        if k in outliers:
            rel_t = rel_t + np.array([1.0, -0.7, 0.2])
        has_loop[i], loop_index[i] = 1, index[a]
        info[i] = np.concatenate([rel_t, [1, 0, 0, 0], [rel_yaw]])
    g = dict(index=index.astype(np.int32), sequence=seq, has_loop=has_loop, loop_index=loop_index, vio_T=vio_T, vio_R=vio_R, loop_info=info,
             first_looped_index=int(index[0]), n_opt=n)
    if huber_delta is not None:
        g['huber_delta'] = huber_delta
    return g


CASE_ARGS = {
    'n12_one': dict(seed=1, n=12, loops=[(11, 0)]),
    'n40_four': dict(seed=2, n=40, loops=[(24, 4), (29, 9), (34, 14), (39, 19)]),
    'n60_two_seq': dict(seed=3, n=60, loops=[(35, 5), (45, 15), (58, 28)], split=30),
    'n200_thirty': dict(seed=4, n=200, loops=[(100 + 3 * k + (k % 2), 3 * k + 1) for k in range(30)], outliers=(4, 17, 26)),
    'seq0_constant': dict(seed=5, n=40, loops=[(22, 2), (30, 8), (38, 5), (36, 16)], seq0=10),
    'tail': dict(seed=6, n=30, loops=[(20, 5), (29, 14)], n_tail=25),
    'in_band_loop': dict(seed=7, n=20, loops=[(10, 7), (18, 2)]),
    'no_free': dict(seed=8, n=8, loops=[(6, 1)], all_seq0=True),
    'wrap': dict(seed=9, n=24, loops=[(23, 11), (17, 5)], wrap_node=20),
    # rejected steps: a second sequence turned by 150 degrees that hangs on three loop edges with HuberLoss(10), which leaves them their
    # full pull: the first two steps are rejected, and so is one behind an accepted step (the residuals, the blocks and the gradient of
    # the point that stays are used again at a smaller radius)
    'rejected': dict(seed=0, n=24, loops=[(14, 2), (19, 7), (23, 10)], split=12, split_yaw=150.0, huber_delta=10.0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(**CASE_ARGS[name])


@functools.lru_cache(maxsize=None)
def reference(name, route='ld'):
    return solve(case(name), route)


DECISIONS = ('status', 'termination', 'iterations', 'n_edges', 'n_loop_edges', 'n_free')
# the quantities of the bound, each in its own scale, and the outputs that are of that quantity: positions by the graph's extent, rotation
# entries by 1, angles in degrees (their range, 180), costs (the model change is a cost difference) by the initial cost, the radius by the
# largest radius of the trace
KINDS = dict(position=('extent', ('T', 't_drift')), rotation=(1.0, ('R', 'r_drift')), angle=(180.0, ('yaw_drift',)),
             cost=('cost', ('initial_cost', 'final_cost', 'it_cost', 'it_cost_cand', 'it_model')), radius=('radius', ('it_radius',)))
VALUES = {k: s for s, keys in KINDS.values() for k in keys}


def qualify(name):
    """the three routes agree on every decision and the ld route's tests have their margin: asserted, as kf_pnp_ref does for its gates"""
    refs = [reference(name, r) for r in ROUTES]
    for r in refs[1:]:
        for k in DECISIONS:
            assert r[k] == refs[0][k], (name, k, r[k], refs[0][k])
        assert np.array_equal(r['it_flags'], refs[0]['it_flags']), (name, 'it_flags')
    assert refs[0]['margin'] >= MARGIN, (name, 'margin', refs[0]['margin'])
    cg = refs[2]['it_cg']
    assert len(cg) == 0 or cg.max() <= MAX_CG // 2, (name, 'cg', cg)
    return refs


def _scale(name, key, ld):
    s = VALUES[key]
    if s == 'extent':
        T = np.asarray(case(name)['vio_T'], np.float64)
        return float(np.abs(T - T.mean(0)).max())
    if s == 'cost':
        return float(ld['initial_cost'])
    if s == 'radius':
        return float(np.max(np.asarray(ld['it_radius'], np.float64), initial=1.0))
    return s


def _dev(x, ref):
    x, ref = np.asarray(x, LD).reshape(-1), np.asarray(ref, LD).reshape(-1)
    return float(np.abs(x - ref).max()) if len(ref) else 0.0


def ratios(name, got, refs=None):
    """per quantity (KINDS): max |got - ld| over max(E64, floor), E64 the larger disagreement of the two float64 routes with ld over the
    outputs of that quantity"""
    ld, d64, p64 = refs or qualify(name)
    out = {}
    for kind, (_, keys) in KINDS.items():
        e64 = max([_dev(o[k], ld[k]) for o in (d64, p64) for k in keys] + [E64_FLOOR * _scale(name, keys[0], ld)])
        out[kind] = max(_dev(got[k], ld[k]) for k in keys) / e64
    return out


def _fe():
    import __graft_entry__ as graft
    graft.load_package()
    from vins_mono_amd import fe
    return fe


def check_graph(name, got, tag):
    refs = qualify(name)
    ld, p64 = refs[0], refs[2]
    for k in DECISIONS:
        assert got[k] == ld[k], (name, k, got[k], ld[k])
    assert np.array_equal(got['it_flags'], ld['it_flags']), (name, got['it_flags'], ld['it_flags'])
    assert len(got['it_cg']) == len(p64['it_cg']) and np.all(np.abs(got['it_cg'] - p64['it_cg']) <= 1), (name, got['it_cg'], p64['it_cg'])
    r = ratios(name, got, refs)
    worst = max(r.values())
    print(f"kf_pgo[{tag}] {name}: iterations {got['iterations']} termination {got['termination']} cg {list(got['it_cg'])} "
          f"worst ratio {worst:.3g} ({max(r, key=r.get)}) margin {ld['margin']:.2e}")
    assert worst <= M, (name, r)
    return worst


def check_cases(h, tag, names=None):
    fe = _fe()
    table = {}
    for name in names or CASE_ARGS:
        table[name] = check_graph(name, fe.pg_optimize(h, [case(name)])[0], tag)
    print(f"kf_pgo[{tag}] worst ratio over the cases: {max(table.values()):.3g}")
    return table


def told_apart(name, got, route_checked=False):
    """does the case table's check tell `got` from the definition"""
    refs = qualify(name)
    if any(got[k] != refs[0][k] for k in DECISIONS) or not np.array_equal(got['it_flags'], refs[0]['it_flags']):
        return True
    if route_checked and (len(got['it_cg']) != len(refs[2]['it_cg']) or np.any(np.abs(got['it_cg'] - refs[2]['it_cg']) > 1)):
        return True
    return max(ratios(name, got, refs).values()) > M


def check_mutations():
    """every edit of EDITS, run through the restatement (dense64; the CG edit through pcg64), is told from the definition by some case;
    the equivalent one by none.  Returns {edit: the cases that catch it}."""
    out = {}
    for edit in EDITS:
        route = 'pcg64' if edit == 'cg_1e-3' else 'dense64'
        out[edit] = [n for n in CASE_ARGS if told_apart(n, solve(case(n), route, edit), route == 'pcg64')]
        assert bool(out[edit]) != (edit in EQUIVALENT_EDITS), (edit, out[edit])
    return out


def check_case_properties():
    """what the cases are there for"""
    assert reference('n12_one', 'pcg64')['it_cg'].max() == 1
    assert reference('n200_thirty')['huber'] >= 3
    assert reference('no_free')['status'] == NO_EDGES and reference('no_free')['iterations'] == 0
    assert reference('wrap')['wrapped']
    assert reference('seq0_constant')['n_free'] == 30                   # 40 keyframes, 10 of them of sequence 0
    g = case('tail')
    assert len(g['index']) == g['n_opt'] + 25
    fl = list(reference('rejected')['it_flags'])
    assert fl[0] == 1 and any(fl[k] == 3 and fl[k + 1] == 1 for k in range(len(fl) - 1)), fl
    for name in CASE_ARGS:
        if name != 'no_free':
            assert 2 <= reference(name)['iterations'] <= 5 and (reference(name)['it_flags'] == 3).any(), name


OUT_KEYS = ('T', 'R', 'yaw_drift', 'r_drift', 't_drift', 'initial_cost', 'final_cost', 'it_cost', 'it_radius', 'it_cost_cand', 'it_model', 'it_flags', 'it_cg')


def same_output(a, b):
    return all(a[k] == b[k] for k in DECISIONS) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in OUT_KEYS)


def batch(n, seed=77):
    """n graphs of mixed sizes (the cases first, then small seeded scenes)"""
    names = list(CASE_ARGS)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i < 3:
            out.append(case(('n40_four', 'no_free', 'tail')[i]))
        else:
            m = int(rng.integers(6, 30))
            out.append(scene(1000 + i, m, [(m - 1, int(rng.integers(0, max(m - 6, 1))))], n_tail=int(rng.integers(0, 4))))
    return out


def check_batch_equals_single(h, sizes=(1, 3, 33)):
    fe = _fe()
    for n in sizes:
        gs = batch(n)
        together = fe.pg_optimize(h, gs)
        for i, g in enumerate(gs):
            assert same_output(together[i], fe.pg_optimize(h, [g])[0]), (n, i)
        assert len({g['status'] for g in together}) >= min(n, 2) or n == 1


def overflow_graph():
    """finite inputs that overflow inside: VG_PG_NUMERIC"""
    g = dict(case('n12_one'))
    T = g['vio_T'].copy()
    T[5] = [1e308, -1e308, 1e308]
    g['vio_T'] = T
    return g


def check_failed_neighbours(h):
    fe = _fe()
    gs = [case('n40_four'), overflow_graph(), case('in_band_loop')]
    got = fe.pg_optimize(h, gs)
    assert [x['status'] for x in got] == [OK, NUMERIC, OK]
    assert not got[1]['T'].any() and not got[1]['R'].any() and not got[1]['r_drift'].any() and got[1]['yaw_drift'] == 0
    assert same_output(got[0], fe.pg_optimize(h, [gs[0]])[0]) and same_output(got[2], fe.pg_optimize(h, [gs[2]])[0])
    assert solve(gs[1], 'dense64')['status'] == NUMERIC


def _refusals():
    g = case('n12_one')

    def changed(key, i, v):
        a = np.array(g[key]).copy()
        a.reshape(len(a), -1)[i] = v
        return {key: a}
    li = g['loop_index'].copy()
    return {
        'in_struct_size': dict(struct_size=8),
        'out_struct_size': dict(out_struct_size=8),
        'n_kf_zero': dict(n_kf=0),
        'n_kf_over': dict(n_kf=MAX_KEYFRAMES + 1),
        'n_opt_zero': dict(n_opt=0),
        'n_opt_over': dict(n_opt=13),
        'null_table': dict(vio_R=None),
        'index_not_ascending': changed('index', 4, g['index'][3]),
        'first_below_first_looped': dict(first_looped_index=int(g['index'][0]) + 1),
        'negative_sequence': changed('sequence', 2, -1),
        'loop_below_first_looped': changed('loop_index', 11, int(g['index'][0]) - 1),
        'loop_not_in_slice': dict(index=(g['index'] * 2).astype(np.int32), first_looped_index=int(g['index'][0]) * 2, loop_index=li * 2 + 1),
        'loop_not_before': changed('loop_index', 11, int(g['index'][11])),
        'nan_T': changed('vio_T', 3, np.nan),
        'inf_R': changed('vio_R', 7, np.inf),
        'nan_loop_info': changed('loop_info', 11, np.nan),
        'max_iters_zero': dict(max_iters=0),
        'max_iters_over': dict(max_iters=MAX_ITERS + 1),
        'huber_zero': dict(huber_delta=0.0),
        'huber_nan': dict(huber_delta=float('nan')),
    }


REFUSALS = tuple(_refusals())


def check_refusal(h, name):
    """refused with VG_ERR_BAD_ARG, nothing moved (the good neighbour's outputs too), the handle usable"""
    fe = _fe()
    good = case('n12_one')
    bad = dict(good)
    bad.update(_refusals()[name])
    want = fe.pg_optimize(h, [good])[0]
    L = fe.pg_lib(h)
    ins, outs = (fe.PgIn * 2)(), (fe.PgOut * 2)()
    keep = [fe.pg_fill(L, ins[i], outs[i], g) for i, g in enumerate((good, bad))]
    for o in outs:
        o.status, o.iterations, o.final_cost = -7, -7, -7.0
    for _, T, R in keep:
        T[...], R[...] = -7.0, -7.0
    rc = L.vg_pg_optimize(h.h, 2, ins, outs)
    assert rc == -1, (name, rc)                                 # VG_ERR_BAD_ARG
    L.vg_last_error.restype = fe.C.c_char_p
    L.vg_last_error.argtypes = [fe.C.c_void_p]
    msg = L.vg_last_error(h.h).decode()
    assert 'vg_pg_optimize: graph 1' in msg, (name, msg)
    for o in outs:
        assert (o.status, o.iterations, o.final_cost) == (-7, -7, -7.0), name
    for _, T, R in keep:
        assert (T == -7.0).all() and (R == -7.0).all(), name
    assert same_output(fe.pg_optimize(h, [good])[0], want), name


def capacity_graph():
    n = MAX_KEYFRAMES
    return scene(11, n, [(n - 1, 40), (n // 2, 3)], noise=0.02)


def check_capacity(h, tag):
    """VG_PG_MAX_KEYFRAMES keyframes with two loop edges, held to the pcg64 route ONLY: the long-double and the dense float64 routes
    (8188 unknowns) are too large at that size.  E64 is there the disagreement of a second float64 route that still fits, scipy's
    sparse LU on the same system, with pcg64; the bound stays M times it (floored as everywhere).  One keyframe more is refused."""
    fe = _fe()
    g = capacity_graph()
    got = fe.pg_optimize(h, [g])[0]
    ref, other = solve(g, 'pcg64'), solve(g, 'sparse64')
    for k in DECISIONS:
        assert got[k] == ref[k] == other[k], (k, got[k], ref[k], other[k])
    assert np.array_equal(got['it_flags'], ref['it_flags']) and np.array_equal(other['it_flags'], ref['it_flags'])
    assert np.all(np.abs(got['it_cg'] - ref['it_cg']) <= 1) and ref['it_cg'].max() <= MAX_CG // 2
    T = np.asarray(g['vio_T'])
    ext, c0 = float(np.abs(T - T.mean(0)).max()), float(ref['initial_cost'])
    worst = 0.0
    for kind, (s, keys) in KINDS.items():
        sc = ext if s == 'extent' else c0 if s == 'cost' else float(ref['it_radius'].max()) if s == 'radius' else s
        e64 = max([_dev(other[k], ref[k]) for k in keys] + [E64_FLOOR * sc])
        r = max(_dev(got[k], ref[k]) for k in keys) / e64
        worst = max(worst, r)
        print(f"kf_pgo[{tag}] capacity {kind}: ratio {r:.3g}")
    assert worst <= M, worst
    over = scene(12, MAX_KEYFRAMES + 1, [(50, 3)])
    try:
        fe.pg_optimize(h, [over])
    except Exception as e:
        assert 'n_kf outside 1 .. VG_PG_MAX_KEYFRAMES' in str(e), e
    else:
        raise AssertionError('VG_PG_MAX_KEYFRAMES + 1 keyframes were accepted')
    return worst


def check_chain(h):
    """vg_kf_pnp -> loop_info -> vg_pg_optimize on one pair built with the kf_pnp_ref scene: the loop edge of the last keyframe carries the
    device's own loop_info, and the result equals the call fed the same eight numbers from the PnP restatement's output layout"""
    import kf_pnp_ref as K
    fe = _fe()
    pnp = fe.kf_pnp(h, [K.case('n150')])[0]
    assert pnp['status'] == K.OK and pnp['has_loop'] == 1
    g = dict(case('n12_one'))
    info = g['loop_info'].copy()
    info[11] = pnp['loop_info']
    g['loop_info'] = info
    got = fe.pg_optimize(h, [g])[0]
    ref = solve(g, 'pcg64')
    assert got['status'] == OK and got['n_loop_edges'] == 1
    for k in DECISIONS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert np.abs(got['T'] - ref['T']).max() <= 1e-9 and np.abs(got['R'] - ref['R']).max() <= 1e-9
    return got


def _m3v(R, v):
    return R[:, 0] * v[0] + R[:, 1] * v[1] + R[:, 2] * v[2]


def _m3m(A, B):
    return np.stack([A[:, 0] * B[0, j] + A[:, 1] * B[1, j] + A[:, 2] * B[2, j] for j in range(3)], 1)


def _yaw_of(R):
    return math.atan2(R[1, 0], R[0, 0]) / math.pi * 180.0


def _yaw_rotation(yaw):
    y = yaw / 180.0 * math.pi
    return np.array([[math.cos(y), -math.sin(y), 0.0], [math.sin(y), math.cos(y), 0.0], [0.0, 0.0, 1.0]])


def _q2R(q):
    w, x, y, z = (float(v) for v in q)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def bookkeeping(g):
    """PoseGraph::addKeyFrame's pose bookkeeping (pose_graph.cpp:44-62, :82-128) over the keyframes of a graph in list order, with the
    products in the order the C++ class forms them: the graph optimize4DoF then packs (the VIO poses shifted to the base frame, a
    sequence whose first loop crosses sequences moved as a whole; cur_index the last keyframe that pushed a loop)"""
    n, n_opt = len(g['index']), g['n_opt']
    T, R = np.array(g['vio_T'], np.float64), np.array(g['vio_R'], np.float64).reshape(-1, 3, 3)
    seq, index = g['sequence'], list(g['index'])
    w_r, w_t, seq_cnt, seq_loop, earliest, pushed = np.eye(3), np.zeros(3), 0, [0], g['first_looped_index'], []
    for i in range(n):
        if seq_cnt != seq[i]:
            seq_cnt += 1
            seq_loop.append(0)
            w_r, w_t = np.eye(3), np.zeros(3)
        T[i], R[i] = _m3v(w_r, T[i]) + w_t, _m3m(w_r, R[i])
        if g['has_loop'][i] and i < n_opt:
            a = index.index(g['loop_index'][i])
            earliest = min(earliest, index[a])
            w_P_cur, w_R_cur = _m3v(R[a], g['loop_info'][i][:3]) + T[a], _m3m(R[a], _q2R(g['loop_info'][i][3:7]))
            shift_r = _yaw_rotation(_yaw_of(w_R_cur) - _yaw_of(R[i]))
            shift_t = w_P_cur - _m3v(_m3m(w_R_cur, R[i].T), T[i])
            if seq[a] != seq[i] and seq_loop[seq[i]] == 0:
                w_r, w_t = shift_r, shift_t
                for k in [i] + [k for k in range(i) if seq[k] == seq[i]]:
                    T[k], R[k] = _m3v(w_r, T[k]) + w_t, _m3m(w_r, R[k])
                seq_loop[seq[i]] = 1
            pushed.append(i)
    out = dict(g)
    out.update(vio_T=T, vio_R=R, n_opt=pushed[-1] + 1, first_looped_index=earliest)
    return out


# n60_two_seq: its first loop crosses sequences, so addLoop moves the second sequence as a whole (and shiftToBase resets the shift at its
# start); its last loop sits on the keyframe before the last, which therefore only receives the drift
REPLAY_CASES = ('n40_four', 'tail', 'n60_two_seq')


def check_replay(h, exe, tmp_dir, name):
    """PoseGraph's pose bookkeeping and one pass of optimize4DoF (host/pose_graph.h, vg_pack_pg) through `vins_replay pgo` against the
    binding fed the graph that the restated bookkeeping leaves, number for number"""
    import os
    import subprocess
    g = case(name)
    src, dst = os.path.join(str(tmp_dir), name + '.bin'), os.path.join(str(tmp_dir), name + '.txt')
    write_file(src, g)
    subprocess.run([exe, 'pgo', src, dst], check=True, timeout=600)
    g2 = bookkeeping(g)
    if name != 'n60_two_seq':
        assert np.array_equal(g2['vio_T'], g['vio_T']) and g2['n_opt'] == g['n_opt']       # (one sequence: nothing moves)
    else:
        assert not np.allclose(g2['vio_T'][30:], np.asarray(g['vio_T'])[30:], atol=0.1) and g2['n_opt'] == 59
    want = _fe().pg_optimize(h, [g2])[0]
    rows = [ln.split() for ln in open(dst).read().splitlines()]
    assert [int(x) for x in rows[0][1:]] == [1] + [want[k] for k in DECISIONS], rows[0]
    assert [float(x) for x in rows[1][1:]] == [want['initial_cost'], want['final_cost']]
    drift = np.array([float(x) for x in rows[2][1:]])
    assert drift[0] == want['yaw_drift'] and np.array_equal(drift[1:10], want['r_drift'].reshape(-1)) and np.array_equal(drift[10:], want['t_drift'])
    kfs = rows[3:]
    assert len(kfs) == len(g['index'])
    for i, r in enumerate(kfs):
        assert r[0] == 'kf' and int(r[1]) == g['index'][i] and (i >= g2['n_opt'] or int(r[2]) == i)
        v = np.array([float(x) for x in r[3:]])
        assert np.array_equal(v[:3], want['T'][i]) and np.array_equal(v[3:], want['R'][i].reshape(-1)), (name, i)


def write_file(path, g):
    """a graph as the stand-alone programs read it: int32 n_kf n_opt first_looped_index max_iters, float64 huber_delta, then the tables"""
    with open(path, 'wb') as f:
        n = len(g['index'])
        np.array([n, g.get('n_opt', n), g['first_looped_index'], g.get('max_iters', 5)], '<i4').tofile(f)
        np.array([g.get('huber_delta', 0.1)], '<f8').tofile(f)
        for k in ('index', 'sequence', 'has_loop', 'loop_index'):
            np.ascontiguousarray(g[k], '<i4').tofile(f)
        for k in ('vio_T', 'vio_R', 'loop_info'):
            np.ascontiguousarray(g[k], '<f8').tofile(f)
