"""80-bit reference, condition-aware bound and case table for the DLT triangulation kernels (helper module of
tests/test_tri_scale.py; no tests in here).

`dlt_matrix` forms the 2n x 4 matrix of FeatureManager::triangulate (feature_manager.cpp:216-241) in the requested number format
from the widened float64 inputs; `null_vector` takes its right singular vector of the smallest singular value by a one-sided
(Hestenes) Jacobi on the four columns, written out here in the matrix's own dtype (rotating while |gamma| > 1e-20 sqrt(alpha beta));
`reference` returns d = v2 / v3, the singular values s1 >= .. >= s4 and v3.

The bound of one landmark:
    bound = C * eps * (1 + |d|) / |v3| * ( s1 / (s3 - s4) + max(1, max|Ps|) / (s3 - s4) ),  eps = 2^-52
first term: the null vector's sensitivity to rounding in the decomposition (Wedin: angle <= |dA| / gap, |dA| ~ eps s1; d = v2 / v3
moves by (1 + |d|) / |v3| per unit of angle); second term: the cancellation when the matrix is formed from t1 - t0 in float64
(entries of size max|Ps| lose eps max|Ps| absolute before they enter a matrix whose gap is s3 - s4).

With np.float64 the same code is the restatement that takes the EDITS of the mutation condition."""
import functools

import numpy as np

from oracle import ba_numpy as B

LD = np.longdouble
EPS = 2.0 ** -52
K = 12
EDITS = ('largest_column', 'point_not_normalised', 't_by_R1', 'two_sweeps')


# --------------------------------------------------------------------------------------------------- the reference
def dlt_matrix(Ps, Rs, tic, ric, i0, n, pts, dtype=LD, edit=None):
    """pts: the n points of the landmark's observations (feature_per_frame[j].point)"""
    w = lambda v: np.asarray(v, np.float64).astype(dtype)
    Ps, Rs, tic, ric, pts = w(Ps), w(Rs).reshape(-1, 3, 3), w(tic), w(ric).reshape(3, 3), w(pts).reshape(-1, 3)
    t0 = Ps[i0] + Rs[i0] @ tic
    R0 = Rs[i0] @ ric
    A = np.zeros((2 * n, 4), dtype)
    for j in range(n):
        t1 = Ps[i0 + j] + Rs[i0 + j] @ tic
        R1 = Rs[i0 + j] @ ric
        t = (R1.T if edit == 't_by_R1' else R0.T) @ (t1 - t0)
        R = R0.T @ R1
        P = np.zeros((3, 4), dtype)
        P[:, :3] = R.T
        P[:, 3] = -R.T @ t
        f = pts[j] if edit == 'point_not_normalised' else pts[j] / np.sqrt(pts[j] @ pts[j])
        A[2 * j] = f[0] * P[2] - f[2] * P[0]
        A[2 * j + 1] = f[1] * P[2] - f[2] * P[1]
    return A


def null_vector(A, sweeps=60, largest=False):
    """(v, s): the right singular vector of the smallest (largest=True: largest) singular value and s1 >= .. >= s4, A's dtype"""
    A = A.copy()
    dtype = A.dtype.type
    V = np.eye(4, dtype=dtype)
    tol = dtype(1e-20) if dtype is LD else dtype(1e-16)            # (float64: a threshold below eps, every sweep rotates)
    for _ in range(sweeps):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                alpha, beta, gamma = A[:, p] @ A[:, p], A[:, q] @ A[:, q], A[:, p] @ A[:, q]
                if gamma != 0 and abs(gamma) > tol * np.sqrt(alpha * beta):
                    rotated = True
                    zeta = (beta - alpha) / (2 * gamma)
                    tn = (1 if zeta >= 0 else -1) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = 1 / np.sqrt(1 + tn * tn)
                    s = c * tn
                    A[:, p], A[:, q] = c * A[:, p] - s * A[:, q], s * A[:, p] + c * A[:, q]
                    V[:, p], V[:, q] = c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]
        if not rotated:
            break
    norms = np.sqrt((A * A).sum(axis=0))
    pick = int(np.argmax(norms)) if largest else int(np.argmin(norms))
    return V[:, pick], np.sort(norms)[::-1]


def reference(Ps, Rs, tic, ric, i0, n, pts, dtype=LD, edit=None):
    A = dlt_matrix(Ps, Rs, tic, ric, i0, n, pts, dtype, edit)
    with np.errstate(all='ignore'):
        v, s = null_vector(A, sweeps=2 if edit == 'two_sweeps' else 60, largest=(edit == 'largest_column'))
        d = v[2] / v[3]
    return dict(d=d, s=s, v3=v[3], max_ps=float(np.abs(np.asarray(Ps, np.float64)).max()))


def bound(ref, C):
    gap = ref['s'][2] - ref['s'][3]
    if not (gap > 0) or ref['v3'] == 0 or not np.isfinite(float(ref['d'])):
        return np.inf
    return float(C * EPS * (1 + abs(ref['d'])) / abs(ref['v3']) * (ref['s'][0] / gap + max(1.0, ref['max_ps']) / gap))


# --------------------------------------------------------------------------------------------------- the cases
TIC = np.array([0.03, -0.02, 0.05])
RIC = B.q2R(B.qnormalized(np.array([0.01, -0.02, 0.015, 1.0])))


def _poses(rng, origin, baseline):
    """K exact poses: steps of length `baseline` mostly across the optical axis, a few degrees of rotation per frame"""
    Ps, Rs = np.zeros((K, 3)), np.zeros((K, 3, 3))
    p, q = np.full(3, float(origin)) + rng.normal(0, 1, 3), B.qnormalized(np.concatenate([rng.normal(0, 0.2, 3), [1.0]]))
    for k in range(K):
        Ps[k], Rs[k] = p, B.q2R(q)
        step = rng.normal(0, 1, 3) * [1.0, 1.0, 0.3]
        p = p + baseline * step / np.linalg.norm(step)
        q = B.qnormalized(B.qmul(q, np.concatenate([rng.normal(0, 0.01, 3), [1.0]])))
    return Ps, Rs


def _observe(rng, Ps, Rs, i0, n, x_c0, noise, scaled):
    """the n points of a landmark that sits at x_c0 in the camera of frame i0"""
    xw = Rs[i0] @ (RIC @ x_c0 + TIC) + Ps[i0]
    out = np.zeros((n, 3))
    for j in range(n):
        xc = RIC.T @ (Rs[i0 + j].T @ (xw - Ps[i0 + j]) - TIC)
        pt = np.array([xc[0] / xc[2], xc[1] / xc[2], 1.0])
        pt[:2] += rng.normal(0, noise, 2) if noise else 0.0
        out[j] = pt * (rng.uniform(0.5, 3.0) if scaled else 1.0)
    return out


class Scene:
    """One vg_triangulate call: poses and a landmark table (start, nobs, obs_off, points)."""

    def __init__(self, name, Ps, Rs):
        self.name, self.Ps, self.Rs = name, Ps, Rs
        self.start, self.nobs, self.blocks, self.share = [], [], [], []

    def add(self, i0, pts, share=None):
        """share: (index of the landmark whose block this one reads, number of its observations taken)"""
        self.start.append(i0)
        self.nobs.append(len(pts) if share is None else share[1])
        self.blocks.append(pts)
        self.share.append(share)

    def table(self, order=None):
        """(start, nobs, obs_off, points): blocks laid out in `order` (default: reversed, so obs_off is not ascending)"""
        L = len(self.start)
        own = [l for l in range(L) if self.share[l] is None]
        order = list(reversed(own)) if order is None else order
        off, at, chunks = {}, 0, []
        for l in order:
            off[l] = at
            at += len(self.blocks[l])
            chunks.append(self.blocks[l])
        obs_off = [off[l] if self.share[l] is None else off[self.share[l][0]] for l in range(L)]
        return np.array(self.start, np.int32), np.array(self.nobs, np.int32), np.array(obs_off, np.int32), np.concatenate(chunks)

    def points_of(self, l):
        return self.blocks[l] if self.share[l] is None else self.blocks[self.share[l][0]][:self.share[l][1]]

    def sub(self, idx):
        s = Scene(self.name, self.Ps, self.Rs)
        for l in idx:
            s.add(self.start[l], self.points_of(l))
        return s

    def __len__(self):
        return len(self.start)


NOBS = (2, 3, 6, 11, 12)


def _fill(rng, sc, noise, depth, scaled_every=3):
    """every (nobs, start) of the issue's table once, depth drawn log-uniformly from `depth`"""
    for n in NOBS:
        for i0 in range(K - n + 1):
            dep = float(np.exp(rng.uniform(np.log(depth[0]), np.log(depth[1]))))
            x = dep * np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 1.0])
            sc.add(i0, _observe(rng, sc.Ps, sc.Rs, i0, n, x, noise, scaled=(len(sc) % scaled_every == 0)))
    six = next(l for l in range(len(sc)) if sc.nobs[l] == 6)
    sc.add(sc.start[six], None, share=(six, 3))                    # two landmarks on one observation block
    return sc


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> Scene.  The well-posed half (origin 0, baselines 0.1 .. 1 m, depth 0.5 .. 10) is what keeps the table from going
    soft; the rest walks the issue's ranges: origin 1e4, baselines down to 1 mm, depth up to 50, pixel noise 0 and 1e-3."""
    rng = np.random.default_rng(1019)
    out = {}
    for rep in range(2):
        for baseline in (0.1, 0.3, 1.0):
            for noise in (0.0, 1e-3):
                name = f"well_b{baseline}_n{noise}_{rep}"
                out[name] = _fill(rng, Scene(name, *_poses(rng, 0.0, baseline)), noise, (0.5, 10.0))
    for origin in (0.0, 1e4):
        for baseline in (1e-3, 1e-2, 0.1, 1.0):
            noise = 1e-3 if baseline in (1e-2, 1.0) else 0.0
            name = f"wide_o{origin:g}_b{baseline}_n{noise}"
            out[name] = _fill(rng, Scene(name, *_poses(rng, origin, baseline)), noise, (0.5, 50.0))
    # ---- the 0.1 cut: the landmark 0.1 -/+ 1e-3 in front of its first camera (5 mm steps: every observing camera about 0.1 m away),
    #      points behind the camera, pure rotation, identical points
    Ps, Rs = _poses(rng, 0.0, 0.005)
    sc = Scene("cut", Ps, Rs)
    for n in (2, 3, 6, 12):
        for dep in (0.099, 0.101, 0.0995, 0.1005):
            x = dep * np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 1.0])
            sc.add(0, _observe(rng, Ps, Rs, 0, n, x, 0.0, scaled=False))
        for dep in (-0.5, -4.0):                                   # behind the camera: d < 0
            x = dep * np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 1.0])
            sc.add(K - n, _observe(rng, Ps, Rs, K - n, n, x, 0.0, scaled=(n == 3)))
    out["cut"] = sc
    Pr = np.tile(Ps[:1], (K, 1))                                   # the body stands still: the lever arm tic leaves a few mm of baseline
    sc = Scene("degenerate", Pr, Rs)
    sc.add(0, _observe(rng, Pr, Rs, 0, 6, np.array([0.4, -0.2, 3.0]), 0.0, False))
    sc.add(3, _observe(rng, Pr, Rs, 3, 2, np.array([-0.3, 0.1, 8.0]), 0.0, False))
    sc.add(0, np.tile([[0.1, -0.2, 1.0]], (6, 1)))                 # identical points
    sc.add(5, np.tile([[0.0, 0.0, 1.0]], (2, 1)))
    out["degenerate"] = sc
    Pc = np.array([Ps[0] + Rs[0] @ TIC - Rs[k] @ TIC for k in range(K)])       # pure rotation about the camera centre: t1 - t0 = rounding
    sc = Scene("pure_rotation", Pc, Rs)
    sc.add(0, _observe(rng, Pc, Rs, 0, 6, np.array([0.4, -0.2, 3.0]), 0.0, False))
    sc.add(4, _observe(rng, Pc, Rs, 4, 2, np.array([-0.3, 0.1, 8.0]), 1e-3, True))
    out["pure_rotation"] = sc
    return out


@functools.lru_cache(maxsize=None)
def scene_reference(name):
    """per landmark of scenes()[name]: the 80-bit reference"""
    sc = scenes()[name]
    return [reference(sc.Ps, sc.Rs, TIC, RIC, sc.start[l], sc.nobs[l], sc.points_of(l)) for l in range(len(sc))]


@functools.lru_cache(maxsize=None)
def block_scene():
    """130 landmarks on one set of poses for the block-edge calls (L = 1, 63, 64, 65, 130)"""
    rng = np.random.default_rng(130)
    Ps, Rs = _poses(rng, 0.0, 0.3)
    sc = Scene("blocks", Ps, Rs)
    while len(sc) < 130:
        n = int(rng.choice(NOBS))
        i0 = int(rng.integers(0, K - n + 1))
        x = float(rng.uniform(0.5, 10.0)) * np.array([rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4), 1.0])
        sc.add(i0, _observe(rng, Ps, Rs, i0, n, x, 1e-3, scaled=(len(sc) % 4 == 0)))
    return sc
