"""vg_init_exrot (include/vinsgpu.h): scenes, reference, metric and the check bodies that tests/test_init_exrot_simt.py (emulated kernels)
and tests/test_init_exrot_gpu.py (MI355X) both run; tests/test_init_exrot_def.py runs the reference against itself.

REFERENCE
  fundamental matrix   oracle.fe_cpu.reject_with_f(ll, rr, threshold) for the model and the inlier count, RANSAC (15 points or more) and LMedS
                       (9 .. 14) alike; the winning iteration, the bound and the last iteration by init_relpose_ref.ransac_replay (threshold: the window's, 3.0 by default)
  rotation stage       `rotation()`, a restatement of decomposeE / testTriangulation / the pick as the header defines them, taking THE
                       DEVICE'S OWN F TAP: route 'ld' (numpy.longdouble, the header's Jacobi SVDs), 'jac64' (the same in float64) and
                       'svd64' (numpy.linalg.svd for the 3x3 matrix and the 6x4 design matrices).  The float32 roundings the header
                       names are part of the definition and are the same in every route.
  calibration stage    `calib_step()`, one step of CalibrationExRotation in the same three routes ('svd64': numpy.linalg.svd of A).
A LAPACK SVD may name R1 what the header's convention names R2: routes are compared by the picked matrix, not by its index.

WHY EVERY STEP IS SEEDED FROM THE DEVICE'S TAPS.  The block of one record is x -> a x - x m for two unit quaternions, whose singular
values come in two equal PAIRS; after the first step (and while every record turns about one axis) the smallest singular value is
double, the vector the reference takes is decided by rounding, and through Rc_g and the Huber weight of the next record that choice
reaches everything after it.  Three routes run as whole chains therefore part at step 1 for reasons that say nothing about the device.
So step k of every route starts from the device's ric of step k-1 and the device's records 0 .. k-1, and is compared with the device's
step k.  E64, the larger disagreement of the two float64 routes with 'ld', is then the conditioning of that one step: of order one where
the smallest singular value is double (nothing can be held there), 1e-15 where it is not.  Values are held to M = 4 x max(E64, floor).

CONDITIONS the scenes meet (`conditions`, asserted by test_init_exrot_def.py, and again on the device's taps by check_window): the three
routes take the same decisions -- no ratio1 == ratio2, no depth within float32 rounding of zero (every |z| above 1e-4 where its sign
counts), sigma[2] not within 1e-6 of the threshold, no angular distance within 1e-6 degrees of huber_deg."""
import ctypes as C
import functools
import math
import os
import struct
import subprocess
import sys

import numpy as np

import init_relpose_ref as RP

ROOT = RP.ROOT
from oracle import fe_cpu  # noqa: E402

LD = np.longdouble
F32 = np.float32
M = 4.0
OK, NUMERIC = 0, 1
THRESH, MIN_POINTS, HUBER_DEG, MIN_FRAMES, COV = 3.0, 9, 5.0, 10, 0.25
PX = 1.0 / 460.0
NOISE_PX = 0.05
E64_FLOOR = 2.0 ** -52          # one rounding of a unit-scale number


# --------------------------------------------------------------------------------------------------- Eigen's small conversions, any dtype
def inv3(m):
    """Eigen's 3x3 inverse: cofactors over the determinant taken from the first column"""
    m = np.asarray(m)
    dt = m.dtype.type

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[i1, j1] * m[i2, j2] - m[i1, j2] * m[i2, j1]
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = (c00 * m[0, 0] + c10 * m[1, 0]) + c20 * m[2, 0]
    invdet = dt(1) / det
    o = np.zeros((3, 3), m.dtype)
    for r in range(3):
        for c in range(3):
            o[r, c] = cof(c, r) * invdet
    return o


def q_from_R(m):
    """Quaterniond(Matrix3d), returned as x y z w"""
    m = np.asarray(m)
    dt = m.dtype.type
    q = np.zeros(4, m.dtype)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + dt(1))
        q[3] = dt(0.5) * t
        t = dt(0.5) / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + dt(1))
        q[i] = dt(0.5) * t
        t = dt(0.5) / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def R_from_q(q):
    """toRotationMatrix of the coefficients x y z w, not normalised"""
    q = np.asarray(q)
    dt = q.dtype.type
    x, y, z, w = q
    tx, ty, tz = dt(2) * x, dt(2) * y, dt(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[dt(1) - (tyy + tzz), txy - twz, txz + twy], [txy + twz, dt(1) - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, dt(1) - (txx + tyy)]], q.dtype)


def block(Rc, Rimu, Rcg, dtype, huber_deg=HUBER_DEG):
    """(huber (L - R) [4, 4], huber, the angular distance in degrees) of one record"""
    dt = dtype
    a, g, m = q_from_R(np.asarray(Rc, dt)), q_from_R(np.asarray(Rcg, dt)), q_from_R(np.asarray(Rimu, dt))
    bw, bx, by, bz = g[3], -g[0], -g[1], -g[2]
    dw = a[3] * bw - a[0] * bx - a[1] * by - a[2] * bz
    dx = a[3] * bx + a[0] * bw + a[1] * bz - a[2] * by
    dy = a[3] * by + a[1] * bw + a[2] * bx - a[0] * bz
    dz = a[3] * bz + a[2] * bw + a[0] * by - a[1] * bx
    ang = (dt(180) / dt(np.pi if dt is not LD else LD(np.pi))) * (dt(2) * np.arctan2(np.sqrt(dx * dx + dy * dy + dz * dz), np.abs(dw)))
    huber = dt(huber_deg) / ang if ang > huber_deg else dt(1)
    x, y, z, w = a
    X, Y, Z, Wm = m
    L = np.array([[w, -z, y, x], [z, w, -x, y], [-y, x, w, z], [-x, -y, -z, w]], dt)
    Rm = np.array([[Wm, Z, -Y, X], [-Z, Wm, X, Y], [Y, -X, Wm, Z], [-X, -Y, -Z, Wm]], dt)
    return huber * (L - Rm), huber, ang


def jacobi4(A):
    """(squared column norms, V, converged) of the header's one-sided Jacobi on the four columns of A [rows, 4]"""
    A = A.copy()
    dt = A.dtype.type
    V = np.eye(4, dtype=A.dtype)
    signal = dt(1e-26) * np.sum(A * A)
    conv = False
    for _ in range(40):
        big = False
        for p in range(3):
            for q in range(p + 1, 4):
                x, y = A[:, p], A[:, q]
                al, be, ga = np.sum(x * x), np.sum(y * y), np.sum(x * y)
                lim = np.sqrt(al * be)
                if abs(ga) > dt(1e-16) * lim and ga != 0:
                    big = big or (abs(ga) > dt(1e-13) * lim and al > signal and be > signal)
                    zeta = (be - al) / (dt(2) * ga)
                    tn = (dt(1) if zeta >= 0 else dt(-1)) / (abs(zeta) + np.sqrt(dt(1) + zeta * zeta))
                    cs = dt(1) / np.sqrt(dt(1) + tn * tn)
                    sn = cs * tn
                    for Mx in (A, V):
                        u, v = Mx[:, p].copy(), Mx[:, q].copy()
                        Mx[:, p], Mx[:, q] = cs * u - sn * v, sn * u + cs * v
        if not big:
            conv = True
            break
    return np.sum(A * A, 0), V, conv


def solve_A(blocks, dtype, route):
    """(sigma [4] descending, ric, converged) from the list of 4x4 blocks"""
    A = np.concatenate([np.asarray(b, dtype) for b in blocks], 0)
    if route == 'svd':
        _, s, vt = np.linalg.svd(A.astype(np.float64))
        sigma, x, conv = s.astype(dtype), vt[3].astype(dtype), True
    else:
        s2, V, conv = jacobi4(A)
        order = sorted(range(4), key=lambda c: -s2[c])
        sigma, x = np.sqrt(s2[order]), V[:, order[3]]
    return sigma, inv3(R_from_q(x)), conv


def calib_step(prev_records, ric_prev, Rc, dq, dtype, route, huber_deg=HUBER_DEG):
    """one call of CalibrationExRotation after solveRelativeR: dict(Rimu, Rcg, huber, ang, angs, sigma, ric, conv)"""
    dt = dtype
    dq = np.asarray(dq, dt)
    Rimu = R_from_q(np.array([dq[1], dq[2], dq[3], dq[0]], dt))
    ric_prev = np.asarray(ric_prev, dt)
    Rcg = (inv3(ric_prev) @ Rimu) @ ric_prev
    blocks, angs = [], []
    for r in prev_records:
        r = np.asarray(r, dt).reshape(3, 3, 3)
        b, _, a = block(r[0], r[1], r[2], dt, huber_deg)
        blocks.append(b)
        angs.append(float(a))
    b, huber, ang = block(Rc, Rimu, Rcg, dt, huber_deg)
    blocks.append(b)
    angs.append(float(ang))
    sigma, ric, conv = solve_A(blocks, dt, route)
    return dict(Rimu=Rimu, Rcg=Rcg, huber=huber, ang=float(ang), angs=angs, sigma=sigma, ric=ric, conv=conv)


# --------------------------------------------------------------------------------------------------- the rotation stage
def rotation(Fm, ll, rr, dtype=LD, route='jacobi'):
    """solveRelativeR after findFundamentalMat: dict(front [4], picked, Rc, conv, zmin)"""
    R1, R2, t, conv = RP.decompose(Fm, dtype, route)
    front, zmin = [], np.inf
    n = len(ll)
    with np.errstate(all='ignore'):
        for Rm, tt in ((R1, t), (R1, -t), (R2, t), (R2, -t)):
            Rf, tf = np.asarray(Rm, dtype).astype(F32).astype(dtype), np.asarray(tt, dtype).astype(F32).astype(dtype)
            q = RP._triangulate(Rf, tf, ll, rr, dtype, route).astype(F32)
            inv = (1.0 / q[:, 3].astype(np.float64)).astype(F32)
            a = (q * inv[:, None]).astype(F32)
            a64, R64, t64 = a.astype(np.float64), Rf.astype(np.float64), tf.astype(np.float64)
            zl = (0.0 * a64[:, 0] + 0.0 * a64[:, 1] + 1.0 * a64[:, 2] + 0.0 * a64[:, 3]).astype(F32)
            zr = (R64[2, 0] * a64[:, 0] + R64[2, 1] * a64[:, 1] + R64[2, 2] * a64[:, 2] + t64[2] * a64[:, 3]).astype(F32)
            front.append(int(np.count_nonzero((zl > 0) & (zr > 0))))
            fin = np.isfinite(zl) & np.isfinite(zr)
            if fin.any():
                zmin = min(zmin, float(np.abs(zl[fin]).min()), float(np.abs(zr[fin]).min()))
    r11, r12, r21, r22 = (f / n for f in front)
    first = max(r11, r12) > max(r21, r22)
    Rp = np.asarray(R1 if first else R2, dtype)
    return dict(front=front, picked=1 if first else 2, Rc=Rp.T.copy(), conv=conv, zmin=zmin, tie=max(front[0], front[1]) == max(front[2], front[3]))


def fundamental(ll, rr, with_replay=True, thresh=THRESH):
    """dict(branch, F, ransac_inliers, ransac_iter / best / bound, used_fallback, model) of findFundamentalMat(ll, rr)"""
    n = len(ll)
    out = dict(branch=0 if n < MIN_POINTS else (1 if n < 15 else 2), F=np.zeros((3, 3)), ransac_inliers=0, ransac_iter=0, ransac_best=0, ransac_bound=0,
               used_fallback=0, model=False)
    if out['branch'] == 0:
        return out
    st, Fm = fe_cpu.reject_with_f(ll, rr, thresh)
    out.update(F=Fm, model=bool(np.any(Fm != 0)))
    if out['branch'] == 2:
        out['used_fallback'] = int(RP.schedule_needs_fallback(ll, rr))
        if out['model']:
            out['ransac_inliers'] = int(st.sum())
            if with_replay:
                best, bound, cnt, _, last = RP.ransac_replay(ll, rr, thresh)
                assert cnt == out['ransac_inliers']
                out.update(ransac_iter=last, ransac_best=best, ransac_bound=bound)
        else:
            out.update(ransac_iter=-1, ransac_best=-1)       # the exact schedule is empty: no iteration was looked at
    return out


def points(step):
    c = np.asarray(step, np.float64).reshape(-1, 4)
    return c[:, :2].astype(F32), c[:, 2:].astype(F32)


# --------------------------------------------------------------------------------------------------- a whole run, one route (def test)
def run(win, dtype=np.float64, route='jacobi', with_replay=False):
    """the run of a window as ONE chain in one route: dict(status, first_ok, calib_ric, steps [S])"""
    recs = [np.asarray(r, np.float64).reshape(27) for r in np.asarray(win.get('prev', np.zeros((0, 27)))).reshape(-1, 27)]
    ric = np.asarray(win.get('ric_prev', np.eye(3)), dtype)
    n_prev, steps, status, first_ok, calib = len(recs), [], OK, -1, np.zeros((3, 3))
    for k, (cr, dq) in enumerate(zip(win['corr'], np.asarray(win['delta_q']).reshape(-1, 4))):
        ll, rr = points(cr)
        f = fundamental(ll, rr, with_replay, win.get('ransac_threshold', THRESH))
        if f['branch'] == 0:
            rot = dict(front=[0] * 4, picked=0, Rc=np.eye(3, dtype=dtype), conv=True, zmin=np.inf, tie=False)
        elif not f['model']:
            rot = dict(front=[0] * 4, picked=0, Rc=np.eye(3, dtype=dtype), conv=False, zmin=np.inf, tie=False)
        else:
            rot = rotation(f['F'], ll, rr, dtype, route)
        c = calib_step(recs, ric, rot['Rc'], dq, dtype, route, win.get('huber_deg', HUBER_DEG))
        m = n_prev + k + 1
        ok = m >= win.get('min_frames', MIN_FRAMES) and c['sigma'][2] > COV
        if not (rot['conv'] and c['conv']):
            status = NUMERIC
        if ok and first_ok < 0:
            first_ok, calib = m, np.asarray(c['ric'], np.float64)
        recs.append(np.concatenate([np.asarray(rot['Rc'], np.float64).reshape(9), np.asarray(c['Rimu'], np.float64).reshape(9), np.asarray(c['Rcg'], np.float64).reshape(9)]))
        ric = c['ric']
        steps.append({**f, **rot, **c, 'conv': bool(rot['conv'] and c['conv']), 'ok': int(ok), 'n': len(ll), 'record': recs[-1]})
    if status != OK:
        first_ok, calib = -1, np.zeros((3, 3))
    return dict(status=status, first_ok=first_ok, calib_ric=calib, steps=steps)


# --------------------------------------------------------------------------------------------------- the scenes
def _rot(v):
    return RP._rot(np.asarray(v, np.float64))


def _quat(Rm):
    q = q_from_R(np.asarray(Rm, np.float64))
    q = q / np.linalg.norm(q)
    return np.array([q[3], q[0], q[1], q[2]])


def scene(seed, counts, ric_deg=(0.0, 0.0, 0.0), rot_deg=12.0, axis=None, noise=NOISE_PX, still=(), collinear=None):
    """The window dict of ba.Handle.init_exrot: len(counts) steps with that many correspondences each.  ric_deg: the true camera-to-IMU
    rotation as a rotation vector in degrees; rot_deg: the inter-frame rotation angle (0.8 .. 1.2 of it), about `axis` or a random axis;
    still: the steps without rotation (pure translation); collinear: (step, iteration): the last point of that sample of the step's
    n-only schedule is put on the line of its first two, on a grid float32 holds exactly.  truth: ric, and the camera rotation per step."""
    rng = np.random.default_rng(seed)
    ric = _rot(np.radians(ric_deg))
    corr, dqs, Rcs = [], [], []
    for k, n in enumerate(counts):
        ax = rng.normal(size=3) if axis is None else np.asarray(axis, float)
        ang = 0.0 if k in still else math.radians(rot_deg) * rng.uniform(0.8, 1.2)
        Rimu = _rot(ax / np.linalg.norm(ax) * ang)
        Rc = ric.T @ Rimu @ ric                                   # camera k in the coordinates of camera k-1
        t = rng.normal(size=3)
        t = t / np.linalg.norm(t) * rng.uniform(0.12, 0.2)
        z = rng.uniform(4.0, 8.0, n)
        X = np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1)
        X1 = (X - t) @ Rc                                         # Rc^T (X - t), row-wise
        rows = np.concatenate([X[:, :2] / X[:, 2:], X1[:, :2] / X1[:, 2:]], 1) + rng.normal(0, noise, (n, 4)) * PX
        if collinear is not None and collinear[0] == k:
            idx = RP.n_only_schedule(n, collinear[1] + 1)[collinear[1]]
            g = 4096.0
            ia, ib, ic = idx[0], idx[1], idx[6]
            rows[ia, :2] = np.round(rows[ia, :2] * g) / g
            rows[ib, :2] = np.round(rows[ib, :2] * g) / g
            rows[ic, :2] = 2 * rows[ib, :2] - rows[ia, :2]
        corr.append(rows)
        dqs.append(_quat(Rimu))
        Rcs.append(Rc)
    return dict(corr=corr, delta_q=np.array(dqs), truth=dict(ric=ric, Rc=Rcs))


# name -> scene arguments (the issue's list; the comment names what the case is about)
CASE_ARGS = {
    'S1': dict(seed=1, counts=[150]),                                                        # one step from the constructor's state
    'sizes': dict(seed=2, counts=[0, 8, 9, 14, 15, 64, 65, 40, 40], rot_deg=4.0),             # identity | LMedS ends | RANSAC minimum | one pass, one more
    'success10': dict(seed=3, counts=[60] * 12, rot_deg=25.0),                                # sigma[2] > 0.25 at step 9 already, ok from step 10
    'never': dict(seed=4, counts=[40] * 12, axis=(0.0, 0.0, 1.0)),                            # one axis: sigma[2] stays under 0.25
    'ric90': dict(seed=5, counts=[60] * 12, ric_deg=(0.0, 0.0, 90.0), rot_deg=10.0),          # the Huber branch at the early steps
    'still': dict(seed=6, counts=[50] * 4, still=(2,)),                                       # a pure-translation step
    'full64': dict(seed=7, counts=[16] * 64, rot_deg=6.0),                                    # n_prev + S = 64: every lane holds a record
    'collinear': dict(seed=8, counts=[48, 48], collinear=(1, 0)),                             # the exact schedule from the host
}
SPLIT_CASE = 'success10'


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(**CASE_ARGS[name])


@functools.lru_cache(maxsize=None)
def capacity_scene():
    """two steps, the second at VG_SFM_MAX_FEATURES correspondences: 16 ballot words"""
    return scene(20, [40, 1024])


@functools.lru_cache(maxsize=None)
def numeric_scene():
    """a second step whose 15 correspondences coincide: every sample is redrawn until the attempts run out, no model"""
    w = scene(21, [40, 15, 40])
    w = dict(w, corr=[w['corr'][0], np.zeros((15, 4)), w['corr'][2]])
    return w


# --------------------------------------------------------------------------------------------------- the metric and the device checks
# one body for the emulator and the MI355X; h: a ba.Handle.  `as_device(run(...))` stands in for the device in the def test.
INT_TAPS = ('ok', 'branch', 'ransac_iter', 'ransac_bound', 'ransac_inliers', 'ransac_best', 'front', 'picked', 'used_fallback')
TAPS = ('records', 'ric', 'sigma', 'huber', 'F') + INT_TAPS


def as_device(r):
    """a result of run() in the shape of Handle.init_exrot"""
    s = r['steps']
    g = dict(status=r['status'], first_ok=r['first_ok'], calib_ric=np.asarray(r['calib_ric'], np.float64))
    g['records'] = np.array([x['record'] for x in s])
    g['ric'] = np.array([np.asarray(x['ric'], np.float64) for x in s])
    g['sigma'] = np.array([np.asarray(x['sigma'], np.float64) for x in s])
    g['huber'] = np.array([float(x['huber']) for x in s])
    g['F'] = np.array([np.asarray(x['F'], np.float64).reshape(3, 3) for x in s])
    for k in INT_TAPS:
        g[k] = np.array([x[k] for x in s])
    return g


def same_output(a, b):
    """two results of Handle.init_exrot, bit for bit"""
    return (a['status'] == b['status'] and a['first_ok'] == b['first_ok'] and np.array_equal(a['calib_ric'], b['calib_ric']) and
            all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in TAPS))


def _err(got, ld):
    return float(np.abs(np.asarray(got, LD) - np.asarray(ld, LD)).max())


def check_window(name, win, g, tag, with_replay=True, quiet=False):
    """one window's result against the reference, step by step from the device's own taps; returns the worst value ratio and asserts the
    conditions of the module docstring on the way"""
    recs = [np.asarray(r, np.float64).reshape(27) for r in np.asarray(win.get('prev', np.zeros((0, 27)))).reshape(-1, 27)]
    ric_prev = np.asarray(win.get('ric_prev', np.eye(3)), np.float64)
    n_prev, worst, status, first_ok, calib = len(recs), (0.0, None), OK, -1, np.zeros((3, 3))
    hd = win.get('huber_deg', HUBER_DEG)
    dqs = np.asarray(win['delta_q']).reshape(-1, 4)
    for k, cr in enumerate(win['corr']):
        ll, rr = points(cr)
        f = fundamental(ll, rr, with_replay, win.get('ransac_threshold', THRESH))
        for key in ('branch', 'used_fallback', 'ransac_inliers') + (('ransac_iter', 'ransac_best', 'ransac_bound') if with_replay else ()):
            assert g[key][k] == f[key], (name, k, key, g[key][k], f[key])
        Fd = np.asarray(g['F'][k], np.float64)
        Rc_dev = g['records'][k][:9].reshape(3, 3)
        if f['branch'] == 0 or not f['model']:
            assert not Fd.any() and np.array_equal(Rc_dev, np.eye(3)) and not np.asarray(g['front'][k]).any() and g['picked'][k] == 0, (name, k)
            if f['branch'] != 0:
                status = NUMERIC
        else:
            assert np.abs(Fd - f['F']).max() <= 1e-6 * np.abs(f['F']).max(), (name, k, np.abs(Fd - f['F']).max())
            ld = rotation(Fd, ll, rr, LD, 'jacobi')
            assert ld['conv'] and not ld['tie'] and ld['zmin'] > 1e-4, (name, k, ld['front'], ld['zmin'])
            assert list(g['front'][k]) == ld['front'] and g['picked'][k] == ld['picked'], (name, k, list(g['front'][k]), ld['front'], g['picked'][k], ld['picked'])
            e64 = 0.0
            for route in ('jacobi', 'svd'):
                r = rotation(Fd, ll, rr, np.float64, route)
                assert sorted(r['front']) == sorted(ld['front']) and not r['tie'], (name, k, route, r['front'], ld['front'])
                e64 = max(e64, _err(r['Rc'], ld['Rc']))
            assert e64 <= RP.E64_CEILING, (name, k, e64)
            ratio = _err(Rc_dev, ld['Rc']) / max(e64, E64_FLOOR)
            assert ratio <= M, (name, k, 'Rc', ratio)
            worst = max(worst, (ratio, f'Rc step {k}'))
        # the calibration step of every route from the device's state before it and the device's Rc
        ld = calib_step(recs, ric_prev, Rc_dev, dqs[k], LD, 'jacobi', hd)
        r64 = [calib_step(recs, ric_prev, Rc_dev, dqs[k], np.float64, route, hd) for route in ('jacobi', 'svd')]
        assert ld['conv'] and r64[0]['conv'], (name, k)
        assert all(abs(a - hd) > 1e-6 for a in ld['angs']), (name, k, 'an angular distance at huber_deg')
        assert abs(float(ld['sigma'][2]) - COV) > 1e-6, (name, k, 'sigma[2] at the threshold')
        m = n_prev + k + 1
        ok = int(m >= win.get('min_frames', MIN_FRAMES) and ld['sigma'][2] > COV)
        assert all(int(m >= win.get('min_frames', MIN_FRAMES) and r['sigma'][2] > COV) == ok for r in r64), (name, k)
        assert g['ok'][k] == ok, (name, k, g['ok'][k], ok, float(ld['sigma'][2]))
        if ok and first_ok < 0:
            first_ok, calib = m, g['ric'][k]
        got = dict(Rimu=g['records'][k][9:18].reshape(3, 3), Rcg=g['records'][k][18:].reshape(3, 3), huber=g['huber'][k], sigma=g['sigma'][k], ric=g['ric'][k])
        for key, scale in (('Rimu', 1.0), ('Rcg', 1.0), ('huber', 1.0), ('sigma', max(1.0, float(ld['sigma'][0]))), ('ric', 1.0)):
            e64 = max(_err(r[key], ld[key]) for r in r64)
            ratio = _err(got[key], ld[key]) / max(e64, E64_FLOOR * scale)
            assert ratio <= M, (name, k, key, ratio, e64)
            worst = max(worst, (ratio, f'{key} step {k}'))
        assert np.all(np.diff(g['sigma'][k]) <= 0), (name, k, 'sigma descends')
        recs.append(np.asarray(g['records'][k], np.float64))
        ric_prev = np.asarray(g['ric'][k], np.float64)
    if status != OK:
        first_ok, calib = -1, np.zeros((3, 3))
    assert (g['status'], g['first_ok']) == (status, first_ok), (name, g['status'], g['first_ok'], status, first_ok)
    assert np.array_equal(g['calib_ric'], calib), name
    if not quiet:
        print(f"init_exrot {tag} {name}: status {g['status']} first_ok {g['first_ok']}  worst ratio {worst[0]:.2f} ({worst[1]})")
    return worst[0]


def check_case_properties(g):
    """what each case is about, on results keyed by case name"""
    if 'S1' in g:
        assert g['S1']['first_ok'] == -1 and list(g['S1']['branch']) == [2]
    if 'sizes' in g:
        assert list(g['sizes']['branch']) == [0, 0, 1, 1, 2, 2, 2, 2, 2]
    if 'success10' in g:
        s = g['success10']
        assert s['first_ok'] == MIN_FRAMES and s['sigma'][8][2] > COV and s['ok'][8] == 0 and s['ok'][9] == 1, (s['first_ok'], s['sigma'][:, 2])
    if 'never' in g:
        assert g['never']['first_ok'] == -1 and g['never']['status'] == OK and np.all(g['never']['sigma'][:, 2] < COV)
    if 'ric90' in g:
        assert np.all(g['ric90']['huber'][:2] < 1.0), g['ric90']['huber']
    if 'still' in g:
        assert g['still']['status'] == OK
    if 'full64' in g:
        assert len(g['full64']['ok']) == 64 and g['full64']['status'] == OK
    if 'collinear' in g:
        assert list(g['collinear']['used_fallback']) == [0, 1]
    # (a redrawn sample is not rare on normalised coordinates: about one step in ten of these scenes has one by itself, 'ric90' among them)
    for k, v in g.items():
        # with normalised coordinates at threshold 3 the first sample's model takes every point: iteration 0, bound 0
        r = np.asarray(v['branch']) == 2
        assert np.all(np.asarray(v['ransac_best'])[r] == 0) and np.all(np.asarray(v['ransac_bound'])[r] == 0), k


def check_cases(h, tag, names=None):
    """the cases in ONE call"""
    names = list(names or CASE_ARGS)
    got = dict(zip(names, h.init_exrot([case(n) for n in names])))
    worst = max((check_window(n, case(n), got[n], tag), n) for n in names)
    print(f"init_exrot {tag}: worst ratio {worst[0]:.3f} ({worst[1]}; bound {M})")
    check_case_properties(got)
    return got


def resume(win, res, lo, hi):
    """the window of steps [lo, hi) carrying the state the results `res` of the steps before left (a list of result dicts in order)"""
    recs = np.concatenate([np.asarray(win.get('prev', np.zeros((0, 27)))).reshape(-1, 27)] + [r['records'] for r in res]) if res else \
        np.asarray(win.get('prev', np.zeros((0, 27)))).reshape(-1, 27)
    w = dict(win, corr=win['corr'][lo:hi], delta_q=np.asarray(win['delta_q'])[lo:hi], prev=recs)
    if res:
        w['ric_prev'] = res[-1]['ric'][-1]
    return w


def check_split(h):
    """a run of 12 steps split at 1, at 9|10 and at 11 against the unsplit run, to bit patterns"""
    win = case(SPLIT_CASE)
    S = len(win['corr'])
    whole = h.init_exrot([win])[0]
    assert S == 12 and whole['first_ok'] == MIN_FRAMES
    for cut in (1, 9, 11):
        a = h.init_exrot([resume(win, [], 0, cut)])[0]
        b = h.init_exrot([resume(win, [a], cut, S)])[0]
        for k in TAPS:
            assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), (cut, k)
        first = a['first_ok'] if a['first_ok'] >= 0 else b['first_ok']
        assert first == whole['first_ok'] and np.array_equal((a if a['first_ok'] >= 0 else b)['calib_ric'], whole['calib_ric']), cut
    # one step per call, as a per-frame caller feeds it
    res = []
    for k in range(S):
        res.append(h.init_exrot([resume(win, res, k, k + 1)])[0])
    for k in TAPS:
        assert np.array_equal(np.concatenate([r[k] for r in res]), whole[k]), k
    assert [r['first_ok'] for r in res][MIN_FRAMES - 1] == MIN_FRAMES


def batch(n, seed=700):
    """n small windows of mixed S and statuses for the batch-equals-single checks"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 8 == 3:
            out.append(numeric_scene())
            continue
        S = int(rng.choice([1, 2, 3]))
        out.append(scene(seed + i, [int(rng.choice([0, 9, 12, 20, 30, 70])) for _ in range(S)]))
    return out


def check_batch_equals_single(h, sizes=(1, 3, 33)):
    wins = batch(max(sizes))
    single = [h.init_exrot([w])[0] for w in wins]
    assert {s['status'] for s in single} == {OK, NUMERIC}, "the batch mixes statuses"
    assert len({len(w['corr']) for w in wins}) >= 3, "the batch mixes S"
    for n in sizes:
        for k, g in enumerate(h.init_exrot(wins[:n])):
            assert same_output(g, single[k]), (n, k)


def check_numeric_neighbours(h):
    """a window that ends with VG_EXROT_NUMERIC between two good ones: they are what they are alone"""
    wins = [case('S1'), numeric_scene(), case('still')]
    alone = [h.init_exrot([w])[0] for w in wins]
    together = h.init_exrot(wins)
    assert [a['status'] for a in alone] == [OK, NUMERIC, OK]
    for a, b in zip(alone, together):
        assert same_output(a, b)
    t = together[1]
    assert t['first_ok'] == -1 and not t['calib_ric'].any() and list(t['branch']) == [2, 2, 2] and t['used_fallback'][1] == 1
    check_window('numeric', wins[1], t, 'numeric', quiet=True)


def check_growing_table(h_new):
    """a call at 40 correspondences followed by one at 300 on the same (fresh) handle: the resident tables grow, both calls are what a
    handle that saw the large call first returns"""
    small, large = scene(31, [40, 40]), scene(32, [300])
    a1 = h_new.init_exrot([small])[0]
    b1 = h_new.init_exrot([large])[0]
    a2 = h_new.init_exrot([small])[0]
    assert same_output(a1, a2)
    check_window('grow_small', small, a1, 'grow')
    check_window('grow_large', large, b1, 'grow')


def check_capacity(h, tag):
    win = capacity_scene()
    g = h.init_exrot([win])[0]
    assert list(g['ransac_inliers']) == [40, 1024] and g['status'] == OK
    worst = check_window('capacity', win, g, tag)
    print(f"init_exrot {tag} capacity: worst ratio {worst:.2f}")
    return worst


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
         'S_0': field('in', 'n_steps', 0), 'n_prev_negative': field('in', 'n_prev', -1), 'steps_above': field('in', 'n_prev', 63),
         'corr_off_descends': arr('corr_off', 1, 60), 'corr_off_negative': arr('corr_off', 0, -1), 'step_above_1024': arr('corr_off', 2, 24 + 1025),
         'corr_nan': arr('corr', 4 * 11 + 1, nan), 'corr_inf': arr('corr', 4 * 30 + 2, float('inf')), 'delta_q_nan': arr('delta_q', 5, nan),
         'delta_q_zero': setter(lambda ins, outs, keep: keep[1]['delta_q'].__setitem__(0, 0.0)), 'ric_prev_nan': arr('ric_prev', 4, nan),
         'prev_inf': arr('prev', 30, float('inf')),
         'threshold_0': field('in', 'ransac_threshold', 0.0), 'threshold_negative': field('in', 'ransac_threshold', -3.0), 'threshold_nan': field('in', 'ransac_threshold', nan),
         'confidence_0999': field('in', 'confidence', 0.999), 'huber_0': field('in', 'huber_deg', 0.0), 'cov_negative': field('in', 'cov_threshold', -0.25),
         'min_points_8': field('in', 'min_points', 8)}
    for t in ('corr_off', 'corr', 'delta_q', 'prev', 'ric_prev'):
        r['null_' + t] = null(t)
    return r


REFUSALS = tuple(_refusals())
_REFUSAL_GOOD = {}


@functools.lru_cache(maxsize=None)
def _refusal_windows():
    """two windows of two steps (24 correspondences each) that resume a run of two records"""
    out = []
    for k in range(2):
        w = scene(41 + k, [24, 24, 24, 24])
        r = run(w)
        out.append(dict(corr=w['corr'][2:], delta_q=w['delta_q'][2:], prev=np.array([s['record'] for s in r['steps'][:2]]), ric_prev=np.asarray(r['steps'][1]['ric'])))
    return out


def check_refusal(h, name):
    """the spoiled call returns VG_ERR_BAD_ARG with a message, writes nothing, and the handle goes on working"""
    wins = _refusal_windows()
    if id(h) not in _REFUSAL_GOOD:
        _REFUSAL_GOOD[id(h)] = h.init_exrot(wins)
    good = _REFUSAL_GOOD[id(h)]
    ins, outs, keep = h.init_exrot_pack(wins)
    for o, b in zip(outs, keep):
        o.status, o.first_ok = 77, 55
        o.calib_ric[0] = 3.25
        for k in TAPS:
            b[k][...] = 9
    n = _refusals()[name](ins, outs, keep)
    rc = h.lib.vg_init_exrot(h.h, n, ins, outs)
    assert rc == -1, (name, rc)                              # VG_ERR_BAD_ARG
    assert b"vg_init_exrot" in h.lib.vg_last_error(h.h), name
    for o, b in zip(outs, keep):
        assert (o.status, o.first_ok, o.calib_ric[0]) == (77, 55, 3.25), name
        assert all(np.all(b[k] == 9) for k in TAPS), name
    assert same_output(good[1], h.init_exrot(wins[1:])[0]), name


def check_stream_limit(h, run_limit=False):
    """more than VG_RELPOSE_MAX_STREAMS (window, step) pairs in one call: refused, nothing written, the handle goes on"""
    w = dict(corr=[np.zeros((0, 4))] * 64, delta_q=np.tile([1.0, 0, 0, 0], (64, 1)))
    few = h.init_exrot([case('S1')])[0]
    wins = [w] * 65                                             # 4160 streams
    ins, outs, keep = h.init_exrot_pack(wins)
    for o in outs:
        o.status, o.first_ok = 77, 55
    rc = h.lib.vg_init_exrot(h.h, len(wins), ins, outs)
    assert rc == -1 and b"VG_RELPOSE_MAX_STREAMS" in h.lib.vg_last_error(h.h), rc
    assert all((o.status, o.first_ok) == (77, 55) for o in outs)
    if run_limit:                                               # exactly the limit runs
        assert h.lib.vg_init_exrot(h.h, 64, ins, outs) == 0
        assert all((o.status, o.first_ok) == (OK, -1) for o in list(outs)[:64]) and (outs[64].status, outs[64].first_ok) == (77, 55)
    assert same_output(few, h.init_exrot([case('S1')])[0])


# --------------------------------------------------------------------------------------------------- the chain into the rest
@functools.lru_cache(maxsize=None)
def chain_scene():
    """(the window of vg_init_relpose / vg_init_sfm, the window of vg_init_align, the window of vg_init_exrot over the same frames): the
    IMU scene of tests/init_align_ref.py at F = 16 frames 0.175 s apart (a seed whose rotation carries sigma[2] over 0.25 by step 10 and whose views the SfM stage accepts), its cameras (body rotation times the scene's ric) looking at
    noise-free landmarks as in tests/init_sfm_ref.chain_scene; the exrot steps are the correspondences of consecutive frames and the
    scene's own body rotation increments (an ideal gyro)"""
    import init_sfm_ref as S
    A = S.A
    F = 16
    al = A.scene(5, F=F, spi=35, key='all')
    ric = A._small_rotation(np.array([0.1, -0.2, 0.15]))
    win = S.scene(21, F=F, l=F // 2, n_feat=120, noise=0.0, poses=([Rb @ ric for Rb in al['R']], list(al['T']), None))
    start, nobs = np.asarray(win['start']), np.asarray(win['nobs'])
    off = np.concatenate([[0], np.cumsum(nobs)[:-1]])
    pts = np.asarray(win['points'], np.float64).reshape(-1, 3)
    corr, dqs = [], []
    for i in range(F - 1):
        rows = [np.concatenate([pts[off[j] + i - start[j], :2], pts[off[j] + i + 1 - start[j], :2]]) for j in range(len(start))
                if start[j] <= i and start[j] + nobs[j] - 1 >= i + 1]
        corr.append(np.array(rows).reshape(-1, 4))
        dqs.append(_quat(al['R'][i].T @ al['R'][i + 1]))
    return win, al, dict(corr=corr, delta_q=np.array(dqs), truth=dict(ric=ric))


CHAIN_THRESHOLD = RP.THRESH     # 0.3 / 460: the threshold solveRelativeRT gives findFundamentalMat, in the units of the points
# What the REFERENCE may be off by on the chain scene at that threshold: the points are exact but for their float32 rounding (2^-24 of
# coordinates below 0.5: 3e-8), a seven-point model turns a point error into a rotation error of about depth / baseline (6 / 0.1 = 60)
# times it (2e-6 rad), and ric sees a record's error over the record's own rotation angle (0.1 rad): 2e-5 rad = 1e-3 degrees; ten times
# that is allowed.  (Measured: 3.3e-5 degrees.)
CHAIN_RIC_DEG = 1e-2


@functools.lru_cache(maxsize=None)
def chain_window():
    """the exrot window of chain_scene() as the chain runs it: ransac_threshold = CHAIN_THRESHOLD.

    At the DEFAULT threshold (3.0, cv::findFundamentalMat's, on normalised coordinates) the reference's own calibration of this
    noise-free scene succeeds at step 10 with calib_ric 6.26 degrees from the scene's ric, and the alignment behind it finds the scale to
    9.4e-3, not 1e-3: every root of the first sample's cubic takes all points, and on about half of the steps of a rendered window (240
    scenes counted) the tie goes to a spurious root, whose Rc is degrees off.  That is a property of the definition the header keeps,
    not of the device, which equals the reference on every step there too; no rendered window was found on which ten steps in a row
    take the true root.  The threshold is a field of vg_exrot_in; in the units of the points the RANSAC separates the roots, and what
    the chain checks -- calib_ric in the layout and convention vg_init_sfm takes, the scale and gravity behind it -- can be checked."""
    return dict(chain_scene()[2], ransac_threshold=CHAIN_THRESHOLD)


def _angle_deg(d):
    return float(np.degrees(np.arccos(max(-1.0, min(1.0, (np.trace(d) - 1) / 2)))))


def check_chain(h):
    """vg_init_exrot -> calib_ric as ric of vg_init_sfm (behind vg_init_relpose) -> vg_init_align on one rendered window (chain_window()
    says at which threshold and why): the device's run is held like every case of the table, calib_ric is the scene's within
    CHAIN_RIC_DEG, the scale within what check_chain of tests/init_relpose_ref.py accepts (init_sfm_ref.SCALE_BOUND) and gravity's norm within
    the same figure of the scene's (its direction is in the frame the SfM chose and is not compared, as in that check)"""
    import init_sfm_ref as S
    A = S.A
    win, al, _ = chain_scene()
    ex = chain_window()
    g = h.init_exrot([ex])[0]
    check_window('chain', ex, g, 'chain')
    err_ric = _angle_deg(g['calib_ric'] @ ex['truth']['ric'].T)
    print(f"init_exrot chain: status {g['status']} first_ok {g['first_ok']}  calib_ric {err_ric:.2e} degrees from the scene's")
    assert g['status'] == OK and g['first_ok'] == MIN_FRAMES and err_ric <= CHAIN_RIC_DEG
    rp = h.init_relpose([win])[0]
    assert rp['status'] == RP.OK
    sf = h.init_sfm([dict(win, ric=g['calib_ric'], l=rp['l'], relative_R=rp['relative_R'], relative_T=rp['relative_T'])])[0]
    assert sf['status'] == S.OK, sf['status']
    res = h.init_align([dict(al, R=sf['R_all'], T=sf['T_all'])])[0]
    base_l = np.linalg.norm(win['truth']['cam'][-1][1] - win['truth']['cam'][rp['l']][1]) * win['truth']['base']
    s_here = al['truth']['s'] * base_l
    err = abs(res['s'] - s_here) / s_here
    g_dev = np.asarray(res['g_c0'], np.float64)
    gnorm_err = abs(np.linalg.norm(g_dev) - np.linalg.norm(al['truth']['g'])) / np.linalg.norm(al['truth']['g'])
    print(f"init_exrot chain: l {rp['l']}  align status {res['status']}  scale {res['s']:.9g} (scene {s_here:.9g}, relative error {err:.1e})  |g| relative error {gnorm_err:.1e}")
    assert res['status'] == A.OK and err < S.SCALE_BOUND and gnorm_err < S.SCALE_BOUND
    # the same chain at the DEFAULT threshold, the configuration estimator.cpp runs: no bound can be met there (chain_window() says why);
    # what it gives is RECORDED, to the digits below, so that a change is noticed: first_ok 10, calib_ric 6.262 degrees from the scene's,
    # the scale 1.75663769 against the scene's 1.77323176 (relative error 9.36e-3)
    ex3 = chain_scene()[2]
    g3 = h.init_exrot([ex3])[0]
    check_window('chain_default', ex3, g3, 'chain', quiet=True)
    err3 = _angle_deg(g3['calib_ric'] @ ex3['truth']['ric'].T)
    sf3 = h.init_sfm([dict(win, ric=g3['calib_ric'], l=rp['l'], relative_R=rp['relative_R'], relative_T=rp['relative_T'])])[0]
    res3 = h.init_align([dict(al, R=sf3['R_all'], T=sf3['T_all'])])[0]
    rel3 = abs(res3['s'] - s_here) / s_here
    print(f"init_exrot chain at the default threshold (recorded, not bounded): first_ok {g3['first_ok']}  calib_ric {err3:.3f} degrees  scale {res3['s']:.9g} (relative error {rel3:.2e})")
    assert g3['status'] == OK and g3['first_ok'] == MIN_FRAMES and abs(err3 - 6.262) < 5e-3
    assert sf3['status'] == S.OK and res3['status'] == A.OK and abs(rel3 - 9.36e-3) < 5e-5


def check_separating(h):
    """the noisy scenes 'success10' and 'ric90' at the separating threshold 0.3 / 460, where the RANSAC runs for several iterations: held
    like every case of the table, and calib_ric within the bound of tests/test_init_exrot_def.py's perturbation argument, evaluated on the
    device's own records, Huber weights and sigma[2]"""
    wins = [dict(case(n), ransac_threshold=CHAIN_THRESHOLD) for n in ('success10', 'ric90')]
    for name, win, g in zip(('success10', 'ric90'), wins, h.init_exrot(wins)):
        check_window(name + '_separating', win, g, 'separating')
        m = g['first_ok']
        assert g['status'] == OK and m == MIN_FRAMES and np.asarray(g['ransac_iter']).max() >= 5, (name, m, g['ransac_iter'])
        delta = np.array([_angle_deg(g['records'][k][:9].reshape(3, 3) @ win['truth']['Rc'][k].T) for k in range(m)])
        arg = np.sqrt(np.sum(np.radians(g['huber'][:m] * delta) ** 2)) / (2 * float(g['sigma'][m - 1][2]))
        bound = float(np.degrees(2 * np.arcsin(min(1.0, arg)))) + 1e-9
        err = _angle_deg(g['calib_ric'] @ win['truth']['ric'].T)
        print(f"init_exrot separating {name}: calib_ric {err:.3f} degrees from the scene's (bound {bound:.3f})")
        assert err <= bound


# --------------------------------------------------------------------------------------------------- the C++ class and the replay tool
REPLAY_CASES = ('success10', 'sizes', 'never')             # a success (the block stops applying) / the small branches / no success


def check_replay(h, exe, tmp_dir, name):
    """Estimator::calibrateExtrinsicRotation / class InitialEXRotation (host/estimator.cpp, vg_pack_exrot) through `vins_replay exrot`,
    one frame per call: number for number the batched binding's, up to the step the reference stops calling at"""
    win = case(name)
    S = len(win['corr'])
    path, out = os.path.join(str(tmp_dir), name + ".bin"), os.path.join(str(tmp_dir), name + ".txt")
    write_file(path, win)
    r = subprocess.run([exe, "exrot", path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in open(out).read().splitlines()]
    g = h.init_exrot([win])[0]
    last = g['first_ok'] if g['first_ok'] >= 0 else S           # steps 1 .. last are made
    steps = [ln for ln in lines if ln[0] == 'step']
    assert [int(x[1]) for x in steps] == list(range(last)) and [int(x[1]) for x in lines if x[0] == 'skipped'] == list(range(last, S)), name
    rics = [np.array([float(v) for v in ln[1:]]) for ln in lines if ln[0] == 'ric']
    sigmas = [np.array([float(v) for v in ln[1:]]) for ln in lines if ln[0] == 'sigma']
    for k in range(last):
        ok = int(k + 1 == g['first_ok'])
        assert [int(v) for v in steps[k][2:]] == [ok, g['status'], 1 if ok else 2], (name, k, steps[k])
        assert np.array_equal(rics[k], g['ric'][k].reshape(-1)) and np.array_equal(sigmas[k], g['sigma'][k]), (name, k)
    calib = np.array([float(v) for v in lines[-1][1:]])
    assert lines[-1][0] == 'calib' and np.array_equal(calib, (g['calib_ric'] if g['first_ok'] >= 0 else np.eye(3)).reshape(-1)), name


def check_replay_cap(h, exe, tmp_dir):
    """70 frames about one axis, which never succeed, through the class: from the 64th invocation on it drops its oldest record (the call
    holds VG_EXROT_MAX_STEPS); every step equals the binding fed one frame at a time with the same rule"""
    win = scene(61, [16] * 70, axis=(0.0, 0.0, 1.0), rot_deg=6.0)
    path, out = os.path.join(str(tmp_dir), "cap.bin"), os.path.join(str(tmp_dir), "cap.txt")
    write_file(path, win)
    r = subprocess.run([exe, "exrot", path, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in open(out).read().splitlines()]
    steps = [ln for ln in lines if ln[0] == 'step']
    rics = [np.array([float(v) for v in ln[1:]]) for ln in lines if ln[0] == 'ric']
    assert len(steps) == 70 and all([int(v) for v in st[2:]] == [0, OK, 2] for st in steps)
    prev, ric = np.zeros((0, 27)), np.eye(3)
    for k in range(70):
        if len(prev) >= 64:
            prev = prev[1:]
        g = h.init_exrot([dict(corr=win['corr'][k:k + 1], delta_q=win['delta_q'][k:k + 1], prev=prev, ric_prev=ric)])[0]
        assert g['status'] == OK and g['first_ok'] == -1, k
        prev, ric = np.concatenate([prev, g['records']]), g['ric'][0]
        assert np.array_equal(rics[k], ric.reshape(-1)), k
    assert len(prev) == 64


# --------------------------------------------------------------------------------------------------- files for the stand-alone programs
def write_file(path, win):
    """VEX1: int32 magic, S, rows; corr_off (S + 1 int32); corr (float64 x0 y0 x1 y1 rows); delta_q (float64 w x y z rows)"""
    steps = [np.asarray(c, np.float64).reshape(-1, 4) for c in win['corr']]
    off = np.concatenate([[0], np.cumsum([len(c) for c in steps])]).astype(np.int32)
    corr = np.concatenate(steps + [np.zeros((0, 4))])
    with open(path, "wb") as f:
        f.write(struct.pack("<3i", 0x31584556, len(steps), len(corr)))
        f.write(off.tobytes()); f.write(np.ascontiguousarray(corr).tobytes()); f.write(np.ascontiguousarray(win['delta_q'], np.float64).tobytes())


@functools.lru_cache(maxsize=None)
def sanitizer_windows():
    """the windows of the stand-alone sanitizer run: the 9-, 15- and 65-point steps, the split run and the capacity step"""
    return (scene(51, [9, 30]), scene(52, [15]), scene(53, [30, 65]), case(SPLIT_CASE), capacity_scene())
