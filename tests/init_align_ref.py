"""Reference, scene generator, case table, metric and edits for vg_init_align (helper module of tests/test_init_align_def.py,
test_init_align_simt.py and test_init_align_gpu.py; no tests in here).

`align(win, dtype, route)` restates VisualIMUAlignment (initial/initial_aligment.cpp:3-207) and the state change of
Estimator::visualInitialAlign (estimator.cpp:376-435) as include/vinsgpu.h describes them, quirks included, over
tests/imu_ref.integrate for the records.  The inputs are the float64 inputs, widened: the reference answers for the numbers the
device got.
    dtype = np.longdouble, route 'ld'     the 80-bit reference (Gaussian elimination with partial pivoting in 80 bits)
    dtype = np.float64,    route 'solve'  numpy.linalg.solve, pairs summed ascending
    dtype = np.float64,    route 'ldlt'   an unpivoted LDL^T, pairs summed descending (another order and another solver: what two
                                          honest float64 implementations differ by)
`edit` (one of EDITS) changes one thing the header documents; each must exceed the device's bound on some noisy case.

The scene (`scene`): an analytic trajectory (sums of sines for the position and for yaw / pitch / roll), IMU samples of it at 200 Hz
with a constant gyro bias, frames every `spi` samples; the SfM poses are the true ones rotated by a random Q, the camera positions
divided by the true scale, optionally with pose noise (a small rotation and a relative position error per frame).  Truth: the scale,
the gyro bias, Q g.

The metric (`errors`): per output group max|d| / max|ref|, divided by kappa 2^-53, kappa = the 2-norm condition number of the
Jacobi-scaled (D^-1/2 A D^-1/2) system of the 80-bit route the group comes from: the 3x3 system for the gyro bias, the
LinearAlignment system for g_lin / s_lin, the system of RefineGravity's last pass for everything after it.  The device may reach
M = imu_ref.M = 4; both float64 routes stay at or below 1 on every case (asserted in tests/test_init_align_def.py).
    The gyro bias is the one group whose scale is not max|ref|.  Its right-hand side is sum J^T 2 vec(delta_q^-1 (x) q_ij): the
    vector part of a product of UNIT quaternions, each rounded to 2^-53 of one, not of the vector part, which is the rotation a bias
    of a few hundredths of a rad/s makes in a tenth of a second, 1e-3.  No float64 evaluation can give delta_bg to kappa 2^-53 of
    itself (kappa is 1.0 here): the two NumPy routes are at 9 .. 120 times that on the table below, 1e-15 .. 1.3e-14 relative.  So
    delta_bg is measured against the bias that a rounding error of one unit in every quaternion component maps to,
    max(|A^-1| sum |J^T| 2), and then like the others; errors(..., literal=True) gives the figure against max|ref|, which the tests
    print beside it.
    g_c0 and what follows from it start from normalised(g_lin) and the older passes dominate the accumulated system, so they
    inherit the error of LinearAlignment: on scenes whose linear system is much worse conditioned than the final one (many
    F = 4 and F = 5 seeds here) the float64 routes exceed 1 in the final system's scale.  Such scenes are not in the table.

Statuses.  The gravity-norm failure is made with a g_norm the scene does not have ('gnorm'), s_lin < 0 with mirrored SfM positions
('mirrored'); s < 0 only after RefineGravity happens on a few F = 4 / 5 scenes with 3 % pose noise, 'F5_refine_fails' is one
(s_lin = 0.25, s = -0.37)."""
import functools

import numpy as np

import imu_ref

LD = np.longdouble
M = imu_ref.M
EPS = 2.0 ** -53
NOISE = imu_ref.NOISE
OK, FAILED_LINEAR, FAILED_REFINE, NUMERIC = 0, 1, 2, 3
EDITS = ('A_cleared_per_pass', 'no_x1000', 'reprop_with_ba0', 'Vs_by_frame_position', 'T_not_divided_by_100', 'tic_dropped', 'yaw_kept')
GROUPS_OF = dict(bias=('delta_bg',), lin=('g_lin', 's_lin'), fin=('g_c0', 's', 'v_body', 'Ps', 'Rs', 'Vs', 'g_w', 'R0'))


# --------------------------------------------------------------------------------------------------- small math, any dtype
def _R2q(m, dtype):
    """Eigen's quaternion from a rotation matrix, [x y z w]"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4, dtype)
    if t > 0:
        t = np.sqrt(t + dtype(1))
        q[3] = dtype(0.5) * t
        t = dtype(0.5) / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + dtype(1))
        q[i] = dtype(0.5) * t
        t = dtype(0.5) / t
        q[3], q[j], q[k] = (m[k, j] - m[j, k]) * t, (m[j, i] + m[i, j]) * t, (m[k, i] + m[i, k]) * t
    return q


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _q2R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _normalized(v):
    return v / np.sqrt((v * v).sum())


def _yaw_deg(R, dtype):
    return np.arctan2(R[1, 0], R[0, 0]) / dtype(np.pi) * dtype(180)


def _Rz_deg(yaw, dtype):
    y = yaw / dtype(180) * dtype(np.pi)
    c, s, o, l = np.cos(y), np.sin(y), dtype(0), dtype(1)
    return np.array([[c, -s, o], [s, c, o], [o, o, l]])


def _solve_pivoted(A, b):
    """Gaussian elimination with partial pivoting in the dtype of A (numpy.linalg has no 80-bit solver), of the Jacobi-scaled
    system where the diagonal allows: the error is then of the order kappa_s 2^-64, kappa_s as in `kappa`"""
    n = len(b)
    d = np.diag(A)
    if np.all(d > 0):
        sc = 1 / np.sqrt(d)
        return sc * _solve_pivoted_plain(A * np.outer(sc, sc), b * sc)
    return _solve_pivoted_plain(A, b)


def _solve_pivoted_plain(A, b):
    A, b = A.copy(), b.copy()
    n = len(b)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if p != j:
            A[[j, p]], b[[j, p]] = A[[p, j]], b[[p, j]]
        f = A[j + 1:, j] / A[j, j]
        A[j + 1:, j:] -= np.outer(f, A[j, j:])
        b[j + 1:] -= f * b[j]
    x = np.zeros_like(b)
    for j in range(n - 1, -1, -1):
        x[j] = (b[j] - A[j, j + 1:] @ x[j + 1:]) / A[j, j]
    return x


def _solve_ldlt(A, b):
    """unpivoted LDL^T; None when a pivot is not a positive finite number"""
    W, n = A.copy(), len(b)
    for j in range(n):
        d = W[j, j]
        if not (d > 0 and np.isfinite(d)):
            return None
        col = W[j + 1:, j] / d
        W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], col)
        W[j + 1:, j] = col
    x = b.copy()
    for j in range(n - 1):
        x[j + 1:] -= W[j + 1:, j] * x[j]
    x /= np.diag(W)
    for j in range(n - 1, 0, -1):
        x[:j] -= W[j, :j] * x[j]
    return x


def _solve(A, b, route):
    if route == 'ld':
        return _solve_pivoted(A, b)
    if route == 'solve':
        return np.linalg.solve(A, b)
    return _solve_ldlt(A, b)


def kappa(A):
    """2-norm condition number of D^-1/2 A D^-1/2"""
    A = np.asarray(A, LD)
    d = np.sqrt(np.diag(A))
    return float(np.linalg.cond((A / np.outer(d, d)).astype(np.float64)))


# --------------------------------------------------------------------------------------------------- the restatement
def _tangent_basis(g0, dtype):
    a = _normalized(g0)
    tmp = np.array([0, 0, 1], dtype)
    if np.array_equal(a, tmp):
        tmp = np.array([1, 0, 0], dtype)
    b = _normalized(tmp - a * (a @ tmp))
    return np.stack([b, np.cross(a, b)], axis=1)


def _accumulate(F, R, T, recs, tic, order, edit, dtype, lxly=None, g0=None, A=None, b=None):
    """tmp_A^T tmp_A / tmp_A^T tmp_b of every pair added to A, b (initial_aligment.cpp:75-113 with lxly, :138-175 without)"""
    ng = 3 if lxly is None else 2
    n = 3 * F + ng + 1
    if A is None:
        A, b = np.zeros((n, n), dtype), np.zeros(n, dtype)
    I3 = np.eye(3, dtype=dtype)
    for i in order:
        Ri, Rj, dt = R[i], R[i + 1], dtype(recs[i]['sum_dt'])
        tA, tb = np.zeros((6, 6 + ng + 1), dtype), np.zeros(6, dtype)
        tA[0:3, 0:3] = -dt * I3
        half = Ri.T * dt * dt / 2
        tA[0:3, 6:6 + ng] = half if lxly is None else half @ lxly
        tA[0:3, 6 + ng] = Ri.T @ (T[i + 1] - T[i]) / (dtype(1) if edit == 'T_not_divided_by_100' else dtype(100))
        tb[0:3] = recs[i]['delta_p'] + (0 if edit == 'tic_dropped' else Ri.T @ Rj @ tic - tic)
        tA[3:6, 0:3] = -I3
        tA[3:6, 3:6] = Ri.T @ Rj
        tA[3:6, 6:6 + ng] = Ri.T * dt if lxly is None else (Ri.T * dt) @ lxly
        tb[3:6] = recs[i]['delta_v']
        if lxly is not None:
            tb[0:3] = tb[0:3] - half @ g0
            tb[3:6] = tb[3:6] - (Ri.T * dt) @ g0
        rA, rb = tA.T @ tA, tA.T @ tb
        A[3 * i:3 * i + 6, 3 * i:3 * i + 6] += rA[:6, :6]
        b[3 * i:3 * i + 6] += rb[:6]
        A[n - ng - 1:, n - ng - 1:] += rA[6:, 6:]
        b[n - ng - 1:] += rb[6:]
        A[3 * i:3 * i + 6, n - ng - 1:] += rA[:6, 6:]
        A[n - ng - 1:, 3 * i:3 * i + 6] += rA[6:, :6]
    return A, b


def align(win, dtype=LD, route='ld', edit=None):
    """One window.  Returns status, the outputs of vg_align_out that the status reaches (the rest absent), and `systems`: the
    matrices of the three solves (bias, lin, fin) for kappa."""
    w = lambda v: np.asarray(v, np.float64).astype(dtype)
    R, T, tic = w(win['R']).reshape(-1, 3, 3), w(win['T']).reshape(-1, 3), w(win['tic'])
    F, g_norm = len(R), dtype(np.float64(win['g_norm']))
    order = range(F - 1) if route != 'ldlt' else range(F - 2, -1, -1)
    out = dict(status=NUMERIC, systems={})
    # ---- solveGyroscopeBias
    recs = [imu_ref.integrate(iv, win['ba0'], win['bg0'], win['noise'], dtype=dtype) for iv in win['intervals']]
    A3, b3, Jabs = np.zeros((3, 3), dtype), np.zeros(3, dtype), np.zeros(3, dtype)
    for i in order:
        q_ij = _R2q(R[i].T @ R[i + 1], dtype)
        dq = recs[i]['delta_q']
        inv = np.array([-dq[0], -dq[1], -dq[2], dq[3]]) / (dq @ dq)
        J = recs[i]['jacobian'][3:6, 12:15]
        A3 += J.T @ J
        b3 += J.T @ (2 * _qmul(inv, q_ij)[:3])
        Jabs += 2 * np.abs(J.T).sum(axis=1)
    out['systems']['bias'] = A3
    if route == 'ld':                                       # |A^-1| sum |J^T| 2: see `errors`
        out['bias_scale'] = float((np.abs(np.stack([_solve(A3, e, route) for e in np.eye(3, dtype=dtype)])) @ Jabs).max())
    dbg = _solve(A3, b3, route)
    if dbg is None or not np.all(np.isfinite(dbg.astype(np.float64))):
        return out
    bg = w(win['bg0']) + dbg
    out.update(delta_bg=dbg, bg=bg)
    ba = w(win['ba0']) if edit == 'reprop_with_ba0' else np.zeros(3, dtype)
    recs = [imu_ref.integrate(iv, ba, bg, win['noise'], dtype=dtype) for iv in win['intervals']]
    out['records'] = recs
    if F < 4:                                               # 6 (F - 1) rows for 3 F + 4 unknowns
        return out
    # ---- LinearAlignment
    n = 3 * F + 4
    A, b = _accumulate(F, R, T, recs, tic, order, edit, dtype)
    if edit != 'no_x1000':
        A, b = A * 1000, b * 1000
    out['systems']['lin'] = A
    x = _solve(A, b, route)
    if x is None or not np.all(np.isfinite(x.astype(np.float64))):
        return out
    g, s = x[n - 4:n - 1], x[n - 1] / 100
    out.update(g_lin=g, s_lin=s)
    if abs(np.sqrt(g @ g) - g_norm) > 1 or s < 0:
        out['status'] = FAILED_LINEAR
        return out
    # ---- RefineGravity: A and b are cleared once, before the four passes
    n = 3 * F + 3
    g0 = _normalized(g) * g_norm
    A = b = None
    for _ in range(4):
        lxly = _tangent_basis(g0, dtype)
        if edit == 'A_cleared_per_pass':
            A = b = None
        A, b = _accumulate(F, R, T, recs, tic, order, edit, dtype, lxly, g0, A, b)
        if edit != 'no_x1000':
            A, b = A * 1000, b * 1000
        x = _solve(A, b, route)
        if x is None or not np.all(np.isfinite(x.astype(np.float64))):
            return out
        g0 = _normalized(g0 + lxly @ x[n - 3:n - 1]) * g_norm
    out['systems']['fin'] = A
    s = x[n - 1] / 100
    out.update(g_c0=g0, s=s, v_body=x[:3 * F].reshape(F, 3))
    if s < 0:
        out['status'] = FAILED_REFINE
        return out
    key = win.get('key')
    if key is None or len(key) == 0:
        out['status'] = OK
        return out
    # ---- the window (estimator.cpp:376-435)
    gn = _normalized(g0)
    if 1 + gn[2] < 1e-12:
        return out
    v0 = _normalized(gn)
    sq = np.sqrt((1 + v0[2]) * 2)
    R0 = _q2R(np.array([v0[1] / sq, -v0[0] / sq, dtype(0), sq * dtype(0.5)]))
    R0 = _Rz_deg(-_yaw_deg(R0, dtype), dtype) @ R0
    Rs = np.array([R[f] for f in key])
    if edit != 'yaw_kept':
        R0 = _Rz_deg(-_yaw_deg(R0 @ Rs[0], dtype), dtype) @ R0
    P0 = s * T[key[0]] - Rs[0] @ tic
    Ps = np.array([s * T[f] - R[f] @ tic - P0 for f in key])
    Vs = np.array([R[f] @ x[3 * (f if edit == 'Vs_by_frame_position' else k):][:3] for k, f in enumerate(key)])
    out.update(status=OK, R0=R0, g_w=R0 @ g0, Ps=Ps @ R0.T, Rs=np.array([R0 @ r for r in Rs]), Vs=Vs @ R0.T)
    return out


# --------------------------------------------------------------------------------------------------- the metric
def errors(got, ref, literal=False):
    """{output: max|d| / max|ref| / (kappa 2^-53)} for every output `ref` has; inf for one that `got` lacks or has non-finite"""
    out = {}
    for system, names in GROUPS_OF.items():
        if system not in ref['systems']:
            continue
        k = kappa(ref['systems'][system])
        for name in names:
            if name not in ref:
                continue
            r = np.asarray(ref[name], LD)
            g = got.get(name)
            if g is None or not np.all(np.isfinite(np.asarray(g, np.float64))):
                out[name] = np.inf
                continue
            d = np.abs(np.asarray(g).astype(LD) - r).max()
            scale = ref['bias_scale'] if name == 'delta_bg' and not literal else np.abs(r).max()
            out[name] = float(d / scale / (k * EPS))
    return out


# --------------------------------------------------------------------------------------------------- the scene
def _Rzyx(y, p, r):
    cy, sy, cp, sp, cr, sr = np.cos(y), np.sin(y), np.cos(p), np.sin(p), np.cos(r), np.sin(r)
    return np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @ \
        np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])


def _small_rotation(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


G_TRUE = 9.81


def scene(seed, F, spi, noise=0.0, key=None, g_norm=G_TRUE, mirrored=False, ba0=(0.0, 0.0, 0.0), imu_dt=0.005):
    """spi: samples per interval, a number or a list of F - 1; key: None, 'all' or a list.  Returns the window dict of
    ba.Handle.init_align with `truth` = dict(s, bg, g)."""
    rng = np.random.default_rng(seed)
    spi = [int(spi)] * (F - 1) if np.isscalar(spi) else [int(x) for x in spi]
    amp, om, ph = rng.uniform(0.5, 1.5, 3), rng.uniform(1.5, 3.5, 3), rng.uniform(0, 2 * np.pi, 3)
    aamp, aom, aph = rng.uniform(0.2, 0.5, 3), rng.uniform(1.0, 2.5, 3), rng.uniform(0, 2 * np.pi, 3)
    bg_true = rng.normal(0, 0.02, 3)
    tic = rng.normal(0, 0.05, 3)
    s_true = float(rng.uniform(0.5, 3.0))
    Q = _small_rotation(rng.normal(0, 1.0, 3))
    pos = lambda t: amp * np.sin(om * t + ph)
    acc = lambda t: -amp * om * om * np.sin(om * t + ph)
    ang = lambda t: aamp * np.sin(aom * t + aph)
    dang = lambda t: aamp * aom * np.cos(aom * t + aph)

    def imu(t):
        (y, p, r), (dy, dp, dr) = ang(t), dang(t)
        gyr = np.array([dr - dy * np.sin(p), dp * np.cos(r) + dy * np.sin(r) * np.cos(p), -dp * np.sin(r) + dy * np.cos(r) * np.cos(p)])
        return _Rzyx(y, p, r).T @ (acc(t) + np.array([0, 0, G_TRUE])), gyr + bg_true

    R, T, intervals, k = [], [], [], 0
    for f in range(F):
        t = k * imu_dt
        Rw = _Rzyx(*ang(t))
        Rn = _small_rotation(rng.normal(0, noise, 3)) if noise else np.eye(3)
        Tc = (pos(t) + Rw @ tic) / s_true
        R.append(Q @ Rw @ Rn)
        T.append(Q @ Tc * (1 + (rng.normal(0, noise, 3) if noise else 0)))
        if f < F - 1:
            iv = [(0.0,) + imu(t)]
            for j in range(1, spi[f] + 1):
                iv.append((imu_dt,) + imu((k + j) * imu_dt))
            intervals.append(iv)
            k += spi[f]
    T = np.array(T)
    if mirrored:
        T = -T
    key = list(range(F)) if key == 'all' else key
    return dict(R=np.array(R), T=T, intervals=intervals, ba0=np.asarray(ba0, float), bg0=np.zeros(3), noise=NOISE, tic=tic,
                g_norm=float(g_norm), key=key, truth=dict(s=s_true, bg=bg_true, g=Q @ np.array([0, 0, G_TRUE])))


# --------------------------------------------------------------------------------------------------- the cases
def _ragged(F, seed):
    return [int(x) for x in np.random.default_rng(seed).integers(1, 25, F - 1)]


# name -> scene arguments.  `noisy`: 1 % pose noise (the cases the EDITS are judged on).
CASE_ARGS = {
    'F2': dict(seed=1, F=2, spi=20),                                          # singular by count: status != OK, nothing else pinned
    'F4': dict(seed=31, F=4, spi=20, key='all'),
    'F5': dict(seed=35, F=5, spi=20),
    'F11': dict(seed=4, F=11, spi=20, key='all'),                             # the EuRoC shape
    'F32': dict(seed=5, F=32, spi=20, key=list(range(21, 32))),
    'F11_spi1': dict(seed=31, F=11, spi=1, imu_dt=0.05),
    'F11_ragged': dict(seed=7, F=11, spi=_ragged(11, 7), key=[0, 3, 4, 9]),
    'F4_noisy': dict(seed=30, F=4, spi=20, noise=0.01, key='all'),
    'F4_noisy_fails': dict(seed=22, F=4, spi=20, noise=0.01, key='all'),                     # |g_lin| = 6.4
    'F5_noisy': dict(seed=45, F=5, spi=20, noise=0.01, key=[1, 2, 4]),
    'F5_refine_fails': dict(seed=142, F=5, spi=20, noise=0.03, key='all'),                   # s < 0 only after RefineGravity
    'F11_noisy': dict(seed=10, F=11, spi=20, noise=0.01, key='all', ba0=(0.05, -0.03, 0.08)),
    'F11_noisy_subset': dict(seed=10, F=11, spi=20, noise=0.01, key=[2, 3, 5, 6, 7, 8, 9, 10], ba0=(0.05, -0.03, 0.08)),   # non-key frames in front: Vs
    'F32_noisy': dict(seed=12, F=32, spi=_ragged(32, 12), noise=0.01, key=list(range(21, 32))),
    'F11_gnorm': dict(seed=13, F=11, spi=20, noise=0.01, g_norm=12.5, key='all'),            # | |g| - g_norm | > 1
    'F11_mirrored': dict(seed=14, F=11, spi=20, noise=0.01, mirrored=True, key='all'),       # s_lin < 0
}
NOISY = tuple(n for n, a in CASE_ARGS.items() if a.get('noise'))
TRUTH_CASES = ('F4', 'F5', 'F11', 'F32', 'F11_ragged')


@functools.lru_cache(maxsize=None)
def case(name):
    return scene(**CASE_ARGS[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    return align(case(name))


def batch(n, seed=99):
    """n windows of mixed F for the batch-equals-single checks"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        F = int(rng.choice([2, 4, 5, 7, 11, 32])) if i % 9 else 32
        keys = None if i % 3 == 0 else ('all' if i % 3 == 1 else sorted(rng.choice(F, size=max(2, F // 2), replace=False).tolist()))
        out.append(scene(1000 + i, F, _ragged(F, 2000 + i) if i % 2 else 6, noise=0.01 * (i % 4 == 1), key=keys))
    return out


# --------------------------------------------------------------------------------------------------- the device checks
# one body for the emulator (tests/test_init_align_simt.py) and the MI355X (tests/test_init_align_gpu.py); h: a ba.Handle
OUT_KEYS = ('delta_bg', 'bg', 'g_lin', 's_lin', 'g_c0', 's', 'v_body', 'Ps', 'Rs', 'Vs', 'g_w', 'R0')
REC_KEYS = ('sum_dt', 'lin_ba', 'lin_bg', 'delta_p', 'delta_q', 'delta_v', 'jacobian', 'covariance')


def same_record(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in REC_KEYS)


def same_output(a, b):
    """two results of Handle.init_align, bit for bit"""
    return (a['status'] == b['status'] and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in OUT_KEYS)
            and len(a['records']) == len(b['records']) and all(same_record(x, y) for x, y in zip(a['records'], b['records'])))


def check_cases(h, tag):
    """every case of the table in ONE call: the reference's status, every output the status reaches within M, the rest zero"""
    names = list(CASE_ARGS)
    got = dict(zip(names, h.init_align([case(n) for n in names])))
    worst = 0.0
    for n in names:
        ref, g = reference(n), got[n]
        if n == 'F2':                                       # singular by count: only that it fails and stays inside its arrays
            assert g['status'] != OK, g['status']
            continue
        assert g['status'] == ref['status'], (n, g['status'], ref['status'])
        e = errors(g, ref)
        lit = errors(g, ref, literal=True)['delta_bg']
        print(f"init_align {tag} {n}: status {g['status']}  " + "  ".join(f"{k} {v:.3f}" for k, v in e.items()) + f"  (delta_bg against max|ref|: {lit:.1f})")
        for k, v in e.items():
            assert v <= M, f"{n} {k}: {v:.3f} x kappa 2^-53 > {M}"
        worst = max(worst, max(e.values()))
        for k in OUT_KEYS:
            if k not in ref:
                assert not np.asarray(g[k]).any(), (n, k)
        assert np.array_equal(g['bg'], np.asarray(case(n)['bg0']) + g['delta_bg']), n
    print(f"init_align {tag}: worst ratio {worst:.3f} (bound {M})")
    return got


def check_records(h, got=None):
    """`records` = vg_imu_preintegrate with (0, bg) over the same rows, bit for bit"""
    names = list(CASE_ARGS)
    got = got or dict(zip(names, h.init_align([case(n) for n in names])))
    for n in names:
        w, g = case(n), got[n]
        again = h.imu_preintegrate(w['intervals'], [(np.zeros(3), g['bg'])] * len(w['intervals']), w['noise'])
        assert len(again) == len(g['records']) == len(w['R']) - 1
        for k, (a, b) in enumerate(zip(again, g['records'])):
            assert same_record(a, b), (n, k)


def check_batch_equals_single(h, sizes=(1, 3, 70)):
    wins = batch(max(sizes))
    single = [h.init_align([w])[0] for w in wins]
    assert len({s['status'] for s in single}) >= 3, "the batch mixes statuses"
    for n in sizes:
        for k, g in enumerate(h.init_align(wins[:n])):
            assert same_output(g, single[k]), (n, k)
    return single


def check_numeric_neighbours(h):
    """a window that ends with VG_ALIGN_NUMERIC between two that do not (the second with noise densities of its own): their results
    are what they are alone"""
    wins = [case('F11_noisy'), case('F2'), dict(case('F32'), noise=(0.1, 0.01, 1e-4, 1e-5)), case('F5')]
    alone = [h.init_align([w])[0] for w in wins]
    together = h.init_align(wins)
    assert alone[1]['status'] == NUMERIC and alone[0]['status'] == OK and alone[2]['status'] == OK
    assert not np.array_equal(alone[2]['records'][0]['covariance'], h.init_align([case('F32')])[0]['records'][0]['covariance'])
    for a, b in zip(alone, together):
        assert same_output(a, b)


def _refusals():
    """name -> a function that spoils the packed call (ins, outs, keep) and returns the n_windows to pass"""
    import ctypes as C
    nan = float('nan')

    def setter(fn, n=2):
        def f(ins, outs, keep):
            fn(ins, outs, keep)
            return n
        return f

    def arr(name, idx, val):
        def f(ins, outs, keep):
            keep[1][name].reshape(-1)[idx] = val
        return setter(f)

    def null(field):
        def f(ins, outs, keep):
            setattr(ins[1], field, C.cast(None, type(getattr(ins[1], field))))
        return setter(f)

    def field(obj, name, val):
        def f(ins, outs, keep):
            setattr((ins if obj == 'in' else outs)[1], name, val)
        return setter(f)

    def vec(name, idx, val):
        def f(ins, outs, keep):
            getattr(ins[1], name)[idx] = val
        return setter(f)

    r = {'n_windows_0': setter(lambda *a: None, 0), 'in_struct_size': field('in', 'struct_size', 8), 'out_struct_size': field('out', 'struct_size', 0),
         'F_1': field('in', 'n_frames', 1), 'F_33': field('in', 'n_frames', 33), 'n_key_1': field('in', 'n_key', 1), 'n_key_above_F': field('in', 'n_key', 12),
         'off_descends': arr('off', 3, 1), 'interval_empty': arr('off', 5, 80), 'key_descends': arr('key', 2, 0), 'key_repeats': arr('key', 2, 1),
         'key_is_F': arr('key', 10, 11), 'key_negative': arr('key', 0, -1), 'R_nan': arr('R', 17, nan), 'T_inf': arr('T', 4, float('inf')),
         'sample_nan': arr('smp', 7 * 33 + 2, nan), 'first_inf': arr('first', 8, float('-inf')), 'ba0_nan': vec('ba0', 1, nan), 'bg0_nan': vec('bg0', 2, nan),
         'noise_nan': vec('noise', 3, nan), 'tic_nan': vec('tic', 0, nan), 'g_norm_nan': field('in', 'g_norm', nan)}
    for t in ('R', 'T', 'sample_off', 'samples', 'first', 'key'):
        r['null_' + t] = null(t)
    r['null_Ps'] = lambda ins, outs, keep: (setattr(outs[1], 'Ps', C.cast(None, type(outs[1].Ps))), 2)[1]
    return r


REFUSALS = tuple(_refusals())


def check_refusal(h, name):
    """the spoiled call returns VG_ERR_BAD_ARG with a message, writes nothing, and the handle goes on working"""
    wins = [case('F5_noisy'), case('F11_noisy')]
    good = h.init_align(wins)
    ins, outs, keep = h.init_align_pack(wins)
    for o, b in zip(outs, keep):
        o.status, o.s = 77, -5.0
        for k in ('v_body', 'Ps', 'Rs', 'Vs'):
            b[k][...] = 3.25
        b['records'][0].sum_dt = -1.0
    n = _refusals()[name](ins, outs, keep)
    rc = h.lib.vg_init_align(h.h, n, ins, outs)
    assert rc == -1, (name, rc)                              # VG_ERR_BAD_ARG
    assert b"vg_init_align" in h.lib.vg_last_error(h.h), name
    for o, b in zip(outs, keep):
        assert o.status == 77 and o.s == -5.0 and b['records'][0].sum_dt == -1.0
        assert all(np.all(b[k] == 3.25) for k in ('v_body', 'Ps', 'Rs', 'Vs')), name
    for a, b in zip(good, h.init_align(wins)):
        assert same_output(a, b), name


# --------------------------------------------------------------------------------------------------- the stand-alone class
REPLAY_CASES = ('F11_noisy_subset', 'F11_mirrored')         # the class succeeds / returns false after solveGyroscopeBias
INIT_DEPTH = 5.0


def replay_scene(name, L=12, seed=5):
    """the case's window with a camera rotation and L landmarks seen from its window frames: (win, ric, start, nobs, points)"""
    import struct  # noqa: F401
    win = case(name)
    rng = np.random.default_rng(seed)
    ric = _small_rotation(rng.normal(0, 0.3, 3))
    key = win['key']
    K = len(key)
    start, nobs, points = [], [], []
    for _ in range(L):
        s0 = int(rng.integers(0, min(K - 2, 7)))
        n = int(rng.integers(2, K - s0 + 1))
        Rc, Tc = win['R'][key[s0]] @ ric, win['T'][key[s0]]
        X = Tc + Rc @ np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(2.0, 6.0)])
        start.append(s0)
        nobs.append(n)
        for j in range(s0, s0 + n):
            p = (win['R'][key[j]] @ ric).T @ (X - win['T'][key[j]])
            points.append(p / p[2])
    return win, ric, start, nobs, np.array(points)


def write_replay(path, win, ric, start, nobs, points):
    import struct
    F, key = len(win['R']), win['key'] or []
    with open(path, 'wb') as f:
        f.write(struct.pack('<4i', 0x314C4156, F, len(key), len(start)))
        d = lambda a: f.write(np.ascontiguousarray(a, '<f8').tobytes())
        d(win['ba0']); d(win['bg0']); d(win['noise']); d(win['tic']); d(ric); d([win['g_norm'], INIT_DEPTH])
        for k in range(F):
            d([0.05 * k + 100.0]); d(win['R'][k]); d(win['T'][k])
        for iv in win['intervals']:
            f.write(struct.pack('<i', len(iv) - 1))
            d(np.concatenate([iv[0][1], iv[0][2]]))
            d([[dt, *a, *g] for dt, a, g in iv[1:]])
        f.write(np.asarray(key, '<i4').tobytes())
        o = 0
        for s0, n in zip(start, nobs):
            f.write(struct.pack('<2i', s0, n))
            d(points[o:o + n])
            o += n


def check_replay(h, exe, tmp_dir, name):
    """`vins_replay align` (Estimator::visualInitialAlign of host/estimator.cpp) against the binding, number for number"""
    import os
    import subprocess
    win, ric, start, nobs, points = replay_scene(name)
    src, dst = os.path.join(str(tmp_dir), name + '.bin'), os.path.join(str(tmp_dir), name + '.txt')
    write_replay(src, win, ric, start, nobs, points)
    r = subprocess.run([exe, 'align', src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in open(dst)]
    res = h.init_align([win])[0]
    assert rows[0] == ['result', '1' if res['status'] == OK else '0', str(res['status'])]
    num = lambda row: np.array([float(x) for x in row[1:]])
    assert rows[1][0] == 'bg' and np.array_equal(num(rows[1]), res['bg'])
    frames = [num(r_) for r_ in rows if r_[0] == 'frame']
    depth = np.array([float(r_[1]) for r_ in rows if r_[0] == 'depth'])
    if res['status'] != OK:
        assert not frames and np.all(depth == -1.0)
        return
    assert np.array_equal(num(rows[2]), res['g_w'])
    key = win['key']
    assert len(frames) == len(key)
    for k, fr in enumerate(frames):
        assert np.array_equal(fr[:3], res['Ps'][k]) and np.array_equal(fr[3:12], res['Rs'][k].ravel()) and np.array_equal(fr[12:], res['Vs'][k]), k
    off = np.concatenate([[0], np.cumsum(nobs)[:-1]])
    want = h.triangulate(win['T'][key], win['R'][key], np.zeros(3), ric, start, nobs, off, points, INIT_DEPTH) * res['s']
    assert np.array_equal(depth, want)
    assert np.all(want > 0)
