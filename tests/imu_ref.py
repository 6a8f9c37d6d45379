"""80-bit reference, metric and case table for the IMU pre-integration kernels (helper module of tests/test_imu_scale.py and
tests/seq_imu_model.py; no tests in here).

`integrate` restates IntegrationBase::push_back (integration_base.h:30-158: mid-point states, F, V, jacobian <- F jacobian,
covariance <- F P F^T + V N V^T) in the requested number format, from the identity or from a stored record (the continuation of
pre_integrations[WINDOW_SIZE - 1] in slideWindow).  The inputs are the float64 inputs, widened: the reference answers for the
numbers the device got.  With np.longdouble (80-bit) it is the reference; with np.float64 it repeats oracle/ba_numpy.Preintegration
operation by operation (bit-identical, asserted in tests/test_imu_scale.py) and takes the EDITS of the mutation condition.

`record_error(got, ref)` measures a record in its own scale, one number per field:
    covariance   max_ij |dC_ij| / sqrt(C_ii C_jj), C from the reference (C is positive semi-definite, so the scale bounds every
                 entry); where C_ii C_jj == 0 the entry must be exactly 0
    jacobian     per 3x3 block of the [p, theta, v, ba, bg] partition max|dJ| / max|J_block|, the largest over the blocks; a block
                 the reference has identically zero must be exactly zero, the ba / bg rows exactly the identity rows
    delta_p / delta_q / delta_v      max|d| / max|ref| of the field
    sum_dt       bit pattern against the sequential float64 sum; lin_ba / lin_bg exactly
A violated exactness demand gives inf.

The yardstick: e64(case) = record_error of the float64 oracle (B.Preintegration) against the 80-bit reference, per field kind
('covariance', 'jacobian', 'state'); E64 = the largest over CASES.  No device takes part in either."""
import functools

import numpy as np

from oracle import ba_numpy as B

LD = np.longdouble
M = 4                     # the device's bound is M * E64 (tests/test_imu_scale.py: MEASURED)
NOISE = (0.08, 0.004, 4e-5, 2e-6)
KINDS = ('covariance', 'jacobian', 'state')
KIND_OF = dict(covariance='covariance', jacobian='jacobian', delta_p='state', delta_q='state', delta_v='state')
EDITS = ('Rr_normalised', 'V_p_gyr1_doubled', 'F_p_bg_sign', 'gyr_w_for_acc_w', 'F_theta_theta_identity', 'cov_bg_entry')


# --------------------------------------------------------------------------------------------------- the reference
def integrate(iv, ba=None, bg=None, noise=NOISE, dtype=LD, start=None, edit=None):
    """iv: [(0, acc_0, gyr_0), (dt, acc, gyr), ...] (the layout of synth.preintegrate); start: a stored record to continue (its
    linearisation biases hold, ba / bg are not read); edit: one of EDITS."""
    w = lambda v: np.asarray(v).astype(dtype)                  # (a float64 input is widened, an 80-bit record kept as it is)
    acc_n, gyr_n, acc_w, gyr_w = (dtype(np.float64(x)) for x in noise)
    if edit == 'gyr_w_for_acc_w':
        acc_w = gyr_w
    n = np.zeros(18, dtype)
    n[0:3] = acc_n * acc_n
    n[3:6] = gyr_n * gyr_n
    n[6:9] = acc_n * acc_n
    n[9:12] = gyr_n * gyr_n
    n[12:15] = acc_w * acc_w
    n[15:18] = gyr_w * gyr_w
    N = np.diag(n)
    acc_0, gyr_0 = w(iv[0][1]), w(iv[0][2])
    if start is None:
        ba, bg = w(ba), w(bg)
        J, P = np.eye(15, dtype=dtype), np.zeros((15, 15), dtype)
        dp, dq, dv = np.zeros(3, dtype), np.array([0, 0, 0, 1], dtype), np.zeros(3, dtype)
        sum_dt = 0.0
    else:
        ba, bg = w(start['lin_ba']), w(start['lin_bg'])
        J, P = w(start['jacobian']).reshape(15, 15), w(start['covariance']).reshape(15, 15)
        dp, dq, dv = w(start['delta_p']), w(start['delta_q']), w(start['delta_v'])
        sum_dt = float(start['sum_dt'])
    I3 = np.eye(3, dtype=dtype)
    for dt64, a1, g1 in iv[1:]:
        dt, acc_1, gyr_1 = dtype(np.float64(dt64)), w(a1), w(g1)
        Rq = B.q2R(dq)
        un_acc_0 = Rq @ (acc_0 - ba)
        un_gyr = 0.5 * (gyr_0 + gyr_1) - bg
        res_q = B.qmul(dq, np.array([un_gyr[0] * dt / 2, un_gyr[1] * dt / 2, un_gyr[2] * dt / 2, 1.0], dtype))
        Rr = B.q2R(B.qnormalized(res_q) if edit == 'Rr_normalised' else res_q)        # the reference's quirk: un-normalised
        un_acc_1 = Rr @ (acc_1 - ba)
        un_acc = 0.5 * (un_acc_0 + un_acc_1)
        res_p = dp + dv * dt + 0.5 * un_acc * dt * dt
        res_v = dv + un_acc * dt
        w_x = 0.5 * (gyr_0 + gyr_1) - bg
        R_w_x, R_a_0_x, R_a_1_x = B.skew(w_x), B.skew(acc_0 - ba), B.skew(acc_1 - ba)
        F = np.zeros((15, 15), dtype)
        F[0:3, 0:3] = I3
        F[0:3, 3:6] = -0.25 * Rq @ R_a_0_x * dt * dt + -0.25 * Rr @ R_a_1_x @ (I3 - R_w_x * dt) * dt * dt
        F[0:3, 6:9] = I3 * dt
        F[0:3, 9:12] = -0.25 * (Rq + Rr) * dt * dt
        F[0:3, 12:15] = -0.25 * Rr @ R_a_1_x * dt * dt * -dt
        F[3:6, 3:6] = I3 - R_w_x * dt
        F[3:6, 12:15] = -1.0 * I3 * dt
        F[6:9, 3:6] = -0.5 * Rq @ R_a_0_x * dt + -0.5 * Rr @ R_a_1_x @ (I3 - R_w_x * dt) * dt
        F[6:9, 6:9] = I3
        F[6:9, 9:12] = -0.5 * (Rq + Rr) * dt
        F[6:9, 12:15] = -0.5 * Rr @ R_a_1_x * dt * -dt
        F[9:12, 9:12] = I3
        F[12:15, 12:15] = I3
        V = np.zeros((15, 18), dtype)
        V[0:3, 0:3] = 0.25 * Rq * dt * dt
        V[0:3, 3:6] = 0.25 * -Rr @ R_a_1_x * dt * dt * 0.5 * dt
        V[0:3, 6:9] = 0.25 * Rr * dt * dt
        V[0:3, 9:12] = V[0:3, 3:6]
        V[3:6, 3:6] = 0.5 * I3 * dt
        V[3:6, 9:12] = 0.5 * I3 * dt
        V[6:9, 0:3] = 0.5 * Rq * dt
        V[6:9, 3:6] = 0.5 * -Rr @ R_a_1_x * dt * 0.5 * dt
        V[6:9, 6:9] = 0.5 * Rr * dt
        V[6:9, 9:12] = V[6:9, 3:6]
        V[9:12, 12:15] = I3 * dt
        V[12:15, 15:18] = I3 * dt
        if edit == 'V_p_gyr1_doubled':
            V[0:3, 9:12] = 2 * V[0:3, 9:12]
        if edit == 'F_p_bg_sign':
            F[0:3, 12:15] = -F[0:3, 12:15]
        if edit == 'F_theta_theta_identity':
            F[3:6, 3:6] = I3
        J = F @ J
        P = F @ P @ F.T + V @ N @ V.T
        dp, dv = res_p, res_v
        dq = B.qnormalized(res_q)
        sum_dt += float(dt64)                                                    # sample order, float64: what the kernel does
        acc_0, gyr_0 = acc_1, gyr_1
    if edit == 'cov_bg_entry':
        P = P.copy()
        P[13, 13] = P[13, 13] * (1 + dtype(1e-9))                               # (the gyro-bias block is diagonal)
    return dict(sum_dt=sum_dt, delta_p=dp, delta_q=dq, delta_v=dv, lin_ba=ba, lin_bg=bg, jacobian=J, covariance=P)


def oracle64(iv, ba=None, bg=None, noise=NOISE, start=None):
    """The float64 oracle (oracle/ba_numpy.Preintegration) on the same inputs; start: a record it continues."""
    if start is None:
        p = B.Preintegration(iv[0][1], iv[0][2], ba, bg, *noise)
    else:
        p = B.Preintegration(iv[0][1], iv[0][2], start['lin_ba'], start['lin_bg'], *noise)
        p.jacobian, p.covariance = np.array(start['jacobian'], float).reshape(15, 15), np.array(start['covariance'], float).reshape(15, 15)
        p.delta_p, p.delta_q, p.delta_v = np.array(start['delta_p'], float), np.array(start['delta_q'], float), np.array(start['delta_v'], float)
        p.sum_dt = float(start['sum_dt'])
    for dt, a, g in iv[1:]:
        p.push_back(dt, a, g)
    return p.as_dict()


# --------------------------------------------------------------------------------------------------- the metric
def record_error(got, ref):
    """One number per field (module docstring); `ref` in np.longdouble, `got` whatever the device or an oracle returned."""
    out = {}
    C = np.asarray(ref['covariance'], LD).reshape(15, 15)
    G = np.asarray(got['covariance'], np.float64).astype(LD).reshape(15, 15)
    d = np.diag(C)
    assert np.all(d >= 0), "the reference covariance has a negative diagonal entry"
    scale = np.sqrt(np.outer(d, d))
    zero = scale == 0
    e = 0.0
    if np.any(~zero):
        e = float((np.abs(G - C)[~zero] / scale[~zero]).max())
    if np.any(G[zero] != 0) or not np.all(np.isfinite(G.astype(np.float64))):
        e = np.inf
    out['covariance'] = e
    Jr = np.asarray(ref['jacobian'], LD).reshape(15, 15)
    Jg = np.asarray(got['jacobian'], np.float64).astype(LD).reshape(15, 15)
    e = 0.0
    for bi in range(5):
        for bj in range(5):
            r, g = Jr[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3], Jg[3 * bi:3 * bi + 3, 3 * bj:3 * bj + 3]
            m = np.abs(r).max()
            if m == 0:
                e = e if np.all(g == 0) else np.inf
            else:
                e = max(e, float(np.abs(g - r).max() / m))
    if not np.array_equal(Jg[9:15], np.eye(15, dtype=LD)[9:15]) or not np.all(np.isfinite(Jg.astype(np.float64))):
        e = np.inf
    out['jacobian'] = e
    for key in ('delta_p', 'delta_q', 'delta_v'):
        r, g = np.asarray(ref[key], LD), np.asarray(got[key], np.float64).astype(LD)
        m = np.abs(r).max()
        if m == 0:
            out[key] = 0.0 if np.all(g == 0) else np.inf
        else:
            out[key] = float(np.abs(g - r).max() / m) if np.all(np.isfinite(g.astype(np.float64))) else np.inf
    out['sum_dt'] = 0.0 if np.float64(got['sum_dt']).tobytes() == np.float64(ref['sum_dt']).tobytes() else np.inf
    for key in ('lin_ba', 'lin_bg'):
        if key in got:
            out[key] = 0.0 if np.array_equal(np.asarray(got[key], np.float64), np.asarray(ref[key], LD).astype(np.float64)) else np.inf
    return out


def by_kind(err):
    """record_error's fields folded into the kinds the yardstick has"""
    out = dict.fromkeys(KINDS, 0.0)
    for key, kind in KIND_OF.items():
        out[kind] = max(out[kind], err[key])
    return out


def exact_ok(err):
    return all(err[k] == 0.0 for k in ('sum_dt', 'lin_ba', 'lin_bg') if k in err)


# --------------------------------------------------------------------------------------------------- the cases
def _interval(rng, n, dt, gyr_sigma=0.3, gyr_mean=(0, 0, 0)):
    """n samples; dt: a number or a (lo, hi) range drawn per sample"""
    step = (lambda: dt) if np.isscalar(dt) else (lambda: float(rng.uniform(*dt)))
    g = lambda: rng.normal(0, gyr_sigma, 3) + np.asarray(gyr_mean, float)
    iv = [(0.0, rng.normal(0, 1, 3) + [0, 0, 9.8], g())]
    for _ in range(n):
        iv.append((step(), rng.normal(0, 1, 3) + [0, 0, 9.8], g()))
    return iv


def _bias(rng):
    return rng.normal(0, 0.05, 3), rng.normal(0, 0.02, 3)


def _build_cases():
    """name -> dict(iv, ba, bg, noise); every entry of the issue's table that one vg_imu_preintegrate interval can express"""
    rng = np.random.default_rng(20261019)
    cases = {}

    def add(name, iv, bias=None, noise=NOISE):
        ba, bg = bias if bias is not None else _bias(rng)
        cases[name] = dict(iv=iv, ba=np.asarray(ba, float), bg=np.asarray(bg, float), noise=noise)

    add('n0', _interval(rng, 0, 0.005))                                # identity record, covariance exactly 0
    for n in (1, 2, 20, 64):
        add(f'n{n}', _interval(rng, n, 0.005))
    add('n7_dt4.9ms', _interval(rng, 7, 0.0049))
    add('n120_dt0.1', _interval(rng, 120, 0.1))                        # sum_dt > 10
    add('varying_dt', _interval(rng, 30, (0.001, 0.010)))
    iv = _interval(rng, 10, 0.005)
    iv[6] = (0.0,) + iv[6][1:]                                         # a repeated time stamp in the middle
    add('dt0_sample', iv)
    ba, bg = _bias(rng)
    iv = _interval(rng, 20, 0.005)
    add('gyro_equals_bias', [(dt, a, bg.copy()) for dt, a, _ in iv], (ba, bg))      # w = 0 exactly: I - [w]x dt = I
    add('zero_biases', _interval(rng, 20, 0.005), (np.zeros(3), np.zeros(3)))
    add('fast_rotation', _interval(rng, 65, 0.0025, gyr_sigma=0.2, gyr_mean=(1.8, -1.7, 1.7)))   # |w| ~ 3 rad/s: the un-normalised Rr matters
    add('noise_zero', _interval(rng, 20, 0.005), noise=(0.0, 0.0, 0.0, 0.0))
    add('repropagated', cases['n20']['iv'])                            # the same samples with other biases
    return cases


CASES = _build_cases()

RAGGED_N = 70
RAGGED_EMPTY = (0, 33, 69)


@functools.lru_cache(maxsize=None)
def ragged():
    """70 intervals of 0 .. 24 samples for one call (grid = intervals), three of them empty: [(iv, ba, bg)]"""
    rng = np.random.default_rng(70)
    out = []
    for k in range(RAGGED_N):
        n = 0 if k in RAGGED_EMPTY else int(rng.integers(1, 25))
        out.append((_interval(rng, n, (0.002, 0.008)),) + _bias(rng))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = CASES[name]
    return integrate(c['iv'], c['ba'], c['bg'], c['noise'])


@functools.lru_cache(maxsize=None)
def ragged_reference(k):
    iv, ba, bg = ragged()[k]
    return integrate(iv, ba, bg, NOISE)


def e64_of(iv, ba=None, bg=None, noise=NOISE, start=None, ref=None):
    """what the float64 oracle loses on these inputs, per kind"""
    ref = ref if ref is not None else integrate(iv, ba, bg, noise, start=start)
    err = record_error(oracle64(iv, ba, bg, noise, start=start), ref)
    assert exact_ok(err), err
    return by_kind(err)


@functools.lru_cache(maxsize=None)
def e64(name):
    c = CASES[name]
    return e64_of(c['iv'], c['ba'], c['bg'], c['noise'], ref=reference(name))


@functools.lru_cache(maxsize=None)
def yardstick():
    """E64 per kind: the largest e64 over CASES and the ragged intervals"""
    out = dict.fromkeys(KINDS, 0.0)
    table = [e64(name) for name in CASES] + [e64_of(*ragged()[k], ref=ragged_reference(k)) for k in range(RAGGED_N)]
    for e in table:
        for k in KINDS:
            out[k] = max(out[k], e[k])
    return out
