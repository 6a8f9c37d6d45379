"""The marginalization prior entry by entry, in the prior's own scale, on every elimination path of ba_marg_kernel.

Every case marginalises a window at a FIXED state (max_iters = 0), asserts the path word the kernel left (vg_ba_batch_marg_info: which
variant removed the dropped block, whether the certificate lambda_min(Amm) > 1e-7 held, where the Schur product took its operands, which
factorisation produced J0 / r0) and holds the prior to tests/marg_ref.py: J0^T J0, J0^T r0 and |r0|^2 against an 80-bit generalised
Schur complement of the same factors, each in the scale of the entry it lands on, bounded by  M x E64(kind, class)  where E64 is what
the float64 run of the SAME reference loses against the 80-bit one (the largest over the cases of a class; no device takes part).

The cut of the kept block.  On the EuRoC-shape windows the pivots of the kept block just above eps = 1e-8 (2e-7 .. 3e-4 on the second
window of seed 40) lie BELOW the float64 rounding noise of A' at the same entries (~1e-4: the accelerometer-bias block is what is left
of IMU weights of 1e7 after the Schur complement), so whether those directions are kept is decided by rounding -- in this kernel, in
the float64 run of the reference and in the NumPy oracle alike (ranks 66, 67, 66 of 69 there).  marg_ref.cut_ambiguity measures that noise
(float64 against 80-bit remaining diagonals under the same pivot order, no device) and prior_error grants g and c exactly what such a
direction carries: J0^T r0 may differ on the unpivoted columns by |b_r|_i + sqrt(A_r,ii c_amb), |r0|^2 lies in [c_det, c_det + c_amb];
a DETERMINED direction must be kept (rank_ok).  This is the "60 x worse J0^T r0" of the square-root form on that window: one direction
with an 80-bit pivot of 1.8e-7 that the kernel's rounding put below eps -- 3.8e-5 of the gradient's scale on one accelerometer-bias
column, 1e-10 everywhere else; the eigen form on the same window loses 9e-5, the oracle 4e-5.  Inherent to the cut, not to the direct path.
The eigen form cuts eigen-directions, not columns: its g is the error of J0^T r0 along the DETERMINED eigenvectors of A*, each component
in its scale sqrt(lambda_k) rho and less what a cut direction tilted by the same noise leaks onto it (only the eigenvalues next to the
ambiguous ones are spared); its c is held to [c_lo, c_hi] like the square-root form's.

MEASURED (E64 per kind and class -- for H a window is bounded by at most SPLIT = 10 x its own float64 loss --; worst ratio prior_error / E64
per class, emulator | MI355X; the case that set it)
    class        E64 H     E64 g     E64 c      H                              g                                  c
    first        5.1e-5    2e-9 *    2e-9 *     1.73 ml17      | 1.54 K4_ml8    0.20 K4_ml8_eig | 0.20 K4_ml8_eig   7e-6   | 7e-6
    prior        4.2e-5    2e-9 *    1.8e-3     2.03 plain_eig | 2.28 plain_eig 0.051 plain     | 0.051 plain       1.59 plain_eig | 1.48 ex_td
    no_imu0      2e-9 *    2e-9 *    2e-9 *     0.0096         | 0.0096         0.0023          | 0.0023            6.4e-4 | 6.4e-4
    blind        1.9e-2    2e-9 *    2e-9 *     1.35 K11 (own 1.0e-5: bound 1.0e-4) | 0.70 K11    4.73 K11 | 1.53 K11    4.9e-3 | 3.1e-3
    second_new   1.2e-12   5.4e-11   3.0e-9     0.758 rank2    | 0.224 full     0.517 full      | 0.617 full        1.9 full | 2.07 full
    collinear    2.3e-13 -> 2e-9 *  2e-9 *  2e-9 *   0.014 ml40 | 0.014        0.0024 ml40     | 0.0024            0      | 0
    enlarged     9.0e-3    2e-9 *    2e-9 *     4.71           | 3.41           6.45            | 0.443             1.4e-3 | 6.5e-4
    (* = the floor: the library evaluates the factors itself, to the 1e-9 of test_factor_parity; second_new: 1e-14.)
    Factors (smallest power of two with a factor two to spare): emulator H 8 (16 for the enlarged window), g 16, c 4; MI355X H 8, g 4, c 8.
    The enlarged window's own float64 loss IS 9e-3 (bias_a x bias_a of a 16-frame first window): no float64 implementation is held tighter
    there; every other pair of blocks of that window is reported by H_by_pair.
    A blind landmark sent through the eigen pseudo-inverse of the whole dropped block instead of being cut inside the eliminations
    (measured on the emulator with that edit): blind_K11_ml60 (m = 75, Jacobi in LDS) H 6.6 at bias_a x bias_a (the entry 0.569 for
    0.075), g 2.9e-5; blind_K5_ml60 (m > ld, Jacobi in global memory) H 2.2e-2, g 3.3e-4, c 3.8e-6; blind_K4_ml8 H 1.9e-2.  As the
    kernel stands: H 1.4e-4 / 2.1e-3 / 1.4e-3, g 9.5e-9 / 4.5e-9 / 6.5e-10.
"""
import functools

import numpy as np
import pytest

from oracle import ba_numpy as B
from vins_mono_amd import ba, synth

import ba_step_ref as S
import marg_ref as R

OLD, SECOND_NEW, NONE = ba.VG_MARGIN_OLD, ba.VG_MARGIN_SECOND_NEW, ba.VG_MARGIN_NONE
SQRT, EIGEN = ba.VG_MARG_SQRT, ba.VG_MARG_EIGEN


# --------------------------------------------------------------------------------------------------- windows
def _at(prob, x=None):
    """`prob` pinned at state x (default: its own): max_iters = 0, both sides marginalise there."""
    at = dict(prob)
    if x is not None:
        at.update(pose=x['pose'], sb=x['sb'], ex=x['ex'], td=x['td'], inv_depth=x['inv_depth'])
    at['max_iters'] = 0
    return at


def _first(K, ml, seed=None):
    """A window of K frames whose `ml` landmarks ALL start at frame 0, with a diagonal prior on its oldest frame
    (SyntheticSequence.anchor_prior), pinned at its initial state: the dropped block is pose 0 | speed-bias 0 | ml inverse depths.
    The prior is what makes small ml a test: without one a window with a few landmarks leaves kept columns without any information
    (A*_ii = 0: no scale), and with ml = 0 the only marginalised factor is the first IMU factor, whose 15 dropped unknowns take all
    of its 15 equations along."""
    prob = S.ruled_window(600 + ml if seed is None else seed, K=K, n_landmarks=ml, anchor='all_at_0', length='mixed')
    assert int((np.asarray(prob['lm_start']) == 0).sum()) == ml
    return _at(synth.SyntheticSequence.anchor_prior(prob))


@functools.lru_cache(maxsize=None)
def _chain(seed, L, ex, td, steps):
    """SyntheticSequence(seed, L): window 0 solved by the oracle and marginalised (MARGIN_OLD) `steps` times; returns (sequence, the
    window after the last step pinned at ITS oracle optimum)."""
    seq = synth.SyntheticSequence(seed, L=L, n_frames=11 + steps, estimate_extrinsic=ex, estimate_td=td)
    prob = seq.window(0)
    for k in range(steps):
        x, _ = B.solve(prob)
        st = B.double2vector(prob, x)
        prob = seq.next_window(st, B.marginalize(prob, st, B.MARGIN_OLD), k + 1)
    x, _ = B.solve(prob)
    return seq, _at(prob, x)


def _second(seed=40, L=60, ex=0, td=0, relo=False, steps=1):
    seq, at = _chain(seed, L, ex, td, steps)
    at = dict(at)
    if td:
        at['tr'] = 0.02
    if relo:
        S.add_relocalisation(at, seq.cfg)
    return at


def _no_first_imu(kind):
    """MARGIN_OLD without the first IMU factor (estimator.cpp:836: pre_integrations[1]->sum_dt > 10 skips it): speed-bias 0 is in no
    marginalised factor, so it is not dropped (md = 6) and pose 1 / speed-bias 1 enter only through projection factors."""
    at = _first(6, 12, seed=661)
    at['imu'] = [dict(m) for m in at['imu']]
    if kind == 'sum_dt':
        at['imu'][0]['sum_dt'] = 10.5
    else:
        at['imu'][0] = None
    return at


def _blind_landmark(K, ml, seed):
    """A first window in which ONE frame-0 landmark carries no information: it is seen from frames 0 and 1 only and the camera centre
    of frame 1 is moved onto that of frame 0 (pure rotation: the reprojection does not depend on the depth).  Its pivot is <= 1e-10 in
    the 80-bit reference: the direction is cut, and the rest of the dropped block must still leave by elimination."""
    seq = S.ruled_sequence(seed, K=K, n_landmarks=ml, anchor='all_at_0', length='full')
    seq.lm[0]['obs'] = seq.lm[0]['obs'][:2]
    prob = seq.window(0)
    tic = prob['ex'][:3]
    R0, R1 = B.q2R(prob['pose'][0][3:]), B.q2R(prob['pose'][1][3:])
    prob['pose'][1][:3] = prob['pose'][0][:3] + R0 @ tic - R1 @ tic
    assert prob['lm_nobs'][0] == 2 and np.all(prob['lm_nobs'][1:] > 2)
    return _at(prob)


def _collinear(ml, seed=680):
    """A K = 6 first window without a prior and without the first IMU factor whose `ml` frame-0 landmarks all lie on ONE ray of camera 0
    (the same first observation, depths 2 .. 12 m): rotating pose 0 about that ray moves no point, so P' (pose 0 after the landmarks)
    is rank deficient while every landmark has d_l >> eps.  The certificate fails and the eigen pseudo-inverse of the whole dropped
    block (m = 6 + ml) has to run and cut that direction."""
    seq = S.ruled_sequence(seed, K=6, n_landmarks=ml, anchor='all_at_0', length='full')
    c = seq.cfg
    rng = np.random.default_rng([seed, 31])
    ray = np.array([0.05, -0.04, 1.0])
    for l, lm in enumerate(seq.lm):
        Xw = seq.Rm[0] @ (c['ric'] @ (ray * (2.0 + 10.0 * l / max(1, ml - 1))) + c['tic']) + seq.P[0]
        pts = [c['ric'].T @ (seq.Rm[f].T @ (Xw - seq.P[f]) - c['tic']) for f in range(len(lm['obs']))]
        assert all(p[2] >= 0.2 for p in pts)
        obs = np.array([p[:2] / p[2] + rng.normal(0, 0.3 / 460.0, 2) for p in pts])
        obs[0] = ray[:2]
        lm.update(Xw=Xw, obs=obs)
    at = _at(seq.window(0))
    at['imu'] = [dict(m) for m in at['imu']]
    at['imu'][0] = None
    return at


def _many_frame0(K, L, w0, n_frames):
    """A window that has slid for a while (most landmarks anchored at frame 0), pinned at its initial state."""
    return _at(synth.SyntheticSequence(47, n_frames=n_frames, K=K, L=L).window(w0))


def _second_new_weak_pivot():
    """MARGIN_SECOND_NEW on a hand-made diagonal prior over pose K - 2 | pose K - 1 | speed-bias K - 1 in which ONE kept column carries
    1e-7 of information: ten times the cut, and exact in float64 (nothing cancels), so the direction is determined and must be kept --
    the case that tells eps = 1e-8 from a larger one.  The dropped pose block is definite: the only MARGIN_SECOND_NEW case that passes
    the certificate."""
    prob = S.ruled_window(690, K=4, n_landmarks=6, anchor='all_at_0', length='full')
    K = prob['pose'].shape[0]
    w = np.array([50.0] * 3 + [100.0] * 3 + [40.0, 60.0, 80.0] + [90.0, np.sqrt(1e-7), 110.0] + [20.0] * 3 + [50.0] * 6)
    prob['prior'] = dict(n=21, blocks=[(B.KIND_POSE, K - 2), (B.KIND_POSE, K - 1), (B.KIND_SB, K - 1)], J0=np.diag(w),
                         r0=0.05 * np.cos(np.arange(21.0)), x0=[prob['pose'][K - 2].copy(), prob['pose'][K - 1].copy(), prob['sb'][K - 1].copy()])
    return _at(prob)


def _second_new_absent():
    _, at = _chain(7, 8, 0, 0, 1)
    return at


WINDOWS = {
    # MARGIN_OLD: the trip counts of the rank-ml update (16-wide chunks, 4-wide tail inside)
    **{f'first_K6_ml{ml}': (functools.partial(_first, 6, ml), OLD) for ml in (0, 1, 2, 15, 16, 17, 63, 64, 65, 94, 95)},
    **{f'first_K4_ml{ml}': (functools.partial(_first, 4, ml), OLD) for ml in (8, 55, 56, 80, 81)},
    'prior_plain': (functools.partial(_second), OLD),
    'prior_ex_td': (functools.partial(_second, seed=41, ex=1, td=1), OLD),
    'prior_relo': (functools.partial(_second, relo=True), OLD),
    'no_imu0_sum_dt': (functools.partial(_no_first_imu, 'sum_dt'), OLD),
    'no_imu0_invalid': (functools.partial(_no_first_imu, 'invalid'), OLD),
    'blind_K4_ml8': (functools.partial(_blind_landmark, 4, 8, 671), OLD),
    'blind_K11_ml60': (functools.partial(_blind_landmark, 11, 60, 672), OLD),
    'blind_K5_ml60': (functools.partial(_blind_landmark, 5, 60, 673), OLD),
    'second_new_rank2': (functools.partial(_second), SECOND_NEW),
    'second_new_full': (functools.partial(_second, steps=3), SECOND_NEW),
    'second_new_absent': (_second_new_absent, SECOND_NEW),
    'second_new_weak_pivot': (_second_new_weak_pivot, SECOND_NEW),
    **{f'collinear_ml{ml}': (functools.partial(_collinear, ml), OLD) for ml in (40, 59, 60)},
    'enlarged_K16': (functools.partial(_many_frame0, 16, 40, 1, 20), OLD),
}

# class of a window: E64 is the largest float64 loss over the windows of ONE class (the classes differ by decades: a speed-bias that
# only projection factors reach, a 16-frame window, a dropped block that leaves through the eigen pseudo-inverse)
def group_of(window):
    for prefix in ('first', 'prior', 'no_imu0', 'blind', 'second_new', 'enlarged', 'collinear'):
        if window.startswith(prefix):
            return prefix
    raise KeyError(window)


PINV_GROUPS = ('second_new', 'collinear')      # rank-deficient dropped block: the yardstick takes the reference's eigen pseudo-inverse too


def _path(stage1, cert, schur, stage2):
    return dict(stage1=stage1, cert=cert, schur=schur, stage2=stage2)


DIRECT = _path('direct', 'passed', None, 'sqrt')
# (case id, window, form, the path word it exists for).  Thresholds, from build_layout / marg_lds / ba_marg_kernel: K = 4: mcap = 56,
# ld = 57, n = 33 -> q = md + n + 1 = 49 pads to 64 > ld: never direct; right-hand sides staged while 15 ml + (15 + ml) 34 <= ld^2
# (ml <= 55); Schur product through LDS while m (n + 1) <= ld^2 (ml <= 80).  K = 6: ld = 65, n = 45: direct while 31 ml <= n ld
# (ml <= 94).  vh_eig takes at most 64 columns (MG_NT / 16 pairs), the LDS Jacobi m, n <= ld, K = 16: ld < n = 105.
CASES = [
    *[(f'first_K6_ml{ml}', f'first_K6_ml{ml}', 'sqrt', DIRECT) for ml in (0, 1, 2, 15, 16, 17, 63, 64, 65, 94)],
    ('first_K6_ml95', 'first_K6_ml95', 'sqrt', _path('block_glb', 'passed', 'glb', 'sqrt')),
    ('first_K4_ml8', 'first_K4_ml8', 'sqrt', _path('block_lds', 'passed', 'lds', 'sqrt')),
    ('first_K4_ml55', 'first_K4_ml55', 'sqrt', _path('block_lds', 'passed', 'lds', 'sqrt')),
    ('first_K4_ml56', 'first_K4_ml56', 'sqrt', _path('block_glb', 'passed', 'lds', 'sqrt')),
    ('first_K4_ml80', 'first_K4_ml80', 'sqrt', _path('block_glb', 'passed', 'lds', 'sqrt')),
    ('first_K4_ml81', 'first_K4_ml81', 'sqrt', _path('block_glb', 'passed', 'glb', 'sqrt')),
    ('first_K4_ml8_eigen', 'first_K4_ml8', 'eigen', _path('block_lds', 'passed', 'lds', 'vh_eig')),
    ('prior_plain', 'prior_plain', 'sqrt', DIRECT),
    ('prior_ex_td', 'prior_ex_td', 'sqrt', DIRECT),
    ('prior_relo', 'prior_relo', 'sqrt', DIRECT),
    ('prior_plain_eigen', 'prior_plain', 'eigen', _path('block_lds', 'passed', 'lds', 'jacobi_lds')),
    ('prior_ex_td_eigen', 'prior_ex_td', 'eigen', _path('block_lds', 'passed', 'lds', 'jacobi_lds')),
    ('prior_relo_eigen', 'prior_relo', 'eigen', _path('block_lds', 'passed', 'lds', 'jacobi_lds')),
    ('no_imu0_sum_dt', 'no_imu0_sum_dt', 'sqrt', DIRECT),
    ('no_imu0_invalid', 'no_imu0_invalid', 'sqrt', DIRECT),
    # (one frame-0 landmark without information: it is cut INSIDE the eliminations, the certificate holds for the rest)
    ('blind_K4_ml8', 'blind_K4_ml8', 'sqrt', _path('block_lds', 'passed', 'lds', 'sqrt')),
    ('blind_K11_ml60', 'blind_K11_ml60', 'sqrt', DIRECT),
    ('blind_K5_ml60', 'blind_K5_ml60', 'sqrt', _path('block_glb', 'passed', 'lds', 'sqrt')),
    ('second_new_rank2', 'second_new_rank2', 'sqrt', _path('vh_eig', 'failed', 'lds', 'sqrt')),
    ('second_new_full', 'second_new_full', 'sqrt', _path('vh_eig', 'failed', 'lds', 'sqrt')),
    ('second_new_weak_pivot', 'second_new_weak_pivot', 'sqrt', DIRECT),
    # failed certificate with every landmark well above the cut: P' is rank deficient (all landmarks on one ray of camera 0).  m = 6 + ml:
    # vh_eig up to 64 columns, the LDS Jacobi up to ld = 65, the global one beyond
    ('collinear_ml40', 'collinear_ml40', 'sqrt', _path('vh_eig', 'failed', 'lds', 'sqrt')),
    ('collinear_ml59', 'collinear_ml59', 'sqrt', _path('jacobi_lds', 'failed', 'lds', 'sqrt')),
    ('collinear_ml60', 'collinear_ml60', 'sqrt', _path('jacobi_glb', 'failed', 'lds', 'sqrt')),
    ('enlarged_K16', 'enlarged_K16', 'sqrt', _path('block_lds', 'passed', 'lds', 'sqrt_glb')),
    ('enlarged_K16_eigen', 'enlarged_K16', 'eigen', _path('block_lds', 'passed', 'lds', 'jacobi_glb')),
]
CASE = {c[0]: c for c in CASES}
ORDER_CASES = ('prior_plain_eigen', 'collinear_ml59', 'collinear_ml60', 'first_K4_ml81')      # run again with the lanes reversed / shuffled
KIND_OF_FORM = {'sqrt': ('H', 'g', 'c'), 'eigen': ('H', 'g', 'c')}
NOISE_FACTOR = R.NOISE_FACTOR
FLOOR = {g: R.FLOOR_FACTORS for g in ('first', 'prior', 'no_imu0', 'blind', 'enlarged', 'collinear')}      # (marg_ref.py: why)
FLOOR['second_new'] = R.FLOOR_PRIOR_ONLY

# the bound: prior_error(kind) <= bound_factor(launch form, kind, class) x E64(kind, class).  Smallest power of two with a factor two to
# spare over the worst measured ratio (MEASURED above); the 16-frame window sets a factor of its own on the emulator instead of
# everyone's.
M = R.M
M_CLASS = {('simt', 'H', 'enlarged'): 16}
# what the recorded mutations of the kernel produced on the emulator (tests/simt/README.md, "Mutations of ba_marg_kernel"):
# (mutation, case, H, g, c).  `eps` raised to 1e-6 is not in it: on these windows every kept pivot between 1e-8 and 1e-6 lies below the
# measured noise of A', so no float64 measure can tell the two cuts apart there; second_new_weak_pivot (one exact pivot of 1e-7) is the
# case that does, through rank_ok.
MUTATIONS = [
    ('kept diagonal x (1 + 1e-3)', 'prior_plain', 9.98e-4, 1.02e-10, 0.0),
    ('kept diagonal x (1 + 1e-3)', 'first_K6_ml17', 1.00e-3, 1.56e-13, 0.0),
    ('kept diagonal x (1 + 1e-3)', 'first_K6_ml64', 1.00e-3, 1.01e-13, 6.67e-16),
    ('rank-ml update stops at ml - 1', 'prior_plain', 3.78e-2, 4.22e-6, 0.0),
    ('rank-ml update stops at ml - 1', 'first_K6_ml17', 2.85e-2, 1.95e-5, 1.12e-8),
    ('rank-ml update stops at ml - 1', 'first_K6_ml64', 2.66e-2, 3.20e-5, 3.80e-8),
    ('sqrt(rho1) dropped from one Jacobian', 'prior_plain', 5.97e-5, 1.53e-5, 0.0),
    ('sqrt(rho1) dropped from one Jacobian', 'first_K6_ml17', 1.48e-1, 1.39e-4, 8.91e-8),
    ('sqrt(rho1) dropped from one Jacobian', 'first_K6_ml64', 7.80e-1, 3.42e-3, 1.41e-5),
    ('gradient left out of the last tile', 'prior_plain', 6.76e-6, 2.15e-2, 5.52e2),
    ('gradient left out of the last tile', 'first_K6_ml17', 8.77e-5, 4.96e1, 2.64e3),
    ('gradient left out of the last tile', 'first_K6_ml64', 3.94e-5, 4.30e1, 2.13e3),
    ("b' taken before the second stage", 'prior_plain', 6.76e-6, 2.88e-1, 4.92e5),
    ("b' taken before the second stage", 'first_K6_ml17', 8.77e-5, 3.89e2, 2.93e5),
    ("b' taken before the second stage", 'first_K6_ml64', 3.94e-5, 2.86e2, 3.05e5),
    # the eigen form (block elimination, Schur product through LDS): H is untouched, g is measured along the determined eigenvectors
    ("eigen form: last term of b''s Schur dot product dropped", 'prior_plain_eigen', 8.61e-5, 1.58e-3, 3.24e-3),
    ("eigen form: last term of b''s Schur dot product dropped", 'first_K4_ml8_eigen', 3.04e-5, 5.88e-4, 4.77e-7),
    ("eigen form: last term of b''s Schur dot product dropped", 'enlarged_K16_eigen', 4.25e-2, 5.04e-4, 2.43e-6),
    ("eigen form: b' of the last 16 columns taken before the Schur product", 'prior_plain_eigen', 8.61e-5, 2.53e1, 3.08e4),
    ("eigen form: b' of the last 16 columns taken before the Schur product", 'first_K4_ml8_eigen', 3.04e-5, 6.72e1, 4.85e3),
    ("eigen form: b' of the last 16 columns taken before the Schur product", 'enlarged_K16_eigen', 4.25e-2, 6.74e2, 1.30e6),
]


def bound_factor(launch, kind, group):
    return M_CLASS.get((launch, kind, group), M[launch][kind])


# --------------------------------------------------------------------------------------------------- reference, once per session
@functools.lru_cache(maxsize=None)
def reference(window):
    """(window pinned at its state, flag, 80-bit reference, ambiguity of its cut, {form: prior_error of the float64 yardstick})."""
    build, flag = WINDOWS[window]
    at = build()
    forms = tuple(sorted({c[2] for c in CASES if c[1] == window} | {'sqrt'}))
    ref = R.reference_prior(at, flag, np.longdouble, forms)
    if ref is None:
        return at, flag, None, None, None
    assert R.has_gap(ref), (window, ref['pivots'].min(), ref['left'])      # a pivot of the dropped block near the cut: not a test of the kernel
    r64 = R.reference_prior(at, flag, np.float64, forms)
    amb = R.cut_ambiguity(ref, r64, NOISE_FACTOR)
    e64 = {f: R.prior_error(r64[f], ref, amb, form=f) for f in forms}
    if group_of(window) in PINV_GROUPS:
        # the kernel has to take the reference's eigen pseudo-inverse here (marginalization_factor.cpp:272-283): the yardstick is the worst
        # of three float64 implementations -- the pivoted elimination above and that pseudo-inverse from a Jacobi and from a tridiagonal
        # eigen-solver (the reference's kind)
        for solver in ('pinv_jacobi', 'pinv_lapack'):
            yard = R.reference_prior(at, flag, np.float64, forms, elimination=solver)
            for f in forms:
                other = R.prior_error(yard[f], ref, amb, form=f)
                for k in KIND_OF_FORM[f]:
                    e64[f][k] = max(e64[f][k], other[k])
    return at, flag, ref, amb, e64


SPLIT = 10          # a window is never bounded more than 10 x above its own float64 loss, whatever the worst window of its class loses


@functools.lru_cache(maxsize=None)
def _class_E64():
    out = {}
    for window in WINDOWS:
        e64 = reference(window)[4]
        for f in (e64 or {}):
            for k in KIND_OF_FORM[f]:
                key = (k, group_of(window))
                out[key] = max(out.get(key, FLOOR[key[1]]), e64[f][k])
    return out


def E64(kind, window):
    """The float64 loss the bound is a multiple of: the largest over the windows of the class (no device takes part), but no more than
    SPLIT x the window's own (the worse of its forms) for H -- one ill-conditioned window does not set everyone's bound -- and no less
    than FLOOR[class].  g and c keep the class's: a window's own float64 g / c is zero whenever its run happens to stay inside the cut's
    allowance, which says nothing about its conditioning."""
    g = group_of(window)
    own = max(e[kind] for f, e in reference(window)[4].items() if kind in KIND_OF_FORM[f])
    cls = _class_E64()[(kind, g)]
    return max(FLOOR[g], min(cls, SPLIT * own) if kind == 'H' else cls)


def run_case(h, case):
    _, window, form, _ = CASE[case]
    at, flag, ref, amb, _ = reference(window)
    h.ba_set_marg_mode(EIGEN if form == 'eigen' else SQRT)
    try:
        st, sm, pr = h.ba_optimize(at, flag)
        info = h.ba_marg_info(0)
    finally:
        h.ba_set_marg_mode(SQRT)
    assert sm['status'] == 0 and sm['num_iterations'] == 0
    return st, pr, info


def check_case(h, case, launch):
    _, window, form, path = CASE[case]
    _, _, ref, amb, _ = reference(window)
    st, pr, info = run_case(h, case)
    assert pr is not None and info['valid'] == 1
    assert {k: info[k] for k in path} == path, (case, info)
    e = R.prior_error(pr, ref, amb, state=st, form=form)
    ratios = {k: e[k] / E64(k, window) for k in KIND_OF_FORM[form]}
    print(f"[marg_scale] {launch} {case}: {R.describe(e)}; ratio to E64 " + ', '.join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert e['same_shape'] and info['n'] == ref['n'] and info['m'] == ref['m'], case
    assert e['x0_equal'], case
    assert e['rank_ok'] and e['rank'] <= ref['n'], (case, e['rank'], e['r_min'])
    if form == 'sqrt':
        assert e['tail_zero'] and info['eig2'] >> 16 == e['rank'], case
    for k, v in ratios.items():
        where = f" at {e['H_pair'][0]} x {e['H_pair'][1]}" if k == 'H' else ''
        assert v <= bound_factor(launch, k, group_of(window)), (f"{case}: {k} = {e[k]:.3e}{where} is {v:.3g} x E64 = "
                                                               f"{E64(k, window):.3e} (bound {bound_factor(launch, k, group_of(window))} x)")


def check_absent(h):
    """MARGIN_SECOND_NEW without pose K - 2 in the prior (estimator.cpp:935-936): the old prior stays, bit for bit -- the library
    reports NO new prior and the caller keeps the one it has."""
    at, flag, ref, _, _ = reference('second_new_absent')
    assert ref is None and (B.KIND_POSE, at['pose'].shape[0] - 2) not in at['prior']['blocks']
    before = {k: np.array(v, copy=True) for k, v in at['prior'].items() if k in ('J0', 'r0')}
    _, sm, pr = h.ba_optimize(at, flag)
    info = h.ba_marg_info(0)
    assert sm['status'] == 0 and pr is None and info['valid'] == 0 and info['word'] == 0
    assert all(np.array_equal(at['prior'][k], v) for k, v in before.items())


RAGGED = (('prior_plain', OLD), ('second_new_rank2', SECOND_NEW), ('blind_K11_ml60', NONE), ('second_new_full', OLD))


def check_ragged_batch(h):
    """Four K = 11 windows of different landmark counts and flags in ONE batch: every window equals its single-window run bit for bit
    (the per-window strides of mout / miout / scratch), the window without a flag reports no prior."""
    probs = [reference(w)[0] for w, _ in RAGGED]
    flags = [f for _, f in RAGGED]
    assert len({len(p['inv_depth']) for p in probs}) >= 3
    h.ba_upload(probs, flags)
    h.ba_run_async()
    _, sm, pri = h.ba_download()
    infos = [h.ba_marg_info(w) for w in range(len(probs))]
    for w, (p, f) in enumerate(zip(probs, flags)):
        assert sm[w]['status'] == 0
        if f == NONE:
            assert pri[w] is None and infos[w]['valid'] == 0 and infos[w]['word'] == 0
            continue
        _, _, one = h.ba_optimize(p, f)
        assert h.ba_marg_info(0) == infos[w], w
        assert one['blocks'] == pri[w]['blocks'] and one['n'] == pri[w]['n'] and one['m'] == pri[w]['m']
        assert np.array_equal(one['J0'], pri[w]['J0']) and np.array_equal(one['r0'], pri[w]['r0']), w
        assert all(np.array_equal(a, c) for a, c in zip(one['x0'], pri[w]['x0'])), w


# --------------------------------------------------------------------------------------------------- no device
def test_every_path_word_value_is_reached_by_a_case():
    """Coverage is asserted FROM THE TABLE (each case asserts its own word when it runs): every value of every field of the path word
    has a case.  Not reachable by any window, hence in no case: the certificate 'not evaluated' (it needs md outside 1 .. 16; md is 15,
    or 6 without speed-bias 0) -- DESIGN.md names it."""
    reached = {k: {c[3][k] for c in CASES} for k in ('stage1', 'cert', 'schur', 'stage2')}
    assert reached['stage1'] == set(ba.MARGPATH_STAGE1) - {None}
    assert reached['cert'] == set(ba.MARGPATH_CERT) - {None}
    assert reached['schur'] == set(ba.MARGPATH_SCHUR)
    assert reached['stage2'] == set(ba.MARGPATH_STAGE2) - {None}
    assert {c[1] for c in CASES} | {'second_new_absent'} == set(WINDOWS)


def test_bound_conditions():
    """Conditions on the bound, not measurements: (1) every recorded mutation of the kernel, on every window it was run on, exceeds the
    bound of at least one kind by a factor two -- M x E64 stays below half of what the mutation produced there, on the emulator and on
    the MI355X bound alike; (2) every window's own float64 loss is within M / 2 x E64 of its class, so the table hides no case behind
    its worst one."""
    for launch in M:
        for name, case, *err in MUTATIONS:
            g = group_of(CASE[case][1])
            assert max(v / (bound_factor(launch, k, g) * E64(k, CASE[case][1])) for k, v in zip('Hgc', err)) >= 2, (launch, name, case)
    for window in WINDOWS:
        e64 = reference(window)[4]
        for f in (e64 or {}):
            for k in KIND_OF_FORM[f]:
                g = group_of(window)
                assert e64[f][k] <= min(bound_factor(launch, k, g) for launch in M) / 2 * E64(k, window)


# --------------------------------------------------------------------------------------------------- emulator
@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_emulated_case(simt_handle, case):
    check_case(simt_handle, case, 'simt')


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
@pytest.mark.parametrize("case", ORDER_CASES)
def test_emulated_case_under_other_fiber_orders(simt_handle, monkeypatch, case, order):
    monkeypatch.setenv("SIMT_ORDER", order)
    check_case(simt_handle, case, 'simt')


def test_emulated_second_new_without_the_pose_keeps_the_old_prior(simt_handle):
    check_absent(simt_handle)


def test_emulated_ragged_batch(simt_handle):
    check_ragged_batch(simt_handle)


# --------------------------------------------------------------------------------------------------- MI355X
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c[0] for c in CASES])
def test_gpu_case(handle, case):
    check_case(handle, case, 'gpu')


@pytest.mark.gpu
def test_gpu_second_new_without_the_pose_keeps_the_old_prior(handle):
    check_absent(handle)


@pytest.mark.gpu
def test_gpu_ragged_batch(handle):
    check_ragged_batch(handle)
