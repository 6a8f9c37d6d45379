"""Reference for the marginalization prior, entry by entry in the prior's own scale (helper module of tests/test_marg_scale.py; no
tests in here).

`reference_prior` evaluates the factors a marginalization consumes (oracle.ba_numpy._marg_factors: float64, as ba_step_ref._gram takes
its Jacobian), assembles the normal equations (A, b) in the requested number format and removes the dropped block by a diagonally
pivoted elimination: the largest remaining diagonal entry of the dropped block is the next pivot, and the elimination STOPS when that
entry is no longer above the reference's eps = 1e-8 (marginalization_factor.h:70) -- the generalised Schur complement, which is what
the reference's eigen pseudo-inverse with its `lambda > eps` cut computes when the spectrum of the dropped block has a gap there, and
the plain Schur complement when the block is positive definite.  The pivots come back so that a test can assert the gap.  The kept
system (A*, b*) is then factored as the library documents it (include/vinsgpu.h vg_ba_set_marg_mode): the diagonally pivoted Cholesky
factor cut at eps (largest remaining diagonal, lowest index on ties) and the eigen form S^1/2 V^T from a cyclic Jacobi
eigen-decomposition.  With np.longdouble (80-bit) this is the reference, with np.float64 the yardstick: what a correct float64
implementation of the documented steps loses.  Nothing is shared with the kernel's block elimination or with
oracle.ba_numpy.marginalize / schur_extended.

`prior_error` measures a prior (J0, r0) against the reference in the prior's OWN scale, s_i = sqrt(A*_ii):
    H   max_ij |J0^T J0 - A*|_ij / (s_i s_j)       (and which pair of block kinds holds the maximum)
    g   max_i  |J0^T r0 - b*|_i / (s_i rho)        rho = 2-norm of the stacked residuals of the marginalised factors
    c   | |r0|^2 - |r0*|^2 | / rho^2
so that an entry of scale 0.35 is not measured against a neighbour of scale 1e7."""
import numpy as np

from oracle import ba_numpy as B

EPS = 1e-8            # marginalization_factor.h:70
GAP_KEPT, GAP_DROPPED = 1e-5, 1e-10      # a case of the table must have no pivot of the dropped block in between
# the bound of a kind: prior_error(kind) <= M[launch form][kind] x the float64 loss (tests/test_marg_scale.py: how it was measured);
# the float64 loss is floored: the reference takes the ORACLE's float64 residuals and Jacobians as exact, the library evaluates the factors
# itself and reproduces them to the 1e-9 relative that tests/test_ba_gpu.py::test_factor_parity asserts; J^T J and J^T r are quadratic in
# them.  A MARGIN_SECOND_NEW window evaluates no factor but the (linear) prior: there the floor is ~64 u.
M = {'simt': dict(H=8, g=16, c=4), 'gpu': dict(H=8, g=4, c=8)}
FLOOR_FACTORS, FLOOR_PRIOR_ONLY = 2e-9, 1e-14
NOISE_FACTOR = 8      # a pivot of the kept block is determined when it exceeds eps + 8 x the float64 restatement's noise there
KINDS = ('position', 'rotation', 'velocity', 'bias_a', 'bias_g', 'extrinsic', 'td')
_ORDER = {B.KIND_POSE: 0, B.KIND_SB: 1, B.KIND_EX: 2, B.KIND_TD: 3, B.KIND_LM: 4}


def state_at(prob):
    """The state a window with max_iters = 0 is marginalised at: its own, after the gauge fix."""
    return B.double2vector(prob, B.state_of(prob))


def column_kinds(blocks):
    """Kind of every tangent column of the kept blocks [(kind, index)...]."""
    out = []
    for kind, _ in blocks:
        out += {B.KIND_POSE: ['position'] * 3 + ['rotation'] * 3, B.KIND_SB: ['velocity'] * 3 + ['bias_a'] * 3 + ['bias_g'] * 3,
                B.KIND_EX: ['extrinsic'] * 6, B.KIND_TD: ['td']}[kind]
    return out


# --------------------------------------------------------------------------------------------------- linear algebra in `dtype`
def schur_pivoted(A, b, m, eps=EPS):
    """Generalised Schur complement of the leading m x m block of (A, b): diagonally pivoted elimination, stopped when the largest
    remaining diagonal entry of the block is <= eps.  Returns (A*, b*, pivots taken, diagonal entries left behind)."""
    n = A.shape[0]
    aug = np.concatenate([0.5 * (A + A.T), b[:, None]], axis=1)
    alive = np.ones(m, bool)
    taken = []
    while alive.any():
        d = np.where(alive, np.diagonal(aug)[:m], -np.inf)
        k = int(np.argmax(d))
        if not d[k] > eps:
            break
        taken.append(d[k])
        col = aug[k, :n].copy()
        aug -= np.outer(col / d[k], aug[k])
        alive[k] = False
    left = np.diagonal(aug)[:m][alive]
    As = aug[m:, m:n]
    return 0.5 * (As + As.T), aug[m:, n].copy(), np.array(taken, A.dtype), np.array(left, A.dtype)


def schur_pinv(A, b, m, eps=EPS, solver='jacobi'):
    """The reference's own elimination (marginalization_factor.cpp:272-283) in A's dtype: Amm^+ from the eigen-decomposition of the
    dropped block with the lambda > eps cut, A* = Arr - Arm Amm^+ Amr.  The yardstick of the windows whose dropped block is rank
    deficient: there the kernel has to take this route (the certificate of its eliminations fails).  solver = 'lapack' (float64 only):
    numpy.linalg.eigh, a tridiagonal solver like the reference's SelfAdjointEigenSolver -- absolute accuracy u |Amm|, where Jacobi's is
    relative."""
    Amm = 0.5 * (A[:m, :m] + A[:m, :m].T)
    w, V = jacobi_eigh(Amm) if solver == 'jacobi' else np.linalg.eigh(Amm)
    keep = w > eps
    X = (V * np.where(keep, 1 / np.where(keep, w, 1), 0)) @ (V.T @ np.concatenate([A[:m, m:], b[:m, None]], axis=1))
    As = A[m:, m:] - A[m:, :m] @ X[:, :-1]
    return 0.5 * (As + As.T), b[m:] - A[m:, :m] @ X[:, -1], w[keep], w[~keep]


def sqrt_form(A, b, eps=EPS):
    """J0 = L^T, r0 = L^-1 b of the diagonally pivoted Cholesky factor of A (largest remaining diagonal, lowest index on ties), cut
    where no remaining diagonal exceeds eps: rows rank.. are zero.  `full` is the same factorisation carried on below the cut for as
    long as a pivot is positive (pivots, their columns, L^T, y): what cut_ambiguity() reads."""
    n = A.shape[0]
    Lc, y = np.zeros_like(A), np.zeros_like(b)
    d, alive = np.diagonal(A).copy(), np.ones(n, bool)
    rank, piv_val, piv_col = None, [], []
    for k in range(n):
        dd = np.where(alive, d, -np.inf)
        p = int(np.argmax(dd))
        if not dd[p] > eps and rank is None:
            rank = k
        if not dd[p] > 0:
            break
        piv = np.sqrt(dd[p])
        col = (A[:, p] - Lc[:, :k] @ Lc[p, :k]) / piv
        col[~alive] = 0
        col[p] = piv
        y[k] = (b[p] - y[:k] @ Lc[p, :k]) / piv
        Lc[:, k] = col
        d = d - col * col
        alive[p] = False
        piv_val.append(dd[p])
        piv_col.append(p)
    rank = len(piv_val) if rank is None else rank
    J0, r0 = Lc.T.copy(), y.copy()
    J0[rank:], r0[rank:] = 0, 0
    return dict(J0=J0, r0=r0, rank=rank, full=dict(pivots=np.array(piv_val, A.dtype), cols=np.array(piv_col, int), Lt=Lc.T.copy(), y=y))


def jacobi_eigh(A, max_sweeps=40):
    """Cyclic two-sided Jacobi in A's own dtype: (eigenvalues, eigenvectors as columns), not sorted."""
    A = A.copy()
    n = A.shape[0]
    V = np.eye(n, dtype=A.dtype)
    u = np.finfo(A.dtype).eps
    floor = u * 1e-6 * np.sqrt((A * A).sum())
    for _ in range(max_sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if not abs(apq) > u * np.sqrt(abs(A[p, p] * A[q, q])) + floor:
                    continue
                rotated = True
                theta = (A[q, q] - A[p, p]) / (2 * apq)
                t = np.sign(theta) / (abs(theta) + np.sqrt(theta * theta + 1)) if theta != 0 else A.dtype.type(1)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * rp - s * rq, s * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    return np.diagonal(A).copy(), V


def eigen_form(A, b, eps=EPS):
    """The reference's J0 = S^1/2 V^T, r0 = S^-1/2 V^T b (marginalization_factor.cpp:285-296), rows by ascending eigenvalue."""
    w, V = jacobi_eigh(A)
    order = np.argsort(w, kind='stable')
    w, V = w[order], V[:, order]
    keep = w > eps
    S = np.where(keep, w, 0)
    Sinv = np.where(keep, 1 / np.where(keep, w, 1), 0)
    return dict(J0=np.sqrt(S)[:, None] * V.T, r0=np.sqrt(Sinv) * (V.T @ b), rank=int(keep.sum()), w=w, V=V)


# --------------------------------------------------------------------------------------------------- the reference
def reference_prior(prob_at, flag, dtype=np.longdouble, forms=('sqrt', 'eigen'), elimination='pivoted'):
    """The prior a marginalization of `prob_at` (at its own state) with `flag` must produce, in `dtype`.  None when the reference leaves
    the old prior untouched (MARGIN_SECOND_NEW without pose K - 2 in the prior).  dict(A, b = the kept system, n, m, blocks = kept
    blocks re-labelled for the slid window, unslid = the same under their labels in this window, x0, rho, pivots, left = pivots taken / diagonal left behind in the dropped block,
    sqrt / eigen = dict(J0, r0, rank)).  elimination = 'pinv_jacobi' / 'pinv_lapack': the dropped block leaves by schur_pinv instead (yardsticks only)."""
    K = prob_at['pose'].shape[0]
    pr = prob_at.get('prior')
    if flag == B.MARGIN_SECOND_NEW and (pr is None or (B.KIND_POSE, K - 2) not in pr['blocks']):
        return None
    st = state_at(prob_at)
    facs = B._marg_factors(prob_at, st, flag)
    if not facs:
        return None
    dropped, seen = set(), set()
    for (_, _, blocks, drop) in facs:
        seen.update(blocks)
        dropped.update(blocks[p] for p in drop)
    key = lambda blk: (_ORDER[blk[0]], blk[1])
    drop_list, keep_list = sorted(dropped, key=key), sorted(seen - dropped, key=key)
    col, pos = {}, 0
    for blk in drop_list + keep_list:
        col[blk] = pos
        pos += B.LSIZE[blk[0]]
    m = sum(B.LSIZE[blk[0]] for blk in drop_list)
    A, b = np.zeros((pos, pos), dtype), np.zeros(pos, dtype)
    rho2 = dtype(0)
    for (rf, Js, blocks, _) in facs:
        cols = np.concatenate([np.arange(col[blk], col[blk] + B.LSIZE[blk[0]]) for blk in blocks])
        J = np.hstack(Js).astype(dtype)
        r = np.asarray(rf).astype(dtype)
        A[np.ix_(cols, cols)] += J.T @ J
        b[cols] += J.T @ r
        rho2 += r @ r
    if elimination == 'pivoted':
        As, bs, pivots, left = schur_pivoted(A, b, m)
    else:
        As, bs, pivots, left = schur_pinv(A, b, m, solver=elimination[5:])
    x0, new_blocks = [], []
    for (kind, i) in keep_list:
        x0.append(np.array(B.get_block(st, kind, i), float).copy())
        if kind in (B.KIND_POSE, B.KIND_SB):
            i = i - 1 if (flag == B.MARGIN_OLD or i == K - 1) else i
        new_blocks.append((kind, i))
    out = dict(A=As, b=bs, n=pos - m, m=m, blocks=new_blocks, unslid=keep_list, x0=x0, rho=np.sqrt(rho2), pivots=pivots, left=left)
    if 'sqrt' in forms:
        out['sqrt'] = sqrt_form(As, bs)
    if 'eigen' in forms:
        out['eigen'] = eigen_form(As, bs)
    return out


def has_gap(ref):
    """Every pivot taken in the dropped block >= 1e-5, everything left behind <= 1e-10: the case tests the kernel, not the cut."""
    return bool(np.all(ref['pivots'] >= GAP_KEPT) and np.all(ref['left'] <= GAP_DROPPED))


# --------------------------------------------------------------------------------------------------- the measure
def _forced_diagonals(A, b, cols):
    """Pivoted factorisation of A in its own dtype with the pivot order PRESCRIBED: row k = the remaining diagonal before step k
    (rows after a breakdown -- a pivot that is not positive -- are NaN)."""
    n = A.shape[0]
    Lc = np.zeros_like(A)
    d = np.diagonal(A).copy()
    out = np.full((len(cols), n), np.nan, A.dtype)
    for k, p in enumerate(cols):
        out[k] = d
        if not d[p] > 0:
            break
        col = (A[:, p] - Lc[:, :k] @ Lc[p, :k]) / np.sqrt(d[p])
        col[cols[:k]] = 0
        Lc[:, k] = col
        d = d - col * col
    return out


def cut_ambiguity(ref, ref64, factor):
    """What the eps cut of the kept block leaves undetermined for a float64 implementation.  The rounding noise of the remaining
    diagonal is MEASURED, not guessed: the float64 restatement's kept system is factored with the 80-bit run's pivot order, and
    nu_k = the largest |d64 - d80| over the columns still unpivoted at step k (no device takes part).  Step k (pivot pi_k) is
    DETERMINED when pi_k > eps + factor nu_k: every implementation whose noise is within `factor` times the restatement's takes it.
    The steps from the first one that is not are ambiguous: whether their pivots come out above eps is decided by rounding (they are
    the window's gauge directions, exactly or nearly), and a prior may keep any part of them.  After the r determined steps the
    residual system (A_r, b_r) lives on the columns not pivoted so far, and whatever is cut of it
        - changes J0^T r0 on those columns only, by at most |b_r|_i + sqrt(A_r,ii c_amb)   (Cauchy-Schwarz on the kept part L_S y_S),
        - leaves |r0|^2 inside [c_det, c_det + c_amb],   c_det = sum of y_k^2 over the determined steps, c_amb = b_r^T A_r^+ b_r.
    The EIGEN form cuts eigen-directions, not columns.  Where both runs carry the eigen form, the same is done with the (ascending)
    eigenvalues: lambda_k is determined when it exceeds eps + factor x the larger of the largest |w64 - w80| among the eigenvalues not
    above it and the diagonal noise nu at the first ambiguous pivot, the
    error of J0^T r0 is then measured along the determined eigenvectors only, each component in ITS scale sqrt(lambda_k) rho (since
    |v^T b*| <= sqrt(lambda) rho) and less what a cut direction, tilted by the same noise, leaks onto it (`leak`: it falls off as
    1 / (lambda_k - lam), so only the eigenvalues next to the ambiguous ones are spared), and |r0|^2 lies in [sum over the determined
    (v^T b*)^2 / lambda less that leak, c_hi].
    Returns dict(r_min = number of determined steps, g_slack = the per-column allowance (absolute), c_lo, c_hi[, eig = dict(V, w =
    the determined eigenpairs, c_lo)])."""
    L = np.longdouble
    f = ref['sqrt']['full']
    cols, piv = f['cols'], f['pivots'].astype(L)
    Lt, y = f['Lt'].astype(L), f['y'].astype(L)
    diag = np.diagonal(ref['A']).astype(L)
    d80 = diag[None, :] - np.concatenate([np.zeros((1, ref['n']), L), np.cumsum(Lt[:len(cols)] ** 2, axis=0)])[:len(cols)]
    d64 = _forced_diagonals(ref64['A'], ref64['b'], cols).astype(L)
    r, nu = len(cols), L(0)
    for k in range(len(cols)):
        live = np.ones(ref['n'], bool)
        live[cols[:k]] = False
        nu = np.abs(d64[k] - d80[k])[live].max()
        if not piv[k] > EPS + factor * nu:          # (NaN after a float64 breakdown: ambiguous)
            r = k
            break
    c_det, c_amb = y[:r] @ y[:r], y[r:] @ y[r:]
    free = np.ones(ref['n'], bool)
    free[cols[:r]] = False
    A_r = np.maximum(diag - (Lt[:r] ** 2).sum(axis=0), 0)
    b_r = ref['b'].astype(L) - Lt[:r].T @ y[:r]
    out = dict(r_min=r, g_slack=np.where(free, np.abs(b_r) + np.sqrt(A_r * c_amb), 0), c_lo=c_det, c_hi=c_det + c_amb)
    if 'eigen' in ref and 'eigen' in ref64:
        w80, w64, V = ref['eigen']['w'].astype(L), ref64['eigen']['w'].astype(L), ref['eigen']['V'].astype(L)
        nu_e = np.maximum(np.maximum.accumulate(np.abs(w64 - w80)), nu if np.isfinite(nu) else np.inf)      # (never below the pivots' noise)
        det = w80 > EPS + factor * nu_e
        det &= np.logical_and.accumulate(det[::-1])[::-1]          # (everything above a determined eigenvalue's first ambiguous neighbour)
        vb = V[:, det].T @ ref['b'].astype(L)
        # a direction u the eigen form cuts has u^T A* u <= lam = eps + factor nu, so |u^T b*| <= sqrt(lam c_hi); a float64 u is tilted
        # towards the determined v_k by sin <= factor nu / (lambda_k - lam): what leaks onto v_k of at most q such directions
        q = int((~det).sum())
        lam = EPS + factor * (nu_e[~det].max() if q else L(0))
        gap = np.maximum(w80[det] - lam, np.finfo(np.float64).tiny)
        leak = np.minimum(1, factor * (lam - EPS) / gap) * np.sqrt(q * lam * out['c_hi'])
        out['eig'] = dict(V=V[:, det], w=w80[det], c_lo=(vb * vb / w80[det]).sum() - 2 * np.sqrt((leak * leak).sum() * out['c_hi']), leak=leak)
    return out


def prior_error(got, ref, amb=None, state=None, form='sqrt'):
    """`got` (dict(J0, r0[, n, m, blocks, x0]): a device prior, or ref64[form]) against the 80-bit `ref` in the prior's own scale.
    Returns dict(H, H_pair = the pair of block kinds with the largest H, H_by_pair, rank = non-zero rows of J0, tail_zero = rows
    rank.. of J0 / r0 are exactly zero, same_shape = blocks / n / m agree, x0_equal = x0 is bit-equal to `state`'s blocks (None when not
    asked)) and, when `amb` = cut_ambiguity(...) is given, g and c beyond what the cut leaves undetermined (g_raw, c_raw: without that
    allowance, c_raw against the 80-bit square-root form) plus rank_ok = no determined direction was cut."""
    L = np.longdouble
    As, bs = ref['A'].astype(L), ref['b'].astype(L)
    diag = np.diagonal(As)
    assert np.all(diag > 0), "a kept column without information: the scale s_i = sqrt(A*_ii) is undefined"
    s = np.sqrt(diag)
    rho = L(ref['rho'])
    J0, r0 = np.asarray(got['J0']).astype(L), np.asarray(got['r0']).astype(L)
    EH = np.abs(J0.T @ J0 - As) / np.outer(s, s)
    kinds = np.array(column_kinds(ref['blocks']))
    by_pair = {}
    for a in KINDS:
        for c in KINDS[KINDS.index(a):]:
            ia, ic = np.flatnonzero(kinds == a), np.flatnonzero(kinds == c)
            if ia.size and ic.size:
                by_pair[(a, c)] = float(max(EH[np.ix_(ia, ic)].max(), EH[np.ix_(ic, ia)].max()))
    nz = np.abs(J0).sum(axis=1) > 0
    rank = int(nz.sum())
    out = dict(H=float(EH.max()), H_pair=max(by_pair, key=by_pair.get), H_by_pair=by_pair, rank=rank,
               tail_zero=bool(not nz[rank:].any() and not np.any(r0[rank:] != 0)),
               same_shape=bool(got.get('n', ref['n']) == ref['n'] and got.get('m', ref['m']) == ref['m']
                               and got.get('blocks', ref['blocks']) == ref['blocks']), x0_equal=None)
    if amb is not None:
        cc = r0 @ r0
        dg = J0.T @ r0 - bs
        if form == 'sqrt':
            slack, c_lo = amb['g_slack'], amb['c_lo']
            g = (np.maximum(np.abs(dg) - slack, 0) / (s * rho)).max()
            r_min = amb['r_min']
        else:
            eg = amb['eig']
            slack, c_lo, r_min = np.zeros_like(s), eg['c_lo'], len(eg['w'])
            g = (np.maximum(np.abs(eg['V'].T @ dg) - eg['leak'], 0) / (np.sqrt(eg['w']) * rho)).max() if r_min else L(0)
            slack = slack + (eg['leak'] / (np.sqrt(eg['w']) * rho)).max() * s * rho if r_min else slack
        cref = ref[form]['r0'].astype(L)
        out.update(g=float(g), g_raw=float((np.abs(dg) / (s * rho)).max()),
                   c=float(max(c_lo - cc, cc - amb['c_hi'], 0) / (rho * rho)), c_raw=float(abs(cc - cref @ cref) / (rho * rho)),
                   c_slack=float((amb['c_hi'] - c_lo) / (rho * rho)), g_slack=float((slack / (s * rho)).max()),
                   r_min=r_min, rank_ok=bool(rank >= r_min))
    if state is not None:
        want = [np.asarray(B.get_block(state, k, i), float).ravel() for (k, i) in ref['unslid']]
        out['x0_equal'] = bool(len(want) == len(got['x0']) and all(np.array_equal(np.asarray(a).ravel(), w) for a, w in zip(got['x0'], want)))
    return out


def describe(e):
    t = f"H {e['H']:.2e} at {e['H_pair'][0]} x {e['H_pair'][1]}, rank {e['rank']}"
    if 'g' in e:
        t += (f", g {e['g']:.2e} (before the cut's allowance of {e['g_slack']:.1e}: {e['g_raw']:.2e}), c {e['c']:.2e} (allowance {e['c_slack']:.1e}, "
              f"against the 80-bit cut: {e['c_raw']:.2e}), determined rank {e['r_min']}")
    return t
