"""vg_imu_preintegrate (imu_preint_kernel, csrc/imu_step.h) against an 80-bit restatement of IntegrationBase::push_back, every
field in its own scale (tests/imu_ref.py: reference, record_error, case table, yardstick).

The older checks hold a whole 15x15 field to 1e-11 x its largest entry; the covariance's blocks differ by up to 13 orders of
magnitude, so its small blocks -- the gyro- and accelerometer-bias blocks, the LARGE entries of the information matrix -- could be
wrong by any factor.  Here the covariance is measured entry by entry against sqrt(C_ii C_jj), the jacobian per 3x3 block.

The bound.  e64(case) = record_error of the float64 oracle (oracle/ba_numpy.Preintegration) against the 80-bit reference; E64 = its
largest value over the case table, one per field kind (covariance, jacobian, state); the device must stay within M * E64.  M is
the smallest power of two that the worst measured ratio of emulator and MI355X stays under with a factor 2 to spare (MEASURED).
Every edit of test_each_edit_exceeds_twice_the_bound must produce more than 2 * M * E64 in some case and field.

The emulated half (`not gpu`) runs everything the GPU half runs: nothing is cut."""
import numpy as np
import pytest

import conftest
import imu_ref as R

M = R.M
MEASURED = """E64 (no device involved): covariance 3.91e-15 (n120_dt0.1), jacobian 2.84e-15 (n120_dt0.1), state 6.12e-16 (a ragged interval);
e64 over the named cases with samples: 2.9e-16 .. 3.9e-15 / 1.5e-16 .. 2.8e-15 / 9.1e-17 .. 5.5e-16
worst record_error / E64 per field kind           CPU fiber emulator          MI355X
                                                  covar. jacob. state         covar. jacob. state
    n0                                                0.00  0.00  0.00         0.00  0.00  0.00
    n1                                                0.06  0.06  0.16         0.10  0.06  0.16
    n2                                                0.07  0.09  0.21         0.07  0.05  0.17
    n20                                               0.23  0.14  0.17         0.23  0.10  0.17
    n64                                               0.51  0.38  0.47         0.48  0.38  0.47
    n7_dt4.9ms                                        0.19  0.10  0.24         0.19  0.10  0.24
    n120_dt0.1                                        0.96  1.00  0.61         1.00  1.00  0.70
    varying_dt                                        0.30  0.15  0.31         0.30  0.17  0.27
    dt0_sample                                        0.17  0.09  0.38         0.17  0.09  0.38
    gyro_equals_bias                                  0.11  0.08  0.15         0.12  0.08  0.23
    zero_biases                                       0.39  0.10  0.20         0.39  0.10  0.03
    fast_rotation                                     0.56  0.34  0.42         0.63  0.34  0.70
    noise_zero                                        0.00  0.13  0.16         0.00  0.13  0.22
    repropagated                                      0.20  0.25  0.21         0.20  0.25  0.35
    dt0_sample, continued from the record before it   0.17  0.08  0.14         0.17  0.08  0.22
    ragged (70 intervals)                             0.35  0.25  0.65         0.35  0.25  0.92
  resident sequences (tests/seq_imu_model.check_record, every test of test_seq_imu_simt.py / test_seq_imu_gpu.py; E64 = the larger
  of the table's and the record's own e64 -- the 1.00s are records the device gives bit for bit like the oracle, 21 samples of 0.5 s)
    new record                                        1.01  1.00  0.90         1.00  1.00  1.22
    merged record vs the concatenated list            1.00  1.00  1.00         1.00  1.00  1.00
    merged record vs the 80-bit continuation          1.00  1.00  1.00         1.00  1.00  1.00
The worst ratio is 1.22 (MI355X, delta_v of a sequence's new record): M = 4 is the smallest power of two that leaves a factor 2
(2 would not: 2 x 1.22 > 2).  The kernel contracts to FMAs and sums k ascending; nothing here needs more than the oracle loses.
mutation condition, largest record_error over the cases per edit; 2 * M * E64 = 3.1e-14 / 2.3e-14 / 4.9e-15:
    Rr_normalised            1.6e-4 (covariance), 7.0e-5 (jacobian), 4.8e-5 (state), all n120_dt0.1; on n20 2.2e-11 / 9.7e-10 / 8.6e-10
    V_p_gyr1_doubled         7.8e-4 (covariance, n1); on n20 2.7e-5
    F_p_bg_sign              2.0 (jacobian, n1), 5.4e-7 (covariance, n120_dt0.1); on n20 7.7e-3 / 3.6e-9
    gyr_w_for_acc_w          1.0 (covariance, n1)
    F_theta_theta_identity   0.51 (jacobian), 0.11 (covariance), both n120_dt0.1; on n20 2.9e-3 / 7.2e-5
    cov_bg_entry             1.0e-9 (covariance, every case with noise)"""

ORDER = [n for n in R.CASES if n not in ('n0', 'noise_zero')]
ORDER.insert(3, 'n0')                                              # the empty interval in the middle of the batch


@pytest.fixture(scope="session")
def E64():
    return R.yardstick()


def _run(h, names):
    cs = [R.CASES[n] for n in names]
    assert len({c['noise'] for c in cs}) == 1
    return h.imu_preintegrate([c['iv'] for c in cs], [(c['ba'], c['bg']) for c in cs], cs[0]['noise'])


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ('sum_dt', 'lin_ba', 'lin_bg', 'delta_p', 'delta_q', 'delta_v', 'jacobian', 'covariance'))


def _held(got, ref, E64, what, tag, quiet=False):
    err = R.record_error(got, ref)
    assert R.exact_ok(err), (what, err)
    kinds = R.by_kind(err)
    if not quiet:
        print(f"record_error {tag} {what}: " + "  ".join(f"{k} {kinds[k]:.2e} = {kinds[k] / E64[k]:.2f} x E64" for k in R.KINDS))
    for key, kind in R.KIND_OF.items():
        assert err[key] <= M * E64[kind], f"{what} {key}: {err[key]:.3e} > {M} x {E64[kind]:.3e}"
    return kinds


# ---- the device checks, one body for the emulator and the MI355X ------------------------------------------------------------------
def check_cases(h, E64, tag):
    got = dict(zip(ORDER, _run(h, ORDER)))
    got['noise_zero'] = _run(h, ['noise_zero'])[0]
    for name in R.CASES:
        _held(got[name], R.reference(name), E64, name, tag)
    g = got['n0']                                                  # no samples: the identity record
    assert g['sum_dt'] == 0.0 and not g['delta_p'].any() and not g['delta_v'].any() and np.array_equal(g['delta_q'], [0, 0, 0, 1.0])
    assert np.array_equal(g['jacobian'], np.eye(15)) and not g['covariance'].any()
    assert got['n120_dt0.1']['sum_dt'] > 10.0
    # all four densities zero: covariance exactly 0, the jacobian what it is with noise
    c = R.CASES['noise_zero']
    noisy = h.imu_preintegrate([c['iv']], [(c['ba'], c['bg'])], R.NOISE)[0]
    assert not got['noise_zero']['covariance'].any() and noisy['covariance'].any()
    assert all(np.array_equal(got['noise_zero'][k], noisy[k]) for k in ('jacobian', 'delta_p', 'delta_q', 'delta_v'))


def check_dt0(h, E64, tag):
    """A repeated time stamp changes nothing but acc_0 / gyr_0: the record after it is the record before it, and the next sample
    continues that record from the repeated measurement."""
    c = R.CASES['dt0_sample']
    iv, bias = c['iv'], (c['ba'], c['bg'])
    assert iv[6][0] == 0.0
    before, at, after = h.imu_preintegrate([iv[:6], iv[:7], iv[:8]], [bias] * 3, c['noise'])
    for k in ('sum_dt', 'delta_p', 'delta_v', 'jacobian', 'covariance'):
        assert np.array_equal(before[k], at[k]), k                # F = I, V = 0: exact
    assert np.abs(before['delta_q'] - at['delta_q']).max() <= 2.0 ** -52      # (normalised once more)
    ref = R.integrate([iv[6], iv[7]], start=R.integrate(iv[:6], *bias, c['noise']), noise=c['noise'])
    _held(after, ref, E64, 'dt0_sample, continued from the record before it', tag)


def check_ragged(h, E64, tag, alone):
    rg = R.ragged()
    got = h.imu_preintegrate([r[0] for r in rg], [(r[1], r[2]) for r in rg], R.NOISE)
    worst = dict.fromkeys(R.KINDS, 0.0)
    for k in range(R.RAGGED_N):
        kinds = _held(got[k], R.ragged_reference(k), E64, f"ragged[{k}] ({len(rg[k][0]) - 1} samples)", tag, quiet=True)
        worst = {x: max(worst[x], kinds[x]) for x in worst}
    for k in R.RAGGED_EMPTY:
        assert np.array_equal(got[k]['jacobian'], np.eye(15)) and not got[k]['covariance'].any() and got[k]['sum_dt'] == 0.0
    for k in alone:
        one = h.imu_preintegrate([rg[k][0]], [(rg[k][1], rg[k][2])], R.NOISE)[0]
        assert _same(one, got[k]), k
    print(f"record_error {tag} ragged, worst / E64: " + "  ".join(f"{x} {worst[x] / E64[x]:.2f}" for x in worst))


def check_scratch_growth(h_a, h_b):
    """h_a, h_b: fresh handles.  A small call, one that grows the scratch, the small call again: bit-identical to a fresh handle's."""
    rg = R.ragged()
    small = lambda h: h.imu_preintegrate([rg[1][0], rg[2][0]], [(rg[1][1], rg[1][2]), (rg[2][1], rg[2][2])], R.NOISE)
    first = small(h_a)
    big = h_a.imu_preintegrate([r[0] for r in rg], [(r[1], r[2]) for r in rg], R.NOISE)
    again, fresh = small(h_a), small(h_b)
    for x, y, z, b in zip(first, again, fresh, big[1:3]):
        assert _same(x, y) and _same(x, z) and _same(x, b)


# ---- the reference and the bound themselves (no device) ---------------------------------------------------------------------------
def test_float64_restatement_is_the_oracle():
    """imu_ref.integrate in float64 repeats B.Preintegration bit for bit: the edits below are edits of the oracle."""
    for name, c in R.CASES.items():
        a, b = R.oracle64(c['iv'], c['ba'], c['bg'], c['noise']), R.integrate(c['iv'], c['ba'], c['bg'], c['noise'], dtype=np.float64)
        assert _same(a, b), name


def test_continuation_is_the_integration_of_the_whole_list():
    """the 80-bit reference started from its own record of the first part = the reference of the whole interval"""
    c = R.CASES['n64']
    for cut in (1, 20, 64):
        head = R.integrate(c['iv'][:cut + 1], c['ba'], c['bg'], c['noise'])
        whole = R.integrate([c['iv'][cut]] + c['iv'][cut + 1:], start=head, noise=c['noise'])
        for k in ('delta_p', 'delta_q', 'delta_v', 'jacobian', 'covariance'):
            assert np.array_equal(whole[k], R.reference('n64')[k]), (cut, k)
        assert whole['sum_dt'] == R.reference('n64')['sum_dt']
    # ... and of a float64 record: what the oracle loses from there on is of E64's order
    head64 = R.oracle64(c['iv'][:21], c['ba'], c['bg'], c['noise'])
    e = R.e64_of([c['iv'][20]] + c['iv'][21:], noise=c['noise'], start=head64)
    assert all(0 < e[k] < 1e-14 for k in R.KINDS), e


def test_yardstick(E64):
    """E64 per field kind is rounding noise of float64, nothing else (a reference or a metric gone wrong would show here)"""
    print("E64:", {k: f"{v:.3e}" for k, v in E64.items()})
    for name in R.CASES:
        print(f"e64 {name}: ", {k: f"{v:.2e}" for k, v in R.e64(name).items()})
    assert 2.0 ** -53 < E64['state'] < 64 * 2.0 ** -52 and 2.0 ** -53 < E64['jacobian'] < 64 * 2.0 ** -52 and 2.0 ** -53 < E64['covariance'] < 64 * 2.0 ** -52
    assert R.e64('n0') == dict.fromkeys(R.KINDS, 0.0) and R.e64('noise_zero')['covariance'] == 0.0
    assert M in (1, 2, 4, 8, 16, 32, 64)


def test_metric_sees_what_the_old_one_did_not():
    """the issue's two examples: the gyro-bias block times 1.005, and an entry of it set to zero (120 samples)"""
    for name in ('n20', 'n120_dt0.1'):
        ref = R.reference(name)
        got = {k: np.array(v, np.float64) for k, v in ref.items()}
        got['covariance'][12:15, 12:15] *= 1.005
        old = np.abs(got['covariance'] - np.asarray(ref['covariance'], float)).max() / np.abs(ref['covariance']).max()
        assert old < 1e-11 and R.record_error(got, ref)['covariance'] > 4e-3, (name, old)
        got['covariance'][13, 13] = 0.0
        assert R.record_error(got, ref)['covariance'] > 0.99


@pytest.mark.parametrize("edit", R.EDITS)
def test_each_edit_exceeds_twice_the_bound(E64, edit):
    worst = dict.fromkeys(R.KINDS, (0.0, None))
    for name, c in R.CASES.items():
        e = R.by_kind(R.record_error(R.integrate(c['iv'], c['ba'], c['bg'], c['noise'], dtype=np.float64, edit=edit), R.reference(name)))
        for k in R.KINDS:
            if e[k] > worst[k][0]:
                worst[k] = (e[k], name)
    print(f"edit {edit}: " + "  ".join(f"{k} {v[0]:.2e} ({v[1]})" for k, v in worst.items()))
    assert any(worst[k][0] > 2 * M * E64[k] for k in R.KINDS), worst


# ---- emulated kernels (CPU fiber emulator) ----------------------------------------------------------------------------------------
def test_emulated_cases(simt_handle, E64):
    check_cases(simt_handle, E64, 'emulated')


def test_emulated_repeated_time_stamp(simt_handle, E64):
    check_dt0(simt_handle, E64, 'emulated')


def test_emulated_ragged_batch(simt_handle, E64):
    check_ragged(simt_handle, E64, 'emulated', range(R.RAGGED_N))


def test_emulated_scratch_growth():
    a, b = conftest._simt_handle(), conftest._simt_handle()
    try:
        check_scratch_growth(a, b)
    finally:
        a.close()
        b.close()


# ---- MI355X -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cases(handle, E64):
    check_cases(handle, E64, 'gpu')


@pytest.mark.gpu
def test_repeated_time_stamp(handle, E64):
    check_dt0(handle, E64, 'gpu')


@pytest.mark.gpu
def test_ragged_batch(handle, E64):
    check_ragged(handle, E64, 'gpu', range(R.RAGGED_N))


@pytest.mark.gpu
def test_scratch_growth():
    a, b = conftest.new_handle(), conftest.new_handle()
    try:
        check_scratch_growth(a, b)
    finally:
        a.close()
        b.close()
