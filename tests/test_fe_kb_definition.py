"""The Kannala-Brandt lift as vins-mono_amd/csrc/fe_camera.h defines it (fe_kb_case.lift64_kb: 10 Newton steps from theta = r, the
library's own sine and cosine) against the reference's EquidistantCamera::liftProjective restated with numpy.linalg.eigvals
(fe_kb_case.ref_lift_kb), in NumPy alone: no library, no device.  The five cameras at their own frame sizes, every 8th pixel with the
borders plus 512 random sub-pixel positions.

Fixture condition, evaluated on the reference restatement's theta: points with theta < 1.45 are kept (z >= 0.12; beyond that x / z
grows without bound and the TUM lens looks backwards), and at least 85 % of every camera's points remain.  Then
  - |theta - theta_ref| <= 1e-13,
  - every float coordinate (float)(x / z), (float)(y / z) lies within 1 float ulp of the reference's, and at most 1 in 1000 differs at all
    (a 1e-14 error in theta moves x / z by about 1e-13 relative against a float ulp of 6e-8: the cap only absorbs a coordinate that sits
    on a rounding boundary),
  - the first critical point of r(theta) lies beyond the largest theta in the frame: the monotone-branch claim of include/vinsgpu.h."""
import numpy as np
import pytest

import fe_kb_case as kb


def _ordered(a):
    """float32 -> integers whose difference counts the representable values between two floats"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("name", kb.TABLE)
def test_newton_lift_equals_the_reference_eigenvalue_lift(name):
    p = kb.params(name)
    pts = kb.points_of(name)
    _, _, _, th_ref, _ = kb.ref_theta_kb(pts, p)
    keep = th_ref < 1.45
    assert keep.mean() >= 0.85, (name, keep.mean())
    _, _, _, th = kb.theta64_kb(pts, p)
    err = np.abs(th - th_ref)[keep].max()
    print(name, "points", len(pts), "kept", int(keep.sum()), "max |theta - theta_ref|", err, "largest theta", th_ref.max())
    assert err <= 1e-13, (name, err)
    x, y, z = kb.lift64_kb(pts[keep], p)
    rx, ry, rz = kb.ref_lift_kb(pts[keep], p)
    assert z.min() >= 0.12 and rz.min() >= 0.12
    got = np.stack([x / z, y / z], 1).astype(np.float32)
    want = np.stack([rx / rz, ry / rz], 1).astype(np.float32)
    ulps = np.abs(_ordered(got) - _ordered(want))
    print(name, "coordinates", ulps.size, "differing", int((ulps != 0).sum()), "max ulps", int(ulps.max()))
    assert ulps.max() <= 1, (name, int(ulps.max()))
    assert (ulps != 0).sum() * 1000 <= ulps.size, (name, int((ulps != 0).sum()), ulps.size)


@pytest.mark.parametrize("name", kb.TABLE)
def test_the_frame_lies_on_the_first_monotone_branch(name):
    p = kb.params(name)
    _, _, _, th_ref, _ = kb.ref_theta_kb(kb.points_of(name), p)
    crit = kb.first_critical_point(p)
    print(name, "first critical point", crit, "largest theta in the frame", th_ref.max())
    assert crit > th_ref.max(), (name, crit, th_ref.max())


def test_own_sine_and_cosine_are_accurate():
    """fe_kb_sincos against libm on [0, 3.2] (and on negative arguments and the next quadrants): absolute error <= 1.2e-16 plus libm's own
    half ulp"""
    t = np.concatenate([np.linspace(0.0, 3.2, 200001), np.linspace(-3.2, 0.0, 20001), np.linspace(3.2, 8.0, 20001)])
    s, c = kb.sincos64(t)
    es, ec = np.abs(s - np.sin(t)).max(), np.abs(c - np.cos(t)).max()
    print("max abs error: sin", es, "cos", ec)
    assert es <= 1.2e-16 + 2.0 ** -54 and ec <= 1.2e-16 + 2.0 ** -54, (es, ec)
