"""vg_kf_pnp: the conditions the scenes of tests/kf_pnp_ref.py must meet, asserted on the NumPy reference alone (no library, no GPU): the three
routes (80-bit Jacobi, float64 Jacobi, float64 numpy.linalg) give the same bookkeeping trace and mask, no error of a model in the trace lies
within 1e-6 of the squared threshold, the canonical row leads by 1e-6 in every sample of the trace, n_inliers is not at the loop gate unless
the case is about that, yaw and distance are not at their gates; and the cases are what their names say."""
import pytest

import kf_pnp_ref as K


@pytest.mark.parametrize("name", list(K.CASE_ARGS))
def test_scene_conditions(name):
    K.conditions(name, K.case(name), {r: K.case_reference(name, r) for r in K.ROUTES})


def test_capacity_scene_conditions():
    K.conditions('capacity', K.capacity_scene(), {r: K.reference(K.capacity_scene(), r) for r in K.ROUTES})


def test_cases_are_what_their_names_say():
    K.case_properties()


def test_schedule_is_a_function_of_n():
    s = K.schedule(27, 100)
    assert len(s) == 100 and all(len(set(x)) == 5 and max(x) < 27 for x in s) and s[:30] == K.schedule(27, 30)
    assert K.update_num_iters(0.99, 0.3, 5, 100) == 25 and K.update_num_iters(0.99, 0.0, 5, 100) == 0


def test_sample_kernel_stays_out_of_scratch():
    """kp_sample_kernel keeps its column of M and of the rotations in registers and everything indexed by a loop variable in LDS: no private
    segment, no spilled VGPR in the gfx950 code object (256 VGPRs as compiled); the count and bookkeeping kernels likewise"""
    import test_codegen_guard as G
    md = G._kernel_metadata()
    for name in ("kp_sample_kernel", "kp_count_kernel", "kp_pick_kernel"):
        k = md[name]
        assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0, (name, k)
    assert int(md["kp_tail_kernel"]["vgpr_spill_count"]) == 0, md["kp_tail_kernel"]
