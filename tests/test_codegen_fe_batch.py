"""Static guard on the kernels of vg_fe_read_image_batch in the built libvinsgpu.so (no GPU needed): one workgroup per stream only pays
off while the per-stream bodies stay in registers -- no private segment, no spilled register, no scratch_* access in any of them."""
import os

import pytest

import test_codegen_guard as G

KERNELS = ("fe_rb_after_lk_kernel", "fe_rb_pick_kernel", "fe_rb_setmask_kernel", "fe_rb_finish_kernel", "fe_rb_ransac7_kernel",
           "fe_rb_count_kernel")


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(G.OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    return G._device_functions(), G._kernel_metadata()


@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_kernel_has_no_private_segment_and_no_spills(built, kernel):
    funcs, md = built
    assert kernel in md, "kernel missing from the gfx950 code object: " + kernel
    k = md[kernel]
    assert int(k["private_segment_fixed_size"]) == 0 and int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k
    ops = funcs[kernel]
    assert len(ops) > 20 and not [o for o in ops if o.startswith("scratch_")], kernel
