"""Static guard on the device code of libvinsgpu.so (no GPU needed): the phase functions of the BA solve kernel must keep
their explicit address spaces and their MFMA factorisations.

A pointer handed to a non-inlined device function is generic; every access through it compiles to flat_load / flat_store
(docs/DESIGN_history_r1-r4.md 1.6: re-typing the operands as address_space(3) / address_space(1) was worth 17 % of the solve kernel).  A refactor
that drops a cast silently brings the flat accesses back without failing any parity test, so the instruction mix of the built
library is pinned here: a handful of flat loads per function (the by-reference context structs), LDS traffic as ds_*, HBM
traffic as global_*, and v_mfma_f64_16x16x4 where the dense factors are supposed to use it."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "..", "vins-mono_amd", "lib", "libvinsgpu.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def _device_functions():
    """{symbol: [instruction mnemonics]} over every gfx950 code object embedded in the library."""
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(LIB, so)
        subprocess.run([OBJDUMP, "--offloading", so], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            txt = subprocess.run([OBJDUMP, "-d", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            name = None
            for line in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
                if m:
                    name = m.group(1)
                    out.setdefault(name, [])
                    continue
                m = re.match(r"^\s+([a-z_0-9]+)\s", line)
                if m and name:
                    out[name].append(m.group(1))
    return out


@pytest.fixture(scope="module")
def funcs():
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    return _device_functions()


def _find(funcs, *needles):
    hits = [k for k in funcs if all(n in k for n in needles)]
    assert hits, f"no device function matching {needles}"
    return hits


def _count(ops, prefix):
    return sum(1 for o in ops if o.startswith(prefix))


# function name fragment -> (max flat accesses, min ds accesses, min MFMAs)
PHASES = {
    "cholesky_aug": (12, 30, 32),        # 16 pivots x (diagonal block + panel tile) + the trailing update
    "chain_schurILi4E": (8, 150, 60),    # round 5: chain elimination + Schur complement in one phase (two 9x9 factors in lock step, X^T X of the staged rows, landmark tiles)
    "15back_substituteRK3Ctx": (16, 12, 0),
    "build_scaledILb0E": (16, 20, 0),
    "14assemble_small": (8, 8, 0),       # round 5: plan-driven gather (one LDS store per entry, the pinv reads)
}


@pytest.mark.parametrize("frag", sorted(PHASES))
def test_phase_function_keeps_its_address_spaces(funcs, frag):
    max_flat, min_ds, min_mfma = PHASES[frag]
    for name in _find(funcs, frag):
        ops = funcs[name]
        flat = _count(ops, "flat_load") + _count(ops, "flat_store")
        ds = _count(ops, "ds_read") + _count(ops, "ds_write")
        mfma = _count(ops, "v_mfma_f64_16x16x4")
        assert flat <= max_flat, f"{name}: {flat} flat accesses (generic pointers are back)"
        assert ds >= min_ds, f"{name}: only {ds} LDS accesses"
        assert mfma >= min_mfma, f"{name}: only {mfma} v_mfma_f64_16x16x4"


def test_kernels_do_not_fall_back_to_flat_memory(funcs):
    for k in ("ba_accumulate_kernel", "ba_linacc_proj_kernel", "ba_linearize_imu_kernel", "ba_linearize_proj_kernel", "ba_solve_kernel", "ba_solve_w8_kernel",
              "fe_lk_kernel"):
        for name in _find(funcs, k):
            ops = funcs[name]
            # the top level of the solve kernel re-reads its context struct from the private stack after the phase calls (its
            # address is handed to them on purpose): a few dozen flat accesses per launch, none in a loop
            limit = 40 if name in ("ba_solve_kernel", "ba_solve_w8_kernel") else 4
            assert _count(ops, "flat_load") + _count(ops, "flat_store") <= limit, name


def test_fused_projection_kernel_keeps_its_mfma_and_stays_out_of_scratch(funcs):
    """ba_linacc_proj_kernel: the camera blocks of the projection factors are X^T X products on v_mfma_f64_16x16x4 (one per pair slot
    of a wavefront), the staged records live in LDS, and what it keeps in scratch is the context struct of the two non-inlined IMU /
    prior passes — not the accumulators."""
    (name,) = [n for n in _find(funcs, "ba_linacc_proj_kernel") if "clone" not in n][:1]
    ops = funcs[name]
    assert _count(ops, "v_mfma_f64_16x16x4") >= 10
    assert _count(ops, "ds_read") >= 30 and _count(ops, "ds_write") >= 20
    assert _count(ops, "scratch_store") <= 16 and _count(ops, "scratch_load") <= 16


def _kernel_metadata():
    """{kernel: {private_segment_fixed_size, vgpr_spill_count, ...}} from the notes of the embedded gfx950 code objects."""
    readelf = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "lib.so")
        shutil.copy(LIB, so)
        subprocess.run([OBJDUMP, "--offloading", so], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "gfx950" not in f:
                continue
            txt = subprocess.run([readelf, "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            cur = {}
            for line in txt.splitlines():
                m = re.match(r"^\s*-?\s*\.(\w+):\s+(\S+)\s*$", line)
                if not m:
                    continue
                key, val = m.group(1), m.group(2)
                if key == "agpr_count" and cur.get("name"):          # first key of the next kernel's record
                    out[cur["name"]] = cur
                    cur = {}
                cur[key] = val
            if cur.get("name"):
                out[cur["name"]] = cur
    return out


def test_solve_kernel_keeps_its_uniform_state_out_of_scratch():
    """The solve kernel's top level holds only wave-uniform state between the calls of its phase functions (layout fields through
    the constant address space, control block through readfirstlane, the phases rebuild their context from the kernel
    arguments): nothing of it may be spilled per lane.  Before that arrangement the kernel carried 712 B of private segment
    and 202 spilled VGPRs — three quarters of its HBM traffic (docs/DESIGN_history_r1-r4.md 1.6)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    md = _kernel_metadata()
    k = md["ba_solve_kernel"]
    # round 5 (4 wavefronts per window, 72 KB of LDS: two windows per CU): the top level now keeps ~70 per-lane values across the
    # phase calls (pointers into LDS that the compiler does not prove uniform) -- each is stored and re-read ONCE per launch, outside
    # every loop; what must stay out of scratch is the inner loop of the chain elimination (pinned below)
    assert int(k["vgpr_spill_count"]) <= 80, k
    assert int(k["private_segment_fixed_size"]) <= 640, k
    assert int(k["group_segment_fixed_size"]) == 0, k
    # the 8-wavefront build of the same source (csrc/ba_solve_w8.hip), the kernel of every call with fewer than 32 windows -- the
    # drop-in's single window among them: the same arrangement, the same bounds
    k = md["ba_solve_w8_kernel"]
    assert int(k["vgpr_spill_count"]) <= 80, k
    assert int(k["private_segment_fixed_size"]) <= 640, k
    assert int(k["group_segment_fixed_size"]) == 0, k


def test_chain_elimination_loop_stays_out_of_scratch(funcs):
    """chain_schur<4> (the EuRoC shape: 15 tiles of S over four wavefronts) runs its six elimination steps with the accumulators, the
    previous block's solved column and the staged raw entries in registers: a handful of scratch accesses at most (the first version
    of the phase had 30 stores / 39 loads inside the loop and took 57K cycles for the update step alone)."""
    (name,) = _find(funcs, "chain_schurILi4E")
    ops = funcs[name]
    assert _count(ops, "scratch_store") <= 6 and _count(ops, "scratch_load") <= 6, (name, _count(ops, "scratch_store"), _count(ops, "scratch_load"))


def test_solve_kernel_fits_two_windows_per_cu():
    """Occupancy by construction: 256 threads x <= 256 VGPRs = one wavefront per SIMD and workgroup, so two workgroups fit the register
    file of a CU; the LDS half of the bargain (<= 80 KB for the reference shape) is checked on the layout in tests/test_abi_and_host.py."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    md = _kernel_metadata()
    k = md["ba_solve_kernel"]
    assert int(k["max_flat_workgroup_size"]) == 256 and int(k["vgpr_count"]) <= 256, k
    # the 8-wavefront build: 512 threads = two wavefronts per SIMD, each within 256 of the 512 registers of a SIMD lane, ONE workgroup per CU
    k = md["ba_solve_w8_kernel"]
    assert int(k["max_flat_workgroup_size"]) == 512 and int(k["vgpr_count"]) <= 256, k


def test_widest_single_workgroup_window_fits_the_lds_of_a_cu(simt_handle):
    """build_layout holds the DYNAMIC carve of the solve kernel against 160 KB; a launch must fit together with the kernel's static
    group segment, and a launch that does not fit fails only on the hardware (the emulator has no LDS limit).  The widest window
    of the single-workgroup path -- 12 frames + relocalisation pose + extrinsic + td, Rc = 85, RcPad = 96 -- at the largest
    landmark count of tests/test_ba_step.py: carve + the staged landmark tile of the 8-wavefront build, [RcPad][32 + 1] doubles, +
    the static segment of the compiled kernel <= 160 KB, and likewise for the 4-wavefront build."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    from oracle import ba_numpy as B
    import ba_step_ref as R
    seq = R.ruled_sequence(3, 12, 218, estimate_extrinsic=1, estimate_td=1)
    prob = R.add_relocalisation(seq.window(0), seq.cfg)
    lay = B.Layout(prob)
    Rc = lay.R - 9 * lay.K
    RcPad = (Rc + 1 + 15) // 16 * 16
    assert (Rc, RcPad) == (85, 96)
    simt_handle.ba_upload([prob])
    info = simt_handle.ba_info()
    assert all(info['flops_by_kernel'][k] == 0 for k in ("ba_big_schur_kernel", "ba_solve_big_kernel", "ba_big_step_kernel"))     # not the large path
    md = _kernel_metadata()
    carve = info['lds_bytes']
    assert carve + 8 * RcPad * 33 + int(md["ba_solve_w8_kernel"]["group_segment_fixed_size"]) <= 160 * 1024, carve
    assert carve + int(md["ba_solve_kernel"]["group_segment_fixed_size"]) <= 160 * 1024, carve


def test_factor_and_marginalization_kernels_stay_within_their_register_budgets():
    """Regression bounds (VERDICT r3 item 5 asked for the marginalization kernel to be covered): `ba_linacc_proj_kernel` keeps its
    accumulators and the factor evaluation in registers (the private segment is the context struct of the two non-inlined passes);
    `ba_marg_kernel` ran 1024 threads at 128 VGPRs with ~0.5 KB of scratch per lane until round 6 (a 512-thread build without spills was
    SLOWER in round 4: 408 vs 366 us per 256 windows, profiles/r04p_*); round 6 rebuilt its long phases and the 512-thread build, 247
    VGPRs without a private segment, is the faster one."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    md = _kernel_metadata()
    k = md["ba_linacc_proj_kernel"]
    assert int(k["vgpr_spill_count"]) <= 32 and int(k["private_segment_fixed_size"]) <= 256, k      # (23 / 200 B in the round-4 build)
    k = md["ba_marg_kernel"]
    # round 6: 512 threads x 247 VGPRs, NO spills, NO private segment (rounds 3-5: 1024 threads at 128 VGPRs with ~0.5 KB of scratch per
    # lane -- a 512-thread build was slower then, 408 vs 366 us, because the kernel's long phases were spread over sixteen wavefronts with
    # a barrier per step; since they became one-wavefront chains and matrix-core tiles the 512-thread build wins: 190 -> 166 us,
    # gpurun_out r07c / r07d A/Bs quoted in DESIGN 1.4)
    assert int(k["vgpr_spill_count"]) == 0 and int(k["private_segment_fixed_size"]) <= 64 and int(k["max_flat_workgroup_size"]) == 512, k
    # (VERDICT r4 item 4 asked for <= 256 B here and 0 B for ba_final_kernel: not reached -- the bounds pin what is, so that it cannot grow)
    k = md["ba_final_kernel"]
    assert int(k["private_segment_fixed_size"]) <= 96 and int(k["vgpr_spill_count"]) == 0, k
