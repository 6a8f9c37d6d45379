"""vg_kf_pnp through the EMULATED kernels (tests/simt: csrc/fe_ransac.hip with csrc/kf_pnp.h compiled for the CPU fiber emulator).
Reference, cases, metric and the check bodies are tests/kf_pnp_ref.py; tests/test_kf_pnp_gpu.py runs the same bodies on the MI355X."""
import os
import shutil
import subprocess

import pytest

import conftest
import kf_pnp_ref as K

ROOT = conftest.ROOT


@pytest.fixture(scope="module")
def table(simt_handle):
    return K.check_cases(simt_handle, 'emulated')


def test_every_case_within_the_bound(table):
    assert set(table) == set(K.CASE_ARGS)


def test_capacity_pair(simt_handle):
    K.check_capacity(simt_handle, 'emulated')


def test_batch_equals_single_pairs(simt_handle):
    K.check_batch_equals_single(simt_handle, (1, 3, 33))


def test_failed_pair_leaves_its_neighbours(simt_handle):
    K.check_failed_neighbours(simt_handle)


@pytest.mark.parametrize("name", K.REFUSALS)
def test_refusal(simt_handle, name):
    K.check_refusal(simt_handle, name)


def test_chain_into_the_relocalisation_frame(simt_handle):
    """vg_kf_add -> vg_kf_match -> vg_kf_pnp -> vg_ba_seq_set_relo -> a step -> vg_ba_seq_get_relo: bit-identical to the step fed the reference's lists"""
    h_ref = conftest._simt_handle()
    try:
        K.check_chain(simt_handle, h_ref)
    finally:
        h_ref.close()


@pytest.mark.parametrize("name", K.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path, name):
    """KeyFrame::PnPRANSAC / findConnection (host/keyframe.h, vg_pack_kf_pnp) through `vins_replay_simt kfpnp`"""
    conftest._build_simt()
    K.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


def test_standalone_sanitizer_run(simt_handle, tmp_path):
    """tests/kf_pnp_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on four
    cases (two sizes, both refine modes, a pair without a model, a skipped one): no report, the batch equals the single calls, and the
    decisions equal the unsanitized run through the binding"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "fe_ransac.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "kf_pnp_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "kf_pnp_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    names, files = ('n27', 'n65', 'no_model', 'skipped'), []
    for name in names:
        files.append(str(tmp_path / (name + ".bin")))
        K.write_file(files[-1], K.case(name))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 2 * len(names)
    got = K._fe().kf_pnp(simt_handle, [K.case(n) for n in names])
    for a, b, g in zip(rows[:len(names)], rows[len(names):], got):
        assert a[0] == 'batch' and b[0] == 'alone' and a[1:] == b[1:]
        assert [int(x) for x in a[1:9]] == [g[k] for k in ('status', 'n_inliers', 'ransac_best', 'ransac_iter', 'ransac_bound', 'has_loop', 'refit_iters', 'refit_up')]
