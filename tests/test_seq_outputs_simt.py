"""Keyframe message and point clouds of a resident sequence (vg_ba_seq_outputs_reserve / _async / vg_ba_seq_get_outputs; csrc/ba_seq.hip
ba_seq_publish_kernel), kernel sources under the CPU fiber emulator.  The cases are in tests/seq_outputs_case.py;
tests/test_seq_outputs_gpu.py runs the same ones on the GPU."""
import pytest

import conftest
import seq_outputs_case as S
import seq_outputs_ref as R


@pytest.fixture(scope="module")
def two_handles():
    a, b = conftest._simt_handle(), conftest._simt_handle()
    yield a, b
    a.close(); b.close()


@pytest.mark.parametrize("K", [4, 11])
@pytest.mark.parametrize("name", ["edges", "lanes", "wide", "single"])
def test_planted_tables(two_handles, K, name):
    """Case 1: tracks on every edge of the three predicates; empty and full tables; 1, 63, 64, 65 and 300 selected tracks."""
    S.case_planted(two_handles[0], K, name)


@pytest.mark.parametrize("K", [4, 11])
def test_truncation(two_handles, K):
    """Case 2."""
    S.case_truncation(two_handles[0], K)


@pytest.mark.parametrize("K,imu", [(11, False), (11, True), (4, True)])
def test_after_real_steps(two_handles, K, imu):
    """Case 3: after every step of a small synthetic sequence, host-fed and in IMU mode, a void window between two good ones."""
    S.case_steps(two_handles[0], K, imu, n_steps=4 if K == 11 else 3, void=(K == 11))


def test_the_call_is_read_only(two_handles):
    """Case 4."""
    S.case_read_only(*two_handles)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutated_restatement_is_told_apart(two_handles, mutant):
    """Case 5."""
    S.case_mutation(two_handles[0], mutant)


def test_refusals(two_handles):
    """Case 6."""
    S.case_refusals(two_handles[0])


def test_standalone_sanitizer_run(two_handles, tmp_path):
    """Case 9: tests/seq_outputs_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own
    (like tests/test_kf_bow_simt.py builds its own) and run on cases 1 and 2: no report, and every line (the decisions, the ids, the bit
    patterns of the floats) equals the unsanitized run through the binding."""
    import os
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    root = conftest.ROOT
    src, simt = os.path.join(root, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    kernels = ["vg_core.hip", "ba_host.hip", "ba_pipeline.hip", "ba_solve_w8.hip", "ba_marg.hip", "ba_seq.hip", "imu_preint.hip", "triangulate.hip",
               "fe_host.hip", "fe_kernels.hip", "fe_ransac.hip", "fe_frame.hip"]          # (FILES of tests/simt/Makefile: the whole library)
    units = [["-x", "c++", os.path.join(src, k)] for k in kernels] + [[os.path.join(simt, "simt_runtime.cpp")],
                                                                      [os.path.join(root, "tests", "seq_outputs_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "seq_outputs_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name, make in S.SAN_CASES.items():
        K, tables, max_points = make()
        path = str(tmp_path / (name + ".bin"))
        S.write_san_case(path, K, tables, max_points)
        r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.stdout.splitlines() == S.san_lines(two_handles[0], K, tables, max_points), name


_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import seq_outputs_case as S
import vio_bridge_case as case
A, B = conftest._simt_handle(), conftest._simt_handle()
print("RESULT", S.case_chain(A, B, case.Data(4, 1, True, plan="PPPPP")))
"""


def test_chain_from_the_keyframe_message_into_the_relocalisation_frame():
    """Case 7 at the staged small frame (windows of K = 4 frames, frames of 376x240, a process of its own like
    test_relocalisation_frame_through_the_bridge of tests/test_seq_relo_simt.py)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=root)], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "RESULT" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    n_kf, n_matched, n_inliers, n_factors = eval(r.stdout[r.stdout.index("RESULT") + 6:].strip().splitlines()[0])
    assert n_kf > 8 and n_matched > 8 and n_inliers > 8 and n_factors >= 2, (n_kf, n_matched, n_inliers, n_factors)


def test_cpp_replay_with_published_outputs(two_handles, tmp_path):
    """Case 8: `vins_replay seq` with VINS_REPLAY_OUTPUTS, linked against the emulated library."""
    import os
    conftest._build_simt()
    S.case_cpp(two_handles[0], os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path)
