"""vg_init_align through the EMULATED kernels (tests/simt: csrc/imu_preint.hip with csrc/init_align.h compiled for the CPU fiber
emulator).  Reference, cases, metric and the check bodies are tests/init_align_ref.py; tests/test_init_align_gpu.py runs the same
bodies on the MI355X.

MEASURED, emulator: worst ratio over the table 0.98 x kappa 2^-53 (s_lin of F5_refine_fails; bound 4); delta_bg against max|ref|
instead of its own scale 13 .. 123 (the float64 NumPy routes: 9 .. 120)."""
import os
import shutil
import subprocess

import pytest

import conftest
import init_align_ref as A

ROOT = conftest.ROOT


@pytest.fixture(scope="module")
def table(simt_handle):
    return A.check_cases(simt_handle, 'emulated')


def test_every_case_within_the_bound(table):
    assert set(table) == set(A.CASE_ARGS)


def test_records_are_the_preintegration_kernels(simt_handle, table):
    A.check_records(simt_handle, table)


def test_batch_equals_single_windows(simt_handle):
    A.check_batch_equals_single(simt_handle, (1, 3, 70))


def test_numeric_window_leaves_its_neighbours(simt_handle):
    A.check_numeric_neighbours(simt_handle)


@pytest.mark.parametrize("name", A.REFUSALS)
def test_refusal(simt_handle, name):
    A.check_refusal(simt_handle, name)


@pytest.mark.parametrize("name", A.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path, name):
    """Estimator::visualInitialAlign (host/estimator.cpp) through `vins_replay_simt align`"""
    conftest._build_simt()
    A.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


def test_standalone_sanitizer_run(tmp_path):
    """tests/init_align_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and
    run on F = 2, 4 and 32: no report, and the batch equals the single calls"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "imu_preint.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "init_align_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "init_align_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    files = []
    for name in ('F2', 'F4', 'F32'):
        files.append(str(tmp_path / (name + ".bin")))
        A.write_replay(files[-1], A.case(name), [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [], [], [])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 6
    want = [A.reference(n)['status'] for n in ('F4', 'F32')]
    assert int(rows[0][3]) != A.OK and [int(rows[1][3]), int(rows[2][3])] == want
    for a, b in zip(rows[:3], rows[3:]):
        assert a[0] == 'batch' and b[0] == 'alone' and a[1:] == b[1:]
