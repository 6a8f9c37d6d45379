"""vg_init_sfm through the EMULATED kernels (tests/simt: csrc/triangulate.hip with csrc/init_sfm.h compiled for the CPU fiber emulator).
Reference, cases, metric and the check bodies are tests/init_sfm_ref.py; tests/test_init_sfm_gpu.py runs the same bodies on the MI355X.

MEASURED, emulator: every decision equals the 80-bit route's; worst value ratio over the table 1.98 x E64 (position of F5_50_ok; bound 4),
among the cases whose BA converges 1.70 (position of F11_mid); the capacity window 0.86 x the floor."""
import os
import shutil
import subprocess

import pytest

import conftest
import init_sfm_ref as S

ROOT = conftest.ROOT


@pytest.fixture(scope="module")
def table(simt_handle):
    return S.check_cases(simt_handle, 'emulated')


def test_every_case_within_the_bound(table):
    assert set(table) == set(S.CASE_ARGS)


def test_batch_equals_single_windows(simt_handle):
    S.check_batch_equals_single(simt_handle, (1, 3, 33))


def test_numeric_window_leaves_its_neighbours(simt_handle):
    S.check_numeric_neighbours(simt_handle)


@pytest.mark.parametrize("name", S.REFUSALS)
def test_refusal(simt_handle, name):
    S.check_refusal(simt_handle, name)


@pytest.mark.parametrize("name", S.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path, name):
    """Estimator::initialStructure (host/estimator.cpp, vg_pack_sfm) through `vins_replay_simt sfm`"""
    conftest._build_simt()
    S.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


def test_capacity_window(simt_handle):
    S.check_capacity(simt_handle, 'emulated')


def test_chain_into_the_alignment(simt_handle):
    S.check_chain(simt_handle)


def test_lds_carve(tmp_path):
    """tests/init_sfm_carve_check.cpp: the carve of csrc/init_sfm_carve.h for every F and feature count the call accepts"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "carve_check")
    subprocess.run([cxx, "-std=c++17", "-I" + os.path.join(ROOT, "vins-mono_amd", "csrc"), os.path.join(ROOT, "tests", "init_sfm_carve_check.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout


def test_standalone_sanitizer_run(tmp_path):
    """tests/init_sfm_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on
    F = 3, 11 and 16 and on the capacity window: no report, the reference's statuses, and the batch equals the single calls"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "triangulate.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "init_sfm_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "init_sfm_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    names, files = ('F3_10', 'F11_mid', 'F16'), []
    for name in names:
        files.append(str(tmp_path / (name + ".bin")))
        S.write_file(files[-1], S.case(name))
    files.append(str(tmp_path / "capacity.bin"))            # the whole LDS of a CU, one feature staged at a time
    S.write_file(files[-1], S.capacity_scene())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 8
    assert [int(x[1]) for x in rows[:4]] == [3, 11, 16, 16] and int(rows[3][2]) == S.OK
    assert [int(x[2]) for x in rows[:3]] == [S.reference(n)['dec']['status'] for n in names]
    assert [int(x[3]) for x in rows[:3]] == [S.reference(n)['dec']['ba_iters'] for n in names]
    for a, b in zip(rows[:4], rows[4:]):
        assert a[0] == 'batch' and b[0] == 'alone' and a[1:] == b[1:]
