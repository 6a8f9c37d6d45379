"""vg_init_relpose through the EMULATED kernels (tests/simt: csrc/fe_ransac.hip with csrc/init_relpose.h compiled for the CPU fiber
emulator).  Reference, cases, metric and the check bodies are tests/init_relpose_ref.py; tests/test_init_relpose_gpu.py runs the same
bodies on the MI355X.

MEASURED, emulator: every decision equals the reference's; worst value ratio over the table 1.00 x E64 (bound 4), the capacity window
0.63 (relative_R) and 0.29 (relative_T); the chain finds the scene's scale to 2.5e-5."""
import os
import shutil
import subprocess

import pytest

import conftest
import init_relpose_ref as R

ROOT = conftest.ROOT


@pytest.fixture(scope="module")
def table(simt_handle):
    return R.check_cases(simt_handle, 'emulated')


def test_every_case_within_the_bound(table):
    assert set(table) == set(R.CASE_ARGS)


def test_batch_equals_single_windows(simt_handle):
    R.check_batch_equals_single(simt_handle, (1, 3, 33))


def test_none_window_leaves_its_neighbours(simt_handle):
    R.check_none_neighbours(simt_handle)


@pytest.mark.parametrize("name", R.REFUSALS)
def test_refusal(simt_handle, name):
    R.check_refusal(simt_handle, name)


def test_growing_table():
    h = conftest._simt_handle()
    try:
        R.check_growing_table(h)
    finally:
        h.close()


def test_stream_limit(simt_handle):
    R.check_stream_limit(simt_handle)


def test_capacity_window(simt_handle):
    R.check_capacity(simt_handle, 'emulated')


def test_chain_into_sfm_and_alignment(simt_handle):
    R.check_chain(simt_handle)


@pytest.mark.parametrize("name", R.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path, name):
    """Estimator::relativePose / initialStructure() (host/estimator.cpp, vg_pack_relpose) through `vins_replay_simt relpose`"""
    conftest._build_simt()
    R.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


def test_standalone_sanitizer_run(tmp_path):
    """tests/init_relpose_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on
    three cases (F = 3, the collinear sample with its second submission, F = 5 with a failing candidate) and on the capacity window: no
    report, the reference's statuses and l, and the batch equals the single calls"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "fe_ransac.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "init_relpose_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "init_relpose_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    names, files = ('F3_two', 'collinear', 'few_inliers'), []
    for name in names:
        files.append(str(tmp_path / (name + ".bin")))
        R.write_file(files[-1], R.case(name))
    files.append(str(tmp_path / "capacity.bin"))
    R.write_file(files[-1], R.capacity_scene())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == 8
    assert [int(x[1]) for x in rows[:4]] == [3, 4, 5, 16] and [int(x[2]) for x in rows[:4]] == [R.OK] * 4
    assert [int(x[3]) for x in rows[:3]] == [R.reference(n)['l'] for n in names] and int(rows[3][3]) == 0
    for a, b in zip(rows[:4], rows[4:]):
        assert a[0] == 'batch' and b[0] == 'alone' and a[1:] == b[1:]
