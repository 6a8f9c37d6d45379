"""vg_init_exrot through the EMULATED kernels (tests/simt: csrc/fe_ransac.hip with csrc/init_exrot.h compiled for the CPU fiber
emulator).  Reference, cases, metric and the check bodies are tests/init_exrot_ref.py; tests/test_init_exrot_gpu.py runs the same bodies
on the MI355X.

MEASURED, emulator: every decision equals the reference's on the eight cases, the capacity step and the numeric window; worst value ratio
2.01 x E64 (ric of a step of 'never', bound 4), the capacity window 1.00.

The chain (at ransac_threshold = 0.3 / 460, tests/init_exrot_ref.chain_window): calib_ric 3.3e-5 degrees from the scene's, scale to 1.8e-5."""
import os
import shutil
import subprocess

import pytest

import conftest
import init_exrot_ref as X

ROOT = conftest.ROOT


@pytest.fixture(scope="module")
def table(simt_handle):
    return X.check_cases(simt_handle, 'emulated')


def test_every_case_within_the_bound(table):
    assert set(table) == set(X.CASE_ARGS)


def test_split_run_equals_the_unsplit_one(simt_handle):
    X.check_split(simt_handle)


def test_batch_equals_single_windows(simt_handle):
    X.check_batch_equals_single(simt_handle, (1, 3, 33))


def test_numeric_window_leaves_its_neighbours(simt_handle):
    X.check_numeric_neighbours(simt_handle)


@pytest.mark.parametrize("name", X.REFUSALS)
def test_refusal(simt_handle, name):
    X.check_refusal(simt_handle, name)


def test_growing_table():
    h = conftest._simt_handle()
    try:
        X.check_growing_table(h)
    finally:
        h.close()


def test_stream_limit(simt_handle):
    X.check_stream_limit(simt_handle)


def test_capacity_step(simt_handle):
    X.check_capacity(simt_handle, 'emulated')


@pytest.mark.parametrize("name", X.REPLAY_CASES)
def test_cpp_class_one_frame_at_a_time_through_the_replay_tool(simt_handle, tmp_path, name):
    """Estimator::calibrateExtrinsicRotation / InitialEXRotation (host/estimator.cpp, vg_pack_exrot) through `vins_replay_simt exrot`"""
    conftest._build_simt()
    X.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


def test_standalone_sanitizer_run(simt_handle, tmp_path):
    """tests/init_exrot_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on
    the 9-, 15- and 65-point steps, the split run and the capacity step: no report, the binding's statuses and first_ok, the batch equals
    the single calls and the split run the unsplit one"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "fe_ransac.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "init_exrot_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "init_exrot_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    wins, files = X.sanitizer_windows(), []
    for i, w in enumerate(wins):
        files.append(str(tmp_path / f"w{i}.bin"))
        X.write_file(files[-1], w)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    n = len(wins)
    got = simt_handle.init_exrot(list(wins))
    assert len(rows) == 2 * n + 4 and [x[0] for x in rows] == ['batch'] * n + ['alone'] * n + ['split'] * 4
    assert [[int(v) for v in x[1:4]] for x in rows[:n]] == [[len(w['corr']), g['status'], g['first_ok']] for w, g in zip(wins, got)]
    assert got[3]['first_ok'] == X.MIN_FRAMES and list(got[0]['branch']) == [1, 2] and list(got[1]['ransac_inliers']) == [15]
    for a, b in zip(rows[:n], rows[n:2 * n]):
        assert a[1:] == b[1:]
    for s in rows[2 * n:]:
        assert s[1:] in [x[1:] for x in rows[:n]], s


def test_chain_into_sfm_and_alignment(simt_handle):
    X.check_chain(simt_handle)


def test_noisy_scenes_at_the_separating_threshold(simt_handle):
    X.check_separating(simt_handle)


def test_cpp_class_drops_its_oldest_record_at_the_cap(simt_handle, tmp_path):
    conftest._build_simt()
    X.check_replay_cap(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path)
