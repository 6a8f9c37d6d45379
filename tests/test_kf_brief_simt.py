"""vg_kf_* through the EMULATED kernels (tests/simt: csrc/fe_ransac.hip with csrc/kf_brief.h compiled for the CPU fiber emulator).
Reference, cases and the check bodies are tests/kf_brief_ref.py; tests/test_kf_brief_gpu.py runs the same bodies on the MI355X.
Every comparison is for equality."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import conftest
import kf_brief_ref as K

ROOT = conftest.ROOT


def test_pattern_file():
    K.check_pattern_file()


@pytest.mark.parametrize("size,cam", [((67, 41), "pinhole"), ((67, 41), "mei"), ((100, 70), "kb")])
def test_frames_against_the_reference(simt_handle, size, cam):
    K.check_frame(simt_handle, size, cam)


def test_full_size_frame(simt_handle):
    """752 x 480: the row-major compaction across 5640 segments"""
    K.check_frame(simt_handle, (752, 480), "pinhole", n_window=150)


def test_blur_border(simt_handle):
    K.check_blur_border(simt_handle)


def test_patterns_of_a_wider_reach(simt_handle):
    K.check_wide_pattern(simt_handle)


def test_window_point_counts(simt_handle):
    K.check_window_counts(simt_handle)


def test_fast_cases(simt_handle):
    K.check_fast_cases(simt_handle)


def test_keypoint_cap(simt_handle):
    K.check_cap(simt_handle)


def test_match_on_planted_records(simt_handle):
    K.check_planted(simt_handle)


def test_match_on_rendered_frames(simt_handle):
    assert K.check_rendered(simt_handle) == K.N_RENDERED


def test_batch_and_state(simt_handle):
    K.check_batch_and_state(simt_handle)


@pytest.mark.parametrize("name", K.REFUSALS)
def test_refusal(simt_handle, name):
    bare = conftest._simt_handle() if name.endswith("unconfigured") else None
    try:
        K.check_refusal(simt_handle, name, bare)
    finally:
        if bare is not None:
            bare.close()


def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path):
    """class KeyFrame, BriefExtractor and vg_pack_kf (host/keyframe.h, host/vg_pack.h) through `vins_replay_simt kf`"""
    conftest._build_simt()
    K.check_replay(os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path)


def test_yml_reader_host_only():
    conftest._build_simt()
    K.check_pattern_reader(os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"))


def test_standalone_sanitizer_run(simt_handle, tmp_path):
    """tests/kf_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on the
    67 x 41 frame, the truncated case and the 65-entry match: no report, results equal to the unsanitized run through the binding"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "fe_ransac.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "kf_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "kf_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    size = (67, 41)
    cam = K.cameras(size[0])["pinhole"]
    img, w = K.frames(size)[0], K.window_points(size, 9)
    n = K.scene_ref(size, 0)["n_keypoints"]
    files, want = [], []
    for i, cap in enumerate((n, n - 1)):                          # the whole frame, the truncated case; each with the 65-entry match
        plant = K.planted(65)
        files.append(str(tmp_path / f"c{i}.bin"))
        K.write_san_case(files[-1], size, img, w, cam, cap, plant)
        kf2 = K.fe.KeyFrames(simt_handle, size[0], size[1], cap, 9, 1, K.pattern())
        ga = kf2.add([0], [img], [K.camera_struct(cam)], [w])[0]
        wd, wxy, od, opt, onorm = plant
        kf = K.fe.KeyFrames(simt_handle, size[0], size[1], max(cap, 65), 9, 3, K.pattern())
        kf.set(1, np.zeros((0, 2)), np.zeros(0), np.zeros((0, 2)), np.zeros((0, 4)), wxy, wd)
        kf.set(2, np.zeros((65, 2)), np.zeros(65), np.zeros((65, 2)), od, np.zeros((0, 2)), np.zeros((0, 4)))
        want.append(K.san_expected(ga, kf.match([(1, 2)])[0]))
    assert want[1].split()[1] == str(K.fe.KF_TRUNCATED)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.splitlines() == want, (r.stdout, want)
