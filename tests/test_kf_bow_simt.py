"""vg_voc_load / vg_bow_* / vg_kf_loop_detect through the EMULATED kernels (tests/simt: csrc/fe_ransac.hip with csrc/kf_bow.h compiled for the
CPU fiber emulator).  The restatement of DBoW2, the vocabularies, the scenes and the check bodies are tests/kf_bow_ref.py;
tests/test_kf_bow_gpu.py runs the same bodies on the MI355X."""
import os
import shutil
import subprocess

import pytest

import conftest
import kf_bow_ref as B

ROOT = conftest.ROOT


def test_scene_conditions():
    """CPU only: the planted ties, the repeated sum that differs from 7 * w, the six kinds of frame in the stream, the tie condition"""
    B.check_scene_conditions()


@pytest.mark.parametrize("name", list(B.VOCS))
def test_walk_and_vector(simt_handle, name):
    B.check_walk(simt_handle, name, B.WALK_SIZES)


def test_walk_large_records(simt_handle):
    B.check_walk(simt_handle, "k10L3", B.WALK_LARGE)


def test_vector_cases(simt_handle):
    B.check_vector(simt_handle)


def test_stream_of_70_keyframes(simt_handle):
    B.check_stream(simt_handle)


def test_tie_rule(simt_handle):
    B.check_tie(simt_handle)


def test_flags_and_state(simt_handle):
    B.check_flags_and_state(simt_handle)


def test_batches(simt_handle):
    B.check_batches(simt_handle)


@pytest.mark.parametrize("name", B.VOC_REFUSALS)
def test_vocabulary_refusal(simt_handle, name):
    B.check_voc_refusal(simt_handle, name)


@pytest.mark.parametrize("name", B.CALL_REFUSALS)
def test_call_refusal(simt_handle, name):
    B.check_call_refusal(simt_handle, name, conftest._simt_handle)


def test_chain_into_the_match(simt_handle):
    B.check_chain(simt_handle)


def test_vocabulary_file(simt_handle, tmp_path):
    B.check_voc_file(simt_handle, tmp_path)


@pytest.mark.parametrize("name", list(B.REPLAY_CASES))
def test_cpp_class_through_the_replay_tool(simt_handle, tmp_path, name):
    """BriefVocabulary and PoseGraph::detectLoop (host/pose_graph.h, vg_pack_bow) through `vins_replay_simt bow`"""
    conftest._build_simt()
    B.check_replay(simt_handle, os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, name)


def test_standalone_sanitizer_run(simt_handle, tmp_path):
    """tests/kf_bow_san_main.cpp with the emulated kernels, built with -fsanitize=address,undefined as a program of its own and run on two
    cases: no report, and every line (the decisions, the ids, the scores' bit patterns) equals the unsanitized run through the binding"""
    cxx = shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, simt = os.path.join(ROOT, "vins-mono_amd", "csrc"), conftest.SIMT_DIR
    flags = ["-O1", "-g", "-std=c++17", "-DVINS_SIMT", "-I" + simt, "-I" + src, "-Wno-attributes", "-Wno-unused-variable", "-Wno-unknown-pragmas",
             "-Wno-ignored-attributes", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize=alignment,vptr", "-fno-sanitize-recover=undefined",
             "-fno-omit-frame-pointer", "-Wno-psabi"]
    units = [["-x", "c++", os.path.join(src, "vg_core.hip")], ["-x", "c++", os.path.join(src, "fe_ransac.hip")],
             [os.path.join(simt, "simt_runtime.cpp")], [os.path.join(ROOT, "tests", "kf_bow_san_main.cpp")]]
    procs = [subprocess.Popen([cxx] + flags + ["-c"] + u + ["-o", str(tmp_path / f"u{i}.o")], stderr=subprocess.PIPE, text=True) for i, u in enumerate(units)]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-3000:]
    exe = str(tmp_path / "kf_bow_san")
    subprocess.run([cxx, "-fsanitize=address,undefined"] + [str(tmp_path / f"u{i}.o") for i in range(len(units))] + ["-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in ("stream_head", "nonuniform"):
        vname, frames, first = B.replay_frames(name)
        vb, fr = str(tmp_path / (name + ".voc.bin")), str(tmp_path / (name + ".frames.bin"))
        B.write_voc_bin(vb, B.voc(vname))
        B.write_frames(fr, frames, first)
        r = subprocess.run([exe, vb, fr], capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.stdout.splitlines() == B.binding_lines(simt_handle, name), name
