"""vg_voc_load / vg_bow_* / vg_kf_loop_detect on the MI355X: the check bodies of tests/kf_bow_ref.py through the real library.  Reads nothing
outside the repository."""
import os

import pytest

import conftest
import kf_bow_ref as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(B.VOCS))
def test_walk_and_vector(handle, name):
    B.check_walk(handle, name, B.WALK_SIZES)


def test_walk_large_records(handle):
    B.check_walk(handle, "k10L3", B.WALK_LARGE)


def test_vector_cases(handle):
    B.check_vector(handle)


def test_stream_of_70_keyframes(handle):
    B.check_stream(handle)


def test_tie_rule(handle):
    B.check_tie(handle)


def test_flags_and_state(handle):
    B.check_flags_and_state(handle)


def test_batches(handle):
    B.check_batches(handle)


def test_vocabulary_refusals(handle):
    for name in B.VOC_REFUSALS:
        B.check_voc_refusal(handle, name)


def test_call_refusals(handle):
    for name in B.CALL_REFUSALS:
        B.check_call_refusal(handle, name, conftest.new_handle)


def test_chain_into_the_match(handle):
    B.check_chain(handle)


def test_vocabulary_file(handle, tmp_path):
    B.check_voc_file(handle, tmp_path)


@pytest.mark.parametrize("name", list(B.REPLAY_CASES))
def test_cpp_class_through_the_replay_tool(handle, tmp_path, name):
    """BriefVocabulary and PoseGraph::detectLoop (host/pose_graph.h, vg_pack_bow) through `vins_replay bow`, number for number"""
    B.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)
