"""vg_pg_optimize on the MI355X: the case table, batch-equals-single, the failed graph between good neighbours, every refusal, the chain
from vg_kf_pnp and the capacity pair of tests/kf_pgo_ref.py through the real library.  Reads nothing outside the repository."""
import os

import pytest

import conftest
import kf_pgo_ref as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(handle):
    return K.check_cases(handle, 'gpu')


def test_every_case_within_the_bound(table):
    assert set(table) == set(K.CASE_ARGS)


def test_batch_equals_single_graphs(handle):
    K.check_batch_equals_single(handle, (1, 3, 33))


def test_failed_graph_leaves_its_neighbours(handle):
    K.check_failed_neighbours(handle)


def test_refusals(handle):
    for name in K.REFUSALS:
        K.check_refusal(handle, name)


def test_chain_from_the_pnp_stage(handle):
    K.check_chain(handle)


@pytest.mark.parametrize("name", K.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(handle, tmp_path, name):
    """PoseGraph::addKeyFrame's pose bookkeeping and optimize4DoF (host/pose_graph.h, vg_pack_pg) through `vins_replay pgo`, number for number"""
    K.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)


def test_capacity_pair(handle):
    """VG_PG_MAX_KEYFRAMES keyframes with two loop edges against the pcg64 route ONLY (the long-double and the dense float64 routes are too
    large at 8188 unknowns; E64 there is the disagreement of scipy's sparse LU on the same system with pcg64); one keyframe more is refused"""
    K.check_capacity(handle, 'gpu')
