"""vg_kf_pnp on the MI355X: the case table, the capacity pair, batch-equals-single, the failed pair between good neighbours and every
refusal of tests/kf_pnp_ref.py through the real library.  Reads nothing outside the repository."""
import os

import pytest

import conftest
import kf_pnp_ref as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(handle):
    return K.check_cases(handle, 'gpu')


def test_every_case_within_the_bound(table):
    assert set(table) == set(K.CASE_ARGS)


def test_capacity_pair(handle):
    K.check_capacity(handle, 'gpu')


def test_batch_equals_single_pairs(handle):
    K.check_batch_equals_single(handle, (1, 3, 33))


def test_failed_pair_leaves_its_neighbours(handle):
    K.check_failed_neighbours(handle)


def test_refusals(handle):
    for name in K.REFUSALS:
        K.check_refusal(handle, name)


def test_chain_into_the_relocalisation_frame(handle):
    """vg_kf_add -> vg_kf_match -> vg_kf_pnp -> vg_ba_seq_set_relo -> a step -> vg_ba_seq_get_relo: bit-identical to the step fed the reference's lists"""
    h_ref = conftest.new_handle()
    try:
        K.check_chain(handle, h_ref)
    finally:
        h_ref.close()


@pytest.mark.parametrize("name", K.REPLAY_CASES)
def test_cpp_class_through_the_replay_tool(handle, tmp_path, name):
    """KeyFrame::PnPRANSAC / findConnection (host/keyframe.h, vg_pack_kf_pnp) through `vins_replay kfpnp`, number for number"""
    K.check_replay(handle, os.path.join(conftest.ROOT, "vins-mono_amd", "lib", "vins_replay"), tmp_path, name)
