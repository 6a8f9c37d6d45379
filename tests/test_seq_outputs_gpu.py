"""GPU tests of the keyframe message and the point clouds of a resident sequence (vg_ba_seq_outputs_reserve / _async /
vg_ba_seq_get_outputs; csrc/ba_seq.hip ba_seq_publish_kernel): the cases of tests/seq_outputs_case.py, which
tests/test_seq_outputs_simt.py runs on the emulated kernels, at the same small shapes."""
import pytest

import conftest
import seq_outputs_case as S
import seq_outputs_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def two_handles():
    a, b = conftest.new_handle(), conftest.new_handle()
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


def test_chain_from_the_keyframe_message_into_the_relocalisation_frame(two_handles):
    """Case 7: vg_vio_step_async on rendered 752x480 frames (windows of K = 11) until a keyframe is valid, then the message through
    vg_kf_add -> vg_kf_match -> vg_kf_pnp -> vg_ba_seq_set_relo -> a step -> vg_ba_seq_get_relo, bit-identical to the restatement's lists."""
    import vio_bridge_case as case
    n_kf, n_matched, n_inliers, n_factors = S.case_chain(*two_handles, case.Data(11, 0, False, plan="PPPPPP"))
    assert n_matched > 8 and n_inliers > 8 and n_factors >= 2


def test_cpp_replay_with_published_outputs(two_handles, tmp_path):
    """Case 8: `vins_replay seq` with VINS_REPLAY_OUTPUTS on the GPU."""
    import os
    exe = os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt") if os.environ.get("VINS_TEST_SIMT") == "1" else os.path.join(
        conftest.ROOT, "vins-mono_amd", "lib", "vins_replay")
    S.case_cpp(two_handles[0], exe, tmp_path, timeout=300)
