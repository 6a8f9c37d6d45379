"""The contract of vg_fe_set_camera / vg_fe_lift (include/vinsgpu.h) on the emulated kernels: every refusal is VG_ERR_BAD_ARG and leaves
the stream's next frame identical to a run without the refused call; set_camera(NULL) and a fresh vg_fe_configure return a stream to
results bit-identical to a handle that never had a camera; a PINHOLE vg_fe_camera gives the frame the same numbers in intr give
(tests/fe_camera_case.py: check_abi)."""
import fe_camera_case as case


def test_set_camera_and_lift_contract_on_emulated_kernels():
    assert case.run_emulated("fe_camera_case", "case.check_abi(H(), H())") is True
