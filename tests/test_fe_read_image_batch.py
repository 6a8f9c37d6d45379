"""vg_fe_read_image_batch -- FeatureTracker::readImage of every stream of a handle in one call -- held to vg_fe_read_image on a
single-stream handle, field by field and bit by bit (tests/fe_read_image_batch_case.py), and the host class on top of it
(FeatureTrackerBatch, `vins_replay fe_batch`) held to `vins_replay fe` of each stream alone."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import conftest
import fe_read_image_batch_case as case
print("RESULT", case.%(fn)s(conftest._simt_handle(), conftest._simt_handle()))
"""


def _child(fn):
    r = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT, fn=fn)], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0 and "RESULT" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
    return eval(r.stdout[r.stdout.index("RESULT") + 6:].strip().splitlines()[0])


_REFUSALS = ["points without a previous frame", "n_streams != n_cams", "n > max_points", "mixed equalize",
             "mixed min_dist among publishing streams", "some-but-not-all img NULL", "callback failure"]


@pytest.fixture(scope="module")
def seven_on_the_emulator():
    return _child("run")


def test_batch_equals_the_single_stream_call_on_emulated_kernels(seven_on_the_emulator):
    """seven streams of different kinds at 320x240 advancing together over five frames, every field of every output"""
    import fe_read_image_batch_case as case
    case.check_coverage(seven_on_the_emulator)


def test_resident_frames_equal_uploaded_frames_on_emulated_kernels(seven_on_the_emulator):
    """imgs=None after upload_frames: the same outputs as the call that uploads (compared inside the same run)"""
    assert seven_on_the_emulator["resident_frames"] >= 2, seven_on_the_emulator


def test_refusals_leave_every_stream_where_it_was_on_emulated_kernels():
    assert _child("run_refusals") == _REFUSALS


@pytest.mark.gpu
def test_batch_equals_the_single_stream_call_on_the_gpu(handle):
    import conftest
    import fe_read_image_batch_case as case
    other = conftest.new_handle()
    try:
        seen = case.run(handle, other, W=752, H=480, n_frames=8)
        print("coverage", seen)
        case.check_coverage(seen)
        assert seen["resident_frames"] >= 2
    finally:
        other.close()


@pytest.mark.gpu
def test_256_streams_equal_256_single_stream_runs_on_the_gpu(handle):
    """the headline size: 256 streams, 150 points, 752x480, CLAHE on, two published frames; the single-stream side runs stream after stream
    on ONE handle"""
    import conftest
    import fe_read_image_batch_case as case
    other = conftest.new_handle()
    try:
        seen = case.run_headline(handle, other)
        print("headline", seen)
        assert seen["streams"] == 256 and seen["ransac_device"] >= 128, seen
    finally:
        other.close()


@pytest.mark.gpu
def test_refusals_leave_every_stream_where_it_was_on_the_gpu(handle):
    import conftest
    import fe_read_image_batch_case as case
    other = conftest.new_handle()
    try:
        assert case.run_refusals(handle, other) == _REFUSALS
    finally:
        other.close()


# ---- FeatureTrackerBatch through the replay harness
def _write_frames(path, frames, pub_every):
    with open(path, "wb") as f:
        f.write(struct.pack("4i", len(frames), frames[0].shape[1], frames[0].shape[0], pub_every))
        for im in frames:
            f.write(np.ascontiguousarray(im, np.uint8).tobytes())


def _relabelled(path):
    """the lines of an `fe` output file with the ids renamed by order of first appearance (FeatureTracker::n_id is one counter for all
    trackers of a process: the ids of S trackers interleave); every other column stays the text it is"""
    names, out = {}, []
    for line in open(path):
        t = line.split()
        if t[0] != "frame":
            t[0] = str(names.setdefault(t[0], len(names)))
        out.append(" ".join(t))
    return out


def _host_class_replay(exe, tmp_path, W, H, n_frames):
    import fe_scene
    S, pub_every = 4, 2
    paths = []
    for c in range(S):
        frames = fe_scene.moving_scene(n_frames, seed=21 + 5 * c, width=W, height=H, velocity=(2.4 + 0.5 * c, -1.1 - 0.4 * c))
        paths.append(str(tmp_path / ("frames%d.bin" % c)))
        _write_frames(paths[-1], frames, pub_every)
    (tmp_path / "list.txt").write_text("\n".join(paths) + "\n")
    r = subprocess.run([exe, "fe_batch", str(tmp_path / "list.txt"), str(tmp_path / "batch_")], capture_output=True, text=True, timeout=2400)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    tracked = 0
    for c in range(S):
        r = subprocess.run([exe, "fe", paths[c], str(tmp_path / ("single_%d.txt" % c))], capture_output=True, text=True, timeout=2400)
        assert r.returncode == 0, r.stderr[-3000:]
        got, want = _relabelled(str(tmp_path / ("batch_%d.txt" % c))), _relabelled(str(tmp_path / ("single_%d.txt" % c)))
        assert len(want) > n_frames and got == want, (c, [(a, b) for a, b in zip(got, want) if a != b][:5])
        tracked += sum(1 for line in want if not line.startswith("frame") and int(line.split()[1]) >= 3)
    assert tracked >= 4 * 10, tracked              # (points that lived through three frames on every stream: the lists did carry over)


def test_host_class_replay_of_four_streams_equals_four_single_replays_on_emulated_kernels(tmp_path):
    import conftest
    conftest._build_simt()
    _host_class_replay(os.path.join(conftest.SIMT_DIR, "_build", "vins_replay_simt"), tmp_path, 320, 240, 4)


@pytest.mark.gpu
def test_host_class_replay_of_four_streams_equals_four_single_replays_on_the_gpu(pkg, tmp_path):
    exe = os.path.join(os.path.dirname(pkg.LIB_PATH), "vins_replay")
    assert os.path.exists(exe), "vins_replay is not built"
    _host_class_replay(exe, tmp_path, 752, 480, 8)
