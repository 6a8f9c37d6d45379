"""The stand-alone host class (vins-mono_amd/host/feature_tracker.cpp) with a `model_type: MEI` settings file against the reference's own
FeatureTracker with the same file (oracle/_ref/libvins_ref_fe.so: feature_tracker.cpp + CataCamera.cc compiled unchanged): `vins_replay fe
<frames> <out> <config>` -- one vg_fe_read_image per frame, the camera set with vg_fe_set_camera -- gives per frame identical ids,
track_cnt and the bit patterns of cur_pts, cur_un_pts, pts_velocity; `fe_batch` (FeatureTrackerBatch, vg_fe_read_image_batch) with two
copies of the stream gives the single run's output twice."""
import os
import struct
import subprocess

import numpy as np
import pytest

import fe_scene
from oracle import ref_fe as RF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not RF.available("ref"), reason="oracle/_ref front-end libraries are not built")


def _write_frames(path, frames, pub_every=2):
    with open(path, "wb") as f:
        f.write(struct.pack("4i", len(frames), frames[0].shape[1], frames[0].shape[0], pub_every))
        for im in frames:
            f.write(im.tobytes())


def _parse(path):
    got = []
    for line in open(path):
        t = line.split()
        if t[0] == "frame":
            got.append([])
        else:
            got[-1].append([float(v) for v in t])
    return [np.array(g, np.float64).reshape(-1, 8) for g in got]


def _relabelled(path):
    """the lines of an `fe` output file with the ids renamed by order of first appearance: FeatureTracker::n_id is one counter for all
    trackers of a process, as in the reference, so the ids of the two trackers of a batch interleave; every other column stays the text it is"""
    names, out = {}, []
    for line in open(path):
        t = line.split()
        if t[0] != "frame":
            t[0] = str(names.setdefault(t[0], len(names)))
        out.append(" ".join(t))
    return out


def _check(exe, tmp_path, frames, cfg, min_tracks, min_cnt):
    path = tmp_path / "frames.bin"
    _write_frames(path, frames)
    r = subprocess.run([exe, "fe", str(path), str(tmp_path / "out.txt"), cfg], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    got = _parse(tmp_path / "out.txt")
    assert len(got) == len(frames)
    node = RF.Node(RF.lib(), cfg)
    for k, f in enumerate(frames):
        t = node.read_image(0.05 * k, f, k % 2 == 0)
        g = got[k]
        assert np.array_equal(g[:, 0].astype(np.int32), t['ids']) and np.array_equal(g[:, 1].astype(np.int32), t['track_cnt']), k
        for cols, key in ((slice(2, 4), 'cur_pts'), (slice(4, 6), 'cur_un_pts'), (slice(6, 8), 'pts_velocity')):
            assert np.array_equal(g[:, cols].astype(np.float32).view(np.uint32), t[key].view(np.uint32)), (k, key)
    assert len(t['ids']) >= min_tracks and t['track_cnt'].max() >= min_cnt, (len(t['ids']), t['track_cnt'].max())      # fixture condition
    # the lifted points are the MEI camera's: a pinhole with the same eight numbers gives other values
    # (x / z with z < 1 away from the principal point)
    assert np.abs(t['cur_un_pts']).max() > 0.3
    # fe_batch: two copies of the stream and the configuration -> the single run, twice
    lst = tmp_path / "list.txt"
    lst.write_text("%s\n%s\n" % (path, path))
    r = subprocess.run([exe, "fe_batch", str(lst), str(tmp_path / "b"), cfg], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    single = _relabelled(tmp_path / "out.txt")
    assert _relabelled(str(tmp_path / "b") + "0.txt") == single and _relabelled(str(tmp_path / "b") + "1.txt") == single


@needs_ref
def test_standalone_class_with_a_mei_file_equals_the_reference_tracker_on_emulated_kernels(tmp_path):
    exe = os.path.join(ROOT, "tests", "simt", "_build", "vins_replay_simt")
    if not os.path.exists(exe):
        pytest.skip("tests/simt is not built")
    frames = fe_scene.moving_scene(8, seed=17, width=320, height=240, velocity=(2.4, -1.1))
    cfg = RF.write_config(str(tmp_path / "cfg.yaml"), width=320, height=240, max_cnt=60, min_dist=16, equalize=1,
                          intr=(310.0, 309.0, 158.0, 121.5), dist=(-0.11, 0.04, 2e-4, -1e-4), mei_xi=0.9)
    _check(exe, tmp_path, frames, cfg, 30, 4)


@needs_ref
@pytest.mark.gpu
def test_standalone_class_with_a_mei_file_equals_the_reference_tracker_on_the_gpu(tmp_path):
    exe = os.path.join(ROOT, "vins-mono_amd", "lib", "vins_replay")
    frames = fe_scene.moving_scene(12, seed=18)
    cfg = RF.write_config(str(tmp_path / "cfg.yaml"), intr=(730.0, 728.0, 371.0, 243.5), dist=(-0.11, 0.04, 2e-4, -1e-4), mei_xi=0.9)
    _check(exe, tmp_path, frames, cfg, 30, 4)


def test_replay_refuses_an_unsupported_camera_model_by_name(tmp_path):
    exe = os.path.join(ROOT, "tests", "simt", "_build", "vins_replay_simt")
    if not os.path.exists(exe):
        pytest.skip("tests/simt is not built")
    frames = fe_scene.moving_scene(1, seed=17, width=320, height=240)
    _write_frames(tmp_path / "frames.bin", frames)
    cfg = RF.write_config(str(tmp_path / "cfg.yaml"), width=320, height=240, mei_xi=0.9)
    text = open(cfg).read().replace("model_type: MEI", "model_type: SCARAMUZZA")
    open(cfg, "w").write(text)
    r = subprocess.run([exe, "fe", str(tmp_path / "frames.bin"), str(tmp_path / "out.txt"), cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "SCARAMUZZA" in r.stderr, r.stderr
