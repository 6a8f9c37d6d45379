"""FeatureTracker::readIntrinsicParameter of the stand-alone host class (vins-mono_amd/host/feature_tracker.cpp) on the two MEI settings
files the reference ships (config/black_box, config/3dm; copies under tests/golden/configs hold settings only): model MEI and exactly the
nine numbers a regular-expression read of the same file finds.  KANNALA_BRANDT is refused by name."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vins-mono_amd", "lib", "libvins_host.so")
CONFIGS = os.path.join(ROOT, "tests", "golden", "configs")
KEYS = ("gamma1", "gamma2", "u0", "v0", "k1", "k2", "p1", "p2")


def _read_camera(path):
    lib = C.CDLL(HOST)
    lib.vins_host_last_error.restype = C.c_char_p
    model, xi, p = C.c_int(-1), C.c_double(-1.0), np.zeros(8)
    rc = lib.vins_host_read_camera(path.encode(), C.byref(model), p.ctypes.data_as(C.POINTER(C.c_double)), C.byref(xi))
    return rc, model.value, p, xi.value, lib.vins_host_last_error().decode()


@pytest.mark.parametrize("name", ["black_box_config.yaml", "3dm_config.yaml"])
def test_reader_takes_the_reference_mei_files(name):
    path = os.path.join(CONFIGS, name)
    text = open(path).read()
    assert re.search(r"^model_type:\s*MEI\s*$", text, re.M)
    found = {k: float(re.search(r"^\s+%s:\s*(\S+)\s*$" % k, text, re.M).group(1)) for k in KEYS + ("xi",)}
    rc, model, p, xi, err = _read_camera(path)
    assert rc == 0, err
    assert model == 1                                            # VG_CAM_MEI
    assert xi == found["xi"] and [float(v) for v in p] == [found[k] for k in KEYS]
    assert xi > 1.0 and p[0] > 100.0                             # (the values are the files', not defaults)


def test_reader_refuses_kannala_brandt_by_name(tmp_path):
    cfg = tmp_path / "kb.yaml"
    cfg.write_text("%YAML:1.0\nmodel_type: KANNALA_BRANDT\ncamera_name: camera\nimage_width: 640\nimage_height: 480\n"
                   "projection_parameters:\n   k2: -0.01\n   k3: 0.03\n   k4: -0.04\n   k5: 0.01\n   mu: 380.0\n   mv: 380.0\n   u0: 320.0\n   v0: 240.0\n")
    rc, _, _, _, err = _read_camera(str(cfg))
    assert rc == -1 and "KANNALA_BRANDT" in err and "readIntrinsicParameter" in err, err
    rc, _, _, _, err = _read_camera(str(tmp_path / "missing.yaml"))
    assert rc == -1 and "missing.yaml" in err
