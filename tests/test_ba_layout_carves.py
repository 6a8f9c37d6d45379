"""The BA layout and the kernels' LDS / scratch carves, checked without a GPU.

tests/layout/ba_layout_check.cpp is built with the plain host compiler from csrc/ba_layout_fn.h and csrc/ba_carve.h -- the
definitions that the host packer and the kernels read -- and walks a grid of window shapes (every branch of the layout code,
both sides of the fused-kernel and 8-wavefront thresholds, the large-window path, one shape per reachable refusal).  Its own
assertions cover the carves: regions ascend and do not overlap except where declared as aliases, every phase need fits the
region it reuses, the end of a carve is the byte count of the launch and inside the limit.  Its output, every BaLayout field
of every shape, is compared byte for byte with tests/golden/ba_layout_grid.txt, recorded from the commit before the carves
had one definition: no size or offset has moved since."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "layout", "ba_layout_check.cpp")
GOLDEN = os.path.join(HERE, "golden", "ba_layout_grid.txt")


@pytest.fixture(scope="module")
def checker_run(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ba_layout") / "ba_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", SRC, "-o", exe], check=True)
    return subprocess.run([exe], capture_output=True)


def test_every_carve_assertion_holds(checker_run):
    assert checker_run.returncode == 0, checker_run.stderr.decode()
    assert checker_run.stderr == b""


def test_layout_grid_matches_the_golden_byte_for_byte(checker_run):
    with open(GOLDEN, "rb") as f:
        golden = f.read()
    assert len(golden) < 100 * 1024
    out = checker_run.stdout
    if out != golden:
        a, b = out.decode().splitlines(), golden.decode().splitlines()
        names = a[0].split()[2:]
        for i, (la, lb) in enumerate(zip(a, b)):
            if la != lb:
                moved = [f"{n}: {y} -> {x}" for n, x, y in zip(names, la.split(), lb.split()) if x != y]
                pytest.fail(f"line {i + 1} ({a[i - 1].split(':')[0] if i else 'header'}) differs from the golden: {moved[:12] or (la, lb)}")
        pytest.fail(f"{len(a)} lines against {len(b)} in the golden")
