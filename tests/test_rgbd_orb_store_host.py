"""CPU side of detector_type ORB on the device-resident RGB-D loop (csrc/orb_plan.h): the pyramid plan that vslam_orb_detect and the device
loop share against make_golden.orb_detect_ref's own level sizes and quotas, and the feature store's index arithmetic walked by
tests/cpp/orb_store_walk.cpp against scalar loops.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("orb_store") / "orb_store_walk")
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "orb_store_walk.cpp")])
    return exe


def _golden_plan(rows, cols, monkeypatch):
    """Level sizes and quotas as make_golden.orb_detect_ref itself computes them: its resize and its retainBest are replaced by recorders."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    sizes, keeps = [(rows, cols)], []
    monkeypatch.setattr(mg, "resize_linear_ref", lambda img, nr, nc: (sizes.append((nr, nc)), np.zeros((nr, nc), np.uint8))[1])
    monkeypatch.setattr(mg, "fast9_16", lambda img, thr: [])
    monkeypatch.setattr(mg, "retain_best_ref", lambda kps, n: (keeps.append(n), kps)[1])
    mg.orb_detect_ref(np.zeros((rows, cols), np.uint8), 5000, 1.2, 8, 31, 31, 20)
    assert len(keeps) == 2 * len(sizes) and all(keeps[2 * l] == 2 * keeps[2 * l + 1] for l in range(len(sizes)))
    return sizes, keeps[1::2]


# the sizes the GPU tests run at (188 x 620 whole and as a 2 x 2 grid's region, the smallest shapes: 83 and 84 rows) and 376 x 1241
@pytest.mark.parametrize("rows,cols", [(188, 620), (96, 312), (83, 845), (84, 845), (70, 70), (376, 1241), (480, 640)])
def test_plan_equals_the_golden_reference(rows, cols, walk, monkeypatch):
    sizes, quotas = _golden_plan(rows, cols, monkeypatch)
    out = subprocess.check_output([walk, "plan", str(rows), str(cols)]).decode().split("\n")
    n = int(out[0])
    got = [tuple(int(v) for v in line.split()) for line in out[1:9]]
    assert n == len(sizes), (n, sizes)
    assert [g[:2] for g in got[:n]] == sizes
    assert [g[2] for g in got[:n]] == quotas
    assert sum(g[2] for g in got) == 5000                     # the quotas are a series over all eight levels, whatever the image holds
    if rows in (83, 84):
        assert n == (1 if rows == 83 else 2) and (rows == 83 or sizes[1][0] == 70)


def test_store_index_arithmetic_walk(walk):
    out = subprocess.check_output([walk]).decode()
    assert out.strip().endswith("300 cases, 0 mismatches"), out
