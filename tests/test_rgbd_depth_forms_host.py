"""CPU: the premises of tests/test_rgbd_depth_forms_gpu.py, from the checker loop (tests/rgbd_loop.py over the oracle) and the oracle's
space maps alone.  With a depth camera that is not the colour camera the tum configuration still locks on, most destinations are filled
from another pixel, and tens of thousands of destinations see a LARGER winning depth than a frame before: a z-buffer left armed with
the previous frame's minimum would keep the smaller one."""
import numpy as np
import pytest

import depth_cases as dc


@pytest.mark.parametrize("kind", ["offset", "crossing"])
def test_premises_of_the_loop_forms(kind):
    run = dc.checker_run(kind, dc.LOOP_SEEDS[0])
    assert dc.is_plain(run["p"]) == (kind == "crossing")
    pr = dc.loop_premises(run)
    dc.assert_loop_premises(pr, kind)
    assert all(len(p["xy"]) >= 100 for p in run["points"])
    for seed in dc.LOOP_SEEDS[1:]:
        other = dc.checker_run(kind, seed)
        assert other["info"][-1]["status"] == 1 and other["info"][-1]["n_tracked"] >= 50
        assert all(not np.array_equal(a[1], b[1]) for a, b in zip(run["frames"], other["frames"]))     # another depth image every frame


def test_premises_of_the_shut_gate_and_the_strip_walk():
    run = dc.checker_run("crossing", dc.LOOP_SEEDS[1], zero_first=True)
    assert not run["frames"][0][1].any() and run["info"][0]["n_points"] == 0
    assert all(i["status"] == 1 for i in run["info"][5:]) and min(i["n_tracked"] for i in run["info"][5:]) >= 50
    reg = dc.checker_run("registered", dc.LOOP_SEEDS[0])
    assert dc.is_plain(reg["p"]) and dc.loop_premises(reg)["moved"] == [0] * dc.LOOP_FRAMES     # every source lands on itself: the gate stays shut
    for B in dc.STRIP_BATCHES:                                                                    # rgbd_device.h: k_depth_direct's grid has fewer row blocks than rows
        assert reg["p"].rows > max(8, 4096 // B)
    # which rows the tracker's outputs can observe: a feature keeps 31 px from the border, so the 24-stream batch's second step (rows 170 ..) is
    # not observable from the point lists, the 48-stream batch's second and third (rows 85 ..) are
    ys = np.concatenate([q["xy"][:, 1] for q in reg["points"]])
    assert ys.max() < 4096 // dc.STRIP_BATCHES[0] and int((ys >= 4096 // dc.STRIP_BATCHES[1]).sum()) >= 500
