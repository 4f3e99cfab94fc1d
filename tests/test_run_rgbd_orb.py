"""tools/run_rgbd.py --detector ORB on the device-resident loop: with --map --observations on a written TUM folder the poses and the bundle
equal a direct API run, and the mask flags end with the library's own message."""
import os
import sys

import numpy as np
import pytest

from test_rgbd_map_gpu import _same, _write_tum_folder
from vslam_pose_estimation_framework_amd import hip
from vslam_pose_estimation_framework_amd.capi import RgbdTracker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
MAP_KEYS = ("id", "xyz", "first_frame", "last_frame", "updates", "desc")
OBS_KEYS = ("id", "frame", "xy", "cam")


@pytest.mark.gpu
def test_run_rgbd_orb_detector_with_map_and_observations(tmp_path, monkeypatch):
    import run_rgbd
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import io_formats
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=67)
        scene.speed_m = 0.25; scene.sway_m = 0.4
        n, unit = 8, 2e-3
        frames = _write_tum_folder(tmp_path / "seq", o, scene, n, unit)
    finally:
        o.destroy()
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    ply, npz = str(tmp_path / "map.ply"), str(tmp_path / "bundle.npz")
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, detector=1, depth_scale=4.0, log=lambda s: None, map_path=ply, obs_path=npz)
    assert res["frames"] == n and res["error_flags"] == 0
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", scene.rows, scene.cols, K, unit, 1, 1, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.enable_map(4000); tr.enable_observations(40000)
        poses = [np.array(tr.process(L, D)[0].camera_left_to_world) for L, D in frames]
        m, ob = tr.map(), tr.observations()
        xy = tr.points()["xy"]
    finally:
        tr.destroy()
    assert len(m["id"]) >= 20 and len(ob["id"]) > 100
    assert (xy != np.rint(xy)).any()                      # float keypoints of the upper pyramid levels: the OrbDetector did run
    b = io_formats.read_bundle_rgbd(npz)
    np.testing.assert_array_equal(b["poses"], np.array(poses).reshape(n, 12))
    _same(b["map"], m, MAP_KEYS, "bundle map")
    _same({k: b["obs_" + k] for k in OBS_KEYS}, ob, OBS_KEYS, "bundle log")
    cloud = io_formats.read_ply(ply)
    np.testing.assert_array_equal(cloud["xyz"].view(np.uint64), m["xyz"].view(np.uint64))
    # a mask flag: refused with the library's message
    mask = np.full((scene.rows, scene.cols), 255, np.uint8)
    io_formats.write_png(str(tmp_path / "mask.png"), mask)
    with pytest.raises(SystemExit) as e:
        run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, detector=1, depth_scale=4.0, log=lambda s: None, mask=str(tmp_path / "mask.png"))
    assert "detector_type ORB" in str(e.value) and "resizes its mask" in str(e.value)
