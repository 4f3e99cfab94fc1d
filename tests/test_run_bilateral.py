"""tools/run_rgbd.py --bilateral end to end on a TUM folder with noisy depth PNGs written from the synthetic renderer: the poses equal a
direct API run bit for bit, with no error flag; the same with --map and --observations."""
import os
import sys

import numpy as np
import pytest

import bilateral_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.gpu
def test_run_rgbd_bilateral(tmp_path, monkeypatch):
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=13)
        scene.speed_m = 0.25; scene.sway_m = 0.4
        n, unit = 12, uc.DEPTH_UNIT
        rng = np.random.default_rng(1013)
        frames = [(L, bc.add_noise(D, rng)) for L, D in uc.render_frames(o, scene, n)]
        gt = uc.ground_truth(o, scene, n)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    lines = []
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, str(tmp_path / "bl.txt"), depth_scale=4.0, log=lines.append, bilateral=(0.0, 2.0))
    assert any("bilateral filter on the GPU" in ln and "sigma colour 2, sigma space 2" in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0 and res["tracking_frames"] >= n - 3
    both = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, str(tmp_path / "bl2.txt"), depth_scale=4.0, log=lambda *_: None, bilateral=(2.0, 2.0),
                        map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"))
    assert both["error_flags"] == 0 and len(both["map"]["id"]) > 50 and len(both["observations"]["id"]) > 200
    np.testing.assert_array_equal(both["poses"], res["poses"])
    plain = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, depth_scale=4.0, log=lambda *_: None)
    assert not np.array_equal(plain["poses"], res["poses"])          # the flag does something
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", scene.rows, scene.cols, K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_bilateral(True)
        for k, (L, D) in enumerate(frames):
            fi, _ = tr.process(L, D)
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
            assert fi.error_flags == 0
    finally:
        tr.destroy()
