"""tools/run_kitti.py --equalize and tools/run_rgbd.py --equalize end to end on low-contrast folders written from the synthetic renderer:
with the flag the run tracks, without it the same folder does not.  The folder lengths and contrasts were chosen on the CPU oracle alone
(stereo: contrast 0.15, 16 frames: equalised TRACKING from frame 1 on, raw never; RGB-D, tum configuration: contrast 0.06, 24 frames:
equalised TRACKING from frame 2 on, raw never — its detector threshold of 10 still tracks at contrast 0.15)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731


@pytest.mark.gpu
def test_run_kitti_equalize(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, io_formats as io
    o = Oracle()
    scene = o.scene_kitti(scale=0.4, seed=7)
    scene.contrast = 0.15
    n = 16
    seq = tmp_path / "seq"
    (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir(parents=True)
    frames, gt = [], []
    for k in range(n):
        L, R = o.render(scene, k)
        io.write_png_gray8(str(seq / "image_0" / ("%06d.png" % k)), L)
        io.write_png_gray8(str(seq / "image_1" / ("%06d.png" % k)), R)
        frames.append((L, R)); gt.append(np.array(o.gt_pose(scene, k)).reshape(12))
    with open(seq / "calib.txt", "w") as f:
        f.write("P0: %r 0 %r 0 0 %r %r 0 0 0 1 0\n" % (scene.fx, scene.cx, scene.fy, scene.cy))
        f.write("P1: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (scene.fx, scene.cx, -scene.fx * scene.baseline_m, scene.fy, scene.cy))
    (seq / "times.txt").write_text("\n".join("%.6f" % (0.1 * k) for k in range(n)) + "\n")
    io.write_trajectory_kitti(str(tmp_path / "gt.txt"), np.array(gt))
    lines = []
    res = run_kitti.run(str(seq), str(tmp_path / "eq.txt"), "kitti", str(tmp_path / "gt.txt"), log=lines.append, equalize=True,
                        map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"))
    assert any("equalising histograms on the GPU" in ln for ln in lines), lines
    plain = run_kitti.run(str(seq), str(tmp_path / "plain.txt"), "kitti", str(tmp_path / "gt.txt"), log=QUIET)
    chunked = run_kitti.run(str(seq), str(tmp_path / "chunks.txt"), "kitti", str(tmp_path / "gt.txt"), log=QUIET, equalize=True, chunks=3, overlap=3)
    print("ATE-RMSE after alignment over %d frames: --equalize %.4f m, --equalize --chunks 3 %.4f m, without the flag %.4f m" % (
        n, res["ate_rmse_aligned"], chunked["ate_rmse_aligned"], plain["ate_rmse_aligned"]))
    assert res["frames"] == n and res["error_flags"] == 0
    assert res["tracking_frames"] >= 0.9 * n, res["tracking_frames"]
    assert n - plain["tracking_frames"] >= 0.9 * n, plain["tracking_frames"]
    assert chunked["frames"] == n and chunked["error_flags"] == 0
    assert len(res["map"]["id"]) > 50 and len(res["observations"]["id"]) > 200
    # exact mode: the poses of a direct API run on the same arrays
    g = hip.load()
    g.create(o.config_for_scene(scene), 0, 1)
    try:
        g.set_equalization(True)
        for L, R in frames:
            g.process_host(L, R)
        np.testing.assert_array_equal(np.asarray(g.poses(0, 0, n)).reshape(n, 12), np.asarray(res["poses"]).reshape(n, 12))
    finally:
        g.destroy(); o.destroy()


@pytest.mark.gpu
def test_run_rgbd_equalize(tmp_path, monkeypatch):
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import evaluation, hip
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=13)
        scene.speed_m = 0.25; scene.sway_m = 0.4; scene.contrast = 0.06
        n, unit = 24, uc.DEPTH_UNIT
        frames = uc.render_frames(o, scene, n)
        gt = uc.ground_truth(o, scene, n)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    lines = []
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, str(tmp_path / "eq.txt"), depth_scale=4.0, log=lines.append, equalize=True,
                       map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"))
    assert any("equalising histograms on the GPU" in ln for ln in lines), lines
    plain = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, depth_scale=4.0, log=QUIET)
    print("ATE RMSE after alignment over %d frames: --equalize %.4f m, without the flag %.4f m" % (
        n, evaluation.ate_rmse(res["poses"], gt), evaluation.ate_rmse(plain["poses"], gt)))
    assert res["frames"] == n and res["error_flags"] == 0
    assert res["tracking_frames"] >= 0.9 * n, res["tracking_frames"]
    assert n - plain["tracking_frames"] >= 0.9 * n, plain["tracking_frames"]
    assert len(res["map"]["id"]) > 50 and len(res["observations"]["id"]) > 200
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", scene.rows, scene.cols, K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_equalization(True)
        for k, (L, D) in enumerate(frames):
            fi, _ = tr.process(L, D)
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
    finally:
        tr.destroy()
