"""tools/run_kitti.py --clahe and tools/run_rgbd.py --clahe end to end on unevenly lit folders written from the synthetic renderer (the
shaded scene of clahe_cases.py): the poses equal a direct API run bit for bit; with the flag the stereo run tracks, without it the same
folder does not (chosen on the CPU oracle alone: 16 frames, with numpy CLAHE TRACKING from frame 1 on, raw never); --chunks 3 equals
--chunks 3 on a twin folder of numpy-CLAHE images."""
import os
import sys

import numpy as np
import pytest

import clahe_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731


def _write_kitti(io, seq, scene, frames):
    (seq / "image_0").mkdir(parents=True); (seq / "image_1").mkdir(parents=True)
    for k, (L, R) in enumerate(frames):
        io.write_png_gray8(str(seq / "image_0" / ("%06d.png" % k)), L)
        io.write_png_gray8(str(seq / "image_1" / ("%06d.png" % k)), R)
    with open(seq / "calib.txt", "w") as f:
        f.write("P0: %r 0 %r 0 0 %r %r 0 0 0 1 0\n" % (scene.fx, scene.cx, scene.fy, scene.cy))
        f.write("P1: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (scene.fx, scene.cx, -scene.fx * scene.baseline_m, scene.fy, scene.cy))
    (seq / "times.txt").write_text("\n".join("%.6f" % (0.1 * k) for k in range(len(frames))) + "\n")


@pytest.mark.gpu
def test_run_kitti_clahe(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, io_formats as io
    o = Oracle()
    scene = cc.shaded_scene(o)
    n = 16
    frames, gt = [], []
    for k in range(n):
        L, R = cc.render_shaded(o, [scene], k)
        frames.append((L[0], R[0])); gt.append(np.array(o.gt_pose(scene, k)).reshape(12))
    _write_kitti(io, tmp_path / "seq", scene, frames)
    _write_kitti(io, tmp_path / "twin", scene, [(cc.clahe_image(L), cc.clahe_image(R)) for L, R in frames])
    io.write_trajectory_kitti(str(tmp_path / "gt.txt"), np.array(gt))
    seq, twin, gtp = str(tmp_path / "seq"), str(tmp_path / "twin"), str(tmp_path / "gt.txt")
    lines = []
    res = run_kitti.run(seq, str(tmp_path / "clahe.txt"), "kitti", gtp, log=lines.append, clahe=40.0, map_path=str(tmp_path / "map.ply"),
                        obs_path=str(tmp_path / "bundle.npz"))
    assert any("CLAHE on the GPU" in ln for ln in lines), lines
    plain = run_kitti.run(seq, str(tmp_path / "plain.txt"), "kitti", gtp, log=QUIET)
    chunked = run_kitti.run(seq, str(tmp_path / "chunks.txt"), "kitti", gtp, log=QUIET, clahe=40.0, chunks=3, overlap=3)
    chunked_twin = run_kitti.run(twin, str(tmp_path / "chunks_twin.txt"), "kitti", gtp, log=QUIET, chunks=3, overlap=3)
    assert res["frames"] == n and res["error_flags"] == 0
    assert res["tracking_frames"] >= 0.9 * n, res["tracking_frames"]
    assert n - plain["tracking_frames"] >= 0.9 * n, plain["tracking_frames"]
    assert chunked["frames"] == n and chunked["error_flags"] == 0
    np.testing.assert_array_equal(np.asarray(chunked["poses"]), np.asarray(chunked_twin["poses"]))
    assert len(res["map"]["id"]) > 50 and len(res["observations"]["id"]) > 200
    # exact mode: the poses of a direct API run on the same arrays, with the tiles the flag's default names
    g = hip.load()
    g.create(o.config_for_scene(scene), 0, 1)
    try:
        g.set_clahe(True, 40.0, (8, 8))
        for L, R in frames:
            g.process_host(L, R)
        np.testing.assert_array_equal(np.asarray(g.poses(0, 0, n)).reshape(n, 12), np.asarray(res["poses"]).reshape(n, 12))
    finally:
        g.destroy(); o.destroy()


@pytest.mark.gpu
def test_run_rgbd_clahe(tmp_path, monkeypatch):
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=13)
        scene.speed_m = 0.25; scene.sway_m = 0.4; scene.contrast = 0.3
        n, unit = 12, uc.DEPTH_UNIT
        frames = [(cc.shade(L), D) for L, D in uc.render_frames(o, scene, n)]
        gt = uc.ground_truth(o, scene, n)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    lines = []
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, str(tmp_path / "clahe.txt"), depth_scale=4.0, log=lines.append, clahe=4.0,
                       clahe_tiles=(4, 2), map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"))
    assert any("CLAHE on the GPU" in ln and "4 x 2" in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", scene.rows, scene.cols, K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_clahe(True, 4.0, (4, 2))
        for k, (L, D) in enumerate(frames):
            fi, _ = tr.process(L, D)
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
    finally:
        tr.destroy()
