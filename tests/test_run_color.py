"""tools/run_rgbd.py --color and tools/run_kitti.py --color end to end on folders of colour PNGs written from the colourised synthetic
renderer: the device conversion gives the poses of the host conversion (the same integers), bit for bit."""
import os
import sys

import numpy as np
import pytest

import color_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731


@pytest.mark.gpu
def test_run_rgbd_color(tmp_path, monkeypatch):
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        cfg0, _, K, frames = cc.rgbd_world(o, cc.RGBD_SEEDS[0])
    finally:
        o.destroy()
    n, unit = len(frames), uc.DEPTH_UNIT
    cc.write_tum_folder_color(tmp_path / "seq", [(c, D) for c, D, _ in frames])
    intr = "%r,%r,%r,%r" % tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    lines = []
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, str(tmp_path / "color.txt"), depth_scale=4.0, log=lines.append, color=True,
                       map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"))
    assert any("converted to grey on the GPU" in ln for ln in lines), lines
    plain = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, depth_scale=4.0, log=QUIET)
    assert res["frames"] == n and res["error_flags"] == 0 and plain["error_flags"] == 0
    np.testing.assert_array_equal(res["poses"], plain["poses"])              # host conversion and device conversion: the same integers
    print("%d of %d frames tracking, %d landmarks, %d observations" % (res["tracking_frames"], n, len(res["map"]["id"]), len(res["observations"]["id"])))
    assert len(res["map"]["id"]) > 0 and len(res["observations"]["id"]) > 0
    g = hip.load()
    cfg, p = run_rgbd.configure(g, "tum", int(cfg0.rows), int(cfg0.cols), K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        for k, (c, D, G) in enumerate(frames):
            fi, _ = tr.process(G, D)
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
    finally:
        tr.destroy()


@pytest.mark.gpu
def test_run_kitti_color(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import color, hip, io_formats as io
    o = Oracle()
    scene = o.scene_kitti(scale=0.4, seed=7)
    n = 12
    frames = cc.stereo_colour_frames(o, [scene], n)
    seq, twin = tmp_path / "seq", tmp_path / "twin"
    for d in ("image_2", "image_3"):
        (seq / d).mkdir(parents=True)
    for d in ("image_0", "image_1"):
        (twin / d).mkdir(parents=True)
    grey = []
    for k, (L, R) in enumerate(frames):
        io.write_png(str(seq / "image_2" / ("%06d.png" % k)), L[0]); io.write_png(str(seq / "image_3" / ("%06d.png" % k)), R[0])
        gl, gr = color.to_gray_u8(L[0], color.RGB8), color.to_gray_u8(R[0], color.RGB8)
        io.write_png_gray8(str(twin / "image_0" / ("%06d.png" % k)), gl); io.write_png_gray8(str(twin / "image_1" / ("%06d.png" % k)), gr)
        grey.append((gl, gr))
    (seq / "calib.txt").write_text(cc.kitti_calib_text(scene))
    K, b = io.parse_kitti_calib(str(seq / "calib.txt"), (2, 3))
    (twin / "calib.txt").write_text("P0: %r 0 %r 0 0 %r %r 0 0 0 1 0\nP1: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % tuple(
        float(v) for v in (K[0, 0], K[0, 2], K[1, 1], K[1, 2], K[0, 0], K[0, 2], b[0], K[1, 1], K[1, 2])))
    lines = []
    res = run_kitti.run(str(seq), str(tmp_path / "color.txt"), "kitti", log=lines.append, color=True,
                        map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"))
    assert any("RGB -> grey on the GPU" in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0 and res["tracking_frames"] >= n - 1
    assert len(res["map"]["id"]) > 0 and len(res["observations"]["id"]) > 0
    # exact mode: a direct API run on the numpy-grey frames with the calibration of the colour cameras
    g = hip.load()
    cfg = io.apply_calib(g.default_config("kitti"), K, b, scene.rows, scene.cols)
    cfg.max_history_frames = 512
    g.create(cfg, 0, 1)
    try:
        for gl, gr in grey:
            g.process_host(gl, gr)
        np.testing.assert_array_equal(np.asarray(g.poses(0, 0, n)).reshape(n, 12), np.asarray(res["poses"]).reshape(n, 12))
    finally:
        g.destroy(); o.destroy()
    # frame-sharded mode: the twin folder of grey images with the same calibration in P0 / P1
    chunked = run_kitti.run(str(seq), None, "kitti", log=QUIET, color=True, chunks=3, overlap=3)
    chunked_twin = run_kitti.run(str(twin), None, "kitti", log=QUIET, chunks=3, overlap=3)
    assert chunked["frames"] == n and chunked["error_flags"] == 0
    np.testing.assert_array_equal(np.asarray(chunked["poses"]), np.asarray(chunked_twin["poses"]))
