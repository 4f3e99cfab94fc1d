"""tools/run_kitti.py --downscale 2 end to end on a written KITTI folder of 301 x 993 (image_0 / image_1 grey, image_2 / image_3 colour): the
poses are those of a direct run through the API at the scaled calibration, in exact and in frame-sharded mode, and with --color --map
--map-color the PLY's colours are the API's; a raw EuRoC-shaped rig through --rectify --downscale 2 (maps over the scaled cameras); a
written TUM folder of 376 x 1241 through tools/run_rgbd.py --downscale 2.  The ATE against the scenes' ground truth, and against the
full-resolution run of the same folder, is printed (DESIGN.md 6o carries the figures), not asserted."""
import os
import sys

import numpy as np
import pytest

import color_cases as cc
import downscale_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731
FRAMES = 12


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """(path, scene, grey frames, colour frames, ground-truth poses [n, 12])"""
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import io_formats as io
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=dc.STEREO_SCALE[2], seed=7)
        grey = [o.render(scene, k) for k in range(FRAMES)]
        gt = np.stack([o.gt_pose(scene, k).reshape(12) for k in range(FRAMES)])
    finally:
        o.destroy()
    rng = np.random.default_rng(107)
    colour = [(cc.colourise(L, rng), cc.colourise(R, rng)) for L, R in grey]
    seq = tmp_path_factory.mktemp("kitti") / "seq"
    for d in ("image_0", "image_1", "image_2", "image_3"):
        (seq / d).mkdir(parents=True)
    for k in range(FRAMES):
        io.write_png_gray8(str(seq / "image_0" / ("%06d.png" % k)), grey[k][0]); io.write_png_gray8(str(seq / "image_1" / ("%06d.png" % k)), grey[k][1])
        io.write_png(str(seq / "image_2" / ("%06d.png" % k)), colour[k][0]); io.write_png(str(seq / "image_3" / ("%06d.png" % k)), colour[k][1])
    fx, fy, cx, cy, b = (float(v) for v in (scene.fx, scene.fy, scene.cx, scene.cy, scene.baseline_m))
    rows = [("P0", 0.0), ("P1", -fx * b), ("P2", 0.0), ("P3", -fx * b)]
    (seq / "calib.txt").write_text("".join("%s: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (n, fx, cx, tx, fy, cy) for n, tx in rows))
    return str(seq), scene, grey, colour, gt


def _config(g, seq, scene, history):
    from vslam_pose_estimation_framework_amd import downscale, io_formats as io
    K, b = io.parse_kitti_calib(os.path.join(seq, "calib.txt"), (0, 1))
    cfg = downscale.apply_to_config(io.apply_calib(g.default_config("kitti"), K, b, scene.rows, scene.cols), 2)
    cfg.max_history_frames = history
    return cfg


@pytest.mark.gpu
def test_run_kitti_downscale_equals_api(folder):
    import run_kitti
    from vslam_pose_estimation_framework_amd import evaluation, hip
    seq, scene, grey, colour, gt = folder
    rows, cols = int(scene.rows), int(scene.cols)
    assert (rows, cols) == (301, 993)
    res = run_kitti.run(seq, None, "kitti", log=QUIET, downscale=2)
    assert res["frames"] == FRAMES and res["error_flags"] == 0 and res["tracking_frames"] == FRAMES - 1
    g = hip.load()
    g.create(_config(g, seq, scene, 512), 0, 1)
    try:
        assert (int(g.cfg.rows), int(g.cfg.cols)) == (150, 496)
        g.set_downscale(2, rows, cols)
        for L, R in grey:
            g.process_host(L, R)
        np.testing.assert_array_equal(res["poses"], g.poses(0, 0, FRAMES))
    finally:
        g.destroy()
    full = run_kitti.run(seq, None, "kitti", log=QUIET)
    print("ATE-RMSE over %d frames: --downscale 2 against the ground truth %.4f m, full resolution against the ground truth %.4f m, --downscale 2 against full resolution %.4f m" % (
        FRAMES, evaluation.ate_rmse(res["poses"], gt), evaluation.ate_rmse(full["poses"], gt), evaluation.ate_rmse(res["poses"], full["poses"])))


@pytest.mark.gpu
def test_run_kitti_downscale_chunks(folder):
    import run_kitti
    from vslam_pose_estimation_framework_amd import hip, sharding
    seq, scene, grey, colour, gt = folder
    rows, cols = int(scene.rows), int(scene.cols)
    res = run_kitti.run(seq, None, "kitti", log=QUIET, downscale=2, chunks=3, overlap=3)
    assert res["frames"] == FRAMES and res["error_flags"] == 0
    plan, _ = sharding.plan_chunks(FRAMES, 3, 3)
    steps = max(e - s for (s, f, e) in plan)
    chunks = []
    for st, fi, en in plan:                                            # every chunk as a stream of its own
        g = hip.load()
        g.create(_config(g, seq, scene, steps + 2), 0, 1)
        try:
            g.set_downscale(2, rows, cols)
            for k in range(st, en):
                g.process_host(*grey[k])
            chunks.append(g.poses(0, 0, en - st))
        finally:
            g.destroy()
    np.testing.assert_array_equal(res["poses"], np.asarray(sharding.assemble_trajectory(chunks, plan)).reshape(FRAMES, 12))


@pytest.mark.gpu
def test_run_kitti_downscale_color_map(folder, tmp_path):
    import run_kitti
    from vslam_pose_estimation_framework_amd import color, hip, io_formats as io
    seq, scene, grey, colour, gt = folder
    rows, cols = int(scene.rows), int(scene.cols)
    ply = str(tmp_path / "m.ply")
    res = run_kitti.run(seq, None, "kitti", log=QUIET, downscale=2, color=True, map_path=ply, map_color=True)
    assert res["frames"] == FRAMES and res["error_flags"] == 0
    m = io.read_ply(ply)
    rgb = np.stack([m["red"], m["green"], m["blue"]], 1)
    assert len(rgb) == len(res["map"]["id"]) >= 100
    g = hip.load()
    g.create(_config(g, seq, scene, 512), 0, 1)
    try:
        g.set_color_input(color.RGB8)
        g.set_downscale(2, rows, cols)
        g.enable_map(run_kitti.MAP_ENTRIES_PER_FRAME * FRAMES)
        g.enable_map_colors(True)
        for L, R in colour:
            g.process_host(L, R)
        np.testing.assert_array_equal(res["poses"], g.poses(0, 0, FRAMES))
        np.testing.assert_array_equal(rgb, g.map_colors(0))
        np.testing.assert_array_equal(m["xyz"], g.map(0)["xyz"])
    finally:
        g.destroy()
    assert (rgb[:, 0] != rgb[:, 2]).mean() >= 0.95                       # colours, not a grey passed through


@pytest.mark.gpu
def test_run_rgbd_downscale_equals_api(tmp_path, monkeypatch):
    """A written TUM folder of 376 x 1241 (the tum premise scene, seed 26) through run_rgbd.py --downscale 2: the poses are those of a direct
    run through the API at the scaled intrinsics, no error flags, TRACKING from frame 2 on."""
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from test_rgbd_mode import setup
    from vslam_pose_estimation_framework_amd import downscale, evaluation, hip
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene, _, _ = setup(o, "tum", scale=1.0, descriptor=1, seed=26)
        frames = uc.render_frames(o, scene, FRAMES)
        gt = uc.ground_truth(o, scene, FRAMES)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    intr = "%r,%r,%r,%r" % tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, uc.DEPTH_UNIT, None, depth_scale=4.0, log=QUIET, downscale=2)
    assert res["frames"] == FRAMES and res["error_flags"] == 0 and res["tracking_frames"] >= FRAMES - 2
    g = hip.load()
    cfg, p = run_rgbd.configure(g, "tum", 188, 620, downscale.scale_intrinsics(K, 2), uc.DEPTH_UNIT, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_downscale(2, 376, 1241)
        poses = [np.array(tr.process(L, D)[0].camera_left_to_world) for L, D in frames]
    finally:
        tr.destroy()
    np.testing.assert_array_equal(np.array(res["poses"]).reshape(FRAMES, 12), np.array(poses).reshape(FRAMES, 12))
    full = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, uc.DEPTH_UNIT, None, depth_scale=4.0, log=QUIET)
    P = lambda r: np.array(r["poses"]).reshape(FRAMES, 12)
    print("RGB-D ATE-RMSE over %d frames: --downscale 2 against the ground truth %.4f m, full resolution against the ground truth %.4f m, --downscale 2 against full resolution %.4f m" % (
        FRAMES, evaluation.ate_rmse(P(res), gt.reshape(FRAMES, 12)), evaluation.ate_rmse(P(full), gt.reshape(FRAMES, 12)), evaluation.ate_rmse(P(res), P(full))))


@pytest.mark.gpu
def test_run_kitti_rectify_downscale_equals_api(tmp_path):
    """The raw, distorted EuRoC-shaped rig of test_rectify_gpu.py at 480 x 752 through run_kitti.py --rectify --downscale 2: the maps are
    built over the raw cameras scaled to 240 x 376; poses == a direct API run with the same maps and the switch, no error flags."""
    import run_kitti
    import test_rectify_gpu as tr
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import downscale, hip, io_formats as io, rectify
    o = Oracle()
    try:
        scene = o.scene_euroc(seed=5)
        n = 8
        tr.write_asl(tmp_path / "raw", o, scene, n, tr.raw_rig(scene))
    finally:
        o.destroy()
    lines = []
    res = run_kitti.run(str(tmp_path / "raw"), None, "kitti", log=lines.append, rectify=True, downscale=2)
    assert res["frames"] == n and res["error_flags"] == 0
    assert any("downscaling on the GPU by 2: 480x752 -> 240x376" in ln for ln in lines) and any("rectifying on the GPU: raw 240x376" in ln for ln in lines)
    seq = io.EurocSequence(str(tmp_path / "raw"))
    raw = seq.raw_calibration()
    cams = [rectify.CameraModel(downscale.scale_intrinsics(c.K, 2), c.dist, c.rows // 2, c.cols // 2) for c in raw[:2]]
    rect = rectify.rectification(cams[0], cams[1], *raw[2:])
    g = hip.load()
    cfg = rectify.apply_to_config(g.default_config("euroc"), rect)
    cfg.max_history_frames = 512
    g.create(cfg, 0, 1)
    try:
        g.set_rectification(rect)
        g.set_downscale(2, 480, 752)
        for k in range(n):
            g.process_host(*seq.pair(k))
        np.testing.assert_array_equal(res["poses"], g.poses(0, 0, n))
        gl, gr = g.downscaled_images(0)
        np.testing.assert_array_equal(gl, downscale.downscale_u8(seq.pair(n - 1)[0], 2))
    finally:
        g.destroy()
    print("--rectify --downscale 2: %d of %d frames TRACKING" % (res["tracking_frames"], n))


def test_tool_flag_and_refusals(tmp_path):
    """Argument parsing needs no GPU."""
    import run_kitti
    a = run_kitti.parse_args(["seq", "--downscale", "2", "--color", "--map", "m.ply", "--map-color", "--clahe", "--chunks", "3"])
    assert a.downscale == 2 and a.color and a.map_color and a.chunks == 3
    assert run_kitti.parse_args(["seq"]).downscale == 1
    for bad in ("0", "5", "-2", "1.5", "two"):
        with pytest.raises(SystemExit):
            run_kitti.parse_args(["seq", "--downscale", bad])
    for bad in (0, 5, 2.0, True):
        with pytest.raises(SystemExit):
            run_kitti.run(str(tmp_path), downscale=bad, log=QUIET)
    import run_rgbd
    b = run_rgbd.parse_args(["folder", "--downscale", "3", "--undistort", "--bilateral", "--color", "--detector", "ORB"])
    assert b.downscale == 3 and run_rgbd.parse_args(["folder"]).downscale == 1
    for bad in ("0", "5", "-1", "x"):
        with pytest.raises(SystemExit):
            run_rgbd.parse_args(["folder", "--downscale", bad])
    for bad in (0, 5, 2.0, True):
        with pytest.raises(SystemExit):
            run_rgbd.run(str(tmp_path), downscale=bad, log=QUIET)
