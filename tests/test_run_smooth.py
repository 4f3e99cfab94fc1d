"""tools/run_kitti.py --smooth and tools/run_rgbd.py --smooth end to end on written 12-frame synthetic folders: the trajectory is that of a
context driven by hand with the switch set, it differs from the unsmoothed run, and --chunks with the flag equals the per-chunk contexts
driven by hand.  The ATE against ground truth of plain, Gaussian and median runs on the noisy variant of the KITTI folder is printed, not
asserted (profiles/smooth_cost_mi355x.txt carries the figures; synthetic, one seed)."""
import os
import sys

import numpy as np
import pytest

from vslam_pose_estimation_framework_amd import smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731
FRAMES = 12
FLAGS = [("gaussian:5", (smooth.GAUSSIAN, 5)), ("median", (smooth.MEDIAN, 3))]


def _write_kitti(seq, scene, frames):
    from vslam_pose_estimation_framework_amd import io_formats as io
    for d in ("image_0", "image_1"):
        (seq / d).mkdir(parents=True)
    for k, (L, R) in enumerate(frames):
        io.write_png_gray8(str(seq / "image_0" / ("%06d.png" % k)), L); io.write_png_gray8(str(seq / "image_1" / ("%06d.png" % k)), R)
    fx, fy, cx, cy, b = (float(v) for v in (scene.fx, scene.fy, scene.cx, scene.cy, scene.baseline_m))
    (seq / "calib.txt").write_text("".join("%s: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (n, fx, cx, tx, fy, cy) for n, tx in (("P0", 0.0), ("P1", -fx * b))))
    return str(seq)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """(path, path of the noisy variant, scene, frames, noisy frames, ground-truth poses [n, 12])"""
    from _oracle import Oracle
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=7)
        grey = [o.render(scene, k) for k in range(FRAMES)]
        gt = np.stack([o.gt_pose(scene, k).reshape(12) for k in range(FRAMES)])
    finally:
        o.destroy()
    rng = np.random.default_rng(3)
    noisy = [tuple(np.clip(x.astype(np.int64) + rng.integers(-14, 15, x.shape), 0, 255).astype(np.uint8) for x in pair) for pair in grey]
    base = tmp_path_factory.mktemp("kitti")
    return _write_kitti(base / "seq", scene, grey), _write_kitti(base / "noisy", scene, noisy), scene, grey, noisy, gt


def _config(g, seq, scene, history):
    from vslam_pose_estimation_framework_amd import io_formats as io
    K, b = io.parse_kitti_calib(os.path.join(seq, "calib.txt"), (0, 1))
    cfg = io.apply_calib(g.default_config("kitti"), K, b, scene.rows, scene.cols)
    cfg.max_history_frames = history
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize("flag,sm", FLAGS, ids=[f for f, _ in FLAGS])
def test_run_kitti_smooth_equals_api(folder, flag, sm):
    import run_kitti
    from vslam_pose_estimation_framework_amd import hip
    seq, _, scene, grey, _, gt = folder
    lines = []
    res = run_kitti.run(seq, None, "kitti", log=lines.append, smooth=flag)
    assert res["frames"] == FRAMES and res["error_flags"] == 0
    assert any("smoothing on the GPU" in ln for ln in lines)
    g = hip.load()
    g.create(_config(g, seq, scene, 512), 0, 1)
    try:
        g.set_smoothing(*sm)
        for L, R in grey:
            g.process_host(L, R)
        np.testing.assert_array_equal(res["poses"], g.poses(0, 0, FRAMES))
        np.testing.assert_array_equal(g.smoothed_images(0)[0], smooth.smooth_u8(grey[-1][0], *sm))
    finally:
        g.destroy()
    plain = run_kitti.run(seq, None, "kitti", log=QUIET)
    assert plain["error_flags"] == 0 and not np.array_equal(plain["poses"], res["poses"])


@pytest.mark.gpu
def test_run_kitti_smooth_chunks(folder):
    import run_kitti
    from vslam_pose_estimation_framework_amd import hip, sharding
    seq, _, scene, grey, _, gt = folder
    res = run_kitti.run(seq, None, "kitti", log=QUIET, smooth="gaussian:5", chunks=3, overlap=3)
    assert res["frames"] == FRAMES and res["error_flags"] == 0
    plan, _ = sharding.plan_chunks(FRAMES, 3, 3)
    steps = max(e - s for (s, f, e) in plan)
    chunks = []
    for st, fi, en in plan:                                            # every chunk as a stream of its own
        g = hip.load()
        g.create(_config(g, seq, scene, steps + 2), 0, 1)
        try:
            g.set_smoothing(smooth.GAUSSIAN, 5)
            for k in range(st, en):
                g.process_host(*grey[k])
            chunks.append(g.poses(0, 0, en - st))
        finally:
            g.destroy()
    np.testing.assert_array_equal(res["poses"], np.asarray(sharding.assemble_trajectory(chunks, plan)).reshape(FRAMES, 12))


@pytest.mark.gpu
def test_ate_on_the_noisy_folder_is_printed(folder):
    import run_kitti
    from vslam_pose_estimation_framework_amd import evaluation
    _, noisy, scene, _, _, gt = folder
    out = []
    for flag in (None, "gaussian:5", "median"):
        res = run_kitti.run(noisy, None, "kitti", log=QUIET, smooth=flag)
        assert res["frames"] == FRAMES and res["error_flags"] == 0
        out.append("%s %.4f m (%d frames TRACKING)" % (flag or "plain", evaluation.ate_rmse(res["poses"], gt), res["tracking_frames"]))
    print("ATE-RMSE over %d frames of the noisy folder (uniform noise -14 .. 14, seed 3) against the ground truth: %s" % (FRAMES, ", ".join(out)))


@pytest.mark.gpu
@pytest.mark.parametrize("flag,sm", FLAGS, ids=[f for f, _ in FLAGS])
def test_run_rgbd_smooth_equals_api(tmp_path, monkeypatch, flag, sm):
    """A written TUM folder (the tum premise scene at half size, seed 26) through run_rgbd.py --smooth: the poses are those of a direct run
    through the API with the switch set, and differ from the unsmoothed run's."""
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from test_rgbd_mode import setup
    from vslam_pose_estimation_framework_amd import hip
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene, _, _ = setup(o, "tum", scale=0.5, descriptor=1, seed=26)
        frames = uc.render_frames(o, scene, FRAMES)
        gt = uc.ground_truth(o, scene, FRAMES)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    rows, cols = frames[0][0].shape
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    intr = "%r,%r,%r,%r" % tuple(float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, uc.DEPTH_UNIT, None, depth_scale=4.0, log=QUIET, smooth=flag)
    assert res["frames"] == FRAMES and res["error_flags"] == 0
    g = hip.load()
    cfg, p = run_rgbd.configure(g, "tum", rows, cols, K, uc.DEPTH_UNIT, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_smoothing(*sm)
        poses = [np.array(tr.process(L, D)[0].camera_left_to_world) for L, D in frames]
        np.testing.assert_array_equal(tr.smoothed(), smooth.smooth_u8(frames[-1][0], *sm))
    finally:
        tr.destroy()
    P = lambda r: np.array(r["poses"]).reshape(FRAMES, 12)      # noqa: E731
    np.testing.assert_array_equal(P(res), np.array(poses).reshape(FRAMES, 12))
    plain = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, uc.DEPTH_UNIT, None, depth_scale=4.0, log=QUIET)
    assert plain["error_flags"] == 0 and not np.array_equal(P(plain), P(res))


def test_tool_flag_and_refusals(tmp_path):
    """Argument parsing needs no GPU."""
    import run_kitti
    import run_rgbd
    a = run_kitti.parse_args(["seq", "--smooth", "median:5", "--color", "--map", "m.ply", "--map-color", "--clahe", "--chunks", "3", "--downscale", "2"])
    assert a.smooth == "median:5" and a.chunks == 3 and a.downscale == 2
    b = run_rgbd.parse_args(["folder", "--smooth", "gaussian", "--undistort", "--bilateral", "--color", "--detector", "ORB", "--equalize"])
    assert b.smooth == "gaussian" and run_rgbd.parse_args(["folder"]).smooth is None
    for tool in (run_kitti, run_rgbd):
        for bad in ("box", "gaussian:4", "median:7", "median:x", "5"):
            with pytest.raises(SystemExit):
                tool.parse_args(["seq", "--smooth", bad])
            with pytest.raises(SystemExit):
                tool.run(str(tmp_path), smooth=bad, log=QUIET)
