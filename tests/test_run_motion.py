"""tools/run_kitti.py --motion-model / --odometry / --dead-reckoning-limit: the flags and the odometry readers without a GPU; on the GPU
a KITTI folder with a four-frame drop-out, written from the synthetic renderer, run with a KITTI pose file and with a TUM trajectory
against a direct API run, bit for bit, and --chunks 3 with every chunk on its own frames' poses."""
import os
import sys

import numpy as np
import pytest

import motion_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731


def test_run_kitti_motion_flags():
    import run_kitti
    a = run_kitti.parse_args(["seq"])
    assert (a.motion_model, a.odometry, a.dead_reckoning_limit) == ("constant-velocity", None, 0)
    a = run_kitti.parse_args(["seq", "--motion-model", "odometry", "--odometry", "poses.txt", "--dead-reckoning-limit", "2", "--chunks", "3"])
    assert (a.motion_model, a.odometry, a.dead_reckoning_limit, a.chunks) == ("odometry", "poses.txt", 2, 3)
    assert run_kitti.parse_args(["seq", "--motion-model", "none"]).motion_model == "none"
    assert run_kitti.MOTION_MODELS == {"constant-velocity": 0, "none": 1, "odometry": 2}
    for bad in (["seq", "--motion-model", "odometry"], ["seq", "--odometry", "poses.txt"], ["seq", "--motion-model", "none", "--odometry", "p.txt"],
                ["seq", "--dead-reckoning-limit", "2"], ["seq", "--motion-model", "none", "--dead-reckoning-limit", "1"],
                ["seq", "--motion-model", "odometry", "--odometry", "p.txt", "--dead-reckoning-limit", "-1"], ["seq", "--motion-model", "imu"]):
        with pytest.raises(SystemExit):
            run_kitti.parse_args(bad)
    with pytest.raises(SystemExit):      # the same rules for a caller of run()
        run_kitti.run("nowhere", motion_model="odometry", log=QUIET)


def test_tum_trajectory_round_trip_and_association(tmp_path):
    from vslam_pose_estimation_framework_amd import io_formats as io
    rng = np.random.default_rng(3)
    poses = mc.random_rigid(rng, 9, 50.0).reshape(-1, 3, 4)
    times = 100.0 + 0.1 * np.arange(9)
    path = str(tmp_path / "traj.txt")
    io.write_trajectory_tum(path, poses, times)
    t, p = io.read_trajectory_tum(path)
    np.testing.assert_allclose(t, times, atol=1e-9)
    np.testing.assert_allclose(p, poses, atol=1e-8)          # nine decimals written
    # frames at other time stamps: nearest within 0.02 s, every pose used once; frames 3 and 4 have none and carry frame 2's
    frame_times = [100.004, 100.099, 100.21, 100.26, 100.35, 100.5]
    g, own = io.read_pose_guesses(path, frame_times)
    assert list(own) == [True, True, True, False, False, True]
    np.testing.assert_array_equal(g[0], p[0].reshape(12)); np.testing.assert_array_equal(g[1], p[1].reshape(12))
    np.testing.assert_array_equal(g[2], p[2].reshape(12)); np.testing.assert_array_equal(g[3], g[2]); np.testing.assert_array_equal(g[4], g[2])
    np.testing.assert_array_equal(g[5], p[5].reshape(12))
    g, own = io.read_pose_guesses(path, [99.0, 100.0])         # no pose ahead of the first: identity
    assert list(own) == [False, True]
    np.testing.assert_array_equal(g[0], mc.identity())
    # a KITTI pose file: line k for frame k, short files carry the last line on
    kpath = str(tmp_path / "poses.txt")
    io.write_trajectory_kitti(kpath, poses[:4])
    g, own = io.read_pose_guesses(kpath, list(range(6)))
    assert list(own) == [True] * 4 + [False] * 2
    np.testing.assert_allclose(g[:4], poses[:4].reshape(4, 12), atol=1e-8)
    np.testing.assert_array_equal(g[5], g[3])
    (tmp_path / "bad.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError):
        io.read_pose_guesses(str(tmp_path / "bad.txt"), [0.0])
    (tmp_path / "short.txt").write_text("# t x y z qx qy qz qw\n1.0 0 0 0 0 0 0 1\n2.0 0 0 0 0 0 1\n")
    with pytest.raises(ValueError):
        io.read_trajectory_tum(str(tmp_path / "short.txt"))


def test_quaternion_reader_inverts_the_writer():
    from vslam_pose_estimation_framework_amd import io_formats as io
    for T in mc.random_rigid(np.random.default_rng(11), 32, 1.0).reshape(-1, 3, 4):
        np.testing.assert_allclose(io.quaternion_to_rotation(*io.rotation_to_quaternion(T[:, :3])), T[:, :3], atol=1e-14)
    np.testing.assert_array_equal(io.quaternion_to_rotation(0.0, 0.0, 0.0, 2.0), np.eye(3))     # normalised on the way in


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
def test_run_kitti_odometry_on_a_folder_with_a_gap(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, io_formats as io
    from vslam_pose_estimation_framework_amd.capi import MOTION_CAMERA_ODOMETRY
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.4, seed=7)
        frames = mc.render_sequence(o, scene, mc.GAP_FRAMES)
        gt = mc.gt_guesses(o, scene, mc.GAP_FRAMES)
        cfg = o.config_for_scene(scene)
    finally:
        o.destroy()
    n = len(frames)
    _write_kitti(io, tmp_path / "seq", scene, frames)
    seq, kpath, tpath = str(tmp_path / "seq"), str(tmp_path / "odometry_kitti.txt"), str(tmp_path / "odometry_tum.txt")
    io.write_trajectory_kitti(kpath, gt)
    io.write_trajectory_tum(tpath, gt, [0.1 * k + 0.003 for k in range(n)])       # the odometry's clock is 3 ms off the camera's
    lines = []
    res = run_kitti.run(seq, str(tmp_path / "out.txt"), "kitti", kpath, log=lines.append, motion_model="odometry", odometry=kpath, dead_reckoning_limit=2)
    assert any("motion model camera odometry: %d of %d frames" % (n, n) in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0 and res["dead_reckoned_frames"] >= 1
    plain = run_kitti.run(seq, None, "kitti", kpath, log=QUIET)
    assert res["ate_rmse_aligned"] < 0.25 * plain["ate_rmse_aligned"], (res["ate_rmse_aligned"], plain["ate_rmse_aligned"])
    tum = run_kitti.run(seq, None, "kitti", log=QUIET, motion_model="odometry", odometry=tpath, dead_reckoning_limit=2)
    # the direct API run on what each file reads back as (nine decimals; the TUM file through its quaternions)
    for path, got in ((kpath, res), (tpath, tum)):
        guesses, own = io.read_pose_guesses(path, [0.1 * k for k in range(n)])
        assert own.all()
        g = hip.load().create(cfg, 0, 1)
        try:
            g.set_motion_model(MOTION_CAMERA_ODOMETRY, 2)
            for k, (L, R) in enumerate(frames):
                g.set_pose_guess(guesses[k], 0)
                g.process_host(L, R)
            np.testing.assert_array_equal(np.asarray(g.poses(0, 0, n)).reshape(n, 12), np.asarray(got["poses"]).reshape(n, 12))
        finally:
            g.destroy()
    none = run_kitti.run(seq, None, "kitti", log=QUIET, motion_model="none")
    assert none["frames"] == n and none["error_flags"] == 0 and "dead_reckoned_frames" not in none
    # --chunks 3: every chunk stream starts from its own frames' poses; the seam that lies on the drop-out is bridged
    chunked = run_kitti.run(seq, None, "kitti", kpath, log=QUIET, motion_model="odometry", odometry=kpath, chunks=3, overlap=3)
    assert chunked["frames"] == n and chunked["error_flags"] == 0
    print("ATE odometry", res["ate_rmse_aligned"], "constant velocity", plain["ate_rmse_aligned"], "chunks 3", chunked["ate_rmse_aligned"])


def test_run_rgbd_motion_flags():
    import run_rgbd
    a = run_rgbd.parse_args(["folder"])
    assert (a.motion_model, a.odometry, a.dead_reckoning_limit) == ("constant-velocity", None, 0)
    a = run_rgbd.parse_args(["folder", "--config", "xtion", "--motion-model", "odometry", "--odometry", "odo.txt", "--dead-reckoning-limit", "2"])
    assert (a.motion_model, a.odometry, a.dead_reckoning_limit) == ("odometry", "odo.txt", 2)
    for bad in (["folder", "--motion-model", "odometry"], ["folder", "--odometry", "odo.txt"], ["folder", "--dead-reckoning-limit", "2"],
                ["folder", "--motion-model", "none", "--dead-reckoning-limit", "1"]):
        with pytest.raises(SystemExit):
            run_rgbd.parse_args(bad)


@pytest.mark.gpu
def test_run_rgbd_odometry_on_a_folder_with_a_blank_frame(tmp_path, monkeypatch):
    """A written TUM folder (xtion configuration, its own model at last) with a black frame 6 and the ground truth as odometry file: the
    tool's poses equal a direct API run on what the file reads back as, no break, and the limit brings Tracking back."""
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, io_formats as io
    from vslam_pose_estimation_framework_amd.capi import MOTION_CAMERA_ODOMETRY, RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=26)
        scene.speed_m = 0.08; scene.sway_m = 0.15
        n, unit = 12, uc.DEPTH_UNIT
        frames = [(np.zeros_like(L) if k == 6 else L, D) for k, (L, D) in enumerate(uc.render_frames(o, scene, n))]
        gt = uc.ground_truth(o, scene, n)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    folder = str(tmp_path / "seq")
    odo = os.path.join(folder, "groundtruth.txt")
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    lines = []
    res = run_rgbd.run(folder, "xtion", intr, unit, None, depth_scale=4.0, log=lines.append, motion_model="odometry", odometry=odo, dead_reckoning_limit=2)
    assert any("motion model camera odometry: %d of %d frames" % (n, n) in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0 and res["dead_reckoned_frames"] >= 1
    seq = io.TumRgbdSequence(folder)
    guesses, own = io.read_pose_guesses(odo, seq.times[:n])
    assert own.all()
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "xtion", scene.rows, scene.cols, K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_motion_model(MOTION_CAMERA_ODOMETRY, 2)
        status = []
        for k, (L, D) in enumerate(frames):
            tr.set_pose_guess(guesses[k])
            fi, _ = tr.process(L, D)
            assert fi.track_broken == 0
            status.append(fi.status)
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
        assert 0 in status[7:] and status[-1] == 1, status
    finally:
        tr.destroy()
