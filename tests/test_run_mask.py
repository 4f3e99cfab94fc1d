"""tools/run_kitti.py --mask / --mask-margin / --frame-masks end to end on a KITTI-layout folder written from the synthetic renderer: the
poses equal those of direct API runs on the same arrays, in exact mode and with --chunks 3 (every chunk stream its own frame's mask)."""
import os
import sys

import numpy as np
import pytest

import mask_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

QUIET = lambda *_: None      # noqa: E731


@pytest.mark.gpu
def test_run_kitti_masks(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, io_formats as io, sharding
    o = Oracle()
    scene = o.scene_kitti(scale=0.4, seed=7)
    rows, cols, n, margin = scene.rows, scene.cols, 12, 3
    seq, fdir = tmp_path / "seq", tmp_path / "fm"
    for d in (seq / "image_0", seq / "image_1", fdir / "image_0", fdir / "image_1"):
        d.mkdir(parents=True)
    frames, fmasks = [], []
    y, x = np.mgrid[0:rows, 0:cols]
    static = [np.where((y > 0.8 * rows) & (abs(x - cols / 2) < cols / 4), 0, 255).astype(np.uint8),      # a bonnet
              np.where(x + y < 60, 0, 200).astype(np.uint8)]                                             # a vignetted corner
    for k in range(n):
        L, R = o.render(scene, k)
        io.write_png_gray8(str(seq / "image_0" / ("%06d.png" % k)), L)
        io.write_png_gray8(str(seq / "image_1" / ("%06d.png" % k)), R)
        frames.append((L, R))
        # left masks on every frame but 4 and 9, right masks on the even frames only: a missing file means no mask
        fm = [mc.frame_rect(rows, cols, k, 0, small=True) * 255 if k not in (4, 9) else None,
              mc.frame_rect(rows, cols, k, 5, small=True) * 255 if k % 2 == 0 else None]
        for d, m in zip(("image_0", "image_1"), fm):
            if m is not None:
                io.write_png_gray8(str(fdir / d / ("%06d.png" % k)), m)
        fmasks.append(fm)
    with open(seq / "calib.txt", "w") as f:
        f.write("P0: %r 0 %r 0 0 %r %r 0 0 0 1 0\n" % (scene.fx, scene.cx, scene.fy, scene.cy))
        f.write("P1: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (scene.fx, scene.cx, -scene.fx * scene.baseline_m, scene.fy, scene.cy))
    (seq / "times.txt").write_text("\n".join("%.6f" % (0.1 * k) for k in range(n)) + "\n")
    paths = [str(tmp_path / "left.png"), str(tmp_path / "right.png")]
    for p, m in zip(paths, static):
        io.write_png_gray8(p, m)
    lines = []
    res = run_kitti.run(str(seq), None, "kitti", log=lines.append, mask=",".join(paths), mask_margin=margin, frame_masks=str(fdir),
                        map_path=str(tmp_path / "map.ply"))
    assert any("detection mask" in ln for ln in lines) and any("per-frame detection masks" in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0 and res["tracking_frames"] >= n // 2
    plain = run_kitti.run(str(seq), None, "kitti", log=QUIET)
    assert not np.array_equal(np.asarray(plain["poses"]), np.asarray(res["poses"]))
    cfg = o.config_for_scene(scene)
    g = hip.load()
    try:
        # exact mode: the poses of a direct API run on the same arrays
        cfg.max_history_frames = 512
        g.create(cfg, 0, 1)
        g.set_detection_mask(static[0], static[1], margin)
        for k, (L, R) in enumerate(frames):
            if fmasks[k][0] is not None or fmasks[k][1] is not None:
                g.set_frame_masks(fmasks[k][0], fmasks[k][1], margin)
            g.process_host(L, R)
        np.testing.assert_array_equal(np.asarray(g.poses(0, 0, n)).reshape(n, 12), np.asarray(res["poses"]).reshape(n, 12))
        # --chunks 3: every chunk stream gets its own frame's mask
        chunked = run_kitti.run(str(seq), None, "kitti", log=QUIET, chunks=3, overlap=3, mask=",".join(paths), mask_margin=margin, frame_masks=str(fdir))
        plan, _ = sharding.plan_chunks(n, 3, 3)
        steps = max(e - s for (s, f, e) in plan)
        cfg.max_history_frames = steps + 2
        g.create(cfg, 0, len(plan))
        g.set_detection_mask(static[0], static[1], margin)
        live = [True] * len(plan)
        Lb, Rb = np.zeros((len(plan), rows, cols), np.uint8), np.zeros((len(plan), rows, cols), np.uint8)
        for k in range(steps):
            sides = [None, None]
            for c, (st, fi, en) in enumerate(plan):
                if st + k < en:
                    Lb[c], Rb[c] = frames[st + k]
                    for d in (0, 1):
                        if fmasks[st + k][d] is not None:
                            if sides[d] is None:
                                sides[d] = np.full((len(plan), rows, cols), 255, np.uint8)
                            sides[d][c] = fmasks[st + k][d]
                elif live[c]:
                    g.set_stream_active(c, False)
                    live[c] = False
            if sides[0] is not None or sides[1] is not None:
                g.set_frame_masks(sides[0], sides[1], margin)
            g.process_host(Lb, Rb)
        chunks = [g.poses(c, 0, en - st) for c, (st, fi, en) in enumerate(plan)]
        want = np.asarray(sharding.assemble_trajectory(chunks, plan)).reshape(n, 12)
        np.testing.assert_array_equal(want, np.asarray(chunked["poses"]).reshape(n, 12))
        assert chunked["frames"] == n and chunked["error_flags"] == 0
    finally:
        g.destroy()
        o.destroy()


@pytest.mark.gpu
def test_run_rgbd_mask(tmp_path, monkeypatch):
    """tools/run_rgbd.py --mask --mask-margin on a written TUM folder: the poses of a direct API run with the same mask, and not those of a
    run without the flag."""
    import run_rgbd
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip, io_formats as io
    from vslam_pose_estimation_framework_amd.capi import RgbdTracker
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene = o.scene_kitti(scale=0.5, seed=13)
        scene.speed_m = 0.25; scene.sway_m = 0.4
        n, unit = 12, uc.DEPTH_UNIT
        frames = uc.render_frames(o, scene, n)
        gt = uc.ground_truth(o, scene, n)
    finally:
        o.destroy()
    uc.write_tum_folder(tmp_path / "seq", frames, gt)
    rows, cols = scene.rows, scene.cols
    y, x = np.mgrid[0:rows, 0:cols]
    blob = np.where((y > 0.7 * rows) & (abs(x - cols / 2) < cols / 5), 0, 255).astype(np.uint8)
    io.write_png_gray8(str(tmp_path / "mask.png"), blob)
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    lines = []
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, depth_scale=4.0, log=lines.append, mask=str(tmp_path / "mask.png"), mask_margin=5)
    assert any("detection mask" in ln for ln in lines), lines
    plain = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, depth_scale=4.0, log=QUIET)
    assert res["frames"] == n and res["error_flags"] == 0
    assert not np.array_equal(np.asarray(res["poses"]), np.asarray(plain["poses"]))
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", rows, cols, K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.set_detection_mask(blob, 5)
        for k, (L, D) in enumerate(frames):
            fi, _ = tr.process(L, D)
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
    finally:
        tr.destroy()
    with pytest.raises(SystemExit):
        run_rgbd.parse_args([str(tmp_path / "seq"), "--mask-margin", "3"])
    with pytest.raises(SystemExit):
        run_rgbd.parse_args([str(tmp_path / "seq"), "--mask", str(tmp_path / "none.png")])
    a = run_rgbd.parse_args([str(tmp_path / "seq"), "--mask", str(tmp_path / "mask.png"), "--mask-margin", "64"])
    assert a.mask_margin == 64
