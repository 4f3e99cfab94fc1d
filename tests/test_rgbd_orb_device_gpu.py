"""detector_type ORB on the device-resident RGB-D loop (csrc/kernels_rgbd_orb.h, rgbd_device.h enqueue_orb_detect): the
OrbDetector of every region, the extractor and the feature store that holds float keypoints of several pyramid levels run on the frame's
queue.  The device loop against the host-driven loop (VSLAM_RGBD_HOST=1) and the checker loop (tests/rgbd_loop.py over the CPU oracle);
then what the device loop alone offers in this mode: batches, the captured launch sequence, map / log / colours, the input stages, the
capacity error and the mask refusals.  Scenes: test_rgbd_mode.setup(o, "tum", seed=67) (188 x 620).  Premises come from the checker."""
import numpy as np
import pytest

from rgbd_loop import RgbdTracker as PyLoop
from test_rgbd_map_gpu import Expect
from test_rgbd_mode import POSE_RTOL, setup
from test_undistort_gpu import RAW_COLS, RAW_ROWS, SHIFT, _same_info, _same_points
from vslam_pose_estimation_framework_amd import hip
from vslam_pose_estimation_framework_amd.capi import ERR_CAPACITY, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

COUNTERS = (("status", "status"), ("n_keypoints", "n_keypoints_left"), ("n_tracked", "n_tracked"), ("n_lost", "n_lost"),
            ("n_tracked_landmarks", "n_tracked_landmarks"), ("aligner_ran", "aligner_ran"), ("n_inliers", "n_inliers"),
            ("aligner_iterations", "aligner_iterations"), ("n_after_prune", "n_after_prune"), ("n_recovered", "n_recovered"),
            ("n_active_landmarks", "n_active_landmarks"), ("n_new", "n_new_stereo"), ("n_points", "n_points"), ("window_pixels", "window_pixels"),
            ("track_attempts", "track_attempts"), ("fallback", "fallback"), ("track_broken", "track_broken"), ("status_at_start", "status_at_start"))


def _world(o, descriptor, grid=(1, 1), seed=67):
    scene, cfg, p = setup(o, "tum", descriptor=descriptor, seed=seed)
    cfg.det_rows, cfg.det_cols = grid
    p.detector_type = 1
    return scene, cfg, p


def _frames(o, scene, ks):
    return [(o.render(scene, k)[0], o.render_depth(scene, k, 2e-3)) for k in ks]


def _trackers(g, cfg, p, monkeypatch):
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    dev = RgbdTracker(g, cfg, p)
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    host = RgbdTracker(g, cfg, p)
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    return dev, host


def _against_checker(a, ref, fi, n_temp, pts, tag):
    for name, field in COUNTERS:
        assert a[name] == getattr(fi, field), (tag, name, a[name], getattr(fi, field))
    assert a["thresholds"] == list(fi.thresholds)[:len(a["thresholds"])], (tag, a["thresholds"], list(fi.thresholds))
    assert a["n_temporary"] == n_temp and a["tau_track"] == fi.tau_track, tag
    To, Tg = a["pose"], np.array(fi.camera_left_to_world).reshape(3, 4)
    assert np.linalg.norm(Tg - To) / np.linalg.norm(To) <= POSE_RTOL, tag
    cur = ref.frames[-1]
    assert len(pts["xy"]) == len(cur.points), tag
    if len(cur.points):
        np.testing.assert_array_equal(pts["xy"].view(np.uint32), np.array([q.xy for q in cur.points], np.float32).view(np.uint32), err_msg=str(tag))
        np.testing.assert_array_equal(pts["desc"], np.array([q.desc for q in cur.points], np.uint8), err_msg=str(tag))
        np.testing.assert_allclose(pts["cam"], np.array([q.cam for q in cur.points]), rtol=1e-12, atol=0, err_msg=str(tag))


def _loops_agree(fa, na, pa, fb, nb, pb, tag):
    for name, _ in fa._fields_:
        va, vb = getattr(fa, name), getattr(fb, name)
        if hasattr(va, "__len__"):
            va, vb = list(va), list(vb)
        if name in ("camera_left_to_world", "previous_to_current", "total_error"):
            np.testing.assert_allclose(np.array(va), np.array(vb), rtol=1e-9, atol=1e-12, err_msg="%s %s" % (tag, name))
        else:
            assert va == vb, (tag, name, va, vb)
    assert na == nb, tag
    np.testing.assert_array_equal(pa["xy"].view(np.uint32), pb["xy"].view(np.uint32), err_msg=str(tag))
    np.testing.assert_array_equal(pa["desc"], pb["desc"], err_msg=str(tag))
    np.testing.assert_array_equal(pa["meta"], pb["meta"], err_msg=str(tag))
    np.testing.assert_allclose(pa["cam"], pb["cam"], rtol=1e-12, atol=0, err_msg=str(tag))


@pytest.mark.gpu
@pytest.mark.parametrize("grid,descriptor", [((1, 1), 1), ((1, 1), 0), ((2, 2), 1), ((2, 2), 0)])
def test_three_way_parity(grid, descriptor, monkeypatch):
    """Device loop == host-driven loop == checker, frame by frame, eight frames."""
    from _oracle import Oracle
    o = Oracle()
    scene, cfg, p = _world(o, descriptor, grid)
    o.create(cfg, 0, 1)
    g = hip.load()
    ref = PyLoop(o, cfg, p)
    dev, host = _trackers(g, cfg, p, monkeypatch)
    try:
        shared, levels, thr = 0, set(), None
        for k, (L, D) in enumerate(_frames(o, scene, range(8))):
            a = ref.process(L, D)
            (fa, na), (fb, nb) = dev.process(L, D), host.process(L, D)
            pa, pb = dev.points(), host.points()
            _against_checker(a, ref, fa, na, pa, ("device", grid, descriptor, k))
            _against_checker(a, ref, fb, nb, pb, ("host", grid, descriptor, k))
            _loops_agree(fa, na, pa, fb, nb, pb, (grid, descriptor, k))
            rc = ref.feat_rc
            key = rc[:, 0].astype(np.int64) * 100000 + rc[:, 1]
            for u in np.unique(key):
                shared += int(len(set(ref.acc_level[key == u])) > 1)
            levels |= set(int(v) for v in ref.acc_level)
            thr = a["thresholds"]
        assert fa.status == 1 and fa.n_tracked > 20 and fa.n_keypoints_left > 300, (fa.status, fa.n_tracked, fa.n_keypoints_left)
        assert len(levels) >= (3 if grid == (1, 1) else 2), levels
        assert shared > 0                                          # a pixel shared by keypoints of different levels
        if grid == (2, 2):
            assert len(set(thr)) > 1, thr                          # the four regions' thresholds moved apart
    finally:
        dev.destroy(); host.destroy(); o.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("descriptor", [1, 0])
def test_reregistration(descriptor, monkeypatch):
    """Frames 0 .. 5, 19, 20, 21: a lost track, further attempts that append their detections; ORB::compute regroups the union level-major."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = _world(o, descriptor)
    o.create(cfg, 0, 1)
    g = hip.load()
    ref = PyLoop(o, cfg, p)
    dev = RgbdTracker(g, cfg, p)
    try:
        most, levels = 0, 0
        for k, (L, D) in zip([0, 1, 2, 3, 4, 5, 19, 20, 21], _frames(o, scene, [0, 1, 2, 3, 4, 5, 19, 20, 21])):
            a = ref.process(L, D)
            fa, na = dev.process(L, D)
            _against_checker(a, ref, fa, na, dev.points(), (descriptor, k))
            if a["track_attempts"] > 1:
                most = max(most, a["track_attempts"])
                levels = max(levels, int(ref.acc_level.max()))
                assert len(ref.detections) == a["track_attempts"]
                if descriptor == 1:
                    assert np.all(np.diff(ref.acc_level) >= 0)          # the union is level-major
                else:
                    assert np.any(np.diff(ref.acc_level) < 0)           # BRIEF leaves the appended order alone
        assert most >= 2 and levels >= 1, (most, levels)
    finally:
        dev.destroy(); o.destroy()


def _batch_worlds(o, descriptor):
    worlds = []
    for i, seed in enumerate((67, 68, 69)):
        scene, cfg, p = _world(o, descriptor, seed=seed)
        ks = list(range(8)) if i != 1 else [0, 1, 2, 3, 4, 19, 20, 21]       # sequence 1 jumps: it re-registers while the others track
        worlds.append(_frames(o, scene, ks))
    return cfg, p, worlds


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_batch_equals_sequences_alone_and_captured_equals_direct(graph, monkeypatch):
    """vslam_rgbd_create_batch with three sequences: each bit-identical to the same sequence alone (direct launches); under
    VSLAM_RGBD_GRAPH=1 the batch and a single sequence are bit-identical to the direct runs as well."""
    from _oracle import Oracle
    o = Oracle()
    try:
        cfg, p, worlds = _batch_worlds(o, 1)
    finally:
        o.destroy()
    g = hip.load()
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    alone = []
    for frames in worlds:
        t = RgbdTracker(g, cfg, p)
        rec = []
        for L, D in frames:
            fi, nt = t.process(L, D)
            rec.append((fi, nt, t.points()))
        alone.append(rec)
        t.destroy()
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))
    batch = RgbdBatch(g, cfg, p, 3)
    one = RgbdTracker(g, cfg, p) if graph else None
    try:
        attempts = set()
        for f in range(8):
            L = np.stack([worlds[i][f][0] for i in range(3)]); D = np.stack([worlds[i][f][1] for i in range(3)])
            res = batch.process(L, D)
            for i, (fi, nt) in enumerate(res):
                fa, na, pa = alone[i][f]
                _same_info(fa, fi, "graph %d frame %d sequence %d" % (graph, f, i))
                assert na == nt
                _same_points(pa, batch.points(i), "graph %d frame %d sequence %d" % (graph, f, i))
                attempts.add((i, fi.track_attempts))
            if one is not None:
                fi, nt = one.process(worlds[1][f][0], worlds[1][f][1])
                _same_info(alone[1][f][0], fi, "captured single frame %d" % f)
                _same_points(alone[1][f][2], one.points(), "captured single frame %d" % f)
        assert any(i == 1 and a >= 2 for i, a in attempts) and all(a <= 1 for i, a in attempts if i != 1), attempts
        assert all(fi.n_keypoints_left > 300 for fi, _ in res)
    finally:
        batch.destroy()
        if one is not None:
            one.destroy()


@pytest.mark.gpu
def test_map_log_and_colours_on_colour_frames(monkeypatch):
    """Ids, map entries and log entries are the checker's (test_rgbd_map_gpu.Expect: the id rule of vslam_hip.h on the checker's point lists); the
    colours are map_color_cases.rgbd_step's rebuild, sampled at the float keypoints."""
    import color_cases as cc
    import map_color_cases as mc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import color
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = _world(o, 1)
    o.create(cfg, 0, 1)
    g = hip.load()
    ref = PyLoop(o, cfg, p)
    dev = RgbdTracker(g, cfg, p)
    ex = Expect()
    rng = np.random.default_rng(267)
    rgb, history, fractional = np.zeros((0, 3), np.uint8), [], 0
    try:
        dev.set_color_input(color.RGB8)
        dev.enable_map(4000); dev.enable_observations(40000); dev.enable_map_colors(True)
        for k, (L, D) in enumerate(_frames(o, scene, range(8))):
            c = cc.colourise(L, rng)
            G = color.to_gray_u8(c, color.RGB8)
            info = ref.process(G, D)
            fi, _ = dev.process(c, D)
            assert fi.error_flags == 0 and fi.n_points == info["n_points"]
            ids = ex.step(ref)
            m, ob = ex.check(dev, 0, ref, ids, ("orb detector", k))
            pts = dev.points()
            rgb, sel = mc.rgbd_step(rgb, history, dev.point_ids(), pts["xy"], m["last_frame"], k, c, color.RGB8, None)
            fractional += int((pts["xy"][sel] != np.rint(pts["xy"][sel])).any(axis=1).sum())
            np.testing.assert_array_equal(dev.map_colors(), rgb, err_msg="frame %d" % k)
        ex.check_final(m, ob, ref, "orb detector")
        assert len(ref.landmarks) >= 50 and fractional >= 1, (len(ref.landmarks), fractional)
        assert int(ref.acc_level.max()) >= 1
    finally:
        dev.destroy(); o.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["undistort-clahe-bilateral", "equalize-device-guess"])
def test_stage_combinations(case, monkeypatch):
    """The input stages sit ahead of the detector: a context with the stages on equals a second context fed the numpy-preprocessed frames."""
    import bilateral_cases as bc
    import clahe_cases as clc
    import motion_cases as mcs
    import undistort_cases as uc
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import equalize, rectify
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    o = Oracle()
    try:
        scene, cfg, p = _world(o, 1)
        frames = _frames(o, scene, range(6))
        guesses = mcs.gt_guesses(o, scene, range(6)) if case == "equalize-device-guess" else None
    finally:
        o.destroy()
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        if case == "undistort-clahe-bilateral":
            cam = uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT)
            und, lens = rectify.undistortion(cam, K, int(cfg.rows), int(cfg.cols)), uc.distorting_maps(cam, K)
            a.set_undistortion(und); a.set_clahe(True, 4.0, (8, 8)); a.set_bilateral(True)
        else:
            import torch
            a.set_equalization(True)
            for t in (a, b):
                t.set_motion_model(2)
        for f, (L, D) in enumerate(frames):
            if case == "undistort-clahe-bilateral":
                rawL, rawD = uc.distort_frame(lens, L, D)
                uL, uD = und.apply(rawL, rawD)
                (fa, na), (fb, nb) = a.process(rawL, rawD), b.process(clc.clahe_image(uL, 4.0), bc.filtered(uD, p)[0])
            else:
                T = np.ascontiguousarray(np.asarray(guesses[f], np.float64).reshape(-1)[:12])
                Td = torch.from_numpy(T).to(torch.device("cuda", 0))
                torch.cuda.synchronize()
                a.set_pose_guesses_device(Td.data_ptr()); b.set_pose_guess(T)
                (fa, na), (fb, nb) = a.process(L, D), b.process(equalize.equalize_hist_u8(L)[0], D)
            _same_info(fa, fb, "%s frame %d" % (case, f)); assert na == nb
            _same_points(a.points(), b.points(), "%s frame %d" % (case, f))
        assert fa.status == 1 and fa.n_tracked > 20 and fa.n_keypoints_left > 300, (fa.status, fa.n_tracked, fa.n_keypoints_left)
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_capacity(monkeypatch):
    """max_keypoints one below frame 0's keypoint count (the checker's, before the extractor's border filter): VSLAM_ERR_CAPACITY; the count itself fits."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = _world(o, 1)
    o.create(cfg, 0, 1)
    g = hip.load()
    try:
        (L, D), = _frames(o, scene, [0])
        n = len(o.orb_detect(L, 5000, 1.2, 8, 31, 31, int(cfg.detector_threshold_minimum)))
        assert n > 300
        cfg.max_keypoints = n - 1
        t = RgbdTracker(g, cfg, p)
        with pytest.raises(VslamError) as e:
            t.process(L, D)
        assert e.value.code == ERR_CAPACITY, e.value
        t.destroy()
        cfg.max_keypoints = n
        t = RgbdTracker(g, cfg, p)
        fi, _ = t.process(L, D)
        assert fi.n_detected_left == n and fi.error_flags == 0
        t.destroy()
    finally:
        o.destroy()


@pytest.mark.gpu
def test_mask_refusals_leave_the_context_usable(monkeypatch):
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene, cfg, p = _world(o, 1)
        frames = _frames(o, scene, range(3))
    finally:
        o.destroy()
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.process(*frames[0]); b.process(*frames[0])
        mask = np.full((int(cfg.rows), int(cfg.cols)), 255, np.uint8)
        mask[:, :200] = 0
        for call in (lambda: a.set_detection_mask(mask, 2), lambda: a.set_frame_mask(mask, 2), lambda: a.set_undistortion_mask(True, 2)):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "detector_type ORB" in str(e.value) and "resizes its mask" in str(e.value), e.value    # the message says why
        for f in (1, 2):
            (fa, na), (fb, nb) = a.process(*frames[f]), b.process(*frames[f])
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
        assert fa.n_keypoints_left > 300
    finally:
        a.destroy(); b.destroy()


def _dot_world(o, descriptor, rows, cols, grid, counts):
    """An image of isolated bright pixels on black, four pixels apart: every dot is exactly one FAST corner at any threshold the controller
    can reach (its 16 ring pixels are dark; no other pixel sees nine contiguous ring pixels on one side), so a region holds as many corners
    as dots were put inside its 31-pixel border.  counts[r] dots go into region r, row by row from its corner (31, 31)."""
    from vslam_pose_estimation_framework_amd.capi import DepthParams
    scene, cfg, p0 = setup(o, "tum", descriptor=descriptor, seed=67)
    cfg.rows, cfg.cols = rows, cols
    cfg.det_rows, cfg.det_cols = grid
    K = np.array([[scene.fx, 0, cols / 2.0], [0, scene.fy, rows / 2.0], [0, 0, 1.0]])
    cfg.K[:] = list(K.reshape(-1))
    p = DepthParams.make(rows, cols, K, np.linalg.inv(K), np.linalg.inv(K), np.eye(4)[:3], 2e-3, 0.1, 40.0, 1, 1, 15, descriptor)
    p.detector_type = 1
    ref = PyLoop(o, cfg, p)
    img = np.zeros((rows, cols), np.uint8)
    for (rx, ry, rw, rh), n in zip(ref.regions, counts):
        ys, xs = np.arange(31, rh - 31, 4), np.arange(31, rw - 31, 4)
        assert len(ys) * len(xs) >= n, (len(ys), len(xs), n)
        for k in range(n):
            img[ry + ys[k // len(xs)], rx + xs[k % len(xs)]] = 255
    depth = np.full((rows, cols), 1000, np.uint16)                     # a wall two metres away
    return cfg, p, ref, img, depth


@pytest.mark.gpu
@pytest.mark.parametrize("descriptor", [1, 0])
@pytest.mark.parametrize("shape", ["one-level-2x2", "two-levels-by-one-row"])
def test_smallest_shapes(shape, descriptor, monkeypatch):
    """Regions of 83 rows hold exactly one pyramid level (level 1 would have 69 rows), a region of 84 rows holds two (level 1 has exactly 70);
    the level-0 corner counts straddle k_orb_select's 1024-entry pass: 1023 and 1025.  Both equal the checker."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    if shape == "one-level-2x2":
        cfg, p, ref, img, depth = _dot_world(o, descriptor, 162, 1500, (2, 2), [1023, 1025, 1024, 3])
    else:
        cfg, p, ref, img, depth = _dot_world(o, descriptor, 84, 1500, (1, 1), [1025 if descriptor else 1023])
    o.create(cfg, 0, 1)
    g = hip.load()
    dev = RgbdTracker(g, cfg, p)
    try:
        # premises, from the checker's side: the regions' level sizes and their level-0 corner counts behind runByImageBorder(31)
        counts = []
        for rx, ry, rw, rh in ref.regions:
            assert rh == (83 if shape == "one-level-2x2" else 84)
            assert int(np.rint(np.float32(rh) / np.float32(1.2))) == (69 if shape == "one-level-2x2" else 70)
            pxy, _ = o.fast_detect(np.ascontiguousarray(img[ry:ry + rh, rx:rx + rw]), (0, 0, rw, rh), int(cfg.detector_threshold_minimum))
            counts.append(int(sum(1 for x, y in pxy if 31 <= x < rw - 31 and 31 <= y < rh - 31)))
        if shape == "one-level-2x2":
            assert counts == [1023, 1025, 1024, 3], counts
        else:
            assert counts == [1025 if descriptor else 1023], counts
        top = 0
        for k in range(3):
            L = np.roll(img, 2 * k, axis=1)                            # the wall slides two pixels per frame
            a = ref.process(L, depth)
            fa, na = dev.process(L, depth)
            _against_checker(a, ref, fa, na, dev.points(), (shape, descriptor, k))
            assert fa.error_flags == 0
            top = max(top, int(ref.acc_level.max()))
            if k == 0:
                assert fa.n_detected_left >= sum(counts), (fa.n_detected_left, counts)
        assert top == (0 if shape == "one-level-2x2" else 1), top
    finally:
        dev.destroy(); o.destroy()
