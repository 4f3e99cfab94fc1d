"""Undistortion of raw RGB-D frames on the GPU (k_rectify + k_undistort_depth behind vslam_rgbd_set_undistortion, csrc/kernels_undistort.h;
DESIGN.md 6e): the depth kernel bit-exact against its numpy restatement, the fused path equal bit for bit to undistort-then-run, identity
maps equal to no undistortion, the contract of the switch, and a raw TUM folder end to end through tools/run_rgbd.py --undistort."""
import os
import sys

import numpy as np
import pytest

import undistort_cases as uc
from vslam_pose_estimation_framework_amd import evaluation, hip, io_formats, rectify
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RAW_ROWS, RAW_COLS = 200, 640       # raw frames of the fused cases; the tracker runs at the scene's 188 x 620
SHIFT = (10.0, 6.0)                 # the raw principal point: the pinhole image centred in the raw one
FRAMES = 8
WORLDS = 3                          # scenes rendered once; sequence i of a batch is world i % 3 from frame i // 3 on


@pytest.mark.gpu
def test_remap_nearest_u16_bit_exact():
    from _oracle import Oracle
    o = Oracle()
    g = hip.load()
    g.create(o.config_for_scene(o.scene_kitti(scale=0.5)), 0, 1)
    rng = np.random.default_rng(2)
    fractions = set()
    try:
        for (rows, cols, stride, drows, dcols) in ((5, 7, 7, 3, 5), (9, 13, 13, 9, 9), (61, 67, 80, 64, 64), (200, 640, 640, 188, 620)):
            src = rng.integers(0, 65536, (rows, stride)).astype(np.uint16)
            src[rng.random((rows, stride)) < 0.1] = 0
            src[rng.random((rows, stride)) < 0.1] = 65535
            src[:, cols:] = 12345                                                     # the padding must never be read as a pixel
            xy = np.stack([rng.integers(-3, cols + 3, (drows, dcols)), rng.integers(-3, rows + 3, (drows, dcols))], -1).astype(np.int16)
            a = rng.integers(0, 1024, (drows, dcols)).astype(np.uint16)
            flat_xy, flat_a = xy.reshape(-1, 2), a.reshape(-1)
            n = flat_a.size
            # fixed entries: beyond each of the four borders, the last column / row with a fraction that stays (15) and one that steps out
            # (16), the first column / row reached from -1 by a step, int16 extremes
            fixed = [(-1, 0, 15), (-1, 0, 16), (cols, 0, 0), (cols - 1, 0, 15), (cols - 1, 0, 16), (cols - 1, 0, 31), (0, -1, 15 * 32), (0, -1, 16 * 32),
                     (0, rows, 0), (0, rows - 1, 15 * 32), (0, rows - 1, 16 * 32), (cols - 1, rows - 1, 16 + 16 * 32), (-32768, -32768, 1023), (32767, 32767, 1023),
                     (-32768, 0, 0), (0, 32767, 16 * 32), (cols - 1, rows - 1, 0)]
            where = rng.choice(n, len(fixed), replace=False) if n >= len(fixed) else np.arange(n)
            for i, (x, y, f) in zip(where, fixed):
                flat_xy[i] = (x, y); flat_a[i] = f
            if n >= 4096:                                                            # every one of the 1024 fractions, inside the image
                at = rng.choice(n, 1024, replace=False)
                flat_a[at] = np.arange(1024)
                flat_xy[at, 0] = rng.integers(0, cols - 1, 1024); flat_xy[at, 1] = rng.integers(0, rows - 1, 1024)
            fractions |= set(int(v) for v in np.unique(a))
            got = g.remap_nearest_u16(src, xy, a, cols=cols)
            want = rectify.remap_nearest_u16(src[:, :cols], xy, a)
            assert got.dtype == np.uint16
            if n >= 4096:
                assert (want == 0).any() and (want == 65535).any() and (src[:, :cols] == 0).any()
            np.testing.assert_array_equal(got, want, err_msg=str((rows, cols, stride, drows, dcols)))
        assert len(fractions) == 1024
        # a camera's own maps at the size the fused cases use
        und, _ = _camera_and_maps(np.array([[359.4, 0, 303.6], [0, 359.4, 92.6], [0, 0, 1.0]]), 188, 620)
        src = rng.integers(0, 65536, (RAW_ROWS, RAW_COLS)).astype(np.uint16)
        np.testing.assert_array_equal(g.remap_nearest_u16(src, und.map_xy, und.map_a), rectify.remap_nearest_u16(src, und.map_xy, und.map_a))
        a = und.map_a.copy(); a[3, 4] = 1024                                          # an index >= 1024 is refused
        with pytest.raises(VslamError) as e:
            g.remap_nearest_u16(src, und.map_xy, a)
        assert e.value.code == ERR_INVALID
    finally:
        g.destroy(); o.destroy()


def _camera_and_maps(K, rows, cols):
    """freiburg1's lens in front of a 200 x 640 sensor: (the undistortion to camera K at rows x cols, the maps that make raw frames)."""
    cam = uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT)
    return rectify.undistortion(cam, K, rows, cols), uc.distorting_maps(cam, K)


@pytest.fixture(scope="module")
def worlds():
    """Rendered once for every fused case: the tum configuration at 620 x 188, the camera, and per world FRAMES + 2 frames as
    (raw image, raw depth, undistorted image, undistorted depth), the undistorted pair from the numpy checkers."""
    from _oracle import Oracle
    o = Oracle()
    try:
        out = []
        for w in range(WORLDS):
            scene, cfg, p = uc.setup(o, "tum", descriptor=1, seed=26 + 7 * w)
            K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
            und, lens = _camera_and_maps(K, scene.rows, scene.cols)
            frames = []
            for L, D in uc.render_frames(o, scene, FRAMES + 2):
                rawL, rawD = uc.distort_frame(lens, L, D)
                frames.append((rawL, rawD) + und.apply(rawL, rawD))
            out.append(frames)
    finally:
        o.destroy()
    # the premises: the stage has something to do, and the border handling is exercised
    rows, cols = und.rows, und.cols
    u, v = rectify.source_coordinates(und.cam, np.eye(3), np.concatenate([und.K, np.zeros((3, 1))], axis=1), rows, cols)
    vv, uu = np.mgrid[0:rows, 0:cols]
    moved = np.hypot(u - SHIFT[0] - uu, v - SHIFT[1] - vv) > 2.0
    assert moved.mean() > 0.4, moved.mean()
    x0, y0 = und.map_xy[..., 0].astype(int), und.map_xy[..., 1].astype(int)
    assert (x0 < -1).any() and (x0 >= RAW_COLS).any() and (y0 < -1).any() and (y0 >= RAW_ROWS).any()
    assert (rectify.remap_nearest_u16(np.ones((RAW_ROWS, RAW_COLS), np.uint16), und.map_xy, und.map_a) == 0).any()
    return cfg, p, und, out


def _sequence(worlds_frames, i):
    return worlds_frames[i % WORLDS][i // WORLDS:i // WORLDS + FRAMES]


def _pad(a, extra, fill):
    out = np.full(a.shape[:-1] + (a.shape[-1] + extra,), fill, a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _same_info(fa, fb, tag):
    for name, _ in fa._fields_:
        va, vb = getattr(fa, name), getattr(fb, name)
        if hasattr(va, "__len__"):
            va, vb = list(va), list(vb)
        assert va == vb, (tag, name, va, vb)


def _same_points(pa, pb, tag):
    for key in ("xy", "cam", "meta", "desc"):
        np.testing.assert_array_equal(pa[key], pb[key], err_msg="%s %s" % (tag, key))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "one-graph", "batch3", "batch9-device", "one-map"])
def test_fused_undistortion_equals_undistort_then_run(case, worlds, monkeypatch):
    """Tracker A has the maps and gets raw 200 x 640 frames with padded rows; tracker B gets the numpy-undistorted 188 x 620 frames.
    After every frame: frame info (poses in it) and the complete point lists bit for bit, undistorted() the numpy pair; with the map
    and the log on, ids, map and log too.  batch9-device: nine sequences (more than VS_RECT_SB = 8: a second batch block) whose raw
    frames already lie in device memory."""
    cfg, p, und, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case == "one-graph" else "0")
    g = hip.load()
    B = {"batch3": 3, "batch9-device": 9}.get(case, 1)
    seqs = [_sequence(frames, i) for i in range(B)]
    if B == 1:
        a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    else:
        a, b = RgbdBatch(g, cfg, p, B), RgbdBatch(g, cfg, p, B)
    try:
        a.set_undistortion(und)
        if case == "one-map":
            for t in (a, b):
                t.enable_map(4000); t.enable_observations(40000)
        for f in range(FRAMES):
            rawL = _pad(np.stack([s[f][0] for s in seqs]), 12, 7); rawD = _pad(np.stack([s[f][1] for s in seqs]), 6, 999)
            L = np.stack([s[f][2] for s in seqs]); D = np.stack([s[f][3] for s in seqs])
            if B == 1:
                ia, ib = [a.process(rawL[0], rawD[0])], [b.process(L[0], D[0])]
                pa, pb = [a.points()], [b.points()]
            else:
                if case == "batch9-device":
                    import torch
                    dev = torch.device("cuda", 0)
                    Ld = torch.from_numpy(rawL).to(dev); Dd = torch.from_numpy(rawD.view(np.int16)).to(dev)
                    torch.cuda.synchronize()
                    a.submit_device(Ld.data_ptr(), rawL.shape[2], rawL.shape[1] * rawL.shape[2], Dd.data_ptr(), rawD.shape[2], rawD.shape[1] * rawD.shape[2])
                    ia = a.wait()
                else:
                    ia = a.process(rawL, rawD)
                ib = b.process(L, D)
                pa, pb = [a.points(s) for s in range(B)], [b.points(s) for s in range(B)]
            for s in range(B):
                tag = "%s frame %d sequence %d" % (case, f, s)
                _same_info(ia[s][0], ib[s][0], tag)
                assert ia[s][1] == ib[s][1], tag
                _same_points(pa[s], pb[s], tag)
                gi, gd = a.undistorted(s)
                np.testing.assert_array_equal(gi, L[s], err_msg=tag + " image"); np.testing.assert_array_equal(gd, D[s], err_msg=tag + " depth")
            if case == "one-map":
                np.testing.assert_array_equal(a.point_ids(), b.point_ids())
                ma, mb, oa, ob = a.map(), b.map(), a.observations(), b.observations()
                for k in ma:
                    np.testing.assert_array_equal(ma[k], mb[k], err_msg="map %s frame %d" % (k, f))
                for k in oa:
                    np.testing.assert_array_equal(oa[k], ob[k], err_msg="log %s frame %d" % (k, f))
        assert all(fi.status == 1 and fi.n_tracked > 50 for fi, _ in ia)          # equal and tracking, not equal and empty
        if case == "one-map":
            assert len(ma["id"]) > 50 and len(oa["id"]) > 200
    finally:
        a.destroy(); b.destroy()


class _Identity(object):
    def __init__(self, rows, cols):
        self.rows, self.cols, self.raw_rows, self.raw_cols = rows, cols, rows, cols
        yy, xx = np.mgrid[0:rows, 0:cols]
        self.map_xy = np.stack([xx, yy], -1).astype(np.int16)
        self.map_a = np.zeros((rows, cols), np.uint16)


@pytest.mark.gpu
def test_identity_map_equals_no_undistortion(worlds, monkeypatch):
    """Identity maps change nothing; switching off mid-sequence changes nothing and frees the getter; the maps survive reset()."""
    cfg, p, _, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    g = hip.load()
    seq = [(fr[2], fr[3]) for fr in frames[0][:FRAMES]]
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_undistortion(_Identity(int(cfg.rows), int(cfg.cols)))
        with pytest.raises(VslamError) as e:                       # set, but no frame yet
            a.undistorted()
        assert e.value.code == ERR_STATE
        for f, (L, D) in enumerate(seq):
            if f == 5:
                a.set_undistortion(None)                           # off again: the rest of the sequence as if it had never been on
                with pytest.raises(VslamError) as e:
                    a.undistorted()
                assert e.value.code == ERR_STATE
            (fa, na), (fb, nb) = a.process(L, D), b.process(L, D)
            _same_info(fa, fb, "identity frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "identity frame %d" % f)
            if f < 5:
                gi, gd = a.undistorted()
                np.testing.assert_array_equal(gi, L); np.testing.assert_array_equal(gd, D)
        assert fa.status == 1 and fa.n_tracked > 50
        # the maps survive reset(): set, reset, and the frames still go through them
        a.set_undistortion(_Identity(int(cfg.rows), int(cfg.cols)))
        a.reset(); b.reset()
        with pytest.raises(VslamError) as e:                       # ... while the last frame is forgotten
            a.undistorted()
        assert e.value.code == ERR_STATE
        for f, (L, D) in enumerate(seq[:3]):
            (fa, na), (fb, nb) = a.process(L, D), b.process(L, D)
            _same_info(fa, fb, "after reset frame %d" % f)
            gi, gd = a.undistorted()
            np.testing.assert_array_equal(gi, L); np.testing.assert_array_equal(gd, D)
        assert fa.n_points > 50
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_undistortion_contract(worlds, monkeypatch):
    cfg, p, und, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    g = hip.load()
    raw = [(fr[0], fr[1]) for fr in frames[0][:4]]
    t = RgbdTracker(g, cfg, p)

    class Bad(object):
        pass
    try:
        bad = Bad(); bad.__dict__.update(und.__dict__); bad.map_a = und.map_a.copy(); bad.map_a[7, 9] = 1024
        with pytest.raises(VslamError) as e:
            t.set_undistortion(bad)
        assert e.value.code == ERR_INVALID and "1024" in str(e.value)
        bad = Bad(); bad.__dict__.update(und.__dict__); bad.raw_rows = 0
        with pytest.raises(VslamError) as e:
            t.set_undistortion(bad)
        assert e.value.code == ERR_INVALID
        with pytest.raises(ValueError):                            # maps of another size than the tracker's
            t.set_undistortion(_Identity(int(cfg.rows) + 1, int(cfg.cols)))
        t.set_undistortion(und)
        fi, _ = t.process(*raw[0])                                  # usable after the refusals
        t.submit(*raw[1])
        for call in (lambda: t.set_undistortion(None), lambda: t.set_undistortion(und), t.undistorted):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "in flight" in str(e.value)
        fi, _ = t.wait()
        assert fi.n_points > 50
        # a raw frame narrower than raw_cols (though wider than the tracker's 620) is refused, and the tracker goes on
        with pytest.raises(VslamError) as e:
            t.process(np.ascontiguousarray(raw[2][0][:, :630]), raw[2][1])
        assert e.value.code == ERR_INVALID and "row stride" in str(e.value)
        with pytest.raises(VslamError) as e:
            t.process(raw[2][0], np.ascontiguousarray(raw[2][1][:, :630]))
        assert e.value.code == ERR_INVALID and "row stride" in str(e.value)
        fi, _ = t.process(*raw[2])
        assert fi.n_points > 50
        np.testing.assert_array_equal(t.undistorted()[1], frames[0][2][3])
    finally:
        t.destroy()
    # the host-driven loop does not have the feature and says so; it goes on tracking
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: h.set_undistortion(und), lambda: h.set_undistortion(None), h.undistorted):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
        fi, _ = h.process(frames[0][0][2], frames[0][0][3])
        assert fi.n_points > 50
    finally:
        h.destroy()


@pytest.mark.gpu
def test_run_rgbd_undistort_end_to_end(tmp_path, monkeypatch):
    """The premise scene (test_undistort_host.py) written as a TUM folder of RAW frames of the k1 = -0.28 camera, through
    tools/run_rgbd.py --undistort with --map and --observations: the poses are those of a direct API run on the same arrays, no
    error flags, and the ATE against the renderer's ground truth is within 2 x the direct run's on the pinhole frames + 1 cm.  The same
    folder without the flag prints the hint and is logged for contrast, not asserted.
    First MI355X run: direct 0.0273 m, raw + --undistort 0.0159 m (ratio 0.58), raw without the flag 0.3388 m."""
    import run_rgbd
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene, _, _, K = uc.premise_scene(o)
        n = uc.PREMISE_FRAMES
        frames = uc.render_frames(o, scene, n)
        gt = uc.ground_truth(o, scene, n)
    finally:
        o.destroy()
    cam = uc.raw_camera(K, uc.EUROC_LIKE, scene.rows, scene.cols)
    lens = uc.distorting_maps(cam, K)
    raw = [uc.distort_frame(lens, L, D) for L, D in frames]
    uc.write_tum_folder(tmp_path / "raw", raw, gt)
    # a named camera, as the benchmark's are: the table's coefficients serve the flag without a value and the hint without the flag
    monkeypatch.setitem(io_formats.TUM_INTRINSICS, "synthetic", (scene.fx, scene.fy, scene.cx, scene.cy))
    monkeypatch.setitem(io_formats.TUM_DISTORTION, "synthetic", uc.EUROC_LIKE)
    lines = []
    res = run_rgbd.run(str(tmp_path / "raw"), "tum", "synthetic", uc.DEPTH_UNIT, str(tmp_path / "und.txt"), depth_scale=4.0, log=lines.append,
                       map_path=str(tmp_path / "map.ply"), obs_path=str(tmp_path / "bundle.npz"), undistort="")
    assert any("undistorting on the GPU" in ln for ln in lines), lines
    assert res["frames"] == n and res["error_flags"] == 0
    assert len(res["map"]["id"]) > 50 and len(res["observations"]["id"]) > 200 and res["reprojection"]["valid"] > 0
    g = hip.load()
    cfg, p = run_rgbd.configure(g, "tum", scene.rows, scene.cols, K, uc.DEPTH_UNIT, 1, 0, 4.0)
    a, d = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_undistortion(rectify.undistortion(cam))
        direct = []
        for k in range(n):
            fi, _ = a.process(*raw[k])
            np.testing.assert_array_equal(np.array(fi.camera_left_to_world).reshape(3, 4), res["poses"][k])
            direct.append(np.array(d.process(*frames[k])[0].camera_left_to_world))
    finally:
        a.destroy(); d.destroy()
    hint = []
    plain = run_rgbd.run(str(tmp_path / "raw"), "tum", "synthetic", uc.DEPTH_UNIT, None, depth_scale=4.0, log=hint.append)
    assert any("--undistort" in ln for ln in hint), hint
    nothing = []
    monkeypatch.setitem(io_formats.TUM_DISTORTION, "synthetic", (0.0,) * 5)
    zero = run_rgbd.run(str(tmp_path / "raw"), "tum", "synthetic", uc.DEPTH_UNIT, None, depth_scale=4.0, log=nothing.append, undistort="")
    assert any("nothing to undo" in ln for ln in nothing) and not any("undistorting on the GPU" in ln for ln in nothing)
    np.testing.assert_array_equal(zero["poses"], plain["poses"])               # zero coefficients: as without the flag
    ate0, ate_u, ate_r = evaluation.ate_rmse(np.array(direct), gt), evaluation.ate_rmse(res["poses"], gt), evaluation.ate_rmse(plain["poses"], gt)
    print("ATE RMSE after alignment: direct %.4f m, raw + --undistort %.4f m (ratio %.2f), raw without --undistort %.4f m" % (
        ate0, ate_u, ate_u / max(ate0, 1e-9), ate_r))
    assert ate_u <= 2.0 * ate0 + 0.01, (ate_u, ate0)
