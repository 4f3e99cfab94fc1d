"""Rectification on the GPU (k_rectify behind vslam_set_rectification / vslam_remap_u8): bit-exact against the numpy restatement,
the fused path equal bit for bit to rectify-then-run, identity maps equal to no rectification, and a raw EuRoC-layout rig end to end
through tools/run_kitti.py --rectify."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from vslam_pose_estimation_framework_amd import hip, rectify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

RAW_ROWS, RAW_COLS = 380, 500      # raw images
ROWS, COLS = 360, 480              # rectified size of the random smooth maps


def _api(cfg, n_streams=1):
    g = hip.load()
    g.create(cfg, 0, n_streams)
    return g


def _smooth_maps(rows, cols, raw_rows, raw_cols, seed):
    """A random smooth warp (scale, shear, low-frequency waves) to raw coordinates; the borders reach slightly outside the raw image."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    sx, sy = raw_cols / cols * rng.uniform(0.97, 1.0), raw_rows / rows * rng.uniform(0.97, 1.0)
    u = sx * xx + rng.uniform(-0.02, 0.02) * yy + rng.uniform(-3, 3) + 2.5 * np.sin(yy / 47.0 + rng.uniform(0, 6)) + 1.5 * np.cos(xx / 61.0)
    v = sy * yy + rng.uniform(-0.02, 0.02) * xx + rng.uniform(-3, 3) + 2.0 * np.sin(xx / 53.0 + rng.uniform(0, 6))
    return rectify.encode_map(u, v)


class _Rig(object):
    """What capi.set_rectification needs: raw size and both maps at the context's size."""

    def __init__(self, rows, cols, raw_rows, raw_cols, maps):
        self.rows, self.cols, self.raw_rows, self.raw_cols = rows, cols, raw_rows, raw_cols
        (self.map_xy_left, self.map_a_left), (self.map_xy_right, self.map_a_right) = maps

    def rectify(self, L, R):
        return rectify.remap_u8(L, self.map_xy_left, self.map_a_left), rectify.remap_u8(R, self.map_xy_right, self.map_a_right)


def _scene_and_config(o, seed=11):
    """A KITTI-like scene rendered at the raw size; the tracker's configuration at the rectified size with that scene's camera."""
    scene = o.scene_kitti(scale=0.4, seed=seed)
    scene.rows, scene.cols = RAW_ROWS, RAW_COLS
    scene.cx, scene.cy = RAW_COLS / 2.0, RAW_ROWS / 2.0
    cfg = o.config_for_scene(scene)
    cfg.rows, cfg.cols = ROWS, COLS
    cfg.K[2], cfg.K[5] = COLS / 2.0, ROWS / 2.0
    return scene, cfg


@pytest.mark.gpu
def test_remap_u8_bit_exact():
    from _oracle import Oracle
    o = Oracle()
    g = _api(o.config_for_scene(o.scene_kitti(scale=0.5)))
    rng = np.random.default_rng(1)
    try:
        for (rows, cols, stride, drows, dcols) in ((37, 53, 64, 41, 29), (380, 500, 509, 360, 481), (5, 3, 3, 7, 257), (120, 331, 333, 97, 255)):
            img = rng.integers(0, 256, (rows, stride), dtype=np.uint8)
            # random fractional maps over the image and a margin around it, negative and beyond-border coordinates, int16 extremes
            xy = np.stack([rng.integers(-4, cols + 4, (drows, dcols)), rng.integers(-4, rows + 4, (drows, dcols))], -1).astype(np.int16)
            ext = rng.random((drows, dcols)) < 0.03
            xy[ext, 0] = rng.choice([-32768, 32767, -1, cols - 1], ext.sum())
            xy[ext, 1] = rng.choice([-32768, 32767, -1, rows - 1], ext.sum())
            a = rng.integers(0, 1024, (drows, dcols)).astype(np.uint16)
            got = g.remap_u8(img, xy, a, cols=cols)
            want = rectify.remap_u8(img[:, :cols], xy, a)
            np.testing.assert_array_equal(got, want)
        # smooth maps of the size the fused tests use
        img = rng.integers(0, 256, (RAW_ROWS, RAW_COLS), dtype=np.uint8)
        xy, a = _smooth_maps(ROWS, COLS, RAW_ROWS, RAW_COLS, 5)
        np.testing.assert_array_equal(g.remap_u8(img, xy, a), rectify.remap_u8(img, xy, a))
        # an interpolation index >= 1024 is refused
        a[3, 4] = 1024
        with pytest.raises(Exception, match="-1"):
            g.remap_u8(img, xy, a)
    finally:
        g.destroy()


def _compare(a, b, s, tag):
    fa, fb = a.frame_info(s).as_dict(), b.frame_info(s).as_dict()
    assert fa == fb, (tag, {k: (fa[k], fb[k]) for k in fa if fa[k] != fb[k]})
    for side in (0, 1):
        for x, y in zip(a.keypoints(s, side), b.keypoints(s, side)):
            np.testing.assert_array_equal(x, y, err_msg=tag)
    pa, pb = a.points(s), b.points(s)
    for k in pa:
        np.testing.assert_array_equal(pa[k], pb[k], err_msg="%s %s" % (tag, k))
    n = fa["frame_index"]
    np.testing.assert_array_equal(a.poses(s, 0, n), b.poses(s, 0, n), err_msg=tag)


@pytest.mark.gpu
@pytest.mark.parametrize("B,mode", [(1, "host"), (1, "device"), (1, "stage"), (3, "host"), (3, "device")])
def test_fused_rectification_equals_rectify_then_run(B, mode):
    """Raw 380 x 500 pairs through a rectifying context == the numpy-rectified 360 x 480 pairs through a context without
    rectification: rectified images, keypoints, points, frame info and poses bit for bit, every stream, every frame."""
    import torch
    from _oracle import Oracle
    o = Oracle()
    scene, cfg = _scene_and_config(o)
    rig = _Rig(ROWS, COLS, RAW_ROWS, RAW_COLS, [_smooth_maps(ROWS, COLS, RAW_ROWS, RAW_COLS, 7), _smooth_maps(ROWS, COLS, RAW_ROWS, RAW_COLS, 8)])
    a, b = _api(cfg, B), _api(cfg, B)
    dev = torch.device("cuda", 0)
    try:
        a.set_rectification(rig)
        for k in range(8):
            raw = [o.render(scene, k + 2 * s) for s in range(B)]
            Lr = np.ascontiguousarray(np.stack([p[0] for p in raw]))
            Rr = np.ascontiguousarray(np.stack([p[1] for p in raw]))
            rect = [rig.rectify(L, R) for L, R in raw]
            Lc = np.ascontiguousarray(np.stack([p[0] for p in rect]))
            Rc = np.ascontiguousarray(np.stack([p[1] for p in rect]))
            if mode == "host":
                a.process_host(Lr, Rr)
            elif mode == "device":
                Ld, Rd = torch.from_numpy(Lr).to(dev), torch.from_numpy(Rr).to(dev)
                torch.cuda.synchronize()
                a.process_device(Ld.data_ptr(), Rd.data_ptr(), RAW_COLS, RAW_ROWS * RAW_COLS)
                a.synchronize()                   # the device images go out of scope
            else:
                a.check(a.fn("frame_begin")(a.ctx, Lr.ctypes.data_as(C.c_void_p), Rr.ctypes.data_as(C.c_void_p), C.c_int32(RAW_COLS),
                                            C.c_size_t(RAW_ROWS * RAW_COLS), C.c_int(0)))
                a.check(a.fn("frame_finish")(a.ctx))
            b.process_host(Lc, Rc)
            for s in range(B):
                gl, gr = a.rectified_images(s)
                np.testing.assert_array_equal(gl, Lc[s], err_msg="frame %d stream %d left" % (k, s))
                np.testing.assert_array_equal(gr, Rc[s], err_msg="frame %d stream %d right" % (k, s))
                _compare(a, b, s, "B=%d %s frame %d stream %d" % (B, mode, k, s))
        assert a.frame_info(0).n_points > 0
        # rectification survives a reset
        a.reset(); b.reset()
        raw = [o.render(scene, 1 + 2 * s) for s in range(B)]
        Lr = np.ascontiguousarray(np.stack([p[0] for p in raw])); Rr = np.ascontiguousarray(np.stack([p[1] for p in raw]))
        a.process_host(Lr, Rr)
        rect = [rig.rectify(L, R) for L, R in raw]
        b.process_host(np.ascontiguousarray(np.stack([p[0] for p in rect])), np.ascontiguousarray(np.stack([p[1] for p in rect])))
        for s in range(B):
            _compare(a, b, s, "after reset, stream %d" % s)
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_identity_maps_equal_no_rectification():
    from _oracle import Oracle
    o = Oracle()
    scene = o.scene_kitti(scale=0.5, seed=3)
    cfg = o.config_for_scene(scene)
    rows, cols = int(cfg.rows), int(cfg.cols)
    yy, xx = np.mgrid[0:rows, 0:cols]
    ident = (np.stack([xx, yy], -1).astype(np.int16), np.zeros((rows, cols), np.uint16))
    a, b = _api(cfg), _api(cfg)
    try:
        a.set_rectification(_Rig(rows, cols, rows, cols, [ident, ident]))
        for k in range(10):
            L, R = o.render(scene, k)
            a.process_host(L, R)
            b.process_host(L, R)
        _compare(a, b, 0, "identity maps")
        # switched off again: the context takes rectified images of its own size
        a.set_rectification(None)
        with pytest.raises(Exception, match="-5"):
            a.rectified_images(0)
        L, R = o.render(scene, 10)
        a.process_host(L, R); b.process_host(L, R)
        _compare(a, b, 0, "rectification off")
    finally:
        a.destroy(); b.destroy()


# ---- end to end on a raw, distorted, non-parallel rig -------------------------------------------------------------------------------
RAW_LEFT = dict(K=[[461.2, 0, 371.4], [0, 460.1, 244.6], [0, 0, 1]], dist=[-0.2834, 0.0740, 0.00019, 1.76e-05])
RAW_RIGHT = dict(K=[[455.9, 0, 378.3], [0, 455.0, 252.9], [0, 0, 1]], dist=[-0.2837, 0.0745, -0.00010, -3.56e-05])
Q_LEFT = (0.4, -0.9, 0.3)       # degrees: raw camera k = Q_k * (the scene's rectified camera k)
Q_RIGHT = (-0.6, 0.7, -0.5)


def _bilinear(img, u, v):
    H, W = img.shape
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = u - x0, v - y0
    f = img.astype(np.float64)

    def at(y, x):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, f[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)
    val = (1 - fx) * (1 - fy) * at(y0, x0) + fx * (1 - fy) * at(y0, x0 + 1) + (1 - fx) * fy * at(y0 + 1, x0) + fx * fy * at(y0 + 1, x0 + 1)
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def raw_rig(scene):
    """Both raw cameras and the cam0 -> cam1 transform of the rig that sees the scene's rectified pair through Q_LEFT / Q_RIGHT."""
    rows, cols = int(scene.rows), int(scene.cols)
    cams = [rectify.CameraModel(c["K"], c["dist"], rows, cols) for c in (RAW_LEFT, RAW_RIGHT)]
    Q = [rectify.rodrigues(np.radians(q)) for q in (Q_LEFT, Q_RIGHT)]
    R = Q[1] @ Q[0].T
    T = -Q[1] @ np.array([scene.baseline_m, 0.0, 0.0])
    return cams, Q, R, T


def warp_to_raw(scene, cams, Q, images):
    """For each raw pixel: undistort, rotate into the scene's rectified camera, project with the scene's K, bilinear sample."""
    rows, cols = int(scene.rows), int(scene.cols)
    vv, uu = np.mgrid[0:rows, 0:cols].astype(np.float64)
    out = []
    for cam, Qk, img in zip(cams, Q, images):
        xy = cam.undistort_normalized(np.stack([uu.ravel(), vv.ravel()], 1))
        X = Qk.T @ np.concatenate([xy, np.ones((len(xy), 1))], 1).T
        u = scene.fx * X[0] / X[2] + scene.cx
        v = scene.fy * X[1] / X[2] + scene.cy
        out.append(_bilinear(img, u.reshape(rows, cols), v.reshape(rows, cols)))
    return out


def _sensor_yaml(path, T_BS, cam):
    rows = ",\n         ".join(", ".join(repr(float(x)) for x in T_BS[i]) for i in range(4))
    K = cam.K
    path.write_text("%%YAML:1.0\nsensor_type: camera\nT_BS:\n  cols: 4\n  rows: 4\n  data: [%s]\nrate_hz: 20\nresolution: [%d, %d]\n"
                    "camera_model: pinhole\nintrinsics: [%r, %r, %r, %r]\ndistortion_model: radial-tangential\ndistortion_coefficients: [%s]\n" % (
                        rows, cam.cols, cam.rows, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), ", ".join(repr(float(x)) for x in cam.dist[:4])))


def write_asl(root, o, scene, n, raw=None):
    """An ASL folder of the scene: the rendered (rectified) pairs, or with raw = (cams, Q, R, T) the raw rig's images + sensor.yaml."""
    from vslam_pose_estimation_framework_amd import io_formats as io
    base = root / "mav0"
    for cam in ("cam0", "cam1"):
        (base / cam / "data").mkdir(parents=True)
    stamps = [1403636579763555584 + 50_000_000 * k for k in range(n)]
    lines = ["#timestamp [ns],filename"]
    for k, ts in enumerate(stamps):
        L, R = o.render(scene, k)
        if raw is not None:
            L, R = warp_to_raw(scene, raw[0], raw[1], (L, R))
        io.write_png_gray8(str(base / "cam0" / "data" / ("%d.png" % ts)), L)
        io.write_png_gray8(str(base / "cam1" / "data" / ("%d.png" % ts)), R)
        lines.append("%d,%d.png" % (ts, ts))
    for cam in ("cam0", "cam1"):
        (base / cam / "data.csv").write_text("\n".join(lines) + "\n")
    if raw is not None:
        cams, Q, R, T = raw
        T_B0 = np.eye(4)
        T_B0[:3, :3] = rectify.rodrigues(np.radians([0.5, -1.0, 90.0]))
        T_B0[:3, 3] = [-0.0216, -0.0647, 0.0098]
        T_10 = np.eye(4)
        T_10[:3, :3], T_10[:3, 3] = R, T
        _sensor_yaml(base / "cam0" / "sensor.yaml", T_B0, cams[0])
        _sensor_yaml(base / "cam1" / "sensor.yaml", T_B0 @ np.linalg.inv(T_10), cams[1])
    (base / "state_groundtruth_estimate0").mkdir()
    with open(base / "state_groundtruth_estimate0" / "data.csv", "w") as f:
        f.write("#timestamp [ns], p_x, p_y, p_z\n")
        for j in range(-8, 4 * n + 8):
            k = j / 4.0
            k0 = int(np.floor(k)); a = k - k0
            p0 = np.array(o.gt_pose(scene, k0))[:, 3]; p1 = np.array(o.gt_pose(scene, k0 + 1))[:, 3]
            p = p0 + a * (p1 - p0)
            f.write("%d,%.9f,%.9f,%.9f\n" % (stamps[0] + int(round(k * 50_000_000)), p[0], p[1], p[2]))


@pytest.mark.gpu
def test_run_kitti_rectify_raw_euroc_rig(tmp_path):
    """A raw, distorted (k1 = -0.28), non-parallel (rotations up to 0.9 degrees) EuRoC-shaped rig, rendered from the synthetic scene
    and written as an ASL folder with sensor.yaml, through run_kitti --rectify in exact and in chunked mode.  Required: no error
    flags, and the trajectory_analyzer's optimal RMSE within 2x the direct run's on the scene's own rectified images + 1 cm (+ 2 cm
    chunked).  First MI355X run: direct 0.0023 m, raw + --rectify 0.0027 m (ratio 1.14), chunked 0.0018 m; the same raw folder
    without --rectify 0.283 m (logged for contrast only, not asserted)."""
    import run_kitti
    from _oracle import Oracle
    o = Oracle()
    scene = o.scene_euroc(seed=5)
    n = 24
    write_asl(tmp_path / "direct", o, scene, n)
    raw = raw_rig(scene)
    write_asl(tmp_path / "raw", o, scene, n, raw)
    quiet = lambda *_: None
    direct = run_kitti.run(str(tmp_path / "direct"), str(tmp_path / "direct.txt"), "tum", log=quiet)
    assert direct["error_flags"] == 0
    ate0 = direct["trajectory_analyzer"]["optimal_rmse"]
    lines = []
    res = run_kitti.run(str(tmp_path / "raw"), str(tmp_path / "rect.txt"), "tum", log=lines.append, rectify=True)
    assert any("rectifying on the GPU" in ln for ln in lines)
    chunked = run_kitti.run(str(tmp_path / "raw"), str(tmp_path / "rect_chunks.txt"), "tum", log=quiet, rectify=True, chunks=3, overlap=3)
    hint = []
    plain = run_kitti.run(str(tmp_path / "raw"), str(tmp_path / "plain.txt"), "tum", log=hint.append)
    assert any("--rectify" in ln for ln in hint)
    ate_r, ate_c = res["trajectory_analyzer"]["optimal_rmse"], chunked["trajectory_analyzer"]["optimal_rmse"]
    print("ATE optimal RMSE: direct %.4f m, raw + --rectify %.4f m (ratio %.2f), chunked %.4f m, raw without --rectify %.4f m" % (
        ate0, ate_r, ate_r / max(ate0, 1e-9), ate_c, plain["trajectory_analyzer"]["optimal_rmse"]))
    assert res["frames"] == n and res["error_flags"] == 0
    assert chunked["frames"] == n and chunked["error_flags"] == 0
    assert ate_r <= 2.0 * ate0 + 0.01, (ate_r, ate0)
    assert ate_c <= 2.0 * ate0 + 0.02, (ate_c, ate0)
    with pytest.raises(SystemExit, match="already rectified"):
        run_kitti.run(str(tmp_path / "direct" / "mav0" / "cam0"), None, "kitti", log=quiet, rectify=True, layout="kitti")
