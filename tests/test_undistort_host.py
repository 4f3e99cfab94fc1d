"""Undistortion of raw RGB-D frames, the parts that need no GPU: the maps of rectify.undistortion against the fp64 camera model, the
numpy checker of the depth kernel (rectify.remap_nearest_u16), the distortion table and tools/run_rgbd.py's --undistort handling, and
the premise of test_undistort_gpu.py's end-to-end case on the checker loop (tests/rgbd_loop.py over the CPU oracle)."""
import os
import sys

import numpy as np
import pytest

import undistort_cases as uc
from vslam_pose_estimation_framework_amd import evaluation, io_formats, rectify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SUB = 1.0 / 64.0        # rounding a coordinate to 1/32 px moves it by at most half a step


def _freiburg1(rows=480, cols=640):
    fx, fy, cx, cy = io_formats.TUM_INTRINSICS["freiburg1"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return rectify.CameraModel(K, io_formats.TUM_DISTORTION["freiburg1"], rows, cols)


def _decode(map_xy, map_a):
    a = map_a.astype(np.int64)
    return map_xy[..., 0] + (a & 31) / 32.0, map_xy[..., 1] + ((a >> 5) & 31) / 32.0


def test_maps_follow_the_camera_model():
    """freiburg1 at 480 x 640, output camera = the raw camera's K: every map entry within 1/64 px of K distort(K^-1 pixel) in fp64,
    every fraction index below 1024; the displacement the issue quotes (median 4.8 px, maximum 36.8 px) is what the maps undo."""
    cam = _freiburg1()
    und = rectify.undistortion(cam)
    assert (und.rows, und.cols, und.raw_rows, und.raw_cols) == (480, 640, 480, 640)
    np.testing.assert_array_equal(und.K, cam.K)
    assert und.map_xy.dtype == np.int16 and und.map_a.dtype == np.uint16 and und.map_xy.shape == (480, 640, 2) and und.map_a.shape == (480, 640)
    assert int(und.map_a.max()) < 1024
    vv, uu = np.mgrid[0:480, 0:640].astype(np.float64)
    xd, yd = cam.distort((uu - cam.K[0, 2]) / cam.K[0, 0], (vv - cam.K[1, 2]) / cam.K[1, 1])
    u, v = cam.K[0, 0] * xd + cam.K[0, 2], cam.K[1, 1] * yd + cam.K[1, 2]
    mu, mv = _decode(und.map_xy, und.map_a)
    assert np.abs(mu - u).max() <= SUB + 1e-9 and np.abs(mv - v).max() <= SUB + 1e-9
    d = np.hypot(u - uu, v - vv)
    print("freiburg1 640 x 480: displacement median %.2f px, maximum %.2f px" % (np.median(d), d.max()))
    assert abs(np.median(d) - 4.8) < 0.1 and abs(d.max() - 36.8) < 0.1
    # another output camera and size: the maps have the output size and follow K_new
    K2 = cam.K.copy(); K2[0, 0] *= 0.9; K2[1, 1] *= 0.9; K2[0, 2] = 300.0; K2[1, 2] = 200.0
    und2 = rectify.undistortion(cam, K2, 400, 600)
    assert (und2.rows, und2.cols, und2.raw_rows, und2.raw_cols) == (400, 600, 480, 640) and und2.map_a.shape == (400, 600)
    np.testing.assert_array_equal(und2.K, K2)
    vv, uu = np.mgrid[0:400, 0:600].astype(np.float64)
    xd, yd = cam.distort((uu - 300.0) / K2[0, 0], (vv - 200.0) / K2[1, 1])
    mu, mv = _decode(und2.map_xy, und2.map_a)
    assert np.abs(mu - (cam.K[0, 0] * xd + cam.K[0, 2])).max() <= SUB + 1e-9 and np.abs(mv - (cam.K[1, 1] * yd + cam.K[1, 2])).max() <= SUB + 1e-9


def test_projected_points_land_where_the_map_points():
    """3-D points through the raw camera (CameraModel.project) and through the output K: the map entry at the rounded output pixel is
    the raw pixel, to 1/64 px plus what rounding the output pixel moves the source (half a pixel times the map's local slope)."""
    cam = _freiburg1()
    K2 = cam.K.copy(); K2[0, 2] += 3.25; K2[1, 2] -= 2.5
    und = rectify.undistortion(cam, K2)
    rng = np.random.default_rng(3)
    X = np.stack([rng.uniform(-2.5, 2.5, 4000), rng.uniform(-1.8, 1.8, 4000), rng.uniform(2.0, 9.0, 4000)], axis=1)
    raw = cam.project(X)
    out = np.stack([K2[0, 0] * X[:, 0] / X[:, 2] + K2[0, 2], K2[1, 1] * X[:, 1] / X[:, 2] + K2[1, 2]], axis=1)
    px = np.rint(out).astype(np.int64)
    keep = (px[:, 0] >= 1) & (px[:, 0] < und.cols - 1) & (px[:, 1] >= 1) & (px[:, 1] < und.rows - 1)
    assert keep.sum() > 2000
    px, raw, out = px[keep], raw[keep], out[keep]
    mu, mv = _decode(und.map_xy, und.map_a)
    # the map's slope from its own neighbours (central differences), applied to the rounding offset of the pixel
    dux = (mu[px[:, 1], px[:, 0] + 1] - mu[px[:, 1], px[:, 0] - 1]) / 2.0; duy = (mu[px[:, 1] + 1, px[:, 0]] - mu[px[:, 1] - 1, px[:, 0]]) / 2.0
    dvx = (mv[px[:, 1], px[:, 0] + 1] - mv[px[:, 1], px[:, 0] - 1]) / 2.0; dvy = (mv[px[:, 1] + 1, px[:, 0]] - mv[px[:, 1] - 1, px[:, 0]]) / 2.0
    off = out - px
    pu = mu[px[:, 1], px[:, 0]] + dux * off[:, 0] + duy * off[:, 1]
    pv = mv[px[:, 1], px[:, 0]] + dvx * off[:, 0] + dvy * off[:, 1]
    # slopes from values rounded to 1/32 px carry 1/64 px themselves, times an offset of at most 1/2 in each direction; the map's
    # curvature over half a pixel is below 1e-3 px for this lens
    tol = SUB + 2 * 0.5 * SUB + 2e-3
    err = np.maximum(np.abs(pu - raw[:, 0]), np.abs(pv - raw[:, 1]))
    print("projected points: largest |map - raw pixel| = %.4f px over %d points (bound %.4f)" % (err.max(), len(err), tol))
    assert err.max() <= tol
    # without the slope term: within 1/64 px plus the rounding of the pixel times the largest slope
    slope = max(np.abs(dux).max() + np.abs(duy).max(), np.abs(dvx).max() + np.abs(dvy).max())
    plain = np.maximum(np.abs(mu[px[:, 1], px[:, 0]] - raw[:, 0]), np.abs(mv[px[:, 1], px[:, 0]] - raw[:, 1]))
    assert plain.max() <= SUB + 0.5 * slope + 2e-3


def test_remap_nearest_u16_rule():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 65536, (7, 9)).astype(np.uint16)
    src[0, 0], src[6, 8] = 0, 65535
    yy, xx = np.mgrid[0:7, 0:9]
    ident = np.stack([xx, yy], -1).astype(np.int16)
    zero = np.zeros((7, 9), np.uint16)
    np.testing.assert_array_equal(rectify.remap_nearest_u16(src, ident, zero), src)
    assert rectify.remap_nearest_u16(src, ident, zero).dtype == np.uint16
    # entirely outside: left, right, above, below, int16 extremes
    for dx, dy in ((-9, 0), (9, 0), (0, -7), (0, 7), (-32768, 0), (32767 - 8, 32767 - 6)):
        m = ident.astype(np.int64) + np.array([dx, dy])
        np.testing.assert_array_equal(rectify.remap_nearest_u16(src, np.clip(m, -32768, 32767).astype(np.int16), zero), 0)
    # the hand-worked 2 x 3 case: source
    #   10 20 30
    #   40 50 65535
    s = np.array([[10, 20, 30], [40, 50, 65535]], np.uint16)
    xy = np.array([[[0, 0], [0, 0], [1, 0]], [[1, 0], [2, 0], [2, 1]]], np.int16)
    a = np.array([[15, 16, 15 * 32], [16 * 32, 16 + 16 * 32, 16]], np.uint16)
    #  (0,0) ax 15: stays   -> s[0][0] = 10        (0,0) ax 16: steps right -> s[0][1] = 20      (1,0) ay 15: stays -> s[0][1] = 20
    #  (1,0) ay 16: steps down -> s[1][1] = 50     (2,0) ax 16, ay 16: x = 3 outside -> 0        (2,1) ax 16: x = 3 outside -> 0
    np.testing.assert_array_equal(rectify.remap_nearest_u16(s, xy, a), np.array([[10, 20, 20], [50, 0, 0]], np.uint16))
    xy2 = np.array([[[2, 0], [1, 1], [-1, 0]], [[-1, -1], [2, 1], [0, 1]]], np.int16)
    a2 = np.array([[16 * 32, 31 + 31 * 32, 16], [16 + 16 * 32, 15 + 15 * 32, 31 * 32]], np.uint16)
    #  (2,0) ay 16 -> s[1][2] = 65535   (1,1) ax 31, ay 31 -> (2,2): row outside -> 0   (-1,0) ax 16 -> s[0][0] = 10
    #  (-1,-1) both step -> s[0][0] = 10   (2,1) stays -> 65535   (0,1) ay 31 -> row 2 outside -> 0
    np.testing.assert_array_equal(rectify.remap_nearest_u16(s, xy2, a2), np.array([[65535, 0, 10], [10, 65535, 0]], np.uint16))
    # Undistortion.apply is the pair of checkers on one map
    cam = rectify.CameraModel(np.array([[30.0, 0, 4.0], [0, 30.0, 3.0], [0, 0, 1]]), uc.EUROC_LIKE, 7, 9)
    und = rectify.undistortion(cam)
    img = rng.integers(0, 256, (7, 9)).astype(np.uint8)
    gi, gd = und.apply(img, src)
    np.testing.assert_array_equal(gi, rectify.remap_u8(img, und.map_xy, und.map_a))
    np.testing.assert_array_equal(gd, rectify.remap_nearest_u16(src, und.map_xy, und.map_a))


def test_distortion_table_and_tool_arguments():
    import run_rgbd
    assert set(io_formats.TUM_DISTORTION) == set(io_formats.TUM_INTRINSICS)
    assert all(len(v) == 5 for v in io_formats.TUM_DISTORTION.values())
    assert not any(io_formats.TUM_DISTORTION["freiburg3"]) and not any(io_formats.TUM_DISTORTION["icl"])
    assert io_formats.TUM_DISTORTION["freiburg1"] == uc.FREIBURG1
    a = run_rgbd.parse_args(["folder"])
    assert a.undistort is None and run_rgbd.distortion_of(a.undistort, a.intrinsics) is None
    a = run_rgbd.parse_args(["folder", "--undistort"])                       # the flag alone: the table's entry of --intrinsics
    assert a.undistort == "" and run_rgbd.distortion_of(a.undistort, a.intrinsics) == io_formats.TUM_DISTORTION["freiburg1"]
    a = run_rgbd.parse_args(["folder", "--undistort", "--intrinsics", "freiburg2"])
    assert run_rgbd.distortion_of(a.undistort, a.intrinsics) == io_formats.TUM_DISTORTION["freiburg2"]
    a = run_rgbd.parse_args(["folder", "--undistort", "0.1,-0.2,0.001,-0.002,0.3"])
    assert run_rgbd.distortion_of(a.undistort, a.intrinsics) == (0.1, -0.2, 0.001, -0.002, 0.3)
    a = run_rgbd.parse_args(["folder", "--undistort", "-0.28,0.074,0,0"])      # four numbers, a negative one first
    assert run_rgbd.distortion_of(a.undistort, a.intrinsics) == (-0.28, 0.074, 0.0, 0.0, 0.0)
    a = run_rgbd.parse_args(["folder", "--undistort", "--intrinsics", "icl"])  # zero coefficients: run() says so and runs as without the flag
    assert not any(run_rgbd.distortion_of(a.undistort, a.intrinsics))
    assert run_rgbd.distortion_of((0.0, 0.0, 0.0, 0.0), "freiburg1") == (0.0,) * 5
    with pytest.raises(SystemExit, match="named --intrinsics"):
        run_rgbd.distortion_of("", "500,500,320,240")
    with pytest.raises(SystemExit, match="4 or 5"):
        run_rgbd.distortion_of("0.1,0.2", "freiburg1")
    with pytest.raises(SystemExit, match="expected k1"):
        run_rgbd.distortion_of("somewhere/else", "freiburg1")


@pytest.fixture(scope="module")
def premise():
    """The premise scene run three ways per camera on the checker loop: (direct, {camera: (undistorted, raw as it is)}), each an
    (ATE RMSE after alignment in m, fewest points in a frame) pair."""
    from _oracle import Oracle
    from rgbd_loop import RgbdTracker as PyLoop
    o = Oracle()
    scene, cfg, p, K = uc.premise_scene(o)
    n = uc.PREMISE_FRAMES
    frames = uc.render_frames(o, scene, n)
    gt = uc.ground_truth(o, scene, n)

    def run(fr):
        o.create(cfg, 0, 1)
        tr = PyLoop(o, cfg, p)
        poses, fewest = [], 1 << 30
        for L, D in fr:
            poses.append(tr.process(L, D)["pose"])
            fewest = min(fewest, len(tr.frames[-1].points))
        return evaluation.ate_rmse(np.array(poses), gt), fewest
    try:
        direct = run(frames)
        out = {}
        for name, dist in (("freiburg1", uc.FREIBURG1), ("euroc-like", uc.EUROC_LIKE)):
            cam = uc.raw_camera(K, dist, scene.rows, scene.cols)
            maps = uc.distorting_maps(cam, K)
            raw = [uc.distort_frame(maps, L, D) for L, D in frames]
            und = rectify.undistortion(cam)
            out[name] = (run([und.apply(L, D) for L, D in raw]), run(raw))
    finally:
        o.destroy()
    return direct, out


@pytest.mark.parametrize("camera", ["freiburg1", "euroc-like"])
def test_premise_of_the_end_to_end_case(premise, camera):
    """On the checker loop alone (tum configuration, 620 x 188, 20 frames, 4.76 m of path): raw frames undistorted on the fixed-point
    maps track as well as the renderer's pinhole frames (ATE <= 2 x direct + 1 cm, the bound's form of
    test_run_kitti_rectify_raw_euroc_rig), the same raw frames used as they are do not, and the tracker runs in all three (>= 150
    points in every frame).  Measured: direct 0.0273 m; freiburg1's coefficients 0.0134 m undistorted, 0.1325 m as they are;
    k1 -0.28, k2 0.074: 0.0159 m undistorted, 0.3388 m as they are."""
    (ate0, pts0), runs = premise
    (ate_u, pts_u), (ate_r, pts_r) = runs[camera]
    print("%s: direct %.4f m (%d points), raw then undistorted %.4f m (%d), raw as it is %.4f m (%d)" % (camera, ate0, pts0, ate_u, pts_u, ate_r, pts_r))
    assert min(pts0, pts_u, pts_r) >= 150
    assert ate_u <= 2.0 * ate0 + 0.01, (ate_u, ate0)
    assert ate_r > 2.0 * ate0 + 0.01, (ate_r, ate0)
