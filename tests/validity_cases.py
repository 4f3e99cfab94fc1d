"""What the validity-mask and RGB-D frame-mask tests share (test_validity_host.py, test_validity_gpu.py, test_rgbd_frame_mask_gpu.py,
test_run_validity.py): the scalar restatement of rectify.validity, random maps with the fixed border entries, the wide RGB-D camera
(undistort_cases' freiburg1 lens in front of a 200 x 640 sensor, output camera 0.9 f at 188 x 620), the wide stereo rig (test_rectify_gpu's
380 x 500 rig with both P matrices' f scaled), and the moving frame masks."""
import functools

import numpy as np

import undistort_cases as uc
from vslam_pose_estimation_framework_amd import mask, rectify

SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 129), (9, 13), (61, 67), (70, 200)]
MARGINS = [0, 1, 7, 63, 64]
RAW_ROWS, RAW_COLS = 200, 640       # the RGB-D sensor (test_undistort_gpu.py)
SHIFT = (10.0, 6.0)
F_SCALE = 0.9                       # the output camera's focal length over the scene camera's; 0.9 held every premise (0.85 / 0.8 not needed)
STEREO_F_SCALE = 0.8                # the stereo rig at the raw size: 0.9 and 0.85 leave the right image without invalid pixels inside the border
BORDER = 28
FRAMES = 12


def scalar_validity(map_xy, map_a, raw_rows, raw_cols):
    """rectify.validity entry by entry in plain Python integers: every tap of non-zero weight inside the raw image."""
    rows, cols = map_a.shape
    out = np.zeros((rows, cols), bool)
    for r in range(rows):
        for c in range(cols):
            x0, y0, a = int(map_xy[r, c, 0]), int(map_xy[r, c, 1]), int(map_a[r, c])
            ax, ay = a & 31, (a >> 5) & 31
            taps = [(x0, y0, (32 - ax) * (32 - ay)), (x0 + 1, y0, ax * (32 - ay)), (x0, y0 + 1, (32 - ax) * ay), (x0 + 1, y0 + 1, ax * ay)]
            out[r, c] = all(0 <= x < raw_cols and 0 <= y < raw_rows for x, y, w in taps if w > 0)
    return out


def fixed_entries(raw_rows, raw_cols):
    """(x0, y0, a, valid): the border entries of test_undistort_gpu.py's fixed list, each with what the rule says of it."""
    c, r = raw_cols, raw_rows
    return [(-1, 0, 15, False), (-1, 0, 16, False), (-1, 0, 31, False), (c, 0, 0, False), (c - 1, 0, 0, True), (c - 1, 0, 1, False), (c - 1, 0, 15, False),
            (c - 1, 0, 31, False), (0, -1, 15 * 32, False), (0, -1, 31 * 32, False), (0, r, 0, False), (0, r - 1, 0, True), (0, r - 1, 1 * 32, False),
            (0, r - 1, 16 * 32, False), (c - 1, r - 1, 16 + 16 * 32, False), (c - 1, r - 1, 1 + 1 * 32, False), (c - 1, r - 1, 0, True),
            (-32768, -32768, 1023, False), (32767, 32767, 1023, False), (-32768, 0, 0, False), (0, 32767, 16 * 32, False), (0, 0, 0, True),
            (0, 0, 1023, c > 1 and r > 1), (c - 2, r - 2, 1023, c > 1 and r > 1)]


def random_maps(rows, cols, seed):
    """(map_xy, map_a, raw_rows, raw_cols, fixed [(index, valid)]): entries over the raw image and a margin around it, integer entries on the
    last column / row, the fixed border entries at random places (as many as fit)."""
    rng = np.random.default_rng(100 * rows + cols + seed)
    raw_rows, raw_cols = max(1, rows - 3 + seed % 5), max(1, cols - 2 + seed % 3)
    xy = np.stack([rng.integers(-3, raw_cols + 3, (rows, cols)), rng.integers(-3, raw_rows + 3, (rows, cols))], -1).astype(np.int16)
    a = rng.integers(0, 1024, (rows, cols)).astype(np.uint16)
    whole = rng.random((rows, cols)) < 0.3
    a[whole] = 0                          # integer coordinates: a single tap
    flat_xy, flat_a = xy.reshape(-1, 2), a.reshape(-1)
    fixed = fixed_entries(raw_rows, raw_cols)
    n = flat_a.size
    where = rng.choice(n, min(n, len(fixed)), replace=False)
    placed = []
    for i, (x, y, f, ok) in zip(where, fixed):
        flat_xy[i] = (x, y); flat_a[i] = f
        placed.append((int(i), bool(ok)))
    return xy, a, raw_rows, raw_cols, placed


def words_of(map_xy, map_a, raw_rows, raw_cols, margin):
    return mask.pack_bool(mask.erode(rectify.validity(map_xy, map_a, raw_rows, raw_cols), margin))


def mask_image(keep_bool):
    """The u8 image a caller would upload for a keep-mask."""
    return np.where(keep_bool, 255, 0).astype(np.uint8)


# ---- the wide RGB-D camera ---------------------------------------------------------------------------------------------------------
def wide_undistortion(K, rows, cols, f_scale=F_SCALE):
    """(the undistortion to the camera f_scale * f with K's principal point at rows x cols, the lens maps that make raw frames, K_new)."""
    cam = uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT)
    Kn = np.array(K, np.float64).reshape(3, 3).copy()
    Kn[0, 0] *= f_scale; Kn[1, 1] *= f_scale
    return rectify.undistortion(cam, Kn, rows, cols), uc.distorting_maps(cam, K), Kn


@functools.lru_cache(maxsize=None)
def rgbd_world(seed=26, n=FRAMES):
    """dict(cfg, p, und, frames [(raw image, raw depth, undistorted image, undistorted depth)]): the tum scene of undistort_cases behind the
    wide undistortion, configuration and depth parameters those of the output camera.  Rendered once per process."""
    from _oracle import Oracle
    from test_rgbd_mode import DEPTH_SCALE, YAML
    from vslam_pose_estimation_framework_amd.capi import DepthParams
    o = Oracle()
    try:
        scene, cfg, p = uc.setup(o, "tum", descriptor=1, seed=seed)
        K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
        und, lens, Kn = wide_undistortion(K, scene.rows, scene.cols)
        frames = []
        for L, D in uc.render_frames(o, scene, n):
            rawL, rawD = uc.distort_frame(lens, L, D)
            frames.append((rawL, rawD) + und.apply(rawL, rawD))
    finally:
        o.destroy()
    cfg = cfg.copy()
    for i in range(9):
        cfg.K[i] = float(Kn.reshape(9)[i])
    y = YAML["tum"]
    p = DepthParams.make(scene.rows, scene.cols, Kn, np.linalg.inv(Kn), np.linalg.inv(Kn), np.eye(4)[:3], 2e-3, y["depth"][2], y["depth"][1] * DEPTH_SCALE,
                         y["tri"], 1, y["bin"], 1)
    return dict(cfg=cfg, p=p, und=und, frames=frames, valid=rectify.validity(und.map_xy, und.map_a, RAW_ROWS, RAW_COLS))


def inside_border(rows, cols, border=BORDER):
    m = np.zeros((rows, cols), bool)
    m[border:rows - border, border:cols - border] = True
    return m


def near_invalid(xy, valid, reach=3):
    """Which keypoints (x, y) lie within `reach` pixels (Chebyshev) of an invalid pixel."""
    grown = ~mask.erode(valid, reach)
    xy = np.asarray(xy).astype(np.int64).reshape(-1, 2)
    return grown[xy[:, 1], xy[:, 0]]


# ---- the wide stereo rig -------------------------------------------------------------------------------------------------------------
def wide_rig(scene, rows, cols, f_scale=STEREO_F_SCALE):
    """test_rectify_gpu's raw 380 x 500 rig rectified to rows x cols with both P matrices' f scaled: rectify.Rectification."""
    import test_rectify_gpu as tr
    cams, Q, R, T = tr.raw_rig(scene)
    R1, R2, P1, P2 = rectify.stereo_rectify(cams[0], cams[1], R, T)
    P1, P2 = P1.copy(), P2.copy()
    for P in (P1, P2):
        P[0, 0] *= f_scale; P[1, 1] *= f_scale; P[0, 3] *= f_scale
        P[0, 2] += (cols - cams[0].cols) / 2.0; P[1, 2] += (rows - cams[0].rows) / 2.0
    return rectify.Rectification(cams[0], cams[1], R1, R2, P1, P2, rows, cols), cams, Q


PINCUSHION = (0.25, 0.02)           # k1, k2 of the pincushion rig: the rectified image sees more than the raw one at the raw size and f


def pincushion_rig(scene):
    """test_rectify_gpu's raw rig (its K, tangential terms and rotations) with a pincushion lens at the scene's size:
    (cams, Q, R, T), what test_rectify_gpu.write_asl and warp_to_raw take."""
    import test_rectify_gpu as tr
    rows, cols = int(scene.rows), int(scene.cols)
    cams = [rectify.CameraModel(c["K"], [PINCUSHION[0], PINCUSHION[1], c["dist"][2], c["dist"][3]], rows, cols) for c in (tr.RAW_LEFT, tr.RAW_RIGHT)]
    Q = [rectify.rodrigues(np.radians(q)) for q in (tr.Q_LEFT, tr.Q_RIGHT)]
    return cams, Q, Q[1] @ Q[0].T, -Q[1] @ np.array([scene.baseline_m, 0.0, 0.0])


def raw_sampler(scene, cams, Q):
    """test_rectify_gpu.warp_to_raw with the raw pixels' source coordinates computed once: f(images) -> the raw pair."""
    import test_rectify_gpu as tr
    rows, cols = int(scene.rows), int(scene.cols)
    vv, uu = np.mgrid[0:rows, 0:cols].astype(np.float64)
    at = []
    for cam, Qk in zip(cams, Q):
        xy = cam.undistort_normalized(np.stack([uu.ravel(), vv.ravel()], 1))
        X = Qk.T @ np.concatenate([xy, np.ones((len(xy), 1))], 1).T
        at.append(((scene.fx * X[0] / X[2] + scene.cx).reshape(rows, cols), (scene.fy * X[1] / X[2] + scene.cy).reshape(rows, cols)))
    return lambda images: tuple(tr._bilinear(img, u, v) for img, (u, v) in zip(images, at))


@functools.lru_cache(maxsize=None)
def stereo_world(n=12):
    """dict(cfg, rig, frames [raw pairs], valid [left, right]): test_rectify_gpu's 380 x 500 scene seen through the pincushion rig, the
    configuration that of the rectified camera.  Rendered once per process."""
    import test_rectify_gpu as tr
    from _oracle import Oracle
    o = Oracle()
    try:
        scene, cfg = tr._scene_and_config(o)
        cams, Q, R, T = pincushion_rig(scene)
        rig = rectify.rectification(cams[0], cams[1], R, T)
        cfg = rectify.apply_to_config(cfg.copy(), rig)
        to_raw = raw_sampler(scene, cams, Q)
        frames = [to_raw(o.render(scene, k)) for k in range(n)]
    finally:
        o.destroy()
    valid = [rectify.validity(rig.map_xy_left, rig.map_a_left, rig.raw_rows, rig.raw_cols),
             rectify.validity(rig.map_xy_right, rig.map_a_right, rig.raw_rows, rig.raw_cols)]
    return dict(cfg=cfg, rig=rig, frames=frames, valid=valid)


# ---- moving frame masks ------------------------------------------------------------------------------------------------------------
def moving_rect(rows, cols, k, stream=0):
    """A rectangle of a third of the width by two thirds of the height that moves with the frame and differs per sequence; 0 inside, 200
    (keep) outside.  Its left edge is never a multiple of 64 for long: it shares words with kept pixels.  Frame 0 starts at 9/20 of the
    width, where it removes 18 .. 38 % of the keypoints of every scene the cases use (from the image's first quarter: 8 % on one)."""
    m = np.full((rows, cols), 200, np.uint8)
    w, h = cols // 3, (2 * rows) // 3
    x0 = (41 * k + 97 * stream + (9 * cols) // 20) % (cols - w)
    y0 = (7 * k + 13 * stream + rows // 10) % (rows - h)
    m[y0:y0 + h, x0:x0 + w] = 0
    return m
