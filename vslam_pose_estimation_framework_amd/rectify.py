"""Rectification of a raw, calibrated stereo rig (numpy, fp64): camera model, Bouguet's rectification, fixed-point remap maps.

The product path is `k_rectify` (csrc/kernels_rectify.h) behind `vslam_set_rectification`; this module builds what it consumes:

- `CameraModel`: pinhole + radial-tangential distortion `k1 k2 p1 p2 [k3]` (EuRoC's `sensor.yaml`, KITTI raw's calibration).
- `stereo_rectify`: Bouguet's method as cv::stereoRectify does it with CALIB_ZERO_DISPARITY, alpha = -1 and the raw size [recalled].
  The focal length of the rectified pair is the mean of the two fy; OpenCV parity is not pinned, the tests pin the geometry.
- `undistort_rectify_maps`: per rectified pixel, the raw source coordinate in the fixed-point CV_16SC2 + CV_16UC1 format
  (initUndistortRectifyMap / convertMaps [recalled]).
- `remap_u8`: a numpy restatement of the kernel's arithmetic, the tests' checker (not a product path).
- `Rectification` / `rectification()`: everything a context needs; `apply_to_config` sets the rectified camera.
- `Undistortion` / `undistortion()`: the one-camera case of the RGB-D tracker (`vslam_rgbd_set_undistortion`): one map pair for the image
  and the depth image registered to it; `remap_nearest_u16` restates the depth kernel (`k_undistort_depth`, csrc/kernels_undistort.h).
"""
import numpy as np

MODELS = ("radial-tangential", "radtan", "plumb_bob")


def rodrigues(v):
    """Rotation vector <-> rotation matrix (cv::Rodrigues): a 3-vector gives a 3x3 matrix, a 3x3 matrix its 3-vector."""
    v = np.asarray(v, np.float64)
    if v.shape == (3, 3):
        R = v
        c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
        th = np.arccos(c)
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        s = np.sin(th)
        if th < 1e-12:
            return 0.5 * w
        if np.pi - th < 1e-6:            # near pi: the axis from the symmetric part
            A = (R + np.eye(3)) / 2.0
            axis = np.sqrt(np.maximum(np.diag(A), 0.0))
            i = int(np.argmax(axis))
            axis = A[:, i] / np.sqrt(A[i, i])
            if np.dot(axis, w) < 0:
                axis = -axis
            return th * axis / np.linalg.norm(axis)
        return th / (2.0 * s) * w
    v = v.reshape(3)
    th = np.linalg.norm(v)
    if th < 1e-300:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


class CameraModel(object):
    """One raw camera: K (3x3), radial-tangential distortion (k1, k2, p1, p2[, k3]), image size rows x cols."""

    def __init__(self, K, dist, rows, cols, model="radial-tangential"):
        if model not in MODELS:
            raise ValueError("CameraModel: distortion model %r is not supported (only radial-tangential k1 k2 p1 p2 [k3]; "
                             "fisheye / equidistant cameras are out of scope)" % (model,))
        d = np.asarray(dist, np.float64).reshape(-1)
        if d.size not in (4, 5):
            raise ValueError("CameraModel: radial-tangential distortion takes 4 or 5 coefficients (k1 k2 p1 p2 [k3]), got %d" % d.size)
        self.K = np.asarray(K, np.float64).reshape(3, 3).copy()
        self.dist = np.concatenate([d, np.zeros(5 - d.size)])
        self.rows, self.cols = int(rows), int(cols)

    def distort(self, x, y):
        """Normalised undistorted -> normalised distorted coordinates."""
        k1, k2, p1, p2, k3 = self.dist
        r2 = x * x + y * y
        radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        return (x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x),
                y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)

    def project(self, X):
        """Camera-frame points (n x 3) -> raw pixel coordinates (n x 2)."""
        X = np.asarray(X, np.float64).reshape(-1, 3)
        xd, yd = self.distort(X[:, 0] / X[:, 2], X[:, 1] / X[:, 2])
        K = self.K
        return np.stack([K[0, 0] * xd + K[0, 1] * yd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)

    def undistort_normalized(self, uv, iterations=30):
        """Raw pixel coordinates (n x 2) -> normalised undistorted coordinates (n x 2): fixed-point start, then Newton."""
        uv = np.asarray(uv, np.float64).reshape(-1, 2)
        K = self.K
        yd = (uv[:, 1] - K[1, 2]) / K[1, 1]
        xd = (uv[:, 0] - K[0, 2] - K[0, 1] * yd) / K[0, 0]
        k1, k2, p1, p2, k3 = self.dist
        x, y = xd.copy(), yd.copy()
        for _ in range(5):                        # cv::undistortPoints' iteration as the starting point
            r2 = x * x + y * y
            icdist = 1.0 / (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3)))
            dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
            x, y = (xd - dx) * icdist, (yd - dy) * icdist
        for _ in range(iterations):
            fx, fy = self.distort(x, y)
            ex, ey = fx - xd, fy - yd
            r2 = x * x + y * y
            radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            drad = k1 + r2 * (2.0 * k2 + 3.0 * k3 * r2)
            a = radial + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
            b = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
            c = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
            d = radial + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
            det = a * d - b * c
            sx, sy = (d * ex - b * ey) / det, (a * ey - c * ex) / det
            x, y = x - sx, y - sy
            if max(np.abs(sx).max(initial=0.0), np.abs(sy).max(initial=0.0)) < 1e-15:
                break
        return np.stack([x, y], axis=1)


def stereo_rectify(left, right, R, T):
    """Bouguet's rectification of a rig whose right camera sees X1 = R X0 + T (X0: left camera frame).

    Returns (R1, R2, P1, P2): R_k rotates camera k's frame into its rectified frame, P_k (3x4) projects rectified coordinates;
    both share one K, P2[0, 3] = f * (R2 T)_x (= -f B for a right camera at +x).  cv::stereoRectify with CALIB_ZERO_DISPARITY,
    alpha = -1 and the raw size, except that f = (fy_left + fy_right) / 2 [recalled]."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    T = np.asarray(T, np.float64).reshape(3)
    r = rodrigues(-0.5 * rodrigues(R))           # half of the rotation on each side
    t = r @ T
    idx = 0 if abs(t[0]) > abs(t[1]) else 1      # horizontal rig: rotate t onto +-x
    uu = np.zeros(3)
    uu[idx] = 1.0 if t[idx] > 0 else -1.0
    ww = np.cross(t, uu)
    nw = np.linalg.norm(ww)
    if nw > 0:
        ww *= np.arccos(min(1.0, abs(t[idx]) / np.linalg.norm(t))) / nw
    wR = rodrigues(ww)
    R1 = wR @ r.T
    R2 = wR @ r
    t2 = R2 @ T
    f = 0.5 * (left.K[1, 1] + right.K[1, 1])
    cc = np.zeros((2, 2))
    for k, (cam, Rk) in enumerate(((left, R1), (right, R2))):
        nx, ny = cam.cols, cam.rows
        corners = np.array([[0, 0], [nx - 1, 0], [0, ny - 1], [nx - 1, ny - 1]], np.float64)
        xy = cam.undistort_normalized(corners)
        X = (Rk @ np.concatenate([xy, np.ones((4, 1))], axis=1).T).T
        p = f * X[:, :2] / X[:, 2:3]
        cc[k] = ((nx - 1) / 2.0 - p[:, 0].mean(), (ny - 1) / 2.0 - p[:, 1].mean())
    cx, cy = cc.mean(axis=0)                     # CALIB_ZERO_DISPARITY: one principal point for both
    P1 = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0]], np.float64)
    P2 = P1.copy()
    P2[idx, 3] = f * t2[idx]
    return R1, R2, P1, P2


def encode_map(u, v):
    """fp64 source coordinates -> (map_xy int16 [..., 2], map_a uint16): ix = rint(32 u) (half to even), map_xy = (ix >> 5, iy >> 5)
    saturated to int16, map_a = (iy & 31) * 32 + (ix & 31)."""
    u = np.asarray(u, np.float64)
    v = np.asarray(v, np.float64)
    big = float(1 << 40)
    ix = np.rint(np.clip(np.nan_to_num(u * 32.0, nan=-big), -big, big)).astype(np.int64)
    iy = np.rint(np.clip(np.nan_to_num(v * 32.0, nan=-big), -big, big)).astype(np.int64)
    xy = np.stack([np.clip(ix >> 5, -32768, 32767), np.clip(iy >> 5, -32768, 32767)], axis=-1).astype(np.int16)
    a = ((iy & 31) * 32 + (ix & 31)).astype(np.uint16)
    return xy, a


def source_coordinates(cam, Rk, Pk, rows, cols):
    """fp64 raw coordinates (u, v) of every rectified pixel (rows x cols each): back-project through P_k, rotate back by R_k^T,
    distort, apply K."""
    P = np.asarray(Pk, np.float64).reshape(3, 4)[:, :3]
    Rk = np.asarray(Rk, np.float64).reshape(3, 3)
    vv, uu = np.mgrid[0:rows, 0:cols].astype(np.float64)
    rays = np.stack([uu.ravel(), vv.ravel(), np.ones(rows * cols)], axis=0)
    X = Rk.T @ (np.linalg.inv(P) @ rays)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(X[2] > 0, X[2], np.nan)     # behind the camera: no source (encoded far outside, read as 0)
        xd, yd = cam.distort(X[0] / z, X[1] / z)
    K = cam.K
    u = K[0, 0] * xd + K[0, 1] * yd + K[0, 2]
    v = K[1, 1] * yd + K[1, 2]
    return u.reshape(rows, cols), v.reshape(rows, cols)


def undistort_rectify_maps(cam, Rk, Pk, rows, cols):
    """initUndistortRectifyMap(K, dist, R_k, P_k, (cols, rows), CV_16SC2): (map_xy int16 [rows][cols][2], map_a uint16 [rows][cols])."""
    u, v = source_coordinates(cam, Rk, Pk, rows, cols)
    return encode_map(u, v)


def remap_u8(src, map_xy, map_a):
    """cv::remap(src, map_xy, map_a, INTER_LINEAR, BORDER_CONSTANT, 0) on 8-bit single-channel images, as the kernel computes it:
    w00 = (32-ax)(32-ay)*32, w01 = ax(32-ay)*32, w10 = (32-ax)ay*32, w11 = ax*ay*32, taps outside the image are 0,
    out = (sum w*p + 16384) >> 15.  The tests' checker."""
    src = np.asarray(src, np.uint8)
    H, W = src.shape
    x0 = map_xy[..., 0].astype(np.int64)
    y0 = map_xy[..., 1].astype(np.int64)
    a = np.asarray(map_a).astype(np.int64)
    ax, ay = a & 31, (a >> 5) & 31

    def tap(y, x):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(inside, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64), 0)
    s = ((32 - ax) * (32 - ay) * 32 * tap(y0, x0) + ax * (32 - ay) * 32 * tap(y0, x0 + 1) +
         (32 - ax) * ay * 32 * tap(y0 + 1, x0) + ax * ay * 32 * tap(y0 + 1, x0 + 1))
    return ((s + 16384) >> 15).astype(np.uint8)


def validity(map_xy, map_a, raw_rows, raw_cols):
    """bool [rows, cols]: the output pixels whose every tap of non-zero weight lies inside the raw image (integers, the rule above
    vslam_set_rectification_mask): x0 >= 0, x0 + (ax > 0) <= raw_cols - 1, y0 >= 0, y0 + (ay > 0) <= raw_rows - 1.  remap_u8 fills the
    other pixels' missing taps with 0.  The restatement of k_map_valid's bit; packed and eroded by mask.pack_bool / mask.erode."""
    x0 = np.asarray(map_xy)[..., 0].astype(np.int64)
    y0 = np.asarray(map_xy)[..., 1].astype(np.int64)
    a = np.asarray(map_a).astype(np.int64)
    ax, ay = a & 31, (a >> 5) & 31
    return (x0 >= 0) & (x0 + (ax > 0) <= int(raw_cols) - 1) & (y0 >= 0) & (y0 + (ay > 0) <= int(raw_rows) - 1)


def remap_nearest_u16(src, map_xy, map_a):
    """The depth kernel's arithmetic on 16-bit single-channel images: the nearest raw pixel of the 1/32-px source coordinate, ties up
    (this repository's own rule; depth is not interpolated): x = x0 + (ax >> 4), y = y0 + (ay >> 4), out = src[y][x] inside the raw image,
    else 0 (depth 0 = no measurement).  The tests' checker."""
    src = np.asarray(src, np.uint16)
    H, W = src.shape
    a = np.asarray(map_a).astype(np.int64)
    x = map_xy[..., 0].astype(np.int64) + ((a & 31) >> 4)
    y = map_xy[..., 1].astype(np.int64) + (((a >> 5) & 31) >> 4)
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return np.where(inside, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0).astype(np.uint16)


class Rectification(object):
    """A raw rig made rectifiable: both cameras, (R1, R2, P1, P2) and the fixed-point maps at the rectified size rows x cols."""

    def __init__(self, left, right, R1, R2, P1, P2, rows=None, cols=None):
        if (left.rows, left.cols) != (right.rows, right.cols):
            raise ValueError("Rectification: both raw cameras must have the same image size")
        self.left, self.right = left, right
        self.R1, self.R2 = np.asarray(R1, np.float64), np.asarray(R2, np.float64)
        self.P1, self.P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
        self.raw_rows, self.raw_cols = left.rows, left.cols
        self.rows = int(rows) if rows else left.rows
        self.cols = int(cols) if cols else left.cols
        self.map_xy_left, self.map_a_left = undistort_rectify_maps(left, self.R1, self.P1, self.rows, self.cols)
        self.map_xy_right, self.map_a_right = undistort_rectify_maps(right, self.R2, self.P2, self.rows, self.cols)

    @property
    def K(self):
        return self.P1[:, :3].copy()

    def rectify(self, left_raw, right_raw):
        """The rectified pair in numpy (remap_u8 of both sides): the checker of the device path."""
        return remap_u8(left_raw, self.map_xy_left, self.map_a_left), remap_u8(right_raw, self.map_xy_right, self.map_a_right)


def rectification(left, right, R, T, rows=None, cols=None):
    """stereo_rectify + both maps (rectified size = raw size unless rows / cols are given)."""
    R1, R2, P1, P2 = stereo_rectify(left, right, R, T)
    return Rectification(left, right, R1, R2, P1, P2, rows, cols)


class Undistortion(object):
    """One raw camera made undistortable: the camera, the output camera K and the fixed-point maps at the output size rows x cols
    (default: the raw size and the raw camera's own K)."""

    def __init__(self, cam, K_new=None, rows=None, cols=None):
        self.cam = cam
        self.K = (cam.K if K_new is None else np.asarray(K_new, np.float64).reshape(3, 3)).copy()
        self.raw_rows, self.raw_cols = cam.rows, cam.cols
        self.rows = int(rows) if rows else cam.rows
        self.cols = int(cols) if cols else cam.cols
        P = np.concatenate([self.K, np.zeros((3, 1))], axis=1)
        self.map_xy, self.map_a = undistort_rectify_maps(cam, np.eye(3), P, self.rows, self.cols)

    def apply(self, image, depth):
        """The undistorted frame in numpy (remap_u8 of the image, remap_nearest_u16 of the depth image registered to it): the checker
        of the device path."""
        return remap_u8(image, self.map_xy, self.map_a), remap_nearest_u16(depth, self.map_xy, self.map_a)


def undistortion(cam, K_new=None, rows=None, cols=None):
    """The maps that undo cam's lens distortion: output camera K_new (default cam.K) at rows x cols (default the raw size)."""
    return Undistortion(cam, K_new, rows, cols)


def apply_to_config(cfg, rect):
    """The rectified camera into a vslam_config: rows, cols, K = P1[:, :3], baseline_h = (P2[0, 3], 0, 0)."""
    cfg.rows, cfg.cols = int(rect.rows), int(rect.cols)
    K = rect.P1[:, :3].reshape(9)
    for i in range(9):
        cfg.K[i] = float(K[i])
    cfg.baseline_h[0] = float(rect.P2[0, 3])
    cfg.baseline_h[1] = 0.0
    cfg.baseline_h[2] = 0.0
    return cfg
