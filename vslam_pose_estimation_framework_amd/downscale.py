"""Integer-factor reduction of input frames: the project's own definition in numpy, and the calibration arithmetic that goes with it.

Factor f is 2, 3 or 4.  A full image of R x C gives R // f x C // f; the R % f bottom rows and C % f right columns are never read.
  8 bit:  out[y][x] = (sum of the f x f block at (f y, f x) + f f // 2) // (f f): round half up.  At f = 2 that is (a + b + c + d + 2) >> 2,
          which cv::resize(INTER_AREA) computes at an integer factor of 2 [recalled]; at 3 and 4 OpenCV goes through a float reciprocal and
          may differ on ties.  Parity with OpenCV is not pinned.
  depth:  never blended: the v non-zero values of the block in ascending order, out = the element at index (v - 1) // 2 (the lower
          median), 0 when v == 0.
Calibration: output pixel x covers full pixels f x .. f x + f - 1, whose centre is f x + (f - 1) / 2, so fx' = fx / f, fy' = fy / f,
cx' = (cx + 0.5) / f - 0.5, cy' likewise; a projection matrix's P[0][3] (-fx B) is divided by f; the baseline in metres, the distortion
coefficients and the depth scale are unchanged.

The reference of the tests of the device path (kernels_downscale.h: vslam_downscale_u8, vslam_downscale_depth_u16) and the tools'
calibration arithmetic."""
import numpy as np

FACTORS = (2, 3, 4)
MAX_SIZE = 32767


def _factor(f):
    if isinstance(f, bool) or int(f) != f or int(f) not in FACTORS:
        raise ValueError("downscale: factor %r outside 2 .. 4" % (f,))
    return int(f)


def output_size(full_rows, full_cols, f):
    """(rows, cols) of the reduced image; ValueError unless both full sizes lie in 1 .. 32767 and give at least 1 x 1."""
    f = _factor(f)
    full_rows, full_cols = int(full_rows), int(full_cols)
    if not (1 <= full_rows <= MAX_SIZE and 1 <= full_cols <= MAX_SIZE):
        raise ValueError("downscale: full size %d x %d outside 1 .. %d" % (full_rows, full_cols, MAX_SIZE))
    if full_rows // f < 1 or full_cols // f < 1:
        raise ValueError("downscale: %d x %d holds no %d x %d block" % (full_rows, full_cols, f, f))
    return full_rows // f, full_cols // f


def _blocks(image, f, dtype, name):
    """image [R, C] or [R, C, channels] -> its blocks as [R // f, f, C // f, f(, channels)]"""
    img = np.asarray(image)
    if img.dtype != dtype or img.ndim not in (2, 3):
        raise ValueError("%s: a %s array [rows, cols] or [rows, cols, channels] is required" % (name, np.dtype(dtype).name))
    rows, cols = output_size(img.shape[0], img.shape[1], f)
    return img[:rows * f, :cols * f].reshape((rows, f, cols, f) + img.shape[2:])


def downscale_u8(image, f):
    """uint8 [R, C] (or [R, C, channels], per plane) -> uint8 [R // f, C // f(, channels)]: the rounded block average."""
    f = _factor(f)
    b = _blocks(image, f, np.uint8, "downscale_u8")
    s = b.astype(np.uint32).sum(axis=(1, 3))
    return ((s + (f * f) // 2) // (f * f)).astype(np.uint8)


def downscale_depth_u16(depth, f):
    """uint16 [R, C] -> uint16 [R // f, C // f]: the lower median of each block's non-zero values, 0 where there is none."""
    f = _factor(f)
    d = np.asarray(depth)
    if d.ndim != 2:
        raise ValueError("downscale_depth_u16: a uint16 array [rows, cols] is required")
    b = _blocks(d, f, np.uint16, "downscale_depth_u16")
    rows, cols = b.shape[0], b.shape[2]
    v = b.transpose(0, 2, 1, 3).reshape(rows, cols, f * f).astype(np.uint32)
    valid = (v != 0).sum(axis=2)
    v = np.sort(np.where(v == 0, np.uint32(65536), v), axis=2)            # the holes behind every value
    k = np.maximum(valid - 1, 0) // 2
    out = np.take_along_axis(v, k[:, :, None], axis=2)[:, :, 0]
    return np.where(valid > 0, out, 0).astype(np.uint16)


def scale_intrinsics(K, f):
    """The camera matrix of the reduced image: float64 [3, 3]."""
    f = _factor(f)
    K = np.array(K, np.float64).reshape(3, 3)
    out = K.copy()
    out[0, 0] = K[0, 0] / f
    out[1, 1] = K[1, 1] / f
    out[0, 1] = K[0, 1] / f
    out[0, 2] = (K[0, 2] + 0.5) / f - 0.5
    out[1, 2] = (K[1, 2] + 0.5) / f - 0.5
    return out


def scale_projection(P, f):
    """A 3 x 4 projection matrix [K | (-fx B, 0, 0)] of the reduced image: K as scale_intrinsics, P[0][3] divided by f."""
    f = _factor(f)
    P = np.array(P, np.float64).reshape(3, 4)
    out = P.copy()
    out[:, :3] = scale_intrinsics(P[:, :3], f)
    out[0, 3] = P[0, 3] / f
    return out


def apply_to_config(cfg, f):
    """A vslam_config written for the full image -> the reduced image's, in place: rows, cols, K and baseline_h[0] (-fx B, pixels times
    metres).  Everything else (thresholds in pixels included) stays the caller's."""
    f = _factor(f)
    rows, cols = output_size(cfg.rows, cfg.cols, f)
    K = scale_intrinsics([cfg.K[i] for i in range(9)], f).reshape(9)
    cfg.rows, cfg.cols = rows, cols
    for i in range(9):
        cfg.K[i] = float(K[i])
    cfg.baseline_h[0] = cfg.baseline_h[0] / f
    return cfg
