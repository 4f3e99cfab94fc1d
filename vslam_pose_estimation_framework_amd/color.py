"""Interleaved 8-bit colour to grey, restated in numpy: the one definition of the project,

    gray = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14        all integer; alpha is ignored

[recalled: cvtColor on 8-bit images with 14 fractional bits, the OpenCV 3.x of the reference's image; io_formats.rgb_to_gray_opencv states
the same for RGB arrays].  Newer OpenCV uses 15 bits (9798 / 19235 / 3735): not built.

The reference of the tests of the device path (kernels_gray.h: vslam_set_color_input, vslam_rgbd_set_color_input, vslam_gray_u8) and a host
fallback for callers without a device.  sample_rgb is the definition of the landmark map's colours (kernels_map_color.h) and the reference of
their tests."""
import numpy as np

GRAY8, BGR8, RGB8, BGRA8, RGBA8 = 0, 1, 2, 3, 4      # VSLAM_PIXEL_* of include/vslam_hip.h
FORMATS = (BGR8, RGB8, BGRA8, RGBA8)
NAMES = {GRAY8: "gray8", BGR8: "bgr8", RGB8: "rgb8", BGRA8: "bgra8", RGBA8: "rgba8"}
CR, CG, CB, SHIFT = 4899, 9617, 1868, 14


def channels(fmt):
    """Bytes per pixel of a format."""
    if fmt == GRAY8:
        return 1
    if fmt in (BGR8, RGB8):
        return 3
    if fmt in (BGRA8, RGBA8):
        return 4
    raise ValueError("unknown pixel format %r" % (fmt,))


def to_gray_u8(image, fmt):
    """image: uint8 [..., channels(fmt)] (a GRAY8 image: [...], returned as it is) -> uint8 [...]."""
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError("to_gray_u8: a uint8 image is required")
    if fmt == GRAY8:
        return img
    ch = channels(fmt)
    if img.ndim < 1 or img.shape[-1] != ch:
        raise ValueError("to_gray_u8: %s needs %d channels, the array has shape %r" % (NAMES[fmt], ch, img.shape))
    v = img.astype(np.int32)
    r, b = (v[..., 0], v[..., 2]) if fmt in (RGB8, RGBA8) else (v[..., 2], v[..., 0])
    return ((r * CR + v[..., 1] * CG + b * CB + (1 << (SHIFT - 1))) >> SHIFT).astype(np.uint8)


def sample_rgb(image, fmt, xy, maps=None):
    """The colour of a landmark's pixel, the definition of the map colours (csrc/kernels_map_color.h: vslam_enable_map_colors,
    vslam_rgbd_enable_map_colors, vslam_sample_color_u8).  image: uint8 [rows, cols, channels(fmt)] in BGR8 / RGB8 / BGRA8 / RGBA8 (alpha is
    ignored); xy: [n, 2] pixels (x, y), integer, or float32 (an RGB-D point list), which is rounded with np.rint in float32 (half to even)
    and clamped to the pixel grid first.  Returns uint8 [n, 3], always in R, G, B order.

    maps=None: the pixel grid is the image; a pixel outside it gives (0, 0, 0).
    maps=(map_xy, map_a) in the format of rectify.undistort_rectify_maps: the pixel grid is the map's, the image is the raw one, and the
    result is rectify.remap_u8 of each colour plane at destination pixel (y, x): taps (y0, x0) .. (y0 + 1, x0 + 1), weights
    (32 - ax)(32 - ay) .. ax ay, (sum + 512) >> 10, taps outside the raw image count as 0; a pixel outside the map gives (0, 0, 0)."""
    img = np.asarray(image)
    if img.dtype != np.uint8:
        raise ValueError("sample_rgb: a uint8 image is required")
    if fmt not in FORMATS:
        raise ValueError("sample_rgb: a colour format (BGR8, RGB8, BGRA8, RGBA8) is required, got %r" % (fmt,))
    ch = channels(fmt)
    if img.ndim != 3 or img.shape[2] != ch:
        raise ValueError("sample_rgb: %s needs an image [rows, cols, %d], the array has shape %r" % (NAMES[fmt], ch, img.shape))
    p = np.asarray(xy)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("sample_rgb: xy must be [n, 2], got shape %r" % (p.shape,))
    if maps is not None:
        if len(maps) != 2 or maps[0] is None or maps[1] is None:
            raise ValueError("sample_rgb: maps is the pair (map_xy, map_a)")
        mxy, ma = np.asarray(maps[0]), np.asarray(maps[1])
        if mxy.ndim != 3 or mxy.shape[2] != 2 or ma.shape != mxy.shape[:2]:
            raise ValueError("sample_rgb: map_xy must be [rows, cols, 2] and map_a [rows, cols], got %r and %r" % (mxy.shape, ma.shape))
        if ma.size and int(ma.max()) >= 1024:
            raise ValueError("sample_rgb: interpolation table index >= 1024")
        grid = ma.shape
    else:
        grid = img.shape[:2]
    if p.dtype == np.float32:
        r = np.rint(p)                                    # float32, half to even
        x = np.clip(r[:, 0], 0, max(grid[1] - 1, 0)).astype(np.int64)
        y = np.clip(r[:, 1], 0, max(grid[0] - 1, 0)).astype(np.int64)
    elif np.issubdtype(p.dtype, np.integer):
        x, y = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
    else:
        raise ValueError("sample_rgb: xy must be integer or float32, got %s" % p.dtype)
    order = (0, 1, 2) if fmt in (RGB8, RGBA8) else (2, 1, 0)
    out = np.zeros((len(p), 3), np.uint8)
    inside = (x >= 0) & (x < grid[1]) & (y >= 0) & (y < grid[0])
    if not inside.any():
        return out
    xi, yi = x[inside], y[inside]
    if maps is None:
        out[inside] = img[yi, xi][:, order]
        return out
    H, W = img.shape[:2]
    x0 = mxy[yi, xi, 0].astype(np.int64)
    y0 = mxy[yi, xi, 1].astype(np.int64)
    a = ma[yi, xi].astype(np.int64)
    ax, ay = a & 31, (a >> 5) & 31

    def tap(ty, tx):
        ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        if H == 0 or W == 0:
            return np.zeros((len(tx), 3), np.int64)
        v = img[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)][:, order].astype(np.int64)
        return np.where(ok[:, None], v, 0)
    s = (((32 - ax) * (32 - ay))[:, None] * tap(y0, x0) + (ax * (32 - ay))[:, None] * tap(y0, x0 + 1) +
         ((32 - ax) * ay)[:, None] * tap(y0 + 1, x0) + (ax * ay)[:, None] * tap(y0 + 1, x0 + 1))
    out[inside] = ((s + 512) >> 10).astype(np.uint8)
    return out
