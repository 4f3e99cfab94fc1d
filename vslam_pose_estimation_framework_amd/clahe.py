"""cv::createCLAHE(clipLimit, Size(tilesX, tilesY))->apply on one 8-bit image, restated in numpy [recalled, like the project's other
OpenCV semantics].  Every float operation is one IEEE single operation.

    extension   if cols % tilesX == 0 and rows % tilesY == 0 the image is used as it is; otherwise it grows at the bottom by
                tilesY - rows % tilesY rows AND at the right by tilesX - cols % tilesX columns, BORDER_REFLECT_101 (index i >= n reads
                2 (n - 1) - i) — so a dimension that divides still gets a full tilesY (tilesX) extra lines when the other one does not.
                tw = ext_cols / tilesX, th = ext_rows / tilesY, area = tw * th
    clip        clipLimit > 0 ? max(int(clipLimit * area / 256), 1) : 0          (double arithmetic, truncation)
    per tile    h[256] = counts; with clip > 0: clipped = sum of h[k] - clip over the bins above clip, those bins set to clip,
                batch = clipped / 256, residual = clipped - 256 * batch, every bin += batch, and with step = max(256 / residual, 1)
                bin k gets one more exactly when k % step == 0 and k / step < residual
    table       lut[k] = clamp(rint(float(h[0] + .. + h[k]) * (float(255) / float(area))), 0, 255), ties to even
    per pixel   txf = float(x) * (1.f / float(tw)) - 0.5f, tx1 = floor(txf), tx2 = tx1 + 1, xa = txf - float(tx1), xa1 = 1.f - xa, then
                tx1 = max(tx1, 0), tx2 = min(tx2, tilesX - 1); the same in y;
                res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya
                dst = clamp(rint(res), 0, 255)

The reference of the tests of the device path (kernels_clahe.h: vslam_set_clahe, vslam_clahe_u8) and a host fallback for callers without a
device."""
import math

import numpy as np

MAX_PIXELS = 1 << 24      # the counts stay exact in float32
MAX_TILES = 32            # VS_CLAHE_MAX_TILES

_F = np.float32


def check_arguments(rows, cols, clip_limit, tiles_x, tiles_y):
    """ValueError for what the device entries refuse with VSLAM_ERR_INVALID."""
    if not (1 <= tiles_x <= MAX_TILES and 1 <= tiles_y <= MAX_TILES):
        raise ValueError("clahe: tiles outside 1 .. %d" % MAX_TILES)
    if cols <= tiles_x or rows <= tiles_y:
        raise ValueError("clahe: the image must be larger than the tile grid (the reflected border would leave it)")
    if rows * cols > MAX_PIXELS:
        raise ValueError("clahe: more than 2^24 pixels")
    if not math.isfinite(clip_limit):
        raise ValueError("clahe: clip_limit is not finite")


def extended_size(rows, cols, tiles_x, tiles_y):
    """(ext_rows, ext_cols) of the image the tiles are cut from."""
    if cols % tiles_x == 0 and rows % tiles_y == 0:
        return rows, cols
    return rows + tiles_y - rows % tiles_y, cols + tiles_x - cols % tiles_x


def extend(image, tiles_x, tiles_y):
    rows, cols = image.shape
    er, ec = extended_size(rows, cols, tiles_x, tiles_y)
    ri, ci = np.arange(er), np.arange(ec)
    ri = np.where(ri >= rows, 2 * (rows - 1) - ri, ri)
    ci = np.where(ci >= cols, 2 * (cols - 1) - ci, ci)
    return image[np.ix_(ri, ci)]


def clip_count(clip_limit, area):
    """The integer clip the kernels receive (0: no clipping).  No bin holds more than `area`, so the value is capped there."""
    if not clip_limit > 0:
        return 0
    return int(max(min(float(clip_limit) * area / 256.0, float(area)), 1.0))


def redistribute(hist, clip):
    """hist [..., 256] int64 -> the clipped counts with the excess spread (closed form of the reference's loop)."""
    h = np.asarray(hist, np.int64)
    if clip <= 0:
        return h.copy()
    clipped = np.maximum(h - clip, 0).sum(axis=-1, keepdims=True)
    h = np.minimum(h, clip)
    batch = clipped // 256
    residual = clipped - 256 * batch
    step = np.maximum(256 // np.maximum(residual, 1), 1)
    k = np.arange(256)
    return h + batch + ((k % step == 0) & (k // step < residual))


def clahe_luts(image, clip_limit, tiles_x, tiles_y):
    """uint8 [tilesY, tilesX, 256]: the table of every tile of the extended image."""
    ext = extend(image, tiles_x, tiles_y)
    th, tw = ext.shape[0] // tiles_y, ext.shape[1] // tiles_x
    area = tw * th
    tile = (np.arange(ext.shape[0]) // th)[:, None] * tiles_x + (np.arange(ext.shape[1]) // tw)[None, :]
    hist = np.bincount((tile * 256 + ext).ravel(), minlength=tiles_x * tiles_y * 256).reshape(tiles_y, tiles_x, 256)
    h = redistribute(hist, clip_count(clip_limit, area))
    scale = _F(255) / _F(area)
    lut = np.rint(np.cumsum(h, axis=-1).astype(_F) * scale)
    return np.clip(lut, 0, 255).astype(np.uint8)


def _axis(n, tile, tiles):
    """Per index of one axis: the two tile indices and the two weights."""
    inv = _F(1) / _F(tile)
    f = np.arange(n).astype(_F) * inv - _F(0.5)
    t1 = np.floor(f)
    a = f - t1
    a1 = _F(1) - a
    t1 = t1.astype(np.int64)
    return np.maximum(t1, 0), np.minimum(t1 + 1, tiles - 1), a, a1


def interpolate(image, luts):
    """float32 [rows, cols]: the bilinear blend of the four tables around every pixel, before rounding."""
    rows, cols = image.shape
    tiles_y, tiles_x = luts.shape[:2]
    er, ec = extended_size(rows, cols, tiles_x, tiles_y)
    ty1, ty2, ya, ya1 = (q[:, None] for q in _axis(rows, er // tiles_y, tiles_y))
    tx1, tx2, xa, xa1 = (q[None, :] for q in _axis(cols, ec // tiles_x, tiles_x))
    t = luts.astype(_F)
    top = t[ty1, tx1, image] * xa1 + t[ty1, tx2, image] * xa
    bottom = t[ty2, tx1, image] * xa1 + t[ty2, tx2, image] * xa
    res = top * ya1 + bottom * ya
    assert res.dtype == _F
    return res


def clahe_u8(image, clip_limit=40.0, tiles=(8, 8)):
    """image: 2-D uint8 -> (out, luts): the processed image and the tables, uint8 [tilesY, tilesX, 256].  tiles = (tilesX, tilesY)."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("clahe_u8: a 2-D uint8 image is required")
    tiles_x, tiles_y = int(tiles[0]), int(tiles[1])
    check_arguments(img.shape[0], img.shape[1], float(clip_limit), tiles_x, tiles_y)
    luts = clahe_luts(img, float(clip_limit), tiles_x, tiles_y)
    out = np.clip(np.rint(interpolate(img, luts)), 0, 255).astype(np.uint8)
    return out, luts
