"""cv::equalizeHist on one 8-bit image, restated in numpy [recalled, like the project's other OpenCV semantics].

    h[256]  = counts of the pixels
    i0      = the first v with h[v] != 0
    if h[i0] == rows*cols: output = input                      (a constant image stays as it is)
    scale   = float32(255) / float32(rows*cols - h[i0])        one correctly rounded single-precision division
    sum_v   = h[i0+1] + ... + h[v]                             (integers)
    lut[v]  = 0 for v <= i0, else min(255, rint(float32(sum_v) * scale))    one single-precision multiply, ties to even
    out     = lut[in]

The reference of the tests of the device path (kernels_equalize.h: vslam_set_equalization, vslam_rgbd_set_equalization,
vslam_equalize_hist_u8) and a host fallback for callers without a device."""
import numpy as np

MAX_PIXELS = 1 << 24      # the counts stay exact in float32


def equalize_lut(hist):
    """The 256-entry look-up table of a 256-bin count (identity for a constant image)."""
    h = np.asarray(hist, np.int64)
    assert h.shape == (256,)
    total = int(h.sum())
    nz = np.flatnonzero(h)
    if len(nz) == 0 or int(h[nz[0]]) == total:
        return np.arange(256, dtype=np.uint8)
    i0 = int(nz[0])
    scale = np.float32(255) / np.float32(total - int(h[i0]))
    sums = np.cumsum(h) - int(h[i0])
    lut = np.minimum(255, np.rint(sums.astype(np.float32) * scale)).astype(np.int64)
    lut[:i0 + 1] = 0
    return lut.astype(np.uint8)


def equalize_hist_u8(image):
    """image: 2-D uint8 -> (out, hist, lut): the equalised image, the 256 counts (uint32) and the table."""
    img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("equalize_hist_u8: a 2-D uint8 image is required")
    if img.size > MAX_PIXELS:
        raise ValueError("equalize_hist_u8: more than 2^24 pixels")
    hist = np.bincount(img.ravel(), minlength=256).astype(np.uint32)
    lut = equalize_lut(hist)
    return lut[img], hist, lut
