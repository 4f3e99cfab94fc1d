"""Detection masks, restated in numpy: the semantics of cv::Feature2D::detect(image, keypoints, mask) [recalled, like the project's other
OpenCV semantics] as the device path implements them (kernels_mask.h: vslam_set_detection_mask, vslam_set_frame_masks,
vslam_mask_pack_u8).

    mask     an 8-bit single-channel image at the processed size (rows x cols of the context: the rectified / undistorted image's
             coordinates when those stages are on); non-zero = keep, zero removes every keypoint on that pixel
    margin   m, a whole number 0 .. 64: the keep-mask is eroded by the (2m+1) x (2m+1) square — a pixel stays kept only if every pixel
             within Chebyshev distance m is kept.  Pixels outside the image count as kept (an all-keep mask stays all-keep; the image
             border is the descriptor border filter's business)
    packed   words_per_row = (cols + 63) // 64 little-endian 64-bit words per row, bit b of word t = column 64 t + b, bits beyond cols 0

The detector and its non-maximum suppression run on the whole image; the mask only filters the keypoints afterwards, ahead of the count
the threshold controller sees.  A context holds a static mask (all streams) and a frame mask (per stream, next frame only) per image side;
the effective keep-mask is their AND, each eroded by its own margin, a missing one all-keep (effective())."""
import numpy as np

MAX_MARGIN = 64


def words_per_row(cols):
    return (int(cols) + 63) // 64


def _margin(margin):
    m = int(margin)
    if m != margin or m < 0 or m > MAX_MARGIN:
        raise ValueError("mask: margin must be a whole number in 0 .. %d" % MAX_MARGIN)
    return m


def erode(keep_bool, margin):
    """keep_bool: 2-D bool -> 2-D bool, eroded by the (2 margin + 1)^2 square; outside the image counts as kept."""
    keep = np.asarray(keep_bool)
    if keep.ndim != 2:
        raise ValueError("mask.erode: a 2-D array is required")
    keep = keep.astype(bool)
    m = _margin(margin)
    if m == 0 or keep.size == 0:
        return keep.copy()
    rows, cols = keep.shape
    # zeros within distance m along a row, then along a column: prefix sums of the removed pixels over the clipped windows
    removed = (~keep).astype(np.int64)
    ps = np.concatenate([np.zeros((rows, 1), np.int64), np.cumsum(removed, axis=1)], axis=1)
    lo = np.clip(np.arange(cols) - m, 0, cols)
    hi = np.clip(np.arange(cols) + m + 1, 0, cols)
    hremoved = ((ps[:, hi] - ps[:, lo]) > 0).astype(np.int64)
    ps = np.concatenate([np.zeros((1, cols), np.int64), np.cumsum(hremoved, axis=0)], axis=0)
    lo = np.clip(np.arange(rows) - m, 0, rows)
    hi = np.clip(np.arange(rows) + m + 1, 0, rows)
    return (ps[hi, :] - ps[lo, :]) == 0


def pack_bool(keep_bool):
    """2-D bool -> uint64 [rows, words_per_row]."""
    keep = np.asarray(keep_bool).astype(bool)
    rows, cols = keep.shape
    tx = words_per_row(cols)
    padded = np.zeros((rows, tx * 64), np.uint8)
    padded[:, :cols] = keep
    by = np.packbits(padded.reshape(rows, tx, 8, 8), axis=3, bitorder="little").reshape(rows, tx, 8)
    return np.ascontiguousarray(by).view("<u8").reshape(rows, tx).astype(np.uint64)


def pack(mask_u8, margin=0):
    """mask_u8: 2-D uint8 (non-zero = keep) -> the eroded packed words, uint64 [rows, words_per_row]."""
    mk = np.asarray(mask_u8)
    if mk.dtype != np.uint8 or mk.ndim != 2:
        raise ValueError("mask.pack: a 2-D uint8 image is required")
    return pack_bool(erode(mk != 0, margin))


def unpack(words, cols):
    """uint64 [rows, words_per_row] -> 2-D bool [rows, cols]."""
    w = np.ascontiguousarray(np.asarray(words, np.uint64))
    if w.ndim != 2 or w.shape[1] != words_per_row(cols):
        raise ValueError("mask.unpack: words must be [rows, (cols + 63) // 64]")
    rows = w.shape[0]
    bits = np.unpackbits(w.astype("<u8").view(np.uint8).reshape(rows, -1), axis=1, bitorder="little")
    return bits[:, :cols].astype(bool)


def all_keep(rows, cols):
    return pack_bool(np.ones((rows, cols), bool))


def effective(rows, cols, static=None, frame=None):
    """The packed effective keep-mask of one image side: static / frame = (mask_u8, margin) or None (all-keep)."""
    w = all_keep(rows, cols)
    for one in (static, frame):
        if one is not None:
            mk, m = one
            if np.asarray(mk).shape != (rows, cols):
                raise ValueError("mask.effective: the mask is not %d x %d" % (rows, cols))
            w = w & pack(mk, m)
    return w


def filter_keypoints(xy, keep_bool):
    """xy: int [n, 2] (x, y) -> bool [n]: the keypoints whose pixel is kept (KeyPointsFilter::runByPixelsMask)."""
    p = np.asarray(xy).reshape(-1, 2).astype(np.int64)
    keep = np.asarray(keep_bool).astype(bool)
    return keep[p[:, 1], p[:, 0]]
