"""Smoothing of the 8-bit intensity image ahead of the equalisation slot and the detector (vslam_set_smoothing, csrc/kernels_smooth.h;
DESIGN.md 6p): the numpy restatement of the integer definition.  The tests' checker, not a product path.

Gaussian, ksize 3 / 5 / 7: taps K in 1/256 (TAPS), out = (sum_i sum_j K_i K_j p(y+i-r, x+j-r) + 32768) >> 16 in exact integers, the border
reflected without edge duplication (numpy's "reflect": index -1 -> 1); rows > r and cols > r.  The form of gaussian_blur7_ref in
tests/golden/make_golden.py.  cv::GaussianBlur(src, dst, Size(k, k), 0) on CV_8UC1 with BORDER_REFLECT_101 [recalled, not pinned].
Median, ksize 3 / 5: element k * k // 2 of the sorted k x k window, the border replicated; any size.  cv::medianBlur [recalled]."""
import numpy as np

OFF, GAUSSIAN, MEDIAN = 0, 1, 2
MODES = {"gaussian": GAUSSIAN, "median": MEDIAN}
DEFAULT_KSIZE = {GAUSSIAN: 5, MEDIAN: 3}
KSIZES = {GAUSSIAN: (3, 5, 7), MEDIAN: (3, 5)}
TAPS = {3: (64, 128, 64), 5: (16, 64, 96, 64, 16), 7: (8, 28, 56, 72, 56, 28, 8)}


def check(mode, ksize, rows, cols):
    """Raises ValueError for what vslam_set_smoothing / vslam_smooth_u8 refuse with VSLAM_ERR_INVALID."""
    if mode not in KSIZES:
        raise ValueError("smoothing: unknown mode %r" % (mode,))
    if ksize not in KSIZES[mode]:
        raise ValueError("smoothing: %s has ksize %s, not %r" % ("a Gaussian" if mode == GAUSSIAN else "a median", " / ".join(map(str, KSIZES[mode])), ksize))
    if rows < 1 or cols < 1:
        raise ValueError("smoothing: empty image")
    if mode == GAUSSIAN and (rows <= ksize // 2 or cols <= ksize // 2):
        raise ValueError("smoothing: a Gaussian of %d needs rows and cols above %d, not %d x %d" % (ksize, ksize // 2, rows, cols))


def _image(img):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 2:
        raise ValueError("smoothing: a 2-D uint8 image is required")
    return img


def gaussian_u8(img, ksize):
    img = _image(img)
    check(GAUSSIAN, ksize, *img.shape)
    r = ksize // 2
    k = TAPS[ksize]
    p = np.pad(img.astype(np.int64), r, mode="reflect")
    rows, cols = img.shape
    h = sum(k[j] * p[:, j:j + cols] for j in range(ksize))
    v = sum(k[i] * h[i:i + rows] for i in range(ksize))
    return ((v + 32768) >> 16).astype(np.uint8)


def median_u8(img, ksize):
    img = _image(img)
    check(MEDIAN, ksize, *img.shape)
    r = ksize // 2
    p = np.pad(img, r, mode="edge")
    rows, cols = img.shape
    win = np.stack([p[i:i + rows, j:j + cols] for i in range(ksize) for j in range(ksize)], axis=-1)
    return np.sort(win, axis=-1)[..., ksize * ksize // 2].copy()


def smooth_u8(img, mode, ksize):
    """mode OFF: the image itself."""
    if mode == OFF:
        return _image(img)
    if mode not in KSIZES:
        raise ValueError("smoothing: unknown mode %r" % (mode,))
    return gaussian_u8(img, ksize) if mode == GAUSSIAN else median_u8(img, ksize)


def argument(value, error=ValueError):
    """What the tools take for --smooth: None, "gaussian[:K]" / "median[:K]" or a (mode, ksize) pair -> None or (mode, ksize); anything
    else raises `error` with the reason."""
    if value is None:
        return None
    try:
        if isinstance(value, str):
            return parse(value)
        mode, ksize = value
        if mode not in KSIZES or ksize not in KSIZES[mode]:
            raise ValueError("--smooth: no mode %r with ksize %r" % (mode, ksize))
        return int(mode), int(ksize)
    except (ValueError, TypeError) as e:
        raise error(str(e))


def parse(text):
    """The tools' --smooth argument, "gaussian[:K]" or "median[:K]" -> (mode, ksize); defaults gaussian:5 and median:3.  ValueError for a
    name or a K that does not exist."""
    name, sep, k = str(text).partition(":")
    if name not in MODES:
        raise ValueError("--smooth: %r is neither gaussian nor median" % (name,))
    mode = MODES[name]
    if not sep:
        return mode, DEFAULT_KSIZE[mode]
    try:
        ksize = int(k)
    except ValueError:
        raise ValueError("--smooth: K is not a number in %r" % (text,))
    if ksize not in KSIZES[mode]:
        raise ValueError("--smooth: %s takes K in %s, not %d" % (name, KSIZES[mode], ksize))
    return mode, ksize
