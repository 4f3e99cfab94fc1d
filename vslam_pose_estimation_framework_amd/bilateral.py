"""The optional first step of DepthFramePointGenerator::_computeDepthMap (depth_framepoint_generator.cpp:415-422, enable_bilateral_filtering):
16-bit depth -> metres as float, cv::bilateralFilter(src, dst, -1, 2, 2), back to 16 bit — restated in numpy [recalled: the 32-bit float path of
cv::bilateralFilter and the two convertTo calls around it are written from memory, like the project's other OpenCV semantics; there is no OpenCV
to run beside it].  Every float32 operation is one IEEE single operation, nothing is fused.

    to metres   v = float32(raw) * float32(depth_scale)
    radius      max(1, rint(sigma_space * 1.5)), ties to even (cvRound); sigmas <= 0 count as 1; radius > 8 is refused
    taps        (i, j) over -radius .. radius, i (rows) outer, j inner, kept when sqrt(i*i + j*j) <= radius (the centre included), in that
                order: 29 at radius 3, the 5-tap plus at radius 1.  space_weight = float32(exp_fixed((i*i + j*j) * (-0.5 / sigma_space**2)))
    borders     BORDER_REFLECT_101 through the borderInterpolate loop (p < 0: -p; p >= n: 2 n - 2 - p; until inside); n == 1: index 0
    range       lo, hi = min, max of v over the whole image (holes count).  hi - lo < FLT_EPSILON: the filter is the identity on v
    table       scale_index = float32(4096) / float32(hi - lo); lut[i] = float32(exp_fixed((i / scale_index)**2 * (-0.5 / sigma_color**2))),
                i = 0 .. 4097, quotient and square in float64; once an entry has rounded to 0.0f every later one is 0
    per pixel   over the taps in order, val0 the centre:  alpha = |val - val0| * scale_index, idx = int(alpha), alpha -= idx,
                w = space_weight[k] * (lut[idx] + alpha * (lut[idx + 1] - lut[idx])), sum += val * w, wsum += w;  out = sum / wsum
    to 16 bit   a = float32(1.0 / depth_scale); clip(rint(float32(out * a)), 0, 65535), ties to even

exp_fixed(x), x <= 0, is float64 arithmetic made of IEEE +, -, *, rint and ldexp only, so that numpy, the host compiler and the device agree
on every bit of it (libm's, numpy's SIMD and the device's exp may each differ in the last one): k = rint(x * (1 / ln 2)),
r = (x - k * LN2_HI) - k * LN2_LO, the Taylor polynomial of degree 13 in Horner form, ldexp(p, k).  csrc/exp_fixed.h is the same text in C++.

The reference of the tests of the device path (kernels_bilateral.h: vslam_bilateral_depth_u16, vslam_rgbd_set_bilateral) and a host fallback
for callers without a device."""
import math

import numpy as np

MAX_PIXELS = 1 << 24
MAX_RADIUS = 8            # VS_BL_MAX_RADIUS
LUT_BINS = 4096           # kExpNumBins
LUT_SIZE = LUT_BINS + 2

_F = np.float32
_EPS = np.finfo(np.float32).eps

# exp_fixed's constants: fdlibm's split of ln 2 (LN2_HI has 21 trailing zero bits: k * LN2_HI is exact for |k| < 2^11) and 1 / j!
INV_LN2 = 1.4426950408889634
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
EXP_DEGREE = 13
EXP_COEFF = tuple(1.0 / math.factorial(j) for j in range(EXP_DEGREE + 1))
EXP_UNDERFLOW = -746.0    # below it the result is 0 (exp(-746) < 2^-1076 rounds to 0)


def exp_fixed(x):
    """exp(x) for x <= 0, float64, scalar or array.  x < -746 gives 0."""
    x = np.asarray(x, np.float64)
    xc = np.maximum(x, EXP_UNDERFLOW)
    k = np.rint(xc * INV_LN2)
    r = (xc - k * LN2_HI) - k * LN2_LO
    p = np.full(x.shape, EXP_COEFF[EXP_DEGREE], np.float64)
    for j in range(EXP_DEGREE - 1, -1, -1):
        p = EXP_COEFF[j] + r * p
    out = np.ldexp(p, k.astype(np.int32))
    out = np.where(x < EXP_UNDERFLOW, 0.0, out)
    return out if out.ndim else float(out)


def effective_sigma(sigma):
    sigma = float(sigma)
    if math.isnan(sigma) or math.isinf(sigma):
        raise ValueError("bilateral: sigma is not finite")
    return sigma if sigma > 0 else 1.0


def radius_of(sigma_space):
    """max(1, cvRound(sigma_space * 1.5)); ValueError above MAX_RADIUS."""
    r = max(1, int(np.rint(effective_sigma(sigma_space) * 1.5)))
    if r > MAX_RADIUS:
        raise ValueError("bilateral: radius %d above %d" % (r, MAX_RADIUS))
    return r


def space_taps(sigma_space):
    """(di int32 [n], dj int32 [n], weight float32 [n]) in scan order."""
    s = effective_sigma(sigma_space)
    radius = radius_of(s)
    coeff = -0.5 / (s * s)
    di, dj, w = [], [], []
    for i in range(-radius, radius + 1):
        for j in range(-radius, radius + 1):
            if math.sqrt(float(i * i + j * j)) > radius:
                continue
            di.append(i)
            dj.append(j)
            w.append(_F(exp_fixed(float(i * i + j * j) * coeff)))
    return np.array(di, np.int32), np.array(dj, np.int32), np.array(w, _F)


def color_lut(lo, hi, sigma_color):
    """float32 [4098]: the colour table of an image whose metres span lo .. hi (float32).  A flat image (hi - lo < FLT_EPSILON) has no table:
    zeros."""
    s = effective_sigma(sigma_color)
    span = _F(_F(hi) - _F(lo))
    if span < _EPS:
        return np.zeros(LUT_SIZE, _F)
    scale_index = _F(LUT_BINS) / span
    coeff = -0.5 / (s * s)
    v = np.arange(LUT_SIZE, dtype=np.float64) / np.float64(scale_index)
    lut = exp_fixed(v * v * coeff).astype(_F)
    zero = np.flatnonzero(lut == 0)
    if zero.size:
        lut[zero[0]:] = 0
    return lut


def reflect101(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101) on an integer array."""
    p = np.asarray(p, np.int64).copy()
    if n == 1:
        return np.zeros_like(p)
    while True:
        bad = (p < 0) | (p >= n)
        if not bad.any():
            return p
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def check_arguments(rows, cols, depth_scale, sigma_color, sigma_space):
    """ValueError for what the device entries refuse with VSLAM_ERR_INVALID."""
    if rows < 0 or cols < 0:
        raise ValueError("bilateral: negative size")
    if not (float(depth_scale) > 0 and math.isfinite(float(depth_scale))):
        raise ValueError("bilateral: depth_scale must be positive and finite")
    effective_sigma(sigma_color)
    radius_of(sigma_space)
    if rows * cols > MAX_PIXELS:
        raise ValueError("bilateral: more than 2^24 pixels")


def bilateral_depth_u16(depth_u16, depth_scale, sigma_color=2.0, sigma_space=2.0, return_lut=False):
    """depth_u16: 2-D uint16 -> the filtered image, uint16 (with return_lut: and the colour table, float32 [4098])."""
    img = np.asarray(depth_u16)
    if img.dtype != np.uint16 or img.ndim != 2:
        raise ValueError("bilateral_depth_u16: a 2-D uint16 image is required")
    rows, cols = img.shape
    check_arguments(rows, cols, depth_scale, sigma_color, sigma_space)
    if rows == 0 or cols == 0:
        return (img.copy(), np.zeros(LUT_SIZE, _F)) if return_lut else img.copy()
    v = img.astype(_F) * _F(depth_scale)
    lo, hi = v.min(), v.max()
    lut = color_lut(lo, hi, sigma_color)
    if _F(hi - lo) < _EPS:
        out = v
    else:
        scale_index = _F(LUT_BINS) / _F(hi - lo)
        di, dj, sw = space_taps(sigma_space)
        ri, ci = np.arange(rows), np.arange(cols)
        acc = np.zeros((rows, cols), _F)
        wsum = np.zeros((rows, cols), _F)
        for k in range(di.size):
            val = v[np.ix_(reflect101(ri + int(di[k]), rows), reflect101(ci + int(dj[k]), cols))]
            alpha = np.abs(val - v) * scale_index
            idx = alpha.astype(np.int32)
            alpha = alpha - idx.astype(_F)
            w = sw[k] * (lut[idx] + alpha * (lut[idx + 1] - lut[idx]))
            acc = acc + val * w
            wsum = wsum + w
            assert w.dtype == _F and acc.dtype == _F
        out = acc / wsum
    a = _F(1.0 / float(depth_scale))
    res = np.clip(np.rint(out * a), 0, 65535).astype(np.uint16)
    return (res, lut) if return_lut else res
