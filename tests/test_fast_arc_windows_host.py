"""The arithmetic of fast_pair_scores (csrc/kernels_image.h), restated in numpy float16: a ring pixel p ORed with 0x6400 is the
half-precision number 1024 + p, and a sliding 3-window followed by the windows at offsets 0, 3, 6 of it gives the 16 nine-arcs.
Checked against the integer definition of image_chain_cases.fast_scores.  No GPU."""
import numpy as np
import pytest

import image_chain_cases as icc


def test_biased_pixels_are_exact_halves():
    p = np.arange(256, dtype=np.uint16)
    h = (p + 1024).astype(np.float16)
    np.testing.assert_array_equal(h.view(np.uint16), 0x6400 + p)
    np.testing.assert_array_equal((p | 0x6400).view(np.float16).astype(np.int32), 1024 + p.astype(np.int32))
    assert np.all(np.diff(h.astype(np.float64)) == 1.0)      # ordered like p, nothing rounded


def _min3(a, b, c):
    return np.minimum(np.minimum(a, b), c)


def _max3(a, b, c):
    return np.maximum(np.maximum(a, b), c)


def arc_window_scores(img, t):
    """Byte scores the way the kernel computes them: float16 ring pixels, three-input min / max, centre subtracted at the end."""
    t = min(max(int(t), 0), 255)
    H, W = img.shape
    out = np.zeros((H, W), np.int32)
    bits = img.astype(np.uint16) | np.uint16(0x6400)
    p = np.stack([bits[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] for dx, dy in icc.RING]).view(np.float16)
    assert p.dtype == np.float16
    mn3 = np.stack([_min3(p[k], p[(k + 1) & 15], p[(k + 2) & 15]) for k in range(16)])
    mx3 = np.stack([_max3(p[k], p[(k + 1) & 15], p[(k + 2) & 15]) for k in range(16)])
    amn = np.stack([_min3(mn3[k], mn3[(k + 3) & 15], mn3[(k + 6) & 15]) for k in range(16)])
    amx = np.stack([_max3(mx3[k], mx3[(k + 3) & 15], mx3[(k + 6) & 15]) for k in range(16)])
    M = amx.min(axis=0).view(np.uint16).astype(np.int32) & 0x3FF     # min over the arcs of the arc's max
    m = amn.max(axis=0).view(np.uint16).astype(np.int32) & 0x3FF     # max over the arcs of the arc's min
    v = img[3:H - 3, 3:W - 3].astype(np.int32)
    a, b = v - M, m - v
    out[3:H - 3, 3:W - 3] = np.where((a > t) | (b > t), np.maximum(t, np.maximum(a, b)) - 1, 0)
    return out


def _images():
    rng = np.random.default_rng(950)
    return {
        "noise": rng.integers(0, 256, (64, 64)).astype(np.uint8),
        "two-level": (255 * (rng.random((64, 64)) < 0.5)).astype(np.uint8),
        "four-level": (64 * rng.integers(0, 4, (64, 64))).astype(np.uint8),
    }


@pytest.mark.parametrize("name", ["noise", "two-level", "four-level"])
def test_arc_windows_equal_the_integer_definition(name):
    img = _images()[name]
    for t in (0, 20, 100):
        want = icc.fast_scores(img, t)
        got = arc_window_scores(img, t)
        np.testing.assert_array_equal(got, want, err_msg="%s thr %d" % (name, t))
    assert np.count_nonzero(icc.fast_scores(img, 20)) > 30
