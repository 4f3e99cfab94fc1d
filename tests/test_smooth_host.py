"""Smoothing on the CPU: smooth.py against plain Python loops, the impulse tables, constants, refusals, the tools' --smooth parser, the
header's declarations, the 5 x 5 median's exchange network over every 0/1 input, and the premise of the GPU detection test."""
import os
import sys

import numpy as np
import pytest

import orb_cases
import smooth_cases as sc
from golden import make_golden as mg
from vslam_pose_estimation_framework_amd import smooth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode,ksize", sc.MODES, ids=[sc.mode_name(*m) for m in sc.MODES])
def test_numpy_equals_scalar_restatement(mode, ksize):
    n = 0
    for rows, cols in sc.MEDIAN_ONLY_SHAPES[:2] + sc.SCALAR_SHAPES:
        if (rows, cols) not in sc.shapes_for(mode, ksize):
            continue
        for name in sc.CONTENTS:
            for img in sc.contents(name, rows, cols):
                got = smooth.smooth_u8(img, mode, ksize)
                assert got.dtype == np.uint8 and got.shape == img.shape
                np.testing.assert_array_equal(got, sc.scalar(img.tolist(), mode, ksize), err_msg="%s %d x %d %s" % (sc.mode_name(mode, ksize), rows, cols, name))
                n += 1
    assert n >= 4 * len(sc.CONTENTS)


def test_gaussian_impulse_tables():
    img = np.zeros((9, 13), np.uint8)
    img[0, 0] = 255
    g = smooth.gaussian_u8(img, 5)
    # 255 * K_i K_j >> 16 with the reflection folding tap -1 onto 1 and -2 onto 2: (96, 128, 32) / 256 along each axis
    assert g[0, :4].tolist() == [36, 24, 6, 0] and g[1, :4].tolist() == [24, 16, 4, 0] and g[3:].max() == 0
    # away from the border the output is the tap table itself
    img = np.zeros((15, 15), np.uint8)
    img[7, 7] = 255
    for k in (3, 5, 7):
        taps = np.array(smooth.TAPS[k], np.int64)
        assert taps.sum() == 256
        want = ((255 * np.outer(taps, taps) + 32768) >> 16).astype(np.uint8)
        r = k // 2
        np.testing.assert_array_equal(smooth.gaussian_u8(img, k)[7 - r:8 + r, 7 - r:8 + r], want)
    # a median removes an impulse
    for k in (3, 5):
        assert smooth.median_u8(img, k).max() == 0


@pytest.mark.parametrize("mode,ksize", sc.MODES, ids=[sc.mode_name(*m) for m in sc.MODES])
def test_constants_map_to_themselves(mode, ksize):
    for value in (0, 1, 127, 254, 255):
        img = np.full((9, 13), value, np.uint8)
        np.testing.assert_array_equal(smooth.smooth_u8(img, mode, ksize), img)


def test_median_of_one_pixel():
    for k in (3, 5):
        assert smooth.median_u8(np.array([[77]], np.uint8), k).tolist() == [[77]]
        np.testing.assert_array_equal(smooth.median_u8(np.array([[1, 9, 5]], np.uint8), 3), [[1, 5, 5]])


def test_check_refuses():
    for mode, ksize, rows, cols in [(0, 3, 9, 9), (3, 3, 9, 9), (smooth.GAUSSIAN, 4, 9, 9), (smooth.GAUSSIAN, 9, 20, 20), (smooth.MEDIAN, 7, 9, 9),
                                    (smooth.MEDIAN, 1, 9, 9), (smooth.GAUSSIAN, 3, 1, 9), (smooth.GAUSSIAN, 5, 9, 2), (smooth.GAUSSIAN, 7, 3, 9),
                                    (smooth.MEDIAN, 3, 0, 9)]:
        with pytest.raises(ValueError):
            smooth.check(mode, ksize, rows, cols)
    for mode, ksize in sc.MODES:
        for rows, cols in sc.shapes_for(mode, ksize):
            smooth.check(mode, ksize, rows, cols)
        for rows, cols in sc.refused_shapes(mode, ksize):
            with pytest.raises(ValueError):
                smooth.check(mode, ksize, rows, cols)
    with pytest.raises(ValueError):
        smooth.gaussian_u8(np.zeros((2, 9), np.uint8), 5)
    with pytest.raises(ValueError):
        smooth.median_u8(np.zeros((4, 4), np.uint16), 3)


def test_smooth_argument_of_the_tools():
    assert smooth.parse("gaussian") == (smooth.GAUSSIAN, 5) and smooth.parse("median") == (smooth.MEDIAN, 3)
    assert smooth.parse("gaussian:3") == (smooth.GAUSSIAN, 3) and smooth.parse("gaussian:7") == (smooth.GAUSSIAN, 7) and smooth.parse("median:5") == (smooth.MEDIAN, 5)
    for bad in ("", "box", "Gaussian", "gaussian:4", "gaussian:9", "median:7", "median:x", "median:", "gaussian:5:5"):
        with pytest.raises(ValueError):
            smooth.parse(bad)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import run_kitti
        import run_rgbd
    finally:
        sys.path.pop(0)
    assert smooth.argument(None) is None and smooth.argument("median") == (smooth.MEDIAN, 3) and smooth.argument((smooth.GAUSSIAN, 7)) == (smooth.GAUSSIAN, 7)
    for bad in ("box", "median:7", (smooth.MEDIAN, 7), (5, 3), 5):
        with pytest.raises(ValueError):
            smooth.argument(bad)
        with pytest.raises(SystemExit):
            smooth.argument(bad, SystemExit)
    for tool in (run_kitti, run_rgbd):
        assert tool.parse_args(["folder", "--smooth", "median"]).smooth == "median"
        with pytest.raises(SystemExit):
            tool.parse_args(["folder", "--smooth", "box"])
    assert run_kitti.parse_args(["folder", "--smooth", "gaussian:3"]).smooth == "gaussian:3"
    assert run_kitti.parse_args(["folder"]).smooth is None
    with pytest.raises(SystemExit):
        run_kitti.parse_args(["folder", "--smooth", "median:4"])


def test_header_declares_the_entries():
    text = open(os.path.join(ROOT, "include", "vslam_hip.h")).read()
    for name in ("vslam_set_smoothing", "vslam_get_smoothing", "vslam_get_smoothed_images", "vslam_smooth_u8", "vslam_rgbd_set_smoothing",
                 "vslam_rgbd_get_smoothing", "vslam_rgbd_get_smoothed"):
        assert ("int %s(" % name) in text, name
    for name, value in (("VSLAM_SMOOTH_OFF", smooth.OFF), ("VSLAM_SMOOTH_GAUSSIAN", smooth.GAUSSIAN), ("VSLAM_SMOOTH_MEDIAN", smooth.MEDIAN)):
        assert ("#define %s %d\n" % (name, value)) in text, name


def test_median25_network_of_the_kernel_selects_the_median():
    net = sc.med25_network(open(os.path.join(ROOT, "vslam_pose_estimation_framework_amd", "csrc", "kernels_smooth.h")).read())
    assert len(net) == 99 and all(0 <= a < b < 25 for a, b in net)
    assert sc.network_selects_median(net)
    # the check can fail: one exchange turned round
    broken = list(net)
    broken[50] = broken[50][::-1]
    assert not sc.network_selects_median(broken)


def test_detection_premise_every_mode_changes_the_corner_count_by_a_tenth():
    """block_image(150, 190) plus uniform noise in -14 .. 14 (seed 3): FAST at threshold 20 finds 1455 corners, 1169 / 1036 / 802 behind a
    3 / 5 / 7 Gaussian, 1002 / 887 behind a 3 / 5 median.  So a detection test under the switch is not vacuous."""
    base = orb_cases.block_image(150, 190).astype(np.int64)
    noisy = np.clip(base + np.random.default_rng(3).integers(-14, 15, base.shape), 0, 255).astype(np.uint8)
    plain = len(mg.fast9_16(noisy, 20))
    for mode, ksize in sc.MODES:
        n = len(mg.fast9_16(smooth.smooth_u8(noisy, mode, ksize), 20))
        print("%s: %d corners against %d" % (sc.mode_name(mode, ksize), n, plain))
        assert abs(n - plain) > 0.1 * plain, (sc.mode_name(mode, ksize), n, plain)
