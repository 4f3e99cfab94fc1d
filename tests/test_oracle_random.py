"""CPU: the oracle's stand-alone solver and matcher entries against the Python restatements of tests/golden/make_golden.py on the seeded
random cases of tests/random_cases.py.  This is where the generators, their premises and the tolerances are validated without a GPU; the
sizes the Python references can afford are listed at the top of random_cases.py.  The volume thresholds are about two thirds of what the
oracle produces (counts that the case list fixes are asserted exactly)."""
import pytest

import random_cases as rc
from _oracle import Oracle


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_converged_random_sizes(oracle, uvd):
    rej = rc.Rejections()
    total = rc.sweep_align_converged(oracle, None, rej, uvd, sizes=[n for n in rc.ALIGN_SIZES if n <= rc.PY_ALIGN_MAX])
    rounds = rc.sweep_align_gate(oracle, None, rej, uvd)
    rej.check("aligner uvd=%d" % uvd)
    print("measurement rounds", total, "inlier-only rounds", rounds)
    assert total > 58000 and rounds >= 4


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_first_round_normal_matrix(uvd):
    total = rc.sweep_align_first_round(Oracle, None, uvd, sizes=[n for n in rc.ALIGN_SIZES if n <= rc.PY_ALIGN_MAX])
    assert total == sum(n for n in rc.ALIGN_SIZES if n <= rc.PY_ALIGN_MAX)


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_general_camera_matrix(uvd):
    rej = rc.Rejections()
    o = Oracle()
    o.create(rc.config_with(o, K=rc.SKEW_K), 0, 1)
    try:
        total = rc.sweep_align_converged(o, None, rej, uvd, sizes=[64, 513, 1025], base_seed=6000, K=rc.SKEW_K)
    finally:
        o.destroy()
    total += rc.sweep_align_first_round(Oracle, None, uvd, sizes=[64, 513, 1025], K=rc.SKEW_K)
    rej.check("aligner general K uvd=%d" % uvd)
    assert total > 16000 + 64 + 513 + 1025


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_rank_deficient_fallback(uvd):
    assert rc.sweep_align_fallback(Oracle, None, uvd) == 2 * (64 + 513)


def test_track_match_random(oracle):
    rej = rc.Rejections()
    total = rc.sweep_track(oracle, None, rej)
    rej.check("track_match")
    print("tracked", total)
    assert total > 4300


def test_stereo_match_random():
    total = rc.sweep_stereo(Oracle, None)
    print("stereo matches", total)
    assert total > 17500


def test_stereo_bin_table_forms():
    """bin 5 (16-bit tables) and bin 3 (tables in HBM) on the KITTI geometry; `lost` = candidates that lost their bin, so bins are contested"""
    total, lost = rc.sweep_stereo_forms(Oracle, None, rc.STEREO_BIN_CASES)
    print("stereo matches", total, "lost their bin", lost)
    assert total > 7000 and lost > 150


def test_stereo_dense_row():
    """300 + 300 features on one row: more than 255 right features behind a left feature, whole image and banded"""
    total, lost = rc.sweep_stereo_forms(Oracle, None, rc.STEREO_DENSE_ROW_CASES)
    print("stereo matches", total, "lost their bin", lost)
    assert total > 800 and lost > 50


def test_stereo_single_row_overflow():
    """8192 x 32 image, 5800 + 5800 features on one row: the row's slices alone exceed the arena"""
    total, lost = rc.sweep_stereo_forms(Oracle, None, rc.STEREO_WIDE_CASES, python_max=6000)
    print("stereo matches", total, "lost their bin", lost)
    assert total > 1000 and lost > 500


def test_landmark_update_random(oracle):
    moved, kept, taken = rc.sweep_landmark(oracle, None)
    print("landmarks moved", moved, "kept", kept, "estimates taken", taken)
    assert moved > 4800 and kept > 1200 and taken > 3800


def test_small_entries_random(oracle):
    assert rc.sweep_point_in_camera(oracle, None) == sum(rc.PIC_SIZES)
    pixels, points = rc.sweep_resize_harris(oracle, None)
    assert pixels > 1650000 and points == 1080


def test_depth_track_random(oracle):
    rej = rc.Rejections()
    total, temp = rc.sweep_depth_track(oracle, None, rej)
    rej.check("depth_track")
    print("tracked", total, "temporary", temp)
    assert total > 3200 and temp > 380


def test_stereo_recover_random():
    """orc_stereo_recover == stereo_recover_ref at every size of the sweep, premises and exact cases included (random_cases, section F)"""
    total = rc.sweep_stereo_recover(Oracle, None, python_max=10 ** 9)
    print("stereo_recover", total)
    assert total["recovered"] > 19000 and total["projected_max"] > 2 * rc.VS_RLIST_CAP and total["cases"] == 54 and total["exact"] == 21 * 28


def test_stereo_recover_context_reuse_and_patterns():
    """the oracle keeps no scratch context, so reuse only validates the cases; the patterns run against the restatement under the same table;
    the ORB extractor has no restatement: the oracle runs alone and the volume is checked"""
    reuse = rc.sweep_stereo_recover_reuse(Oracle, None)
    patterns = rc.sweep_stereo_recover_patterns(Oracle, None, python=True)
    orb = rc.sweep_stereo_recover_orb(Oracle, None)
    print("stereo_recover reuse", reuse, "patterns", patterns, "ORB", orb)
    assert reuse > 5100 and patterns > 2000 and orb > 4100


def test_depth_recover_random(oracle):
    rej = rc.Rejections()
    total = rc.sweep_depth_recover(oracle, None, rej)
    rej.check("depth_recover")
    print("depth_recover", total)
    assert total["recovered"] > 10700 and total["cases"] == 38 and total["exact"] == 14 * 19 and total["orb"] > 2400
