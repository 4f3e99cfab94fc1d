"""Stand-alone solver and matcher entries on the seeded random cases of tests/random_cases.py: HIP against the oracle at every size and against
the Python restatements of tests/golden/make_golden.py at the sizes they can afford (listed in random_cases.py), so that a mistake the oracle
and a kernel share is still caught.  The sizes straddle the frame kernel's 512-measurement chunks and 64-lane waves, the scratch context's
1024-point rounding, the matchers' candidate lists (16 left, 8 right, 32 / 6 for the RGB-D tracker) and the 256-thread blocks of the small
entries; the inputs are asserted to force the overflow paths.  Volume thresholds: about two thirds of what the oracle produces, exact where the case list fixes the count."""
import pytest

import random_cases as rc
from _oracle import Oracle
from vslam_pose_estimation_framework_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    api = hip.load()
    api.create(api.default_config("kitti"), 0, 1)
    yield api
    api.destroy()


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_converged_random_sizes(gpu, oracle, uvd):
    """n = 0 .. 3000: chunks beyond the first (reloaded measurements, += into LDS, their chi / inlier stores), partial waves, a whole wave of
    the second chunk skipped, skipped rows and outliers on every seam; the inlier-only rounds on both sides of their gate."""
    rej = rc.Rejections()
    total = rc.sweep_align_converged(gpu, oracle, rej, uvd)
    rounds = rc.sweep_align_gate(gpu, oracle, rej, uvd)
    rej.check("aligner uvd=%d" % uvd)
    assert total > 115000 and rounds >= 4


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_first_round_normal_matrix(uvd):
    assert rc.sweep_align_first_round(hip.load, Oracle, uvd) == sum(rc.ALIGN_SIZES)


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_general_camera_matrix(uvd):
    """K with a skew of 0.3: the !pinhole branch of align_rows."""
    rej = rc.Rejections()
    pair = rc._contexts(hip.load, Oracle, K=rc.SKEW_K)
    try:
        total = rc.sweep_align_converged(pair[0], pair[1], rej, uvd, sizes=[64, 513, 1025], base_seed=6000, K=rc.SKEW_K)
    finally:
        rc._destroy(pair)
    total += rc.sweep_align_first_round(hip.load, Oracle, uvd, sizes=[64, 513, 1025], K=rc.SKEW_K)
    rej.check("aligner general K uvd=%d" % uvd)
    assert total > 16000 + 64 + 513 + 1025


@pytest.mark.parametrize("uvd", [False, True], ids=["stereo", "uvd"])
def test_aligner_rank_deficient_fallback(uvd):
    """No damping, no translation weights: ldlt_solve6 refuses its zero first pivot, wave_solve6 pivots inside the rotational block and stops
    at rank 3."""
    assert rc.sweep_align_fallback(hip.load, Oracle, uvd) == 2 * (64 + 513)


def test_track_match_random(gpu, oracle):
    rej = rc.Rejections()
    total = rc.sweep_track(gpu, oracle, rej)
    rej.check("track_match")
    assert total > 4300


def test_stereo_match_random():
    assert rc.sweep_stereo(hip.load, Oracle) > 17500


def test_stereo_bin_table_forms():
    """The bin competition on its 16-bit LDS tables (bin 5) and on its HBM tables (bin 3); bin 15 of every other test takes the 32-bit LDS tables."""
    assert rc.sweep_stereo_forms(hip.load, Oracle, rc.STEREO_BIN_CASES, python_max=0)[0] > 7000


def test_stereo_dense_row():
    """More than 255 right features behind a left feature: step B's explicit scan from the cursor, in the whole-image sweep and in a band.
    (Step B once skipped such a left feature when the cursor stood past the row's 255th right feature: 194 of the oracle's 199 matches at
    513 x 513, epipolar offset 0.  The count of right features saturates at 255, and 255 now means "scan".)"""
    assert rc.sweep_stereo_forms(hip.load, Oracle, rc.STEREO_DENSE_ROW_CASES, python_max=0)[0] > 800


def test_stereo_single_row_overflow():
    """One row whose slices alone exceed the arena: the reference loop on HBM."""
    assert rc.sweep_stereo_forms(hip.load, Oracle, rc.STEREO_WIDE_CASES, python_max=0)[0] > 1000


def test_landmark_update_random(gpu, oracle):
    moved, kept, taken = rc.sweep_landmark(gpu, oracle)
    assert moved > 4800 and kept > 1200 and taken > 3800


def test_small_entries_random(gpu, oracle):
    assert rc.SHAPES == __import__("test_hip_random_shapes").SHAPES
    assert rc.sweep_point_in_camera(gpu, oracle) == sum(rc.PIC_SIZES)
    pixels, points = rc.sweep_resize_harris(gpu, oracle)
    assert pixels > 1650000 and points == 1080


def test_depth_track_random(gpu, oracle):
    rej = rc.Rejections()
    total, temp = rc.sweep_depth_track(gpu, oracle, rej)
    rej.check("depth_track")
    assert total > 3200 and temp > 380


@pytest.mark.parametrize("shape", rc.REC_SHAPES, ids=["%dx%d" % s for s in rc.REC_SHAPES])
def test_stereo_recover_random(shape):
    """vslam_stereo_recover on four image shapes (one with a single recoverable row pair), n = 0 .. 4096, both poses: more than VS_WG lost points
    in wg_recover_project, runs of 2 .. 8 lost points per thread in wg_recover_append, the work list in LDS up to 1802 projected points and the
    rec[] walk beyond, the scratch context's 1024 rounding, padded rows, every gate on its equality (random_cases, section F)."""
    total = rc.sweep_stereo_recover(hip.load, Oracle, shapes=[shape])
    sizes = rc.stereo_recover_sizes(shape)
    assert total["recovered"] > 0.9 * sum(sizes) and total["cases"] == 2 * len(sizes) and total["exact"] == 28 * sum(1 for n in sizes if n >= 64)


def test_stereo_recover_context_reuse_and_patterns():
    reuse = rc.sweep_stereo_recover_reuse(hip.load, Oracle)
    patterns = rc.sweep_stereo_recover_patterns(hip.load, Oracle)
    orb = rc.sweep_stereo_recover_orb(hip.load, Oracle)
    assert reuse > 5100 and patterns > 2000 and orb > 4100


def test_depth_recover_random(gpu, oracle):
    """vslam_depth_recover, n = 0 .. 3000: more than one block of k_depth_recover_project, more than one grid pass of k_brief_at / k_orb_at,
    three passes of k_depth_recover_finish with survivors on both sides of each seam, the resident map, padded rows, the gates' equalities."""
    rej = rc.Rejections()
    total = rc.sweep_depth_recover(gpu, oracle, rej)
    rej.check("depth_recover")
    assert total["recovered"] > 10700 and total["cases"] == 38 and total["exact"] == 14 * 19 and total["resident"] > 850 and total["orb"] > 2400
