"""The numpy rebuild of the landmark refinement (tests/landmark_rebuild.py) proved against the CPU oracle before it judges a kernel
(tests/test_landmark_refinement_gpu.py): the slow street scene — tracks of up to 110 measurements — with a history ring nothing
outgrows, where the oracle (which keeps every measurement) is a valid second opinion; then the rebuild with shorter rings on the same
exports, where only its bookkeeping of truncated tracks can be checked."""
import numpy as np
import pytest

from landmark_rebuild import ACCEPT, KEEP, RESET, LandmarkRebuild, Tally

SCENE = dict(scale=0.4, seed=7, speed_m=0.15)
FRAMES = 110


def run_oracle(n_frames, kernel=None):
    """The slow scene through the oracle pipeline with a ring nothing outgrows: the exports of every frame."""
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=SCENE["scale"], seed=SCENE["seed"])
    sc.speed_m = SCENE["speed_m"]
    cfg = o.config_for_scene(sc)
    cfg.max_history_frames = 128
    if kernel is not None:
        cfg.landmark_maximum_error_squared_meters = kernel
    o.create(cfg, 0, 1)
    frames = []
    try:
        for k in range(n_frames):
            L, R = o.render(sc, k)
            o.process_host(L, R)
            fi = o.frame_info(0)
            frames.append(dict(points=o.points(0), pose=o.poses(0, k, 1)[0], status=fi.status, fallback=fi.fallback,
                               track_broken=fi.track_broken, error_flags=fi.error_flags))
    finally:
        o.destroy()
    return cfg, frames


@pytest.fixture(scope="module")
def oracle_run():
    return run_oracle(FRAMES)


@pytest.fixture(scope="module")
def oracle_run_tight_kernel():
    """A kernel of 0.05 m instead of 25 m: the far measurements of a track become outliers, so updates are kept and reset as well as accepted."""
    return run_oracle(80, kernel=0.05)


def test_rebuild_equals_the_oracle_on_long_tracks(oracle_run):
    cfg, frames = oracle_run
    rb, tally = LandmarkRebuild(cfg), Tally()
    for k, fr in enumerate(frames):
        assert fr["fallback"] == 0 and fr["track_broken"] == 0 and fr["error_flags"] == 0, (k, fr["fallback"], fr["track_broken"], fr["error_flags"])
        assert k == 0 or fr["status"] == 1, (k, fr["status"])
        res = rb.frame(fr["points"], fr["pose"])
        assert not res.truncated.any()
        tally.check(res, fr["points"], tag="frame %d" % k)       # lm to 1e-9, lmup exact, kept estimates bit for bit
    s = tally.summary()
    print("landmark rebuild == oracle:", s)
    # premises: the run reaches every regime of the fused refinement below the ring
    assert s["ge9"] >= 3000 and s["ge34"] >= 600 and s["ge49"] >= 300, s
    for n_meas in Tally.LENGTHS:
        assert s["exact"][n_meas] >= 1, (n_meas, s["exact"])
    assert s["kinds"].get("accept", 0) >= 1000, s["kinds"]      # (nothing is kept or reset below the ring on this scene: kept estimates need a truncated track)
    assert s["undecidable"] == 0 and s["undecidable"] <= 0.005 * s["updates"], s


@pytest.mark.parametrize("ring,frames_used,min_truncated", [(64, 110, 250), (40, 80, 500), (12, 60, 1800), (8, 40, 1300)])
def test_rebuild_bookkeeping_of_truncated_tracks(oracle_run, ring, frames_used, min_truncated):
    """Rings shorter than the tracks on the oracle's exports: the oracle never truncates, so its `lm` is no target here; the rebuild
    must run and flag exactly the frames that hold an eligible point with more measurements than the ring."""
    cfg, frames = oracle_run
    rb = LandmarkRebuild(cfg, ring=ring)
    flagged, expected, n_truncated = [], [], 0
    for k, fr in enumerate(frames[:frames_used]):
        res = rb.frame(fr["points"], fr["pose"])
        meta = fr["points"]["meta"]
        eligible = meta[:, 3] >= cfg.minimum_track_length_for_landmark_creation
        if (eligible & (meta[:, 3] + 1 > ring)).any():
            expected.append(k)
        if res.truncated.any():
            flagged.append(k)
        assert (res.length <= ring).all() and np.isfinite(res.lm).all()
        n_truncated += int((res.truncated & (res.carried_lmup != 0)).sum())
        # a kept estimate is the carried one whatever the ring
        kept = res.kind == KEEP
        np.testing.assert_array_equal(res.lm[kept], res.carried[kept])
    print("ring %d, %d frames: %d truncated updates, first flagged frame %s" % (ring, frames_used, n_truncated, flagged[:1]))
    assert flagged == expected and flagged and flagged[0] == ring, (flagged[:3], expected[:3])
    assert n_truncated >= min_truncated, n_truncated



def test_rebuild_equals_the_oracle_with_outliers(oracle_run_tight_kernel):
    """All three outcomes of an update against the oracle: accepted, kept (no more inliers than before) and reset to the mean (more outliers
    than inliers), with saturated kernels in the sums."""
    cfg, frames = oracle_run_tight_kernel
    rb, tally = LandmarkRebuild(cfg), Tally()
    for k, fr in enumerate(frames):
        assert fr["fallback"] == 0 and fr["track_broken"] == 0 and fr["error_flags"] == 0 and (k == 0 or fr["status"] == 1), k
        res = rb.frame(fr["points"], fr["pose"])
        tally.check(res, fr["points"], tag="frame %d" % k)
    s = tally.summary()
    print("landmark rebuild == oracle, kernel 0.05:", s)
    assert s["kinds"].get("accept", 0) >= 3000 and s["kinds"].get("keep", 0) >= 500 and s["kinds"].get("reset", 0) >= 40, s["kinds"]
    assert s["kinds"].get("unfinished", 0) == 0 and s["undecidable"] == 0, s


@pytest.mark.parametrize("ring,frames_used,min_accepted,min_reset", [(40, 80, 10, 20), (12, 80, 25, 30)])
def test_tight_kernel_exports_results_of_truncated_updates(oracle_run_tight_kernel, ring, frames_used, min_accepted, min_reset):
    """The premise of the GPU variant of the same name, on the CPU: at these rings the rebuild accepts and resets truncated updates, i.e. values
    computed over a cut list reach the export.  (The carried update counts are the oracle's, of untruncated lists: larger than a
    truncating tracker's, so fewer updates are accepted here than there.)"""
    cfg, frames = oracle_run_tight_kernel
    rb = LandmarkRebuild(cfg, ring=ring)
    accepted = reset = 0
    for fr in frames[:frames_used]:
        res = rb.frame(fr["points"], fr["pose"])
        accepted += int((res.truncated & (res.kind == ACCEPT)).sum())
        reset += int((res.truncated & (res.kind == RESET)).sum())
    print("kernel 0.05, ring %d: %d truncated updates accepted, %d reset" % (ring, accepted, reset))
    assert accepted >= min_accepted and reset >= min_reset, (accepted, reset)
