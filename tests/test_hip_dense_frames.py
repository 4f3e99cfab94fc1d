"""Frames dense enough for the fused frame kernel's over-capacity forms, under frame-by-frame oracle parity (pipeline_compare.compare_frame,
unchanged) or bit-identity between two product paths.

* The unlisted branch of lm_refine_share (csrc/kernels_frame_lm.h): its work lists hold LIST_CAP = 6720 points; a frame whose landmark
  pass sees more is handed out lane by lane, every track on landmark_point (no teams), under the g / G split of k_tail_lm and k_stage_lm.
  The landmark pass runs BEFORE the stereo step appends the frame's new points: its n_cur is n_after_prune + n_recovered
  (= n_points - n_new_stereo of the frame's report), not n_points.  Every premise about the branch below is on that count.
* The bin competition's HBM tables (bin 3) and 16-bit LDS tables (bin 5) with tracked points occupying bins (csrc/kernels_stereo.h).

The dense scene: scene_kitti(seed 7 / 9) at speed_m = 0.15 (the slow scene of the landmark tests), FAST threshold floor 1, bin 3, one
epipolar offset, ring 64.  At scale 1.0 (1241 x 376) a frame has 8.4 - 10.6 k points, but the landmark pass only climbs to ~6.7 k: of the
first 38 frames it is over capacity on frame 37 alone (6776 points, 3356 updates with >= 9 measurements, 259 with >= 34: the trail's
directly addressed part and the link walk behind it).  At scale 1.25 (1551 x 470) it is over capacity from frame 5 on (7.0 - 8.6 k),
which is where the two-stream and stage-path cases reach the branch.  CPU figures in the premises' comments: the oracle alone.

The oracle runs once per (scale, seed) for the whole module (`recordings`): its exports are kept per frame and replayed to compare_frame,
so the CPU twin and the GPU tests share one run.  Oracle time, not the GPU, sets the durations: 0.46 s per frame at scale 1.0, 0.9 s at 1.25."""
import numpy as np
import pytest

import random_cases as rc
from pipeline_compare import compare_frame, create_hip

gpu = pytest.mark.gpu

# LIST_CAP of lm_refine_share is device-side only: restated from the headers' definitions (csrc/kernels_frame_lm.h:318,
# (VS_ARENA - sizeof(LmCache) - VS_LM_TEAM_LDS) / 2; dev_types.h, landmark_math.h)
VS_WG, VS_LM_NP, VS_LM_CN, VS_LM_TEAM_WAVES, VS_LM_TEAM_G = 512, 48, 6, 2, 8
SIZEOF_LMCACHE = 8 * (VS_LM_NP * 12 + VS_LM_NP * 9 + VS_WG * VS_LM_CN * 4)        # struct LmCache: w2c, rtr, cam (doubles)
SIZEOF_LMTERM = 8 * (1 + 6 + 3) + 2 * 4                                          # struct LmTerm: e2, h[6], b[3]; kind, pad
VS_LM_TEAM_LDS = VS_LM_TEAM_WAVES * (64 // VS_LM_TEAM_G) * VS_LM_TEAM_G * SIZEOF_LMTERM
LIST_CAP = (rc.VS_ARENA - SIZEOF_LMCACHE - VS_LM_TEAM_LDS) // 2
assert LIST_CAP == 6720

LONG_FRAMES, SHORT_FRAMES, BIN5_FRAMES = 38, 12, 8


def _dense(cfg):
    cfg.detector_threshold_minimum = 1
    cfg.detector_threshold_maximum_change = 0.9
    cfg.max_keypoints, cfg.max_points = 32768, 16384
    cfg.bin_size_pixels = 3
    cfg.maximum_epipolar_search_offset_pixels = 1
    cfg.max_history_frames = 64


def _bin5(cfg):
    cfg.bin_size_pixels = 5


# name -> (scene scale, speed_m or None for the scene's own, configuration edit, frames recorded per seed)
CASES = {"dense": (1.0, 0.15, _dense, {7: LONG_FRAMES, 9: SHORT_FRAMES}),
         "dense 1.25": (1.25, 0.15, _dense, {7: SHORT_FRAMES, 9: SHORT_FRAMES}),
         "bin 5": (1.0, None, _bin5, {7: BIN5_FRAMES})}


def _scene(o, case, seed):
    scale, speed_m = CASES[case][:2]
    sc = o.scene_kitti(scale=scale, seed=seed)
    if speed_m is not None:
        sc.speed_m = speed_m
    return sc


def config_of(o, case):
    cfg = o.config_for_scene(_scene(o, case, 7))
    CASES[case][2](cfg)
    return cfg


def _record(case, seed):
    """The oracle alone over every frame of one seed of a case: per frame the images and everything compare_frame reads from its checker."""
    from _oracle import Oracle
    o = Oracle()
    sc = _scene(o, case, seed)
    o.create(config_of(o, case), 0, 1)
    frames = []
    try:
        for k in range(CASES[case][3][seed]):
            L, R = o.render(sc, k)
            o.process_host(L, R)
            fi = o.frame_info(0)
            frames.append(dict(L=L, R=R, info=fi, keypoints=(o.keypoints(0, 0), o.keypoints(0, 1)), points=o.points(0),
                               aligner=o.aligner_result(0) if fi.aligner_ran else None, weights=o.aligner_weights_of(0), tracked=o.tracked_keypoints(0)))
    finally:
        o.destroy()
    return frames


@pytest.fixture(scope="module")
def recordings():
    """recordings(case, seed): the oracle's run, made on first use, shared by every test of the module and released with it."""
    have = {}

    def get(case, seed):
        if (case, seed) not in have:
            have[case, seed] = _record(case, seed)
        return have[case, seed]
    yield get
    have.clear()


class Replay(object):
    """The checker side of compare_frame, answered from recordings: stream s is streams[s], the frame is the one `at` was given."""

    def __init__(self, streams):
        self.streams, self.k = streams, 0

    def at(self, k):
        self.k = k
        return self

    def _frame(self, s):
        return self.streams[s][self.k]

    def frame_info(self, s=0):
        return self._frame(s)["info"]

    def keypoints(self, s=0, side=0):
        return self._frame(s)["keypoints"][side]

    def points(self, s=0):
        return self._frame(s)["points"]

    def aligner_result(self, s=0):
        return self._frame(s)["aligner"]

    def aligner_weights_of(self, s=0):
        return self._frame(s)["weights"]


def images(streams, k):
    return np.stack([q[k]["L"] for q in streams]), np.stack([q[k]["R"] for q in streams])


# ---- premises, from a run's own exports (frame_info and points()['meta']) ---------------------------------------------------------------------
def counts_of(fi, points):
    meta = np.asarray(points["meta"])
    update = meta[:, 4] > 0                      # the point carries a landmark; beyond the creation length (2 measurements here) it was refined
    n_meas = meta[:, 3] + 1
    assert fi.n_points - fi.n_new_stereo == fi.n_after_prune + fi.n_recovered and not update[fi.n_points - fi.n_new_stereo:].any()
    return dict(n_points=int(fi.n_points), lm_pass=int(fi.n_points - fi.n_new_stereo), error_flags=int(fi.error_flags), n_tracked=int(fi.n_tracked),
                n_keypoints_left=int(fi.n_keypoints_left), ge9=int((update & (n_meas >= 9)).sum()), ge34=int((update & (n_meas >= 34)).sum()))


def over_capacity(c):
    """the frame's landmark pass took the unlisted branch of lm_refine_share"""
    return c["lm_pass"] > LIST_CAP


def assert_hbm_bin_table_with_tracked_occupants(cfg, counts, tag):
    # bin 3: 126 x 414 bins.  Neither LDS form fits VS_ARENA at any candidate count (a left keypoint yields at most one candidate over all
    # offsets: stereo_band keeps one smatch entry per left feature and stereo_append marks it used)
    rows, cols, size = int(cfg.rows), int(cfg.cols), int(cfg.bin_size_pixels)
    for k, c in enumerate(counts):
        assert rc.bin_table_form(rows, cols, size, 0) == "i32 hbm" and rc.bin_table_form(rows, cols, size, c["n_keypoints_left"]) == "i32 hbm", (tag, k)
        assert k < 3 or c["n_tracked"] > 2000, (tag, k, c["n_tracked"])       # CPU: 2273 .. 2834 from frame 3 on (2263 and 1878 on frames 1 and 2)


def assert_long_premises(cfg, counts, tag):
    """38 frames of the dense scene at scale 1.0.  CPU: n_points 8181, 5661, 6655, then 7467 .. 10571; >= 9 measurements from frame 8 on
    (545 .. 3356 per frame, ~85 k in all), >= 34 from frame 33 on (75, 117, 182, 223, 259); landmark pass 6776 on frame 37, below 6720 before."""
    print(tag, [(c["n_points"], c["lm_pass"], c["ge9"], c["ge34"]) for c in counts])
    assert len(counts) == LONG_FRAMES and all(c["error_flags"] == 0 for c in counts), (tag, [c["error_flags"] for c in counts])
    dense = [c for c in counts if c["n_points"] >= 7000]
    assert len(dense) >= 36, (tag, len(dense))
    assert sum(c["ge9"] for c in dense) >= 50000, (tag, sum(c["ge9"] for c in dense))
    assert counts[-1]["ge34"] >= 100, (tag, counts[-1]["ge34"])
    # the unlisted branch itself: what the frames whose landmark pass is over capacity carry
    over = [c for c in counts if over_capacity(c)]
    assert len(over) >= 1 and sum(c["ge9"] for c in over) >= 2000 and sum(c["ge34"] for c in over) >= 100, (tag, [(c["lm_pass"], c["ge9"], c["ge34"]) for c in over])


def assert_short_premises(case, counts, tag):
    """12 frames of one stream of the dense scene.  CPU, scale 1.0: n_points 8181, 5661, 6655, 7467 .. 9304 (frames 1 and 2, where the tracker
    has just started, stay below 6720), landmark pass <= 5503: the branch is not reached.  Scale 1.25: n_points 12721, 8617, 10117 .. 14462, landmark
    pass 7037, 7795, 8267, 8464, 8398, 8436, 8560 on frames 5 .. 11; updates with >= 9 measurements 1194 + 2049 + 2652 on frames 9 .. 11.
    ("More than 6720 points in every frame" cannot hold at scale 1.0: the scene's own frames 1 and 2 have 5661 and 6655.  They are excepted by
    index; every other frame is held to it.)"""
    print(tag, [(c["n_points"], c["lm_pass"], c["ge9"]) for c in counts])
    assert len(counts) == SHORT_FRAMES and all(c["error_flags"] == 0 for c in counts), (tag, [c["error_flags"] for c in counts])
    thin = (1, 2) if case == "dense" else ()
    assert all(c["n_points"] > LIST_CAP for k, c in enumerate(counts) if k not in thin), (tag, [c["n_points"] for c in counts])
    assert sum(c["ge9"] for c in counts[9:12]) >= 1000, (tag, [c["ge9"] for c in counts[9:12]])
    if case == "dense 1.25":
        assert all(over_capacity(c) for c in counts[5:]), (tag, [c["lm_pass"] for c in counts])


# ---- the 16-bit bin tables: a tracked point's bin that a stereo candidate wants ------------------------------------------------------------------
def bin_of_pixel(cfg, x, y):
    """bin_of_pixel of kernels_stereo.h, as random_cases.ref_stereo_binned restates it"""
    size = float(cfg.bin_size_pixels)
    rows_bin, cols_bin = int(cfg.rows) // int(cfg.bin_size_pixels) + 1, int(cfg.cols) // int(cfg.bin_size_pixels) + 1
    return np.minimum(np.rint(y / size).astype(np.int64), rows_bin - 1) * cols_bin + np.minimum(np.rint(x / size).astype(np.int64), cols_bin - 1)


def contested_bins(lib, cfg, fi, keypoints, points, tracked):
    """The stereo candidates of the frame whose left pixel falls into the bin of a tracked (or recovered) point — the candidates that
    `if (t.occ(k) != VS_BIN_EMPTY) continue` has to turn away — and, as a check of the rebuild, the points the frame should have added.

    The candidates are not exported; they are rebuilt: the stereo sweep (the checker library's stand-alone entry, binning off) over the keypoints the
    tracker left behind.  A tracked point consumed its left and its right keypoint and every right keypoint between them on the right one's row
    (the oracle's track()), whether or not the prune kept it afterwards: `tracked` is the oracle's list of all of them (orc_get_tracked_keypoints; the
    product's fused path keeps none — the GPU test takes the recorded one, after compare_frame found n_tracked, the aligner's per-point errors and
    every export of the frame equal).  Recovered points take no keypoint.  Occupants and keypoints are the run's own exports."""
    assert int(cfg.maximum_epipolar_search_offset_pixels) == 0 and len(tracked) == fi.n_tracked and not fi.track_broken
    kp = np.asarray(points["kp"]).astype(np.int64)
    n_occupants = fi.n_points - fi.n_new_stereo
    (xyL, _, dL), (xyR, _, dR) = keypoints
    xyL, xyR, tracked = xyL.astype(np.int64), xyR.astype(np.int64), np.asarray(tracked).astype(np.int64)
    cols = int(cfg.cols)
    assert np.isin(kp[:fi.n_after_prune, 1] * cols + kp[:fi.n_after_prune, 0], tracked[:, 1] * cols + tracked[:, 0]).all()      # the survivors are among them
    keepL = ~np.isin(xyL[:, 1] * cols + xyL[:, 0], tracked[:, 1] * cols + tracked[:, 0])
    keepR = np.ones(len(xyR), bool)
    for xl, _, xr, yr in tracked:
        keepR &= ~((xyR[:, 1] == yr) & (xyR[:, 0] >= xr) & (xyR[:, 0] < xl))
    order = lambda xy: np.lexsort((xy[:, 0], xy[:, 1]))            # row-major, as the sweep wants its lists
    iL, iR = np.nonzero(keepL)[0], np.nonzero(keepR)[0]
    iL, iR = iL[order(xyL[iL])], iR[order(xyR[iR])]
    sweep = cfg.copy()
    sweep.enable_keypoint_binning = 0
    lib.cfg = sweep
    matches = lib.stereo_match(fi.tau_triangulation, xyL[iL][:, ::-1], dL[iL], xyR[iR][:, ::-1], dR[iR], cap=len(iL) + 1)
    cand = np.hstack([xyL[iL[matches[:, 0]]], xyR[iR[matches[:, 1]]]])         # xL yL xR yR, sweep order
    bins = bin_of_pixel(cfg, cand[:, 0], cand[:, 1])
    occupied = np.unique(bin_of_pixel(cfg, kp[:n_occupants, 0], kp[:n_occupants, 1]))
    turned_away = np.isin(bins, occupied)
    # the competition among the others (bin_takes), winners in bin order: what the frame must have appended
    grid = {}
    for q in np.nonzero(~turned_away)[0]:
        disp, dist, k = int(cand[q, 0] - cand[q, 2]), int(matches[q, 2]), int(bins[q])
        if k not in grid or (disp > grid[k][0] and dist <= grid[k][1]):
            grid[k] = (disp, dist, q)
    np.testing.assert_array_equal(cand[[grid[k][2] for k in sorted(grid)]].reshape(-1, 4), kp[n_occupants:])
    return int(turned_away.sum()), len(cand)


def assert_bin5_premises(lib, cfg, frames, tag):
    """frames: (frame_info, keypoints of both sides, points, the oracle's tracked keypoints) per frame.  CPU: 4160 .. 4322 left keypoints, 1578 .. 1764
    points, 373 .. 590 tracked points"""
    rows, cols = int(cfg.rows), int(cfg.cols)
    assert rc.bin_table_form(rows, cols, 5, 0) == "u16 lds"      # 76 x 249 bins: the 32-bit tables cannot fit at any count, the 16-bit ones up to ~6.9 k candidates
    for k, (fi, keypoints, points, tracked) in enumerate(frames):
        assert fi.error_flags == 0 and int(cfg.bin_size_pixels) == 5
        # at most one candidate per left keypoint (see assert_hbm_bin_table_with_tracked_occupants): the form at n_keypoints_left bounds the frame's
        assert rc.bin_table_form(rows, cols, 5, fi.n_keypoints_left) == "u16 lds", (tag, k, fi.n_keypoints_left)
        assert k == 0 or fi.n_tracked >= 300, (tag, k, fi.n_tracked)
        if k:
            turned_away, n_cand = contested_bins(lib, cfg, fi, keypoints, points, tracked)
            print("%s frame %d: %d candidates, %d of them in the bin of a tracked point" % (tag, k, n_cand, turned_away))
            assert turned_away >= 1, (tag, k)                        # CPU: 33 .. 61 per frame
    assert len(frames) == BIN5_FRAMES


# ---- CPU twin: the scenes still reach what the GPU tests are there for ----------------------------------------------------------------------------
def test_oracle_alone_reaches_the_dense_forms(recordings):
    from _oracle import Oracle
    lib = Oracle()
    cfg = config_of(lib, "dense")
    counts = [counts_of(fr["info"], fr["points"]) for fr in recordings("dense", 7)]
    assert_long_premises(cfg, counts, "oracle")
    assert_hbm_bin_table_with_tracked_occupants(cfg, counts, "oracle")
    cfg = config_of(lib, "bin 5")
    assert_bin5_premises(lib, cfg, [(fr["info"], fr["keypoints"], fr["points"], fr["tracked"]) for fr in recordings("bin 5", 7)], "oracle")


def test_oracle_alone_is_over_capacity_on_both_streams(recordings):
    """The scale at which the two-stream and stage-path cases reach the unlisted branch."""
    for seed in (7, 9):
        counts = [counts_of(fr["info"], fr["points"]) for fr in recordings("dense 1.25", seed)]
        assert_short_premises("dense 1.25", counts, "oracle seed %d" % seed)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------
def run_both_launch_sequences(cfg, streams, n_frames, each_frame=None):
    """The recorded oracle against the library's launch sequence for this stream count (sequence 4: the refinement in workgroups of its own,
    lm_teams_body under k_tail_lm) and, forced through VSLAM_SPLIT as pipeline_compare.run_sequence does, the single fused launch
    (wg_landmarks_lds in the frame workgroup), after every frame.  Returns counts_of per runner, stream and frame."""
    o = Replay(streams)
    runners = [create_hip(cfg, len(streams)), create_hip(cfg, len(streams), split=0)]
    counts = [[[] for _ in streams] for _ in runners]
    try:
        for k in range(n_frames):
            L, R = images(streams, k)
            for r, g in enumerate(runners):
                g.process_host(L, R)
                for s in range(len(streams)):
                    compare_frame(o.at(k), g, s, k, tag="runner %d" % r)
                    counts[r][s].append(counts_of(g.frame_info(s), g.points(s)))
                if each_frame:
                    each_frame(r, k, g)
    finally:
        for g in runners:
            g.destroy()
    return counts


@gpu
def test_unlisted_landmark_pass_long_tracks(recordings):
    from _oracle import Oracle
    cfg = config_of(Oracle(), "dense")
    for r, per_stream in enumerate(run_both_launch_sequences(cfg, [recordings("dense", 7)], LONG_FRAMES)):
        assert_long_premises(cfg, per_stream[0], "runner %d" % r)
        assert_hbm_bin_table_with_tracked_occupants(cfg, per_stream[0], "runner %d" % r)


STAGE_FIELDS = ("n_keypoints_left", "n_keypoints_right", "n_tracked", "n_lost", "n_tracked_landmarks", "n_inliers", "n_outliers", "n_after_prune",
                "n_recovered", "n_active_landmarks", "n_new_stereo", "n_points", "window_pixels", "track_attempts", "error_flags", "tau_track")


@gpu
@pytest.mark.parametrize("case", ["dense", "dense 1.25"])
def test_unlisted_landmark_pass_two_streams_and_stage_path(recordings, case):
    """At scale 1.0 the landmark pass of these 12 frames stays below LIST_CAP (dense frames on two streams and through the stage path, not the
    unlisted branch); at scale 1.25 frames 5 .. 11 of both streams take it: the `s` and g / G indexing of k_tail_lm, and of k_stage / k_stage_lm."""
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import hip
    from vslam_pose_estimation_framework_amd.host_tracker import PoseTracker3D
    cfg = config_of(Oracle(), case)
    streams = [recordings(case, 7), recordings(case, 9)]
    # (a) two streams against the oracle under both launch sequences
    for r, per_stream in enumerate(run_both_launch_sequences(cfg, streams, SHORT_FRAMES)):
        for s, counts in enumerate(per_stream):
            assert_short_premises(case, counts, "%s runner %d stream %d" % (case, r, s))
    # (b) one stream through the stage calls, vslam_update_points (k_stage) and vslam_compute (k_stage_lm), bit for bit the fused context
    fused = create_hip(cfg, 1)
    staged = []
    for one_launch in (False, True):
        api = hip.load()
        api.create(cfg, 0, 1)
        staged.append((api, PoseTracker3D(api, one_launch_compute=one_launch)))
    try:
        counts = []
        for k in range(SHORT_FRAMES):
            L, R = images(streams[:1], k)
            fused.process_host(L, R)
            ff, pf = fused.frame_info(0), fused.points(0)
            counts.append(counts_of(ff, pf))
            for api, tracker in staged:
                tag = "%s one_launch=%s frame %d" % (case, tracker.one_launch_compute, k)
                fs = tracker.compute(L[0], R[0])
                for name in STAGE_FIELDS:
                    assert getattr(fs, name) == getattr(ff, name), (tag, name, getattr(fs, name), getattr(ff, name))
                assert tracker._status == ff.status, tag          # the host tracker owns the status on the stage path
                assert list(fs.camera_left_to_world) == list(ff.camera_left_to_world), tag
                np.testing.assert_array_equal(api.poses(0, k, 1), fused.poses(0, k, 1), err_msg=tag)
                ps = api.points(0)
                for key in ("kp", "meta", "cam", "lm"):
                    np.testing.assert_array_equal(ps[key], pf[key], err_msg=tag + " " + key)
        assert_short_premises(case, counts, case + " fused beside the stage path")
    finally:
        fused.destroy()
        for api, _ in staged:
            api.destroy()


@gpu
def test_bin_table_16bit_with_tracked_occupants(recordings):
    from _oracle import Oracle
    lib = Oracle()
    cfg = config_of(lib, "bin 5")
    recorded = recordings("bin 5", 7)
    seen = [[], []]
    run_both_launch_sequences(cfg, [recorded], BIN5_FRAMES, each_frame=lambda r, k, g: seen[r].append(
        (g.frame_info(0), (g.keypoints(0, 0), g.keypoints(0, 1)), g.points(0), recorded[k]["tracked"])))
    for r, frames in enumerate(seen):
        assert_bin5_premises(lib, cfg, frames, "runner %d" % r)
