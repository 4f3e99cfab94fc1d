"""GPU parity: libvslam_hip.so (through the C ABI) against the committed golden vectors and against the
CPU oracle on the same seeded synthetic stereo sequences.  Integer / byte / index results must be
bit-exact; poses within 1e-4 relative Frobenius (BASELINE.json north_star)."""
import ctypes as C

import numpy as np
import pytest

import parity_cases as pc
from vslam_pose_estimation_framework_amd import hip

pytestmark = pytest.mark.gpu

from pipeline_compare import POSE_RTOL, INT_FIELDS, compare_frame, run_sequence  # noqa: E402,F401


@pytest.fixture(scope="module")
def gpu():
    api = hip.load()
    api.create(api.default_config("kitti"), 0, 1)
    yield api
    api.destroy()


def test_knn2_golden(gpu, golden):
    pc.check_hamming_knn(gpu, golden["hamming"])


def test_fast_golden(gpu, golden):
    pc.check_fast(gpu, golden["fast"])


def test_brief_golden(gpu, golden):
    pc.check_brief(gpu, golden["brief"])


def test_aligner_golden(gpu, golden):
    # the device sums H,b in a tree order -> pose tolerance, discrete outputs must still agree
    pc.check_aligner(gpu, golden["aligner"], rtol_pose=1e-7)


def test_aligner_iteration_limits_vs_oracle(golden):
    from _oracle import Oracle
    pc.check_aligner_iteration_limits(hip.load, Oracle, golden["aligner"])


def test_aligner_stale_weights_golden(gpu, golden):
    pc.check_aligner_weights(gpu, golden["aligner_weights"], gpu.cfg)


def test_aligner_uvd_golden(gpu, golden):
    pc.check_aligner_uvd(gpu, golden["aligner_uvd"], rtol_pose=1e-7)


def test_depth_components_golden(gpu, golden):
    """RGB-D components (space map z-buffer, DepthFramePointGenerator::compute, midpoint triangulation) against the
    pure-Python fixture: bit-exact map / lists, then once more with the map left resident on the device."""
    pc.check_depth_components(gpu, golden["depth"])
    pc.check_depth_components(gpu, golden["depth"], resident_map=True)


def test_depth_track_golden(gpu, golden):
    """DepthFramePointGenerator::track (order-exact parallel resolution) against the pure-Python fixture."""
    pc.check_depth_track(gpu, golden["depth_track"])


def test_depth_edge_cases(gpu, golden):
    pc.check_depth_edge_cases(gpu, golden["depth"])


def test_landmark_update_golden(gpu, oracle, golden):
    """Landmark::update stand-alone: the numpy fixture (1e-9) and the oracle (bit for bit: same arithmetic, same order)."""
    g = golden["landmark"]
    w, u = pc.check_landmark_update(gpu, g, gpu.cfg)
    wo, uo = oracle.landmark_update(oracle.default_config("kitti"), g["offsets"], g["frame_of"], g["w2c"], g["c2w"], g["cam"], g["world"], g["updates"])
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_array_equal(w, wo)


def test_orb_components_golden(gpu, golden):
    """OrbDetector pieces (INTER_LINEAR pyramid level, Harris response, intensity-centroid angle, ORB::detect) against the
    numpy restatement: bytes exact, floats bit for bit."""
    pc.check_orb_components(gpu, golden["orb"])


def test_orb_descriptor_golden(gpu, golden):
    """ORB as descriptor extractor (fixed-point Gaussian + steered rBRIEF) against the numpy restatement, bytes exact."""
    pc.check_orb_descriptor(gpu, golden["orb_descriptor"])


def test_orb_edge_cases(gpu, golden):
    pc.check_orb_edge_cases(gpu, golden["orb"])


def test_depth_recover_golden(gpu, golden):
    """DepthFramePointGenerator::recoverPoints (projection gates, BRIEF at the rounded ROI, descriptor gate)."""
    pc.check_depth_recover(gpu, golden["depth_recover"])


def test_track_golden(golden):
    """vslam_track_match (k_track_candidates + the order-exact resolution of the frame kernel) against the fixture of
    the independent numpy restatement of StereoFramePointGenerator::track: exact tuples, exact lost list."""
    g = golden["track"]
    api = hip.load()
    cfg = api.default_config("kitti")
    cfg.rows, cfg.cols = int(g["rows"]), int(g["cols"])
    for i in range(9):
        cfg.K[i] = float(g["K"].reshape(-1)[i])
    for i in range(3):
        cfg.baseline_h[i] = float(g["bh"][i])
    cfg.minimum_disparity_pixels = 1.0
    cfg.max_keypoints, cfg.max_points, cfg.max_history_frames = 256, 128, 2
    api.create(cfg, 0, 1)
    total = 0
    for k in range(int(g["n_cases"])):
        key = "c%d_" % k
        tracked, lost = api.track_match(g[key + "T"], int(g[key + "d"]), float(g[key + "tau_track"]), float(g[key + "tau_tri"]),
                                        int(g[key + "by_app"]), g[key + "cam"], g[key + "pdL"], g[key + "pdR"], g[key + "epi"],
                                        g[key + "rcL"], g[key + "dL"], g[key + "rcR"], g[key + "dR"])
        np.testing.assert_array_equal(tracked, g[key + "tracked"], err_msg="case %d tracked" % k)
        np.testing.assert_array_equal(lost, g[key + "lost"], err_msg="case %d lost" % k)
        total += len(tracked)
    assert total > 100
    api.destroy()


def test_stereo_sweep_golden(golden):
    """vslam_stereo_match (k_stereo_dist + the suffix-argmin sweep of the frame kernel) against the fixture of the
    independent numpy restatement of StereoFramePointGenerator::compute: ties, ordering constraint, minimum disparity
    without cursor advance, multi-offset pruning — exact (left, right, distance, offset) rows in emission order."""
    g = golden["stereo"]
    for name in ("hand", "random"):
        for epi in (0, 1):
            api = hip.load()
            cfg = api.default_config("kitti")
            cfg.rows, cfg.cols = 128, 640
            cfg.enable_keypoint_binning = 0
            cfg.maximum_epipolar_search_offset_pixels = epi
            cfg.max_keypoints, cfg.max_points, cfg.max_history_frames = 512, 512, 2
            api.create(cfg, 0, 1)
            out = api.stereo_match(float(g[name + "_tau"]), g[name + "_rcL"], g[name + "_dL"], g[name + "_rcR"], g[name + "_dR"])
            np.testing.assert_array_equal(out, g["%s_epi%d_matches" % (name, epi)], err_msg="%s epi %d" % (name, epi))
            api.destroy()


def _recover_ctx(load, g, descriptor_type=0):
    api = load()
    cfg = api.default_config("kitti")
    cfg.rows, cfg.cols = g["imgL"].shape
    for i in range(9):
        cfg.K[i] = float(g["K"].ravel()[i])
    for i in range(3):
        cfg.baseline_h[i] = float(g["bh"][i])
    cfg.descriptor_type = descriptor_type
    cfg.max_keypoints, cfg.max_points, cfg.max_history_frames = 256, 256, 2
    api.create(cfg, 0, 1)
    return api


def test_stereo_recover_golden(golden):
    """vslam_stereo_recover (wg_recover of the frame kernel: projection, depth / border gates, BRIEF from LDS-staged box patches,
    three descriptor gates, minimum disparity, triangulation) against the fixture of the independent pure-Python restatement of
    StereoFramePointGenerator::recoverPoints: exact rows, coordinates bit for bit."""
    g = golden["stereo_recover"]
    api = _recover_ctx(hip.load, g)
    for rep in range(2):   # second call: pooled scratch context
        r = api.stereo_recover(g["imgL"], g["imgR"], g["w2c"], g["has_lm"], g["lm"], g["pdL"], g["pdR"], float(g["tau_track"]), float(g["tau_tri"]))
        assert len(r["index"]) == len(g["rec_index"]) > 20
        np.testing.assert_array_equal(r["index"], g["rec_index"])
        np.testing.assert_array_equal(r["xy4"], g["rec_xy4"])
        np.testing.assert_array_equal(r["dist"], g["rec_dist"])
        np.testing.assert_array_equal(r["desc"], g["rec_desc"])
        np.testing.assert_array_equal(r["xyz"], g["rec_xyz"])
    # nothing to recover / no landmark at all
    none = api.stereo_recover(g["imgL"], g["imgR"], g["w2c"], np.zeros(0, np.uint8), np.zeros((0, 3)), np.zeros((0, 32), np.uint8),
                              np.zeros((0, 32), np.uint8), 35.0, 60.0)
    assert len(none["index"]) == 0
    nolm = api.stereo_recover(g["imgL"], g["imgR"], g["w2c"], np.zeros_like(g["has_lm"]), g["lm"], g["pdL"], g["pdR"], 35.0, 60.0)
    assert len(nolm["index"]) == 0
    api.destroy()


def test_stereo_recover_orb_vs_oracle(golden):
    """The same entry with the ORB extractor (steered tests on the 7 x 7 Gaussian image, keypoint angle -1): HIP against the
    oracle on the fixture's scene with descriptors re-made for ORB; loose gates so that every geometric survivor is compared."""
    from _oracle import Oracle
    g = golden["stereo_recover"]
    hp = _recover_ctx(hip.load, g, 1)
    orc = _recover_ctx(Oracle, g, 1)
    rng = np.random.default_rng(5)
    # previous descriptors: ORB descriptors of the true projections, a few bits flipped
    first = orc.stereo_recover(g["imgL"], g["imgR"], g["w2c"], g["has_lm"], g["lm"], g["pdL"], g["pdR"], 256.0, 256.0)
    assert len(first["index"]) > 60
    pdL, pdR = np.array(g["pdL"]), np.array(g["pdR"])
    for k, i in enumerate(first["index"]):
        for side, dst in ((0, pdL), (1, pdR)):
            bits = np.unpackbits(first["desc"][k, 32 * side:32 * side + 32])
            bits[rng.choice(256, size=int(rng.integers(0, 50)), replace=False)] ^= 1
            dst[i] = np.packbits(bits)
    for tau_track, tau_tri in ((35.0, 70.0), (256.0, 256.0), (20.0, 40.0)):
        a = hp.stereo_recover(g["imgL"], g["imgR"], g["w2c"], g["has_lm"], g["lm"], pdL, pdR, tau_track, tau_tri)
        b = orc.stereo_recover(g["imgL"], g["imgR"], g["w2c"], g["has_lm"], g["lm"], pdL, pdR, tau_track, tau_tri)
        for key in ("index", "xy4", "dist", "desc", "xyz"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="%s at tau %g" % (key, tau_track))
    assert 5 < len(hp.stereo_recover(g["imgL"], g["imgR"], g["w2c"], g["has_lm"], g["lm"], pdL, pdR, 35.0, 70.0)["index"]) < len(first["index"])
    hp.destroy(); orc.destroy()


def test_harness_record(golden):
    """The committed 30-frame record of the whole harness (per-frame counters, thresholds, descriptor distance, poses):
    the HIP path against fixture DATA, no oracle in the loop (the oracle library only renders the images)."""
    import os, sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_harness as mh
    from _oracle import Oracle
    g = golden["harness"]
    counters, thr, tau, poses = mh.run(hip.load, Oracle())
    np.testing.assert_array_equal(counters, g["counters"])
    np.testing.assert_array_equal(thr, g["thresholds"])
    np.testing.assert_array_equal(tau, g["tau_track"])
    for k in range(len(poses)):
        assert np.linalg.norm(poses[k] - g["poses"][k]) / np.linalg.norm(g["poses"][k]) <= POSE_RTOL


def test_pipeline_parity_half_resolution():
    from _oracle import Oracle
    run_sequence(Oracle, dict(scale=0.5), 14)


def test_pipeline_parity_three_streams():
    from _oracle import Oracle
    run_sequence(Oracle, dict(scale=0.4), 8, n_streams=3, seeds=[11, 12, 13])


def test_pipeline_parity_full_resolution_kitti():
    from _oracle import Oracle
    run_sequence(Oracle, dict(scale=1.0), 6)


def test_pipeline_parity_long_run_history_ring():
    # 100 frames at 0.6 scale with a 64-frame history ring: the ring's slots are reused (frame f lives in slot f % 64), but at this
    # scene's speed the longest track has 40 measurements, so no track outgrows the ring, nothing is truncated, error bit 4 stays down
    # and the refinement never leaves its staged pose window (48 frames).  The window and the tracking distance settle, recovery and
    # landmark refinement run — every frame compared in full.  Tracks beyond 33 / 48 / the ring: test_pipeline_parity_slow_scene_long_tracks
    # below (oracle parity, where it is valid) and tests/test_landmark_refinement_gpu.py (a reference that models the ring).
    from _oracle import Oracle

    def edit(cfg):
        cfg.max_history_frames = 64
    run_sequence(Oracle, dict(scale=0.6), 100, cfg_edit=edit)


def test_pipeline_parity_slow_scene_long_tracks():
    # The street scene at a sixth of the default speed: features stay in view for the whole run, so tracks pass the team threshold (9
    # measurements), the predecessor trail (33) and the staged pose window (48) of the fused landmark refinement.  The ring holds 128
    # frames: nothing is truncated, and the oracle — which keeps every measurement — is a valid reference for every frame.  90 frames:
    # the oracle alone shows 12 points with an updated landmark of 49 or more measurements on frame 89 (3 on frame 109: the long
    # tracks leave the image one after the other).
    from _oracle import Oracle

    def edit(cfg):
        cfg.max_history_frames = 128

    def after(o, g):
        for api in (o, g):
            m = api.points(0)["meta"]
            n_long = int(((m[:, 3] + 1 >= 49) & (m[:, 4] >= 49)).sum())
            assert n_long >= 8, n_long
        assert g.frame_info(0).error_flags == 0
    run_sequence(Oracle, dict(scale=0.4, speed_m=0.15), 90, cfg_edit=edit, after=after)


def test_pipeline_parity_large_image():
    # 1613 x 489 (scale 1.3): four mask passes in k_emit, rows with more than 16 keypoints (stereo windows slide), more
    # than 4000 keypoints per image, tiles of every border class
    from _oracle import Oracle

    def edit(cfg):
        cfg.max_keypoints, cfg.max_points = 16384, 8192
    run_sequence(Oracle, dict(scale=1.3), 5, cfg_edit=edit)


@pytest.mark.parametrize("seed,scale,bin_px,epi,binning,recovery", [
    (31, 0.45, 11, 0, 1, 1), (32, 0.7, 22, 3, 1, 1), (33, 0.55, 15, 1, 0, 1), (34, 0.5, 9, 2, 1, 0), (35, 0.62, 30, 0, 0, 0)])
def test_pipeline_parity_config_sweep(seed, scale, bin_px, epi, binning, recovery):
    # different scenes, image sizes, bin grids, epipolar search depths, with / without binning and landmark recovery
    from _oracle import Oracle

    def edit(cfg):
        cfg.bin_size_pixels = bin_px
        cfg.maximum_epipolar_search_offset_pixels = epi
        cfg.enable_keypoint_binning = binning
        cfg.enable_landmark_recovery = recovery
    run_sequence(Oracle, dict(scale=scale), 9, cfg_edit=edit, seeds=[seed])


def test_pipeline_parity_standstill_and_fallback():
    # zero motion: the aligner result is below the movement thresholds -> _fallbackEstimate path
    from _oracle import Oracle
    run_sequence(Oracle, dict(scale=0.4, speed_m=0.0, sway_m=0.0), 5)


def test_pipeline_parity_epipolar_offsets_no_binning():
    from _oracle import Oracle

    def edit(cfg):
        cfg.maximum_epipolar_search_offset_pixels = 2
        cfg.enable_keypoint_binning = 0
    run_sequence(Oracle, dict(scale=0.4), 6, cfg_edit=edit)


def test_pipeline_parity_euroc_grid():
    # 2x2 detector grid with overlapping regions and per-region thresholds (configuration_euroc.yaml)
    from _oracle import Oracle

    def edit(cfg):
        d = Oracle().default_config("euroc")
        for name in ("det_rows", "det_cols", "detector_threshold_minimum", "detector_threshold_maximum",
                     "detector_threshold_maximum_change", "bin_size_pixels", "minimum_descriptor_distance_tracking",
                     "maximum_descriptor_distance_tracking", "maximum_reliable_depth_meters", "maximum_depth_meters",
                     "maximum_matching_distance_triangulation", "minimum_track_length_for_landmark_creation",
                     "good_tracking_ratio", "aligner_damping"):
            setattr(cfg, name, getattr(d, name))
    run_sequence(Oracle, dict(scale=0.5, speed_m=0.3), 8, cfg_edit=edit)


def test_stage_api_equals_fused_path_and_oracle():
    """The reference's plug-in virtuals one C call each (vslam_frame_begin / vslam_track / vslam_align /
    vslam_prune_recover / vslam_update_points / vslam_stereo_new), driven by the host-side PoseTracker3D mirror,
    give the same frames as the fused device path and as the oracle."""
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd.host_tracker import PoseTracker3D
    o = Oracle()
    sc = o.scene_kitti(scale=0.5, seed=21)
    cfg = o.config_for_scene(sc)
    o.create(cfg, 0, 1)
    fused = hip.load()
    fused.create(cfg, 0, 1)
    staged = hip.load()
    staged.create(cfg, 0, 1)
    tracker = PoseTracker3D(staged)
    try:
        for k in range(12):
            L, R = o.render(sc, k)
            o.process_host(L, R)
            fused.process_host(L, R)
            fs = tracker.compute(L, R)
            ff, fo = fused.frame_info(0), o.frame_info(0)
            for name in ("status", "n_keypoints_left", "n_keypoints_right", "n_tracked", "n_lost", "n_tracked_landmarks",
                         "n_inliers", "n_outliers", "n_after_prune", "n_recovered", "n_active_landmarks", "n_new_stereo",
                         "n_points", "window_pixels", "track_attempts"):
                assert getattr(fs, name) == getattr(ff, name) == getattr(fo, name), (k, name, getattr(fs, name), getattr(ff, name), getattr(fo, name))
            assert fs.tau_track == ff.tau_track
            assert list(fs.camera_left_to_world) == list(ff.camera_left_to_world)
            ps, pf = staged.points(0), fused.points(0)
            for key in ("kp", "meta", "cam", "lm"):
                np.testing.assert_array_equal(ps[key], pf[key])
            np.testing.assert_array_equal(ps["kp"], o.points(0)["kp"])
    finally:
        staged.destroy()
        fused.destroy()
        o.destroy()


def test_stage_views_equal_the_array_getters_after_every_stage():
    """vslam_view_keypoints / _track / _aligner / _points (one packed report per stage in pinned memory, the flag polled) against the
    array-by-array getters, after every stage call of every frame: first frame through the stand-alone report kernel (no report buffer
    yet), later frames through the report folded into the stage kernel; a view of a stage that was not the last thing launched falls
    back to packing it on demand.  (vslam_compute, the one-launch form of update + stereo, is what tests/cpp/test_shim.cpp drives.)"""
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd.host_tracker import PoseTracker3D
    o = Oracle()
    sc = o.scene_kitti(scale=0.5, seed=33)
    cfg = o.config_for_scene(sc)
    a = hip.load(); a.create(cfg, 0, 1)          # driven with views checked after every stage, compute() as one launch
    ref = hip.load(); ref.create(cfg, 0, 1)      # the plain stage sequence
    checked = {"begin": 0, "track": 0, "align": 0, "prune": 0, "compute": 0}
    early = {"seen": 0}

    class Checked(PoseTracker3D):
        def compute(self, left, right):
            api = self.api
            real_fn = api.fn

            def fn(name):
                f = real_fn(name)
                if name not in ("frame_begin", "track", "align", "prune_recover", "stereo_new"):
                    return f

                def call(*args):
                    rc = f(*args)
                    assert rc == 0, (name, rc, api.last_error(api.ctx))
                    if name == "frame_begin":
                        e = api.view_keypoints_xy(0)         # coordinates and scores first (early report once the report buffer exists)
                        v = api.view_keypoints(0)
                        for side in (0, 1):
                            np.testing.assert_array_equal(e[side][0], v[side][0]); np.testing.assert_array_equal(e[side][1], v[side][1])
                        early["seen"] += 0 if e[0][2] else 1
                        for side in (0, 1):
                            xy, sc8, d = api.keypoints(0, side)
                            np.testing.assert_array_equal(v[side][0], xy); np.testing.assert_array_equal(v[side][1], sc8); np.testing.assert_array_equal(v[side][2], d)
                        checked["begin"] += 1
                    elif name == "track":
                        v = api.view_track(0)
                        cap = int(self.cfg.max_points)
                        nt, nl = C.c_int32(), C.c_int32()
                        out4 = np.zeros((cap, 4), np.int32); lost = np.zeros(cap, np.int32)
                        api.check(real_fn("get_track_result")(api.ctx, C.c_int(0), C.c_int32(cap), C.byref(nt), out4.ctypes.data_as(C.c_void_p), C.byref(nl), lost.ctypes.data_as(C.c_void_p)))
                        np.testing.assert_array_equal(v["tracked4"], out4[:nt.value]); np.testing.assert_array_equal(v["lost"], lost[:nl.value])
                        assert v["n_tracked_landmarks"] == api.frame_info(0).n_tracked_landmarks
                        checked["track"] += 1
                    elif name == "align":
                        v = api.view_aligner(0)
                        g = api.aligner_result(0)
                        np.testing.assert_array_equal(v["chi"], g["chi"]); np.testing.assert_array_equal(v["inlier"], g["inlier"])
                        np.testing.assert_array_equal(v["T"], g["T"]); np.testing.assert_array_equal(v["H"], g["H"])
                        fi = api.frame_info(0)
                        assert (v["n_inliers"], v["n_outliers"], v["iterations"], v["converged"], v["total_error"]) == (fi.n_inliers, fi.n_outliers, fi.aligner_iterations, fi.aligner_converged, fi.total_error)
                        checked["align"] += 1
                    elif name == "prune_recover":
                        v = api.view_points(0, in_progress=True)
                        g = _frame_points(api, 1)
                        f0 = v["first_full"]
                        assert v["n"] == len(g["kp"]) and f0 == api.frame_info(0).n_after_prune
                        np.testing.assert_array_equal(v["kp"], g["kp"])
                        for key in ("meta", "cam", "desc"):                 # the recovered points behind the survivors
                            np.testing.assert_array_equal(v[key][f0:], g[key][f0:])
                        checked["prune"] += 1
                    elif name == "stereo_new":
                        v = api.view_points(0)
                        g = _frame_points(api, 0)
                        assert v["n"] == len(g["kp"]) and v["first_full"] == 0 and v["desc"] is None
                        for key in ("kp", "meta", "cam"):
                            np.testing.assert_array_equal(v[key], g[key])
                        assert bytes(v["info"]) == bytes(api.frame_info(0))
                        # a view of another stage than the one last launched: packed on demand, same content
                        w = api.view_keypoints(0)
                        np.testing.assert_array_equal(w[0][0], api.keypoints(0, 0)[0])
                        checked["compute"] += 1
                    return 0
                return call
            api.fn = fn
            try:
                return super().compute(left, right)
            finally:
                api.fn = real_fn

    def _frame_points(api, in_progress):
        cap = int(api.cfg.max_points)
        n = C.c_int32()
        kp = np.zeros((cap, 4), np.int16); meta = np.zeros((cap, 6), np.int32); cam = np.zeros((cap, 3), np.float64); desc = np.zeros((cap, 64), np.uint8)
        api.check(api.fn("get_frame_points")(api.ctx, C.c_int(0), C.c_int(in_progress), C.c_int32(cap), C.byref(n), kp.ctypes.data_as(C.c_void_p), meta.ctypes.data_as(C.c_void_p),
                                             cam.ctypes.data_as(C.c_void_p), None, desc.ctypes.data_as(C.c_void_p)))
        k = n.value
        return dict(kp=kp[:k], meta=meta[:k], cam=cam[:k], desc=desc[:k])

    ta, tr = Checked(a), PoseTracker3D(ref)
    try:
        for k in range(10):
            L, R = o.render(sc, k)
            fa, fr = ta.compute(L, R), tr.compute(L, R)
            assert bytes(fa) == bytes(fr), k                  # reading views changes nothing
            pa, pr = a.points(0), ref.points(0)
            for key in ("kp", "meta", "cam", "lm"):
                np.testing.assert_array_equal(pa[key], pr[key])
        assert checked["begin"] == 10 and checked["compute"] == 10 and checked["track"] >= 9 and checked["align"] >= 7 and checked["prune"] == 9, checked
        assert early["seen"] >= 8, early          # from the second frame on the coordinates came through the early report (no descriptors with it)
    finally:
        a.destroy(); ref.destroy(); o.destroy()


@pytest.mark.parametrize("capacities", [None, (1001, 777)])
def test_stage_views_of_any_stream_of_a_multi_stream_context(capacities):
    """The report buffer holds one stream at a time and the folded report is stream 0's: views of the other streams of a three-stream
    context are packed on demand and equal the getters; setters of a multi-stream context are applied at once (no folding).  With
    odd capacities the per-stream arrays start at addresses that are not 16 B aligned: the report kernel copies in narrower units."""
    from _oracle import Oracle
    o = Oracle()
    scenes = [o.scene_kitti(scale=0.4, seed=50 + i) for i in range(3)]
    cfg = o.config_for_scene(scenes[0])
    if capacities:
        cfg.max_keypoints, cfg.max_points = capacities
    g = hip.load(); g.create(cfg, 0, 3)
    try:
        for k in range(3):
            imgs = [o.render(sc, k) for sc in scenes]
            L = np.ascontiguousarray(np.stack([im[0] for im in imgs])); R = np.ascontiguousarray(np.stack([im[1] for im in imgs]))
            g.check(g.fn("frame_begin")(g.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]), C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
            for s in (2, 0, 1):
                v = g.view_keypoints(s)
                for side in (0, 1):
                    xy, sc8, d = g.keypoints(s, side)
                    assert len(xy) > 100
                    np.testing.assert_array_equal(v[side][0], xy); np.testing.assert_array_equal(v[side][1], sc8); np.testing.assert_array_equal(v[side][2], d)
            if k:
                g.check(g.fn("track")(g.ctx, C.c_int(1)))
                g.check(g.fn("prune_recover")(g.ctx))
            g.check(g.fn("compute")(g.ctx))
            for s in (1, 2, 0):
                v = g.view_points(s)
                p = g.points(s)
                assert v["n"] == len(p["kp"]) > 50
                np.testing.assert_array_equal(v["kp"], p["kp"]); np.testing.assert_array_equal(v["meta"], p["meta"]); np.testing.assert_array_equal(v["cam"], p["cam"])
                assert bytes(v["info"]) == bytes(g.frame_info(s))
    finally:
        g.destroy(); o.destroy()


def test_host_images_pageable_staged_and_pinned_direct_give_the_same_frames():
    """vslam_process_host from ordinary memory (small source: staged through pinned memory of the context, the left image's DMA running while the
    right one is staged) and from vslam_host_alloc memory (copied to the device directly): same frames, and both equal the oracle's."""
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=0.5, seed=91)
    cfg = o.config_for_scene(sc)
    o.create(cfg, 0, 1)
    a = hip.load(); a.create(cfg, 0, 1)
    b = hip.load(); b.create(cfg, 0, 1)
    n = cfg.rows * cfg.cols
    pins = []
    for _ in range(4):                                   # two frames in flight at most: [parity][side]
        p = C.c_void_p()
        assert b.lib.vslam_host_alloc(C.byref(p), C.c_size_t(n)) == 0 and p.value
        pins.append(p)
    try:
        for k in range(8):
            L, R = o.render(sc, k)
            o.process_host(L, R)
            a.process_host(L, R)                         # numpy arrays: pageable
            pl, pr = pins[2 * (k & 1)], pins[2 * (k & 1) + 1]
            C.memmove(pl, L.ctypes.data, n); C.memmove(pr, R.ctypes.data, n)
            b.check(b.fn("process_host")(b.ctx, pl, pr, C.c_int32(cfg.cols), C.c_size_t(n)))
            compare_frame(o, a, 0, k, "pageable host images")
            compare_frame(a, b, 0, k, "pinned host images", identical=True)
        assert a.frame_info(0).status == 1
    finally:
        a.destroy(); b.destroy(); o.destroy()
        for p in pins:
            hip.load().lib.vslam_host_free(p)


def test_stage_call_before_frame_begin_is_an_error():
    from vslam_pose_estimation_framework_amd.capi import VslamError, ERR_STATE
    api = hip.load()
    api.create(api.default_config("kitti"), 0, 1)
    try:
        rc = api.fn("track")(api.ctx, 1)
        assert rc == ERR_STATE
        assert "before vslam_frame_begin" in api.last_error(api.ctx)
        rc = api.fn("process_host")(api.ctx, None, None, 1280, 0)
        assert rc == -1 and "empty frame" in api.last_error(api.ctx)   # the reference throws "called with empty frame"
    finally:
        api.destroy()


def _pair_compare(o, g, L, R, k, tag):
    o.process_host(L, R)
    g.process_host(L, R)
    compare_frame(o, g, 0, k, tag)


def test_degenerate_inputs_blank_noise_and_scene_cut():
    """Edge cases the reference would meet in the wild: featureless frames (no keypoints, no points), pure noise
    (keypoints everywhere, no stereo matches), a scene cut (nothing tracks -> recursive registration -> breakTrack),
    then recovery on normal frames.  Everything must stay identical to the oracle and raise no capacity flags."""
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=0.4, seed=9)
    sc2 = o.scene_kitti(scale=0.4, seed=1234)
    cfg = o.config_for_scene(sc)
    o.create(cfg, 0, 1)
    g = hip.load()
    g.create(cfg, 0, 1)
    rng = np.random.default_rng(5)
    try:
        blank = np.full((cfg.rows, cfg.cols), 77, np.uint8)
        k = 0
        for _ in range(2):
            _pair_compare(o, g, blank, blank, k, "blank"); k += 1
        for f in range(4):
            _pair_compare(o, g, *o.render(sc, f), k, "normal"); k += 1
        noise = rng.integers(0, 256, (cfg.rows, cfg.cols), dtype=np.uint8)
        noise2 = rng.integers(0, 256, (cfg.rows, cfg.cols), dtype=np.uint8)
        _pair_compare(o, g, noise, noise2, k, "noise"); k += 1
        stale = False
        for f in range(3):
            _pair_compare(o, g, *o.render(sc2, 40 + f), k, "cut"); k += 1     # different world: track is lost
            fi = g.frame_info(0)
            if fi.status_at_start == 0 and fi.aligner_ran:
                # Localizing after the break: the aligner ran with inverse depth off on the weights the last Tracking frame left
                # behind (stereouv_aligner.cpp:22,57-61) -- not all ones
                stale = stale or bool((g.aligner_weights_of(0) != 1.0).any())
        assert stale
        _pair_compare(o, g, blank, blank, k, "blank-again"); k += 1
        for f in range(3):
            _pair_compare(o, g, *o.render(sc, 10 + f), k, "resume"); k += 1
        assert g.frame_info(0).error_flags == 0
    finally:
        g.destroy()
        o.destroy()


def test_keypoint_capacity_overflow_is_flagged_not_fatal():
    """A device buffer that is too small sets error_flags bit 0 and truncates; nothing is written out of bounds."""
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=0.4, seed=3)
    cfg = o.config_for_scene(sc)
    cfg.max_keypoints = 128
    cfg.max_points = 64
    g = hip.load()
    g.create(cfg, 0, 1)
    try:
        for f in range(4):
            g.process_host(*o.render(sc, f))
        fi = g.frame_info(0)
        assert fi.error_flags & 1
        assert fi.n_keypoints_left <= 128 and fi.n_points <= 64
        xy, score, desc = g.keypoints(0, 0)
        assert len(xy) == fi.n_keypoints_left
    finally:
        g.destroy()


def test_history_ring_shorter_than_tracks_is_flagged_not_fatal():
    """Tracks longer than max_history_frames: landmark refinement uses the newest ring-full of measurements, error_flags
    bit 2 (value 4) reports it, tracking carries on."""
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=0.5, seed=5)
    cfg = o.config_for_scene(sc)
    cfg.max_history_frames = 8
    g = hip.load()
    g.create(cfg, 0, 1)
    try:
        flagged = False
        for f in range(30):
            g.process_host(*o.render(sc, f))
            fi = g.frame_info(0)
            flagged = flagged or bool(fi.error_flags & 4)
        assert flagged
        assert fi.status == 1 and fi.n_tracked > 20 and np.isfinite(np.array(fi.camera_left_to_world)).all()
    finally:
        g.destroy()


def test_odd_image_geometry():
    """Image sizes that are not multiples of the 64x32 / 128x32 tiles, with a row stride larger than the width."""
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=0.37, seed=17)          # 139 x 459
    cfg = o.config_for_scene(sc)
    o.create(cfg, 0, 1)
    g = hip.load()
    g.create(cfg, 0, 1)
    try:
        for k in range(6):
            L, R = o.render(sc, k, stride=sc.cols + 13)
            o.process_host(L, R)
            g.process_host(L, R)
            compare_frame(o, g, 0, k, "odd")
    finally:
        g.destroy()
        o.destroy()


def test_rgbd_components_at_sensor_size_against_oracle(gpu, oracle):
    """640x480 depth frame, 1500 features, 700 previous points, 300 lost landmarks: every RGB-D entry point against the
    oracle (space map with a rotated / shifted depth camera, compute with binning, track in both modes, recovery)."""
    from vslam_pose_estimation_framework_amd.capi import DepthParams
    rng = np.random.default_rng(11)
    rows, cols, f = 480, 640, 525.0
    K = np.array([[f, 0, 319.5], [0, f, 239.5], [0, 0, 1]])
    Kl = np.array([[f * 0.98, 0, 321.0], [0, f * 0.98, 237.5], [0, 0, 1]])
    ang = 0.01
    r2l = np.hstack([np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]), np.array([[0.025], [0.0], [0.001]])])
    depth = rng.integers(500, 8000, (rows, cols)).astype(np.uint16)
    depth[rng.random((rows, cols)) < 0.1] = 0
    p = DepthParams.make(rows, cols, Kl, np.linalg.inv(Kl), np.linalg.inv(K), r2l, 1e-3, 0.1, 10.0, 1, 1, 10)
    sg, rg, cg = gpu.depth_space_map(p, depth)
    so, ro, co = oracle.depth_space_map(p, depth)
    assert np.array_equal(sg.view(np.uint32), so.view(np.uint32)) and np.array_equal(rg, ro) and np.array_equal(cg, co)
    flat = np.sort(rng.choice(rows * cols, 1500, replace=False))
    feats = np.stack([flat // cols, flat % cols], axis=1).astype(np.int32)
    fdesc = rng.integers(0, 256, (1500, 32), dtype=np.uint8)
    sel = rng.choice(1500, 700, replace=False)
    cam = np.zeros((700, 3)); pdesc = np.zeros((700, 32), np.uint8)
    for j, k in enumerate(sel):
        z = float(rng.uniform(0.8, 6.0)); r, c = feats[k] + rng.integers(-3, 4, 2)
        cam[j] = [(c - Kl[0, 2]) * z / Kl[0, 0], (r - Kl[1, 2]) * z / Kl[1, 1], z]
        bits = np.unpackbits(fdesc[k]); bits[rng.choice(256, int(rng.integers(0, 45)), replace=False)] ^= 1; pdesc[j] = np.packbits(bits)
    flags = (rng.random(700) < 0.6).astype(np.uint8) | ((rng.random(700) < 0.1).astype(np.uint8) << 1)
    a = gpu.depth_compute(p, None, feats, feats[sel[:200]]); b = oracle.depth_compute(p, so, feats, feats[sel[:200]])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for by_app, d in ((1, 12), (0, 7)):
        a = gpu.depth_track(p, None, np.eye(4)[:3], d, 35.0, by_app, cam, pdesc, flags, feats, fdesc)
        b = oracle.depth_track(p, so, np.eye(4)[:3], d, 35.0, by_app, cam, pdesc, flags, feats, fdesc)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4] and len(a[0]) > 300
    # rivals: many previous points want the same few features (candidate lists exhausted -> window rescans), and a block of
    # 81 identical features (more candidates than a list holds -> incomplete lists), both search modes
    D = rng.integers(0, 256, 32, dtype=np.uint8)
    blk = np.array([(r, c) for r in range(200, 209) for c in range(300, 309)], np.int32)
    few = np.array([(100, 100 + 2 * k) for k in range(10)], np.int32)
    cfeat = np.vstack([few, blk]); cdesc = np.tile(D, (len(cfeat), 1))
    zc = 2.0
    def at(r, c): return [(c - Kl[0, 2]) * zc / Kl[0, 0], (r - Kl[1, 2]) * zc / Kl[1, 1], zc]
    ccam = np.array([at(100.4, 109.3)] * 14 + [at(204.2, 304.6)] * 40)
    cpd = np.tile(D, (len(ccam), 1)); cfl = np.ones(len(ccam), np.uint8)
    for by_app, d in ((1, 10), (0, 10)):
        a = gpu.depth_track(p, None, np.eye(4)[:3], d, 35.0, by_app, ccam, cpd, cfl, cfeat, cdesc)
        b = oracle.depth_track(p, so, np.eye(4)[:3], d, 35.0, by_app, ccam, cpd, cfl, cfeat, cdesc)
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
        assert len(a[0]) + len(a[2]) + len(a[3]) >= 50          # every rival ends somewhere: tracked, temporary or lost
    img = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    lm = np.stack([rng.uniform(-2, 2, 300), rng.uniform(-1.5, 1.5, 300), rng.uniform(1.0, 6.0, 300)], axis=1)
    ld = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    a = gpu.depth_recover(p, None, img, np.eye(4)[:3], np.ones(300, np.uint8), lm, ld, 7.0, 140.0)
    b = oracle.depth_recover(p, so, img, np.eye(4)[:3], np.ones(300, np.uint8), lm, ld, 7.0, 140.0)
    assert len(a[0]) > 20 and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def test_orb_detect_at_kitti_size_against_oracle(gpu, oracle):
    """The reference's OrbDetector parameters (5000 features, 1.2, 8 levels, edge 31, patch 31) on a KITTI-sized synthetic
    frame: 5000 keypoints over 8 levels, GPU == oracle bit for bit (coordinates, size, angle, response, octave)."""
    scene = oracle.scene_kitti()
    left, _ = oracle.render(scene, 40)
    for thr in (20, 8):
        g = gpu.orb_detect(left, 5000, 1.2, 8, 31, 31, thr)
        o = oracle.orb_detect(left, 5000, 1.2, 8, 31, 31, thr)
        assert g.shape == o.shape and np.array_equal(g.view(np.uint32), o.view(np.uint32))
        assert len(g) >= 4000 and set(np.unique(g[:, 5]).astype(int)) == set(range(8))


def test_rgbd_chain_on_rendered_frames(gpu, oracle):
    """Two consecutive rendered frames (left image + depth of the synthetic street scene, half KITTI size) through the RGB-D
    entry points in the order a depth tracker calls them — space map, FAST + BRIEF, compute; next frame: track from the
    ground-truth motion (both search modes), recovery of the lost points — GPU against oracle at every step, all exact."""
    from vslam_pose_estimation_framework_amd.capi import DepthParams
    from vslam_pose_estimation_framework_amd import evaluation as ev
    scene = oracle.scene_kitti(scale=0.5)
    rows, cols = scene.rows, scene.cols
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    p = DepthParams.make(rows, cols, K, np.linalg.inv(K), np.linalg.inv(K), np.eye(4)[:3], 2e-3, 0.1, 80.0, 1, 1, 15)
    frames = []
    for k in (40, 41):
        left, _ = oracle.render(scene, k)
        depth = oracle.render_depth(scene, k, 2e-3)
        sg = gpu.depth_space_map(p, depth); so = oracle.depth_space_map(p, depth)
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(sg, so))
        xy_g, sc_g = gpu.fast_detect(left, (0, 0, cols, rows), 20); xy_o, sc_o = oracle.fast_detect(left, (0, 0, cols, rows), 20)
        assert np.array_equal(xy_g, xy_o) and np.array_equal(sc_g, sc_o) and len(xy_g) > 300
        keep_g, d_g = gpu.brief_describe(left, xy_g); keep_o, d_o = oracle.brief_describe(left, xy_o)
        assert np.array_equal(keep_g, keep_o) and np.array_equal(d_g, d_o)
        sel = keep_g.astype(bool)
        feats = np.stack([xy_g[sel, 1], xy_g[sel, 0]], axis=1).astype(np.int32)      # (row, col), row-major as FAST emits them
        frames.append(dict(left=left, space=so[0], feats=feats, desc=d_g[sel], c2w=oracle.gt_pose(scene, k)))
    f0, f1 = frames
    new_g = gpu.depth_compute(p, f0["space"], f0["feats"], np.zeros((0, 2), np.int32))
    new_o = oracle.depth_compute(p, f0["space"], f0["feats"], np.zeros((0, 2), np.int32))
    assert all(np.array_equal(a, b) for a, b in zip(new_g, new_o)) and len(new_g[0]) > 100
    idx, cam = new_g[0], new_g[1]                              # the previous frame's points: measured-depth points of frame 40
    pdesc = f0["desc"][idx]
    flags = np.ones(len(idx), np.uint8)
    T = ev.mul34(ev.inv34(f1["c2w"]), f0["c2w"])               # previous -> current camera, ground truth
    lost_all = None
    for by_app, d in ((1, 20), (0, 10)):
        a = gpu.depth_track(p, f1["space"], T, d, 40.0, by_app, cam, pdesc, flags, f1["feats"], f1["desc"])
        b = oracle.depth_track(p, f1["space"], T, d, 40.0, by_app, cam, pdesc, flags, f1["feats"], f1["desc"])
        assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]
        assert len(a[0]) > 0.3 * len(idx)                      # the scene is static and the motion exact: most points are found again
        lost_all = a[3]
    world = np.array([f0["c2w"][:, :3] @ c + f0["c2w"][:, 3] for c in cam[lost_all]]).reshape(-1, 3)
    w2c1 = ev.inv34(f1["c2w"])
    ra = gpu.depth_recover(p, f1["space"], f1["left"], w2c1, np.ones(len(lost_all), np.uint8), world, pdesc[lost_all], 7.0, 60.0)
    rb = oracle.depth_recover(p, f1["space"], f1["left"], w2c1, np.ones(len(lost_all), np.uint8), world, pdesc[lost_all], 7.0, 60.0)
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32))
    assert np.array_equal(ra[2], rb[2]) and np.array_equal(ra[3], rb[3])


def test_orb_describe_keypoints_against_oracle(gpu, oracle):
    """cv::ORB::compute on an OrbDetector's keypoints (pyramid level + own angle per keypoint) at KITTI size: keep flags and descriptor bytes
    GPU == oracle, all eight levels; border and octave edge cases."""
    from vslam_pose_estimation_framework_amd.capi import VslamError
    scene = oracle.scene_kitti()
    left, _ = oracle.render(scene, 40)
    kps = oracle.orb_detect(left, 5000, 1.2, 8, 31, 31, 12)
    extra = np.array([[5.0, 50.0, 31, 10, 1, 0], [600.4, 200.6, 31, 123.5, 1, 3], [45.0, 45.0, 31, 0, 1, 6], [1200.0, 340.0, 31, 359, 1, 1]], np.float32)
    both = np.concatenate([kps, extra])
    kg, dg = gpu.orb_describe_keypoints(left, both, 1.2)
    ko, do = oracle.orb_describe_keypoints(left, both, 1.2)
    np.testing.assert_array_equal(kg, ko)
    np.testing.assert_array_equal(dg, do)
    assert kg[:len(kps)].all() and list(kg[len(kps):]) == [0, 1, 0, 1] and set(np.unique(kps[:, 5]).astype(int)) == set(range(8))
    assert len(gpu.orb_describe_keypoints(left, np.zeros((0, 6), np.float32), 1.2)[0]) == 0
    with pytest.raises(VslamError):
        gpu.orb_describe_keypoints(left, np.array([[50, 50, 31, 0, 1, 16]], np.float32), 1.2)


def test_depth_track_with_features_sharing_a_pixel(gpu, oracle):
    """Several features on one pixel (an OrbDetector finds a corner on more than one pyramid level): setFeatures writes the lattice in list
    order, only the LAST one is ever found by track(), also after it has been taken (intensity_feature_matcher.cpp:48-70).  GPU == oracle
    with a third of the features duplicated in front of / behind their originals with other descriptors."""
    from vslam_pose_estimation_framework_amd.capi import DepthParams
    from vslam_pose_estimation_framework_amd import evaluation as ev
    scene = oracle.scene_kitti(scale=0.5)
    rows, cols = scene.rows, scene.cols
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    p = DepthParams.make(rows, cols, K, np.linalg.inv(K), np.linalg.inv(K), np.eye(4)[:3], 2e-3, 0.1, 80.0, 1, 1, 15)
    fr = []
    for k in (40, 41):
        left, _ = oracle.render(scene, k)
        space = oracle.depth_space_map(p, oracle.render_depth(scene, k, 2e-3))[0]
        xy, _ = oracle.fast_detect(left, (0, 0, cols, rows), 20)
        keep, d = oracle.brief_describe(left, xy)
        sel = keep.astype(bool)
        fr.append(dict(space=space, rc=np.stack([xy[sel, 1], xy[sel, 0]], axis=1).astype(np.int32), desc=d[sel], c2w=oracle.gt_pose(scene, k)))
    f0, f1 = fr
    idx, cam = oracle.depth_compute(p, f0["space"], f0["rc"], np.zeros((0, 2), np.int32))[:2]
    pdesc = f0["desc"][idx]; flags = np.ones(len(idx), np.uint8)
    T = ev.mul34(ev.inv34(f1["c2w"]), f0["c2w"])
    rng = np.random.default_rng(11)
    n = len(f1["rc"])
    dup = rng.choice(n, n // 3, replace=False)
    noise = rng.integers(0, 256, (len(dup), 32), dtype=np.uint8)
    for where in ("behind", "in front"):
        # behind: the original is written first and overwritten by a stranger's descriptor; in front: the original is the last one and wins
        if where == "behind":
            rc = np.concatenate([f1["rc"], f1["rc"][dup]]); desc = np.concatenate([f1["desc"], noise])
        else:
            rc = np.concatenate([f1["rc"][dup], f1["rc"]]); desc = np.concatenate([noise, f1["desc"]])
        perm = rng.permutation(len(rc)) if where == "behind" else np.arange(len(rc))
        if where == "behind":          # any list order: keep every duplicate behind its original
            order = np.argsort(np.concatenate([np.arange(n) * 2, dup * 2 + 1]), kind="stable")
            rc, desc = rc[order], desc[order]
        for by_app, d in ((1, 20), (0, 10)):
            a = gpu.depth_track(p, f1["space"], T, d, 40.0, by_app, cam, pdesc, flags, rc, desc)
            b = oracle.depth_track(p, f1["space"], T, d, 40.0, by_app, cam, pdesc, flags, rc, desc)
            assert all(np.array_equal(x, y) for x, y in zip(a[:4], b[:4])) and a[4] == b[4], (where, by_app)
            plain = oracle.depth_track(p, f1["space"], T, d, 40.0, by_app, cam, pdesc, flags, f1["rc"], f1["desc"])
            if where == "behind":
                assert len(b[0]) < len(plain[0])     # the overwritten originals cannot be found any more
            else:
                assert len(b[0]) == len(plain[0])    # the hidden strangers change nothing
