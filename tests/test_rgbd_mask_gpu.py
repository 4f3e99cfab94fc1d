"""The static detection mask in RGB-D mode (vslam_rgbd_set_detection_mask, csrc/kernels_mask.h): what lies under the mask
cannot matter — one sequence, the captured launch sequence, a batch of 3, with the map and the log on —, the same across a frame with
several registration attempts, the mask does change the detection, and the contract of the switch.  tum configuration at 188 x 620, 12
frames: the scenes of bilateral_cases.py (image and filtered depth), whose CPU premises test_bilateral_host.py holds."""
import ctypes as C

import numpy as np
import pytest

import bilateral_cases as bc
from test_undistort_gpu import _same_info, _same_points
from vslam_pose_estimation_framework_amd import hip, mask
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

MARGIN = 28          # >= the reach of either extractor (test_mask_gpu.brief_reach / orb_reach: 28 and 17)


@pytest.fixture(scope="module")
def worlds():
    seqs = [bc.sequence(seed) for seed in bc.SEEDS]
    return seqs[0]["cfg"], seqs[0]["p"], [[(L, F) for L, _, F, _ in s["frames"]] for s in seqs]


def blob_of(rows, cols):
    """A small ellipse in the upper left part and a strip along the bottom (the robot's own body)."""
    y, x = np.mgrid[0:rows, 0:cols]
    m = np.where(((x - 0.15 * cols) / (0.04 * cols)) ** 2 + ((y - 0.25 * rows) / (0.12 * rows)) ** 2 <= 1.0, 0, 255).astype(np.uint8)
    m[rows - 6:, cols // 3:2 * cols // 3] = 0
    return m


def noise_under(img, blob, rng):
    out = img.copy()
    zero = np.broadcast_to(blob == 0, img.shape)
    out[zero] = rng.integers(0, 256, int(zero.sum()), dtype=np.uint8)
    return out


def on_kept_pixels(points, keep):
    xy = np.rint(points["xy"]).astype(np.int64)
    return len(xy) > 0 and mask.filter_keypoints(xy, keep).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "one-graph", "batch3", "batch3-graph", "one-map"])
def test_pixels_under_the_mask_do_not_matter(case, worlds, monkeypatch):
    """Trackers A and B hold the same mask with a margin of the extractor's reach; B's images carry seeded noise on every zero-mask pixel.
    Frame info (poses in it), the complete point lists, the map and the log are equal bit for bit after every frame."""
    import test_mask_gpu as tm
    assert MARGIN >= tm.brief_reach() and MARGIN >= tm.orb_reach()
    cfg, p, frames = worlds
    cfg = cfg.copy()
    cfg.enable_landmark_recovery = 0
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case.endswith("graph") else "0")
    g = hip.load()
    B = 3 if case.startswith("batch3") else 1
    make = (lambda: RgbdTracker(g, cfg, p)) if B == 1 else (lambda: RgbdBatch(g, cfg, p, B))
    a, b, c = make(), make(), make()
    rows, cols = int(cfg.rows), int(cfg.cols)
    blob = blob_of(rows, cols)
    keep = mask.erode(blob != 0, MARGIN)
    rng = np.random.default_rng(5)
    try:
        for t in (a, b):
            t.set_detection_mask(blob, MARGIN)
            if case == "one-map":
                t.enable_map(6000); t.enable_observations(60000)
        fewer = 0
        for f in range(bc.N_FRAMES):
            L = np.stack([frames[s][f][0] for s in range(B)])
            D = np.stack([frames[s][f][1] for s in range(B)])
            Ln = noise_under(L, blob, rng)
            assert (Ln != L).any()
            if B == 1:
                ia, ib, ic = [a.process(L[0], D[0])], [b.process(Ln[0], D[0])], [c.process(L[0], D[0])]
                pa, pb = [a.points()], [b.points()]
            else:
                ia, ib, ic = a.process(L, D), b.process(Ln, D), c.process(L, D)
                pa, pb = [a.points(s) for s in range(B)], [b.points(s) for s in range(B)]
            for s in range(B):
                tag = "%s frame %d sequence %d" % (case, f, s)
                _same_info(ia[s][0], ib[s][0], tag)
                assert ia[s][1] == ib[s][1], tag
                _same_points(pa[s], pb[s], tag)
                assert on_kept_pixels(pa[s], keep), tag
                fewer += int(ia[s][0].n_detected_left < ic[s][0].n_detected_left)
            for t in (a, b):
                np.testing.assert_array_equal(t.detection_mask(), mask.pack(blob, MARGIN))
            if case == "one-map":
                np.testing.assert_array_equal(a.point_ids(), b.point_ids())
                ma, mb, oa, ob = a.map(), b.map(), a.observations(), b.observations()
                for k in ma:
                    np.testing.assert_array_equal(ma[k], mb[k], err_msg="map %s frame %d" % (k, f))
                for k in oa:
                    np.testing.assert_array_equal(oa[k], ob[k], err_msg="log %s frame %d" % (k, f))
        assert all(fi.status == 1 and fi.n_points >= 50 and fi.error_flags == 0 for fi, _ in ia)      # equal and tracking, not equal and empty
        assert fewer >= bc.N_FRAMES * B // 2, fewer              # the mask does remove detections: it is applied ahead of the count
        if case == "one-map":
            assert len(ma["id"]) > 30 and len(oa["id"]) > 100
    finally:
        a.destroy(); b.destroy(); c.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_mask_applies_to_every_registration_attempt(graph, monkeypatch):
    """The re-registration scenario (icl configuration, a jump from frame 8 to 16): every attempt's detection is masked again, so noise under
    the mask stays without effect across a frame with at least two attempts."""
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))
    sc = bc.reregistration()
    cfg, p = sc["cfg"].copy(), sc["p"]
    cfg.enable_landmark_recovery = 0
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    blob = blob_of(int(cfg.rows), int(cfg.cols))
    keep = mask.erode(blob != 0, MARGIN)
    rng = np.random.default_rng(6)
    try:
        for t in (a, b):
            t.set_detection_mask(blob, MARGIN)
        attempts = []
        for f, (L, _, F, _) in enumerate(sc["frames"]):
            (fa, na), (fb, nb) = a.process(L, F), b.process(noise_under(L, blob, rng), F)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            assert on_kept_pixels(a.points(), keep), f
            attempts.append(fa.track_attempts)
        assert max(attempts) >= 2, attempts
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_rgbd_mask_contract(worlds, monkeypatch):
    cfg, p, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    seq = frames[0]
    rows, cols = int(cfg.rows), int(cfg.cols)
    blob = blob_of(rows, cols)
    t, u = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        assert g.lib.vslam_rgbd_set_detection_mask(None, blob.ctypes.data_as(C.c_void_p), C.c_int32(cols), C.c_int32(0)) == ERR_INVALID
        with pytest.raises(VslamError) as e:                      # off
            t.detection_mask()
        assert e.value.code == ERR_STATE
        for stride, margin in ((cols - 1, 0), (cols, -1), (cols, 65)):
            assert g.lib.vslam_rgbd_set_detection_mask(t.h, blob.ctypes.data_as(C.c_void_p), C.c_int32(stride), C.c_int32(margin)) == ERR_INVALID
        # all-keep == no mask, bit for bit
        t.set_detection_mask(np.full((rows, cols), 9, np.uint8), 64)
        with pytest.raises(VslamError) as e:                      # on, but no frame yet
            t.detection_mask()
        assert e.value.code == ERR_STATE
        for f in range(3):
            (fa, na), (fb, nb) = t.process(*seq[f]), u.process(*seq[f])
            _same_info(fa, fb, "all-keep frame %d" % f); assert na == nb
            _same_points(t.points(), u.points(), "all-keep frame %d" % f)
        np.testing.assert_array_equal(t.detection_mask(), mask.all_keep(rows, cols))
        # in flight
        t.set_detection_mask(blob, 3)
        t.submit(*seq[3])
        for call in (lambda: t.set_detection_mask(None), lambda: t.set_detection_mask(blob, 1), t.detection_mask):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "in flight" in str(e.value)
        t.wait()
        np.testing.assert_array_equal(t.detection_mask(), mask.pack(blob, 3))
        # the mask survives reset(), the last frame is forgotten
        t.reset()
        with pytest.raises(VslamError) as e:
            t.detection_mask()
        assert e.value.code == ERR_STATE
        fi, _ = t.process(*seq[0])
        np.testing.assert_array_equal(t.detection_mask(), mask.pack(blob, 3))
        u.reset()
        fu, _ = u.process(*seq[0])
        assert fi.n_detected_left < fu.n_detected_left
        # on then off: as never set
        t.set_detection_mask(None); t.reset(); u.reset()
        for f in range(3):
            (fa, na), (fb, nb) = t.process(*seq[f]), u.process(*seq[f])
            _same_info(fa, fb, "off frame %d" % f); assert na == nb
            _same_points(t.points(), u.points(), "off frame %d" % f)
    finally:
        t.destroy(); u.destroy()
    # the host-driven loop does not have the feature and says so; it goes on tracking
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: h.set_detection_mask(blob, 0), lambda: h.set_detection_mask(None), h.detection_mask):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
        fi, _ = h.process(*seq[0])
        assert fi.n_points > 50
    finally:
        h.destroy()
