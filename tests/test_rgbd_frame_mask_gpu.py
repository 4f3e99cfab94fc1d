"""Per-frame detection masks in RGB-D mode (vslam_rgbd_set_frame_masks, csrc/kernels_mask.h): a frame mask repeated on every
frame is the static mask, all-keep frame masks are no masks, what lies under a moving mask cannot matter - one sequence, the captured
launch sequence, a batch of 3 with host and device masks, map and log on, together with a static mask, behind undistortion -, a frame
with masks, one without and one with again, every registration attempt of a frame, and the contract of the setter.  tum configuration
at 188 x 620, 12 frames: the scenes of bilateral_cases.py, as test_rgbd_mask_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import bilateral_cases as bc
import validity_cases as vc
from test_rgbd_mask_gpu import MARGIN, blob_of, noise_under, on_kept_pixels
from test_undistort_gpu import _same_info, _same_points
from vslam_pose_estimation_framework_amd import hip, mask
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds():
    seqs = [bc.sequence(seed) for seed in bc.SEEDS]
    return seqs[0]["cfg"], seqs[0]["p"], [[(L, F) for L, _, F, _ in s["frames"]] for s in seqs]


def _make(g, cfg, p, B):
    return RgbdTracker(g, cfg, p) if B == 1 else RgbdBatch(g, cfg, p, B)


def _frame(frames, B, f):
    return np.stack([frames[s][f][0] for s in range(B)]), np.stack([frames[s][f][1] for s in range(B)])


def _run(t, B, L, D):
    if B == 1:
        return [t.process(L[0], D[0])], [t.points()]
    return t.process(L, D), [t.points(s) for s in range(B)]


def _same(ia, ib, pa, pb, B, tag):
    for s in range(B):
        _same_info(ia[s][0], ib[s][0], "%s sequence %d" % (tag, s))
        assert ia[s][1] == ib[s][1], tag
        _same_points(pa[s], pb[s], "%s sequence %d" % (tag, s))


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
def test_frame_mask_on_every_frame_is_the_static_mask(B, graph, worlds, monkeypatch):
    """A gets the blob as a frame mask ahead of every frame, B holds it as the static mask, C gets all-255 frame masks, D has none:
    A == B and C == D bit for bit: frame info, poses, complete point lists."""
    cfg, p, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))
    g = hip.load()
    a, b, c, d = (_make(g, cfg, p, B) for _ in range(4))
    rows, cols = int(cfg.rows), int(cfg.cols)
    blob = blob_of(rows, cols)
    try:
        b.set_detection_mask(blob, 9)
        for f in range(bc.N_FRAMES):
            L, D = _frame(frames, B, f)
            a.set_frame_masks(np.stack([blob] * B), 9)
            c.set_frame_masks(np.full((B, rows, cols), 255, np.uint8), 64)
            (ia, pa), (ib, pb), (ic, pc), (id_, pd) = _run(a, B, L, D), _run(b, B, L, D), _run(c, B, L, D), _run(d, B, L, D)
            _same(ia, ib, pa, pb, B, "frame == static, frame %d" % f)
            _same(ic, id_, pc, pd, B, "all-keep == none, frame %d" % f)
            if f == 0:          # the detector starts at the same threshold: the mask does remove detections, ahead of the count
                assert all(ia[s][0].n_detected_left < id_[s][0].n_detected_left for s in range(B))
            for s in range(B):
                np.testing.assert_array_equal(a.frame_detection_mask(s), mask.pack(blob, 9))
                np.testing.assert_array_equal(b.frame_detection_mask(s), mask.pack(blob, 9))
                np.testing.assert_array_equal(c.frame_detection_mask(s), mask.all_keep(rows, cols))
        assert all(fi.status == 1 and fi.n_points >= 50 and fi.error_flags == 0 for fi, _ in ia)
    finally:
        for t in (a, b, c, d):
            t.destroy()


@pytest.mark.parametrize("case", ["one", "one-graph", "batch3", "batch3-device", "batch3-graph", "one-map", "one-static", "one-undistort", "pattern", "pattern-graph"])
def test_pixels_under_moving_masks_do_not_matter(case, worlds, monkeypatch):
    """Trackers A and B get the same moving rectangles (another one per frame and per sequence) with a margin of the extractor's reach; B's
    images carry seeded noise on every zero pixel of that frame's mask.  Recovery off.  Frame info, the complete point lists, map and log
    are equal bit for bit, every point lies on a kept pixel, and frame_detection_mask is mask.effective.  pattern: only every other frame
    has masks (mask / none / mask ...), a frame without a set runs unmasked; pattern-graph: A replays captured launch sequences, B does not."""
    import test_mask_gpu as tm
    assert MARGIN >= tm.brief_reach() and MARGIN >= tm.orb_reach()
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case.endswith("graph") else "0")
    und = None
    if case == "one-undistort":
        w = vc.rgbd_world()
        cfg, p, und = w["cfg"], w["p"], w["und"]
        frames = [[(fr[0], fr[1]) for fr in w["frames"]]]            # raw frames: the masks are in undistorted coordinates
    else:
        cfg, p, frames = worlds
    cfg = cfg.copy()
    cfg.enable_landmark_recovery = 0
    g = hip.load()
    B = 3 if case.startswith("batch3") else 1
    a = _make(g, cfg, p, B)
    if case == "pattern-graph":                 # against the uncaptured run
        monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    b = _make(g, cfg, p, B)
    rows, cols = int(cfg.rows), int(cfg.cols)
    blob = blob_of(rows, cols)
    rng = np.random.default_rng(11)
    dev_masks = []
    try:
        for t in (a, b):
            if und is not None:
                t.set_undistortion(und)
            if case == "one-map":
                t.enable_map(6000); t.enable_observations(60000)
            if case == "one-static":
                t.set_detection_mask(blob, MARGIN)
        static = (blob, MARGIN) if case == "one-static" else None
        masked_frames = 0
        for f in range(bc.N_FRAMES):
            L, D = _frame(frames, B, f)
            fm = np.stack([vc.moving_rect(rows, cols, f, s) for s in range(B)])
            with_mask = not case.startswith("pattern") or f % 2 == 0
            Ln = L
            if with_mask:
                masked_frames += 1
                zero = fm == 0
                if case == "one-static":
                    zero = zero | (blob == 0)[None]
                if und is None:
                    Ln = L.copy()
                    Ln[zero] = rng.integers(0, 256, int(zero.sum()), dtype=np.uint8)
                else:       # raw pixels that no undistorted pixel outside the zero region reads: the undistorted image moves under the mask only
                    H, W = L.shape[1:]
                    xy = und.map_xy.astype(np.int64)
                    touched = np.zeros((H, W), bool)
                    for dy in (0, 1):
                        for dx in (0, 1):
                            yy, xx = xy[..., 1] + dy, xy[..., 0] + dx
                            ok = ~zero[0] & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                            touched[yy[ok], xx[ok]] = True
                    Ln = L.copy()
                    Ln[0][~touched] = rng.integers(0, 256, int((~touched).sum()), dtype=np.uint8)
                    if f == 0:
                        from vslam_pose_estimation_framework_amd import rectify
                        ua, ub = rectify.remap_u8(L[0], und.map_xy, und.map_a), rectify.remap_u8(Ln[0], und.map_xy, und.map_a)
                        assert (ua != ub)[zero[0]].any() and not (ua != ub)[~zero[0]].any()
                assert (Ln != L).any()
                if case == "batch3-device":
                    import torch
                    td = torch.from_numpy(fm).cuda()
                    dev_masks.append((td, td.clone()))
                    a.set_frame_masks(td, MARGIN); b.set_frame_masks(td, MARGIN)
                else:
                    a.set_frame_masks(fm, MARGIN); b.set_frame_masks(fm, MARGIN)
            (ia, pa), (ib, pb) = _run(a, B, L, D), _run(b, B, Ln, D)
            tag = "%s frame %d" % (case, f)
            _same(ia, ib, pa, pb, B, tag)
            for s in range(B):
                if with_mask:
                    want = mask.effective(rows, cols, static, (fm[s], MARGIN))
                    keep = mask.unpack(want, cols)
                    assert on_kept_pixels(pa[s], keep), tag
                    for t in (a, b):
                        np.testing.assert_array_equal(t.frame_detection_mask(s), want, err_msg=tag)
                elif static is None:
                    with pytest.raises(VslamError) as e:                 # a set lasts one frame: this one used no mask of any kind
                        a.frame_detection_mask(s)
                    assert e.value.code == ERR_STATE
            if case == "one-map":
                np.testing.assert_array_equal(a.point_ids(), b.point_ids())
                ma, mb, oa, ob = a.map(), b.map(), a.observations(), b.observations()
                for k in ma:
                    np.testing.assert_array_equal(ma[k], mb[k], err_msg="map %s frame %d" % (k, f))
                for k in oa:
                    np.testing.assert_array_equal(oa[k], ob[k], err_msg="log %s frame %d" % (k, f))
        assert masked_frames >= bc.N_FRAMES // 2
        assert all(fi.status == 1 and fi.n_points >= 50 and fi.error_flags == 0 for fi, _ in ia)      # equal and tracking, not equal and empty
        if case == "one-map":
            assert len(ma["id"]) > 30 and len(oa["id"]) > 100
        if dev_masks:
            import torch
            torch.cuda.synchronize()
            assert all(torch.equal(x, y) for x, y in dev_masks)          # device masks are only read
    finally:
        a.destroy(); b.destroy()


@pytest.mark.parametrize("graph", [0, 1])
def test_frame_masks_apply_to_every_registration_attempt(graph, monkeypatch):
    """The re-registration scenario (icl configuration, a jump from frame 8 to 16): every attempt's detection is masked again with the
    frame's words, so noise under the frame's mask stays without effect across a frame with at least two attempts."""
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))
    sc = bc.reregistration()
    cfg, p = sc["cfg"].copy(), sc["p"]
    cfg.enable_landmark_recovery = 0
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    rows, cols = int(cfg.rows), int(cfg.cols)
    rng = np.random.default_rng(6)
    try:
        attempts = []
        for f, (L, _, F, _) in enumerate(sc["frames"]):
            fm = blob_of(rows, cols) if f % 2 else np.ascontiguousarray(blob_of(rows, cols)[:, ::-1])
            a.set_frame_mask(fm, MARGIN); b.set_frame_mask(fm, MARGIN)
            (fa, na), (fb, nb) = a.process(L, F), b.process(noise_under(L, fm, rng), F)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            assert on_kept_pixels(a.points(), mask.erode(fm != 0, MARGIN)), f
            np.testing.assert_array_equal(a.frame_detection_mask(), mask.pack(fm, MARGIN))
            attempts.append(fa.track_attempts)
        assert max(attempts) >= 2, attempts
    finally:
        a.destroy(); b.destroy()


def test_rgbd_frame_mask_contract(worlds, monkeypatch):
    cfg, p, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    seq = frames[0]
    rows, cols = int(cfg.rows), int(cfg.cols)
    blob = blob_of(rows, cols)
    ptr = blob.ctypes.data_as(C.c_void_p)
    t, u, b3 = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p), RgbdBatch(g, cfg, p, 3)
    try:
        assert g.lib.vslam_rgbd_set_frame_masks(None, ptr, C.c_int32(cols), C.c_size_t(0), C.c_int32(0), C.c_int(0)) == ERR_INVALID
        with pytest.raises(VslamError) as e:                      # before a frame
            t.frame_detection_mask()
        assert e.value.code == ERR_STATE
        # each refusal; none is sticky, none leaves a set behind
        for stride, margin in ((cols - 1, 0), (cols, -1), (cols, 65)):
            assert g.lib.vslam_rgbd_set_frame_masks(t.h, ptr, C.c_int32(stride), C.c_size_t(0), C.c_int32(margin), C.c_int(0)) == ERR_INVALID
        assert g.lib.vslam_rgbd_set_frame_masks(b3.h, ptr, C.c_int32(cols), C.c_size_t(rows * cols - 1), C.c_int32(0), C.c_int(0)) == ERR_INVALID
        (fa, na), (fb, nb) = t.process(*seq[0]), u.process(*seq[0])
        _same_info(fa, fb, "after refusals"); assert na == nb
        with pytest.raises(VslamError) as e:                      # that frame used no mask
            t.frame_detection_mask()
        assert e.value.code == ERR_STATE
        # a cancelled set
        t.set_frame_mask(blob, 3)
        t.set_frame_masks(None)
        (fa, na), (fb, nb) = t.process(*seq[1]), u.process(*seq[1])
        _same_info(fa, fb, "cancelled"); assert na == nb
        _same_points(t.points(), u.points(), "cancelled")
        # a set lasts one frame
        t.set_frame_mask(blob, 3)
        fa, _ = t.process(*seq[2]); fb, _ = u.process(*seq[2])
        np.testing.assert_array_equal(t.frame_detection_mask(), mask.pack(blob, 3))
        assert fa.n_detected_left < fb.n_detected_left
        t.process(*seq[3])
        with pytest.raises(VslamError) as e:
            t.frame_detection_mask()
        assert e.value.code == ERR_STATE
        with pytest.raises(VslamError) as e:                      # the context-wide getter: no static mask is set
            t.detection_mask()
        assert e.value.code == ERR_STATE
        # a refused submit (no image) changes nothing: the set goes on waiting for the next accepted one
        t.set_frame_mask(blob, 3)
        assert g.lib.vslam_rgbd_submit_host(t.h, None, C.c_int32(cols), None, C.c_int32(cols)) == ERR_INVALID
        t.process(*seq[3])
        np.testing.assert_array_equal(t.frame_detection_mask(), mask.pack(blob, 3))
        t.process(*seq[3])
        # in flight
        t.submit(*seq[4])
        for call in (lambda: t.set_frame_mask(blob, 0), lambda: t.set_frame_masks(None), t.frame_detection_mask):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "in flight" in str(e.value)
        t.wait()
        # reset drops a pending set and forgets the last frame
        t.set_frame_mask(blob, 3)
        t.process(*seq[5])
        np.testing.assert_array_equal(t.frame_detection_mask(), mask.pack(blob, 3))
        t.set_frame_mask(blob, 3)
        t.reset(); u.reset()
        with pytest.raises(VslamError) as e:
            t.frame_detection_mask()
        assert e.value.code == ERR_STATE
        (fa, na), (fb, nb) = t.process(*seq[0]), u.process(*seq[0])
        _same_info(fa, fb, "after reset"); assert na == nb
        # with a static mask the getter returns the context-wide words after a frame without a set
        t.set_detection_mask(blob, 2)
        t.process(*seq[1])
        np.testing.assert_array_equal(t.frame_detection_mask(), mask.pack(blob, 2))
    finally:
        t.destroy(); u.destroy(); b3.destroy()
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: h.set_frame_mask(blob, 0), lambda: h.set_frame_masks(None), h.frame_detection_mask):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
        fi, _ = h.process(*seq[0])
        assert fi.n_points > 50
    finally:
        h.destroy()
