"""Validity masks from remap maps on the device (k_map_valid behind vslam_map_validity_mask, vslam_set_rectification_mask and
vslam_rgbd_set_undistortion_mask): the stand-alone entry against mask.pack_bool(mask.erode(rectify.validity(..))) bit for
bit, and the fused switch equal bit for bit - poses, keypoints, complete point lists - to a context that is fed the same raw frames and
holds the numpy validity mask as a static user mask.  The premises of the scenes: test_validity_host.py."""
import ctypes as C

import numpy as np
import pytest

import validity_cases as vc
from pipeline_compare import create_hip
from test_undistort_gpu import _same_info, _same_points
from vslam_pose_estimation_framework_amd import hip, mask, rectify
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

pytestmark = pytest.mark.gpu
NF = vc.FRAMES - 2                  # frames per RGB-D case: sequence s of a batch starts s frames into the scene


@pytest.fixture(scope="module")
def api():
    g = hip.load()
    g.create(g.default_config("kitti"), 0, 1)
    yield g
    g.destroy()


# ---- the stand-alone entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_map_validity_mask_equals_numpy(api, shape):
    rows, cols = shape
    for seed in range(2):
        xy, a, rr, rc, _ = vc.random_maps(rows, cols, seed)
        for m in vc.MARGINS:
            np.testing.assert_array_equal(api.map_validity_mask(xy, a, rr, rc, m), vc.words_of(xy, a, rr, rc, m), err_msg="seed %d m=%d" % (seed, m))


def test_map_validity_mask_real_maps_and_reuse(api):
    import test_rectify_gpu as tr
    from _oracle import Oracle
    o = Oracle()
    try:
        scene, _ = tr._scene_and_config(o)
    finally:
        o.destroy()
    rig, _, _ = vc.wide_rig(scene, tr.RAW_ROWS, tr.RAW_COLS)
    und = vc.rgbd_world()["und"]
    maps = [(rig.map_xy_left, rig.map_a_left, rig.raw_rows, rig.raw_cols), (rig.map_xy_right, rig.map_a_right, rig.raw_rows, rig.raw_cols),
            (und.map_xy, und.map_a, und.raw_rows, und.raw_cols)]
    for xy, a, rr, rc in maps:
        for m in (0, 4, 28):
            np.testing.assert_array_equal(api.map_validity_mask(xy, a, rr, rc, m), vc.words_of(xy, a, rr, rc, m))
    # KITTI size once: a lens in front of a 376 x 1241 sensor, the output camera 0.9 f
    K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1.0]])
    cam = rectify.CameraModel(K, (-0.28, 0.074, 0.0, 0.0, 0.0), 376, 1241)
    Kn = K.copy(); Kn[0, 0] *= 0.9; Kn[1, 1] *= 0.9
    big = rectify.undistortion(cam, Kn)
    want = vc.words_of(big.map_xy, big.map_a, 376, 1241, 5)
    first = api.map_validity_mask(big.map_xy, big.map_a, 376, 1241, 5)
    np.testing.assert_array_equal(first, want)
    assert 0.5 < mask.unpack(want, 1241).mean() < 0.99
    # one context twice == two fresh contexts
    np.testing.assert_array_equal(api.map_validity_mask(big.map_xy, big.map_a, 376, 1241, 5), first)
    g2 = hip.load()
    g2.create(g2.default_config("kitti"), 0, 1)
    try:
        np.testing.assert_array_equal(g2.map_validity_mask(big.map_xy, big.map_a, 376, 1241, 5), first)
    finally:
        g2.destroy()


def test_map_validity_mask_refusals_write_nothing(api):
    xy, a, rr, rc, _ = vc.random_maps(9, 13, 0)
    fn = api.fn("map_validity_mask")
    words = np.full((9, 1), 0xA5A5A5A5A5A5A5A5, np.uint64)

    def call(xy_, a_, rows, cols, rr_, rc_, m, out=words):
        return fn(*api._ctx_args(), xy_.ctypes.data_as(C.c_void_p) if xy_ is not None else None, a_.ctypes.data_as(C.c_void_p) if a_ is not None else None,
                  C.c_int32(rows), C.c_int32(cols), C.c_int32(rr_), C.c_int32(rc_), C.c_int32(m), out.ctypes.data_as(C.c_void_p) if out is not None else None)
    bad_a = a.copy(); bad_a[2, 3] = 1024
    for args in ((xy, a, 0, 13, rr, rc, 0), (xy, a, 9, 0, rr, rc, 0), (xy, a, 9, 32768, rr, rc, 0), (xy, a, 9, 13, 0, rc, 0), (xy, a, 9, 13, rr, 32768, 0),
                 (xy, a, 9, 13, rr, rc, -1), (xy, a, 9, 13, rr, rc, 65), (None, a, 9, 13, rr, rc, 0), (xy, None, 9, 13, rr, rc, 0), (xy, bad_a, 9, 13, rr, rc, 0)):
        assert call(*args) == ERR_INVALID, args[2:]
        assert (words == 0xA5A5A5A5A5A5A5A5).all()
    assert call(xy, a, 9, 13, rr, rc, 0, None) == ERR_INVALID
    np.testing.assert_array_equal(api.map_validity_mask(xy, a, rr, rc, 1), vc.words_of(xy, a, rr, rc, 1))      # the context stays usable


# ---- RGB-D: vslam_rgbd_set_undistortion_mask ------------------------------------------------------------------------------------------
def _batch(w, B, f, raw):
    """Sequence s of a batch starts s frames into the scene; raw: (image, depth) as the sensor gave them, else the undistorted pair."""
    i = 0 if raw else 2
    fr = [w["frames"][f + s] for s in range(B)]
    return np.stack([x[i] for x in fr]), np.stack([x[i + 1] for x in fr])


def _run(t, B, L, D):
    if B == 1:
        return [t.process(L[0], D[0])], [t.points()]
    return t.process(L, D), [t.points(s) for s in range(B)]


@pytest.mark.parametrize("case,m", [("one", 0), ("one", 4), ("one-graph", 4), ("batch3", 4), ("user5", 4), ("frame-masks", 0)])
def test_rgbd_validity_equals_numpy_static_mask(case, m, monkeypatch):
    """A: undistortion + set_undistortion_mask(True, m).  B: undistortion + the u8 image of the eroded validity as static mask, margin 0.
    user5: both also hold a user mask (A: as the static mask with margin 5, B: ANDed into its image in numpy).  frame-masks: both get the
    moving rectangles as frame masks.  Frame info, poses and complete point lists bit for bit, the getters the numpy words."""
    import test_rgbd_mask_gpu as rm
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case.endswith("graph") else "0")
    w = vc.rgbd_world()
    cfg, p, und, valid = w["cfg"], w["p"], w["und"], w["valid"]
    rows, cols = int(cfg.rows), int(cfg.cols)
    B = 3 if case == "batch3" else 1
    g = hip.load()
    make = (lambda: RgbdTracker(g, cfg, p)) if B == 1 else (lambda: RgbdBatch(g, cfg, p, B))
    a, b, c = make(), make(), make()
    keep = mask.erode(valid, m)
    blob = rm.blob_of(rows, cols)
    if case == "user5":
        keep = keep & mask.erode(blob != 0, 5)
    try:
        for t in (a, b, c):
            t.set_undistortion(und)
        assert a.undistortion_mask() == (False, 0)
        a.set_undistortion_mask(True, m)
        assert a.undistortion_mask() == (True, m)
        if case == "user5":
            a.set_detection_mask(blob, 5)
        b.set_detection_mask(vc.mask_image(keep), 0)
        fewer = 0
        for f in range(NF):
            L, D = _batch(w, B, f, True)
            want = mask.pack_bool(keep)
            if case == "frame-masks":
                fm = vc.moving_rect(rows, cols, f)
                a.set_frame_mask(fm, 3); b.set_frame_mask(fm, 3)
                want = want & mask.pack(fm, 3)
            (ia, pa), (ib, pb), (ic, _) = _run(a, B, L, D), _run(b, B, L, D), _run(c, B, L, D)
            for s in range(B):
                tag = "%s m=%d frame %d sequence %d" % (case, m, f, s)
                _same_info(ia[s][0], ib[s][0], tag)
                assert ia[s][1] == ib[s][1], tag
                _same_points(pa[s], pb[s], tag)
                fewer += int(ia[s][0].n_detected_left < ic[s][0].n_detected_left)
                np.testing.assert_array_equal(a.frame_detection_mask(s), want, err_msg=tag)
                if case != "frame-masks" and f >= 2:               # equal and tracking, not equal and empty
                    assert ia[s][0].status == 1 and ia[s][0].n_points >= 100 and ia[s][0].error_flags == 0, tag
            np.testing.assert_array_equal(a.detection_mask(), mask.pack_bool(keep))
            np.testing.assert_array_equal(b.detection_mask(), mask.pack_bool(keep))
        assert fewer >= NF * B // 2, fewer                         # the mask does remove detections (the seam fires: test_validity_host.py)
    finally:
        a.destroy(); b.destroy(); c.destroy()


def test_rgbd_validity_lifetime(monkeypatch):
    """New maps recompute the words, undistortion off switches the mask off, off equals never on, it survives reset; the refusals."""
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    w = vc.rgbd_world()
    cfg, p, und, valid = w["cfg"], w["p"], w["und"], w["valid"]
    g = hip.load()
    t, u = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    raw = [(f[0], f[1]) for f in w["frames"]]
    try:
        with pytest.raises(VslamError) as e:                       # no maps
            t.set_undistortion_mask(True, 0)
        assert e.value.code == ERR_STATE
        t.set_undistortion_mask(False)                             # off while off: fine
        t.set_undistortion(und); u.set_undistortion(und)
        for margin in (-1, 65):
            with pytest.raises(VslamError) as e:
                t.set_undistortion_mask(True, margin)
            assert e.value.code == ERR_INVALID
        assert t.undistortion_mask() == (False, 0)
        t.set_undistortion_mask(True, 4)
        with pytest.raises(VslamError) as e:                       # on, no frame yet
            t.detection_mask()
        assert e.value.code == ERR_STATE
        t.process(*raw[0])
        np.testing.assert_array_equal(t.detection_mask(), mask.pack_bool(mask.erode(valid, 4)))
        # in flight
        t.submit(*raw[1])
        for call in (lambda: t.set_undistortion_mask(False), lambda: t.set_undistortion_mask(True, 1)):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "in flight" in str(e.value)
        t.wait()
        assert t.undistortion_mask() == (True, 4)
        # survives reset
        t.reset()
        assert t.undistortion_mask() == (True, 4)
        with pytest.raises(VslamError):
            t.detection_mask()
        t.process(*raw[0])
        np.testing.assert_array_equal(t.detection_mask(), mask.pack_bool(mask.erode(valid, 4)))
        # new maps recompute: the narrower camera (the scene's own f) has another validity
        K1 = und.K.copy(); K1[0, 0] /= vc.F_SCALE; K1[1, 1] /= vc.F_SCALE
        und1 = rectify.undistortion(und.cam, K1, und.rows, und.cols)
        valid1 = rectify.validity(und1.map_xy, und1.map_a, und1.raw_rows, und1.raw_cols)
        assert (valid1 != valid).any()
        t.set_undistortion(und1)
        assert t.undistortion_mask() == (True, 4)
        t.reset(); t.process(*raw[0])
        np.testing.assert_array_equal(t.detection_mask(), mask.pack_bool(mask.erode(valid1, 4)))
        # undistortion off switches it off; on again it stays off: as never on
        t.set_undistortion(None)
        assert t.undistortion_mask() == (False, 0)
        t.set_undistortion(und)
        assert t.undistortion_mask() == (False, 0)
        t.reset(); u.reset()
        for f in range(3):
            (fa, na), (fb, nb) = t.process(*raw[f]), u.process(*raw[f])
            _same_info(fa, fb, "off frame %d" % f); assert na == nb
            _same_points(t.points(), u.points(), "off frame %d" % f)
        with pytest.raises(VslamError) as e:
            t.detection_mask()
        assert e.value.code == ERR_STATE
    finally:
        t.destroy(); u.destroy()
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        with pytest.raises(VslamError) as e:
            h.set_undistortion_mask(True, 0)
        assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
    finally:
        h.destroy()


# ---- stereo: vslam_set_rectification_mask -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stereo():
    """validity_cases.stereo_world: the configuration of the rectified camera, the rectification, 12 raw pairs, the numpy validity of both
    sides (its premises: test_validity_host.test_pincushion_rig_premises)."""
    w = vc.stereo_world()
    return w["cfg"], w["rig"], w["frames"], w["valid"]


def _stereo_batch(frames, B, k):
    pairs = [frames[k + 2 * s] for s in range(B)]
    return np.ascontiguousarray(np.stack([p[0] for p in pairs])), np.ascontiguousarray(np.stack([p[1] for p in pairs]))


def _feed(g, L, R, stage):
    if not stage:
        g.process_host(L, R)
        return
    g.check(g.fn("frame_begin")(g.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]), C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
    g.check(g.fn("frame_finish")(g.ctx))


@pytest.mark.parametrize("B,mode,m", [(1, "host", 0), (1, "host", 4), (3, "host", 4), (1, "stage", 4), (1, "split0", 4), (1, "split4", 4), (1, "user5", 4),
                                      (3, "frame-masks", 0)])
def test_stereo_validity_equals_numpy_static_mask(B, mode, m, stereo):
    """A: rectification + set_rectification_mask(True, m).  B: rectification + the u8 images of the eroded validity of each side as static
    masks, margin 0.  Both are fed the same raw pairs."""
    import mask_cases as mc
    from test_rectify_gpu import _compare
    from test_rgbd_mask_gpu import blob_of
    cfg, rig, frames, valid = stereo
    rows, cols = int(cfg.rows), int(cfg.cols)
    split = {"split0": 0, "split4": 4}.get(mode)
    a, b, c = create_hip(cfg, B, split), create_hip(cfg, B, split), create_hip(cfg, B, split)
    keep = [mask.erode(v, m) for v in valid]
    blob = blob_of(rows, cols)
    if mode == "user5":
        keep = [k & mask.erode(blob != 0, 5) for k in keep]
    try:
        for t in (a, b, c):
            t.set_rectification(rig)
        assert a.rectification_mask() == (False, 0)
        a.set_rectification_mask(True, m)
        assert a.rectification_mask() == (True, m)
        if mode == "user5":
            a.set_detection_mask(blob, blob, 5)
        b.set_detection_mask(vc.mask_image(keep[0]), vc.mask_image(keep[1]), 0)
        fewer = 0
        for k in range(6):
            L, R = _stereo_batch(frames, B, k)
            want = [[mask.pack_bool(keep[side]) for side in (0, 1)] for _ in range(B)]
            if mode == "frame-masks":
                fm = np.stack([mc.frame_rect(rows, cols, k, s, small=True) for s in range(B)])
                a.set_frame_masks(fm, fm, 2); b.set_frame_masks(fm, fm, 2)
                want = [[want[s][side] & mask.pack(fm[s], 2) for side in (0, 1)] for s in range(B)]
            for t in (a, b, c):
                _feed(t, L, R, mode == "stage")
            for s in range(B):
                _compare(a, b, s, "B=%d %s m=%d frame %d stream %d" % (B, mode, m, k, s))
                fi = a.frame_info(s)
                fewer += int(fi.n_detected_left < c.frame_info(s).n_detected_left)
                for side in (0, 1):
                    np.testing.assert_array_equal(a.detection_mask(s, side), want[s][side])
                print("B=%d %s m=%d frame %d stream %d: status %d, %d points" % (B, mode, m, k, s, fi.status, fi.n_points))
                if mode != "frame-masks" and k >= 2:                # equal and tracking, not equal and empty
                    assert fi.status == 1 and fi.n_points >= 100 and fi.error_flags == 0, (k, s, fi.status, fi.n_points)
        assert fewer >= 3 * B, fewer
        assert all(a.frame_info(s).n_points > 50 and a.frame_info(s).status == 1 for s in range(B))
    finally:
        a.destroy(); b.destroy(); c.destroy()


def test_stereo_validity_lifetime(stereo):
    from test_rectify_gpu import _compare, _smooth_maps, _Rig
    cfg, rig, frames, valid = stereo
    rows, cols = int(cfg.rows), int(cfg.cols)
    a, b = create_hip(cfg, 1), create_hip(cfg, 1)
    try:
        with pytest.raises(VslamError) as e:
            a.set_rectification_mask(True, 0)
        assert e.value.code == ERR_STATE
        a.set_rectification_mask(False)
        a.set_rectification(rig); b.set_rectification(rig)
        for margin in (-1, 65):
            with pytest.raises(VslamError) as e:
                a.set_rectification_mask(True, margin)
            assert e.value.code == ERR_INVALID
        assert a.rectification_mask() == (False, 0)
        a.set_rectification_mask(True, 2)
        L, R = _stereo_batch(frames, 1, 0)
        a.process_host(L, R)
        for side in (0, 1):
            np.testing.assert_array_equal(a.detection_mask(0, side), mask.pack_bool(mask.erode(valid[side], 2)))
        # inside a frame (between frame_begin and frame_finish) the switch is refused and stays as it is
        a.check(a.fn("frame_begin")(a.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]), C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
        for call in (lambda: a.set_rectification_mask(False), lambda: a.set_rectification_mask(True, 5)):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "inside a frame" in str(e.value)
        a.check(a.fn("frame_finish")(a.ctx))
        assert a.rectification_mask() == (True, 2)
        np.testing.assert_array_equal(a.detection_mask(0, 0), mask.pack_bool(mask.erode(valid[0], 2)))
        a.reset()                                                   # survives reset
        assert a.rectification_mask() == (True, 2)
        a.process_host(L, R)
        np.testing.assert_array_equal(a.detection_mask(0, 1), mask.pack_bool(mask.erode(valid[1], 2)))
        # new maps recompute
        other = _Rig(rows, cols, rig.raw_rows, rig.raw_cols, [_smooth_maps(rows, cols, rig.raw_rows, rig.raw_cols, 7), _smooth_maps(rows, cols, rig.raw_rows, rig.raw_cols, 8)])
        a.set_rectification(other)
        assert a.rectification_mask() == (True, 2)
        a.reset(); a.process_host(L, R)
        v0 = rectify.validity(other.map_xy_left, other.map_a_left, rig.raw_rows, rig.raw_cols)
        assert (~v0).any() and (v0 != valid[0]).any()
        np.testing.assert_array_equal(a.detection_mask(0, 0), mask.pack_bool(mask.erode(v0, 2)))
        # rectification off switches it off; off == never on
        a.set_rectification(None)
        assert a.rectification_mask() == (False, 0)
        a.set_rectification(rig)
        assert a.rectification_mask() == (False, 0)
        a.reset(); b.reset()
        for k in range(3):
            L, R = _stereo_batch(frames, 1, k)
            a.process_host(L, R); b.process_host(L, R)
            _compare(a, b, 0, "off frame %d" % k)
        with pytest.raises(VslamError) as e:
            a.detection_mask(0, 0)
        assert e.value.code == ERR_STATE
    finally:
        a.destroy(); b.destroy()
