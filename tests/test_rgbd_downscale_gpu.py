"""Downscaling in RGB-D mode (vslam_rgbd_set_downscale, csrc/kernels_downscale.h): the tum premise scene of
test_downscale_host.py at f = 2, the fused path equal bit for bit to downscale-with-numpy-then-run — frame info, poses, point lists and
downscaled() (image and depth) — for one sequence, under the captured launch sequence, for a batch (captured, and on device frames), with
map, log and map colours on, behind colour input, ahead of undistortion + bilateral filter + CLAHE, with the ORB detector, at f = 3, and
the contract of the switch."""
import ctypes as C

import numpy as np
import pytest

import downscale_cases as dc
from test_undistort_gpu import _pad, _same_info, _same_points
from vslam_pose_estimation_framework_amd import downscale, hip
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

FULL = (376, 1241)


@pytest.fixture(scope="module")
def worlds():
    """Per factor 2 and 3: (cfg, p, K', per seed the frames (full image, full depth, reduced image, reduced depth)), made once."""
    from _oracle import Oracle
    o = Oracle()
    out = {}
    try:
        for f in (2, 3):
            per_seed = [dc.rgbd_world(o, seed, f) for seed in (dc.RGBD_SEEDS if f == 2 else dc.RGBD_SEEDS[:1])]
            out[f] = per_seed[0][:3] + ([w[3] for w in per_seed],)
    finally:
        o.destroy()
    return out


def _env(monkeypatch, graph=0):
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "one-graph", "batch3", "batch3-graph", "batch3-device", "one-map", "one-f3"])
def test_fused_downscale_equals_numpy_then_run(case, worlds, monkeypatch):
    """Tracker A has the switch on and gets the full frames (image rows padded), tracker B the numpy-downscaled ones.  After every frame:
    frame info (poses in it) and the complete point lists bit for bit, downscaled() the numpy pair; with the map and the log on, ids, map
    and log too."""
    f = 3 if case.endswith("f3") else 2
    cfg, p, _, frames = worlds[f]
    _env(monkeypatch, 1 if case.endswith("graph") else 0)
    g = hip.load()
    B = 3 if case.startswith("batch3") else 1
    if B == 1:
        a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    else:
        a, b = RgbdBatch(g, cfg, p, B), RgbdBatch(g, cfg, p, B)
    try:
        a.set_downscale(f, *FULL)
        assert a.downscale() == (f,) + FULL and b.downscale() == (1, 0, 0)
        if case == "one-map":
            for t in (a, b):
                t.enable_map(6000); t.enable_observations(60000)
        for k in range(dc.RGBD_FRAMES):
            L = _pad(np.stack([frames[s][k][0] for s in range(B)]), 12, 7)
            D = np.stack([frames[s][k][1] for s in range(B)])
            l = np.stack([frames[s][k][2] for s in range(B)])
            d = np.stack([frames[s][k][3] for s in range(B)])
            if B == 1:
                ia, ib = [a.process(L[0], D[0])], [b.process(l[0], d[0])]
                pa, pb = [a.points()], [b.points()]
            else:
                if case == "batch3-device":
                    import torch
                    dev = torch.device("cuda", 0)
                    Ld = torch.from_numpy(L).to(dev); Dd = torch.from_numpy(D.view(np.int16)).to(dev)
                    torch.cuda.synchronize()
                    a.submit_device(Ld.data_ptr(), L.shape[2], L.shape[1] * L.shape[2], Dd.data_ptr(), D.shape[2], D.shape[1] * D.shape[2])
                    ia = a.wait()
                    np.testing.assert_array_equal(Ld.cpu().numpy(), L, err_msg="the caller's device images were written")
                    np.testing.assert_array_equal(Dd.cpu().numpy().view(np.uint16), D, err_msg="the caller's depth images were written")
                else:
                    ia = a.process(L, D)
                ib = b.process(l, d)
                pa, pb = [a.points(s) for s in range(B)], [b.points(s) for s in range(B)]
            for s in range(B):
                tag = "%s frame %d sequence %d" % (case, k, s)
                _same_info(ia[s][0], ib[s][0], tag)
                assert ia[s][1] == ib[s][1], tag
                _same_points(pa[s], pb[s], tag)
                gi, gd = a.downscaled(s)
                np.testing.assert_array_equal(gi, l[s], err_msg=tag + " image")
                np.testing.assert_array_equal(gd, d[s], err_msg=tag + " depth")
                assert k < 2 or (ia[s][0].status == 1 and ia[s][0].n_points >= dc.RGBD_MIN_POINTS[f]), tag
            if case == "one-map":
                np.testing.assert_array_equal(a.point_ids(), b.point_ids())
                ma, mb, oa, ob = a.map(), b.map(), a.observations(), b.observations()
                for key in ma:
                    np.testing.assert_array_equal(ma[key], mb[key], err_msg="map %s frame %d" % (key, k))
                for key in oa:
                    np.testing.assert_array_equal(oa[key], ob[key], err_msg="log %s frame %d" % (key, k))
        if case == "one-map":
            assert len(ma["id"]) > 50 and len(oa["id"]) > 200
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_downscale_behind_color_input_with_map_colors(graph, worlds, monkeypatch):
    """Colour frames of the full size: grey, then downscale on the device == numpy grey, numpy downscale, then run; gray() is the full-size
    grey image; the map's colours are the numpy gather over the block-averaged colour planes."""
    import color_cases as col
    import map_color_cases as mc
    from vslam_pose_estimation_framework_amd import color
    cfg, p, _, frames = worlds[2]
    _env(monkeypatch, graph)
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    rng = np.random.default_rng(9)
    fmt = color.BGRA8
    try:
        a.set_color_input(fmt)
        a.set_downscale(2, *FULL)
        a.enable_map(6000); a.enable_map_colors(True)
        rgb, history = np.zeros((0, 3), np.uint8), []
        for k in range(8):
            L, D, _, d = frames[1][k]
            c = col.as_format(col.colourise(L, rng), fmt, rng)
            G = color.to_gray_u8(c, fmt)
            small = downscale.downscale_u8(G, 2)
            (fa, na), (fb, nb) = a.process(c, D), b.process(small, d)
            _same_info(fa, fb, "frame %d" % k); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % k)
            np.testing.assert_array_equal(a.gray(), G)
            np.testing.assert_array_equal(a.downscaled()[0], small)
            rgb, _ = mc.rgbd_step(rgb, history, a.point_ids(), a.points()["xy"], a.map()["last_frame"], k, downscale.downscale_u8(c, 2), fmt)
            np.testing.assert_array_equal(a.map_colors(), rgb, err_msg="colours frame %d" % k)
        assert fa.status == 1 and len(rgb) > 50 and (rgb[:, 0] != rgb[:, 2]).mean() > 0.9
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_downscale_ahead_of_undistortion_bilateral_and_clahe(worlds, monkeypatch):
    """Full frames of 401 x 1281 of a distorting lens: downscale to the raw 200 x 640, undistort to 188 x 620 (image bilinear, depth
    nearest), bilateral filter on the depth, CLAHE on the image, all on the device == the numpy chain then run."""
    import clahe_cases as cc
    import undistort_cases as uc
    from test_undistort_gpu import RAW_COLS, RAW_ROWS, SHIFT
    from vslam_pose_estimation_framework_amd import bilateral, rectify
    cfg, p, K, frames = worlds[2]
    _env(monkeypatch)
    g = hip.load()
    cam = uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT)
    und, lens = rectify.undistortion(cam, K, int(cfg.rows), int(cfg.cols)), uc.distorting_maps(cam, K)
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    full = (2 * RAW_ROWS + 1, 2 * RAW_COLS + 1)
    try:
        a.set_undistortion(und)
        a.set_downscale(2, *full)
        a.set_bilateral(True, 2.0, 2.0)
        a.set_clahe(True)
        for k in range(6):
            rawL, rawD = uc.distort_frame(lens, frames[0][k][2], frames[0][k][3])       # the raw pair the downscale must produce
            bigL = np.zeros(full, np.uint8); bigD = np.zeros(full, np.uint16)
            bigL[:2 * RAW_ROWS, :2 * RAW_COLS] = np.repeat(np.repeat(rawL, 2, 0), 2, 1)  # constant blocks: their average and their median are the value
            bigD[:2 * RAW_ROWS, :2 * RAW_COLS] = np.repeat(np.repeat(rawD, 2, 0), 2, 1)
            bigL[1::2, ::2][:RAW_ROWS, :RAW_COLS] += (bigL[1::2, ::2][:RAW_ROWS, :RAW_COLS] < 255)      # one pixel of four a count brighter: still rounds to the value
            bigL[-1, :] = 255; bigD[:, -1] = 65535                                       # the dropped row and column
            np.testing.assert_array_equal(downscale.downscale_u8(bigL, 2), rawL)
            np.testing.assert_array_equal(downscale.downscale_depth_u16(bigD, 2), rawD)
            L, D = und.apply(rawL, rawD)
            E = cc.clahe_image(L)
            F = bilateral.bilateral_depth_u16(D, float(p.depth_scale_factor_intensity_to_meters), 2.0, 2.0)
            (fa, na), (fb, nb) = a.process(bigL, bigD), b.process(E, F)
            _same_info(fa, fb, "frame %d" % k); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % k)
            gi, gd = a.downscaled()
            np.testing.assert_array_equal(gi, rawL); np.testing.assert_array_equal(gd, rawD)
            np.testing.assert_array_equal(a.undistorted()[1], D)
            np.testing.assert_array_equal(a.equalized(), E)
            np.testing.assert_array_equal(a.filtered_depth()[0], F)
        assert fa.status == 1 and fa.n_tracked > 50
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_downscale_ahead_of_the_orb_detector(worlds, monkeypatch):
    """detector_type ORB in the device-resident loop, which sits behind the stage: 6 frames, both trackers' outputs equal."""
    cfg, p, _, frames = worlds[2]
    cfg = cfg.copy()
    cfg.detector_type = 1
    _env(monkeypatch)
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_downscale(2, *FULL)
        for k in range(6):
            L, D, l, d = frames[0][k]
            (fa, na), (fb, nb) = a.process(L, D), b.process(l, d)
            _same_info(fa, fb, "frame %d" % k); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % k)
        assert fa.n_points > 0
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_rgbd_downscale_contract(worlds, monkeypatch):
    cfg, p, _, frames = worlds[2]
    _env(monkeypatch)
    g = hip.load()
    lib = g.lib
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    rows, cols = int(cfg.rows), int(cfg.cols)
    img = np.zeros((rows, cols), np.uint8); dep = np.zeros((rows, cols), np.uint16)
    pi, pd = img.ctypes.data_as(C.c_void_p), dep.ctypes.data_as(C.c_void_p)
    try:
        assert lib.vslam_rgbd_set_downscale(None, C.c_int32(2), C.c_int32(FULL[0]), C.c_int32(FULL[1])) == ERR_INVALID
        assert lib.vslam_rgbd_get_downscaled(None, C.c_int32(0), pi, pd) == ERR_INVALID
        assert lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(0), pi, pd) == ERR_STATE                 # off
        for fac, r, c_ in ((0, ) + FULL, (5, ) + FULL, (3, ) + FULL, (2, FULL[0] + 2, FULL[1]), (2, FULL[0], FULL[1] + 2), (2, 0, FULL[1]), (2, 40000, FULL[1])):
            assert lib.vslam_rgbd_set_downscale(a.h, C.c_int32(fac), C.c_int32(r), C.c_int32(c_)) == ERR_INVALID, (fac, r, c_)
            assert a.downscale() == (1, 0, 0)
        # on then off == never on
        a.set_downscale(2, *FULL)
        assert lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(0), pi, pd) == ERR_STATE                 # before a frame
        a.set_downscale(1)
        for k in range(2):
            _, _, l, d = frames[0][k]
            (fa, na), (fb, nb) = a.process(l, d), b.process(l, d)
            _same_info(fa, fb, "off frame %d" % k); _same_points(a.points(), b.points(), "off frame %d" % k)
        # on: a frame in flight refuses the setter and the getter; the switch survives the reset, the getter does not
        a.set_downscale(2, *FULL)
        a.reset(); b.reset()
        assert a.downscale() == (2,) + FULL
        L, D, l, d = frames[0][0]
        a.submit(L, D)
        assert lib.vslam_rgbd_set_downscale(a.h, C.c_int32(1), C.c_int32(0), C.c_int32(0)) == ERR_STATE
        assert lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(0), pi, pd) == ERR_STATE
        fa, na = a.wait()
        fb, nb = b.process(l, d)
        _same_info(fa, fb, "after reset"); _same_points(a.points(), b.points(), "after reset")
        gi, gd = a.downscaled()
        np.testing.assert_array_equal(gi, l); np.testing.assert_array_equal(gd, d)
        assert lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(0), None, pd) == 0 and lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(0), pi, None) == 0
        np.testing.assert_array_equal(img, l); np.testing.assert_array_equal(dep, d)
        assert lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(1), pi, pd) == ERR_INVALID
        a.reset()
        assert lib.vslam_rgbd_get_downscaled(a.h, C.c_int32(0), pi, pd) == ERR_STATE and a.downscale() == (2,) + FULL
        # a frame of the reduced size is refused while the switch is on
        with pytest.raises(VslamError) as e:
            a.process(l, d)
        assert e.value.code == ERR_INVALID
    finally:
        a.destroy(); b.destroy()
    # the size check against the undistortion maps, in both setter orders
    import undistort_cases as uc
    from test_undistort_gpu import RAW_COLS, RAW_ROWS, SHIFT
    from vslam_pose_estimation_framework_amd import rectify
    K = worlds[2][2]
    und = rectify.undistortion(uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT), K, rows, cols)
    t = RgbdTracker(g, cfg, p)
    try:
        t.set_undistortion(und)
        assert lib.vslam_rgbd_set_downscale(t.h, C.c_int32(2), C.c_int32(FULL[0]), C.c_int32(FULL[1])) == ERR_INVALID       # 188 x 620 is not the raw 200 x 640
        t.set_downscale(2, 2 * RAW_ROWS, 2 * RAW_COLS + 1)
        with pytest.raises(VslamError) as e:
            t.set_undistortion(None)
        assert e.value.code == ERR_INVALID and t.downscale() == (2, 2 * RAW_ROWS, 2 * RAW_COLS + 1)
        t.set_downscale(1); t.set_undistortion(None); t.set_downscale(2, *FULL)
        with pytest.raises(VslamError) as e:
            t.set_undistortion(und)
        assert e.value.code == ERR_INVALID and t.downscale() == (2,) + FULL
    finally:
        t.destroy()
    # the host-driven loop does not get the feature
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        assert lib.vslam_rgbd_set_downscale(h.h, C.c_int32(2), C.c_int32(FULL[0]), C.c_int32(FULL[1])) == ERR_STATE
        assert lib.vslam_rgbd_get_downscaled(h.h, C.c_int32(0), pi, pd) == ERR_STATE
        assert h.downscale() == (1, 0, 0)
    finally:
        h.destroy()
