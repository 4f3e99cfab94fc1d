"""CLAHE in RGB-D mode (vslam_rgbd_set_clahe, csrc/kernels_clahe.h): the fused path equal bit for bit to
numpy-CLAHE-then-run for one sequence, under the captured launch sequence, for a batch and for device frames, behind the undistortion and
behind colour input, with the map and the log on, across a frame with several registration attempts, and the contract of the switch."""
import ctypes as C

import numpy as np
import pytest

import clahe_cases as cc
import undistort_cases as uc
from test_rgbd_mode import setup
from test_undistort_gpu import RAW_COLS, RAW_ROWS, SHIFT, _pad, _same_info, _same_points
from vslam_pose_estimation_framework_amd import clahe, hip, rectify
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

FRAMES = 12
SEEDS = (26, 33, 40)


@pytest.fixture(scope="module")
def worlds():
    """Rendered once: the tum configuration at 620 x 188 (neither divisible by 8) and contrast 0.3, shaded; per world FRAMES frames as
    (image, depth, numpy-CLAHE image)."""
    from _oracle import Oracle
    o = Oracle()
    try:
        out = []
        for seed in SEEDS:
            cfg, p, K, frames = cc.rgbd_shaded_frames(o, seed, FRAMES)
            out.append([(L, D, cc.clahe_image(L)) for L, D in frames])
    finally:
        o.destroy()
    assert (out[0][0][2] != out[0][0][0]).mean() > 0.9
    return cfg, p, K, out


def _check_map(a, b, f):
    np.testing.assert_array_equal(a.point_ids(), b.point_ids())
    ma, mb, oa, ob = a.map(), b.map(), a.observations(), b.observations()
    for k in ma:
        np.testing.assert_array_equal(ma[k], mb[k], err_msg="map %s frame %d" % (k, f))
    for k in oa:
        np.testing.assert_array_equal(oa[k], ob[k], err_msg="log %s frame %d" % (k, f))
    return ma, oa


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "one-graph", "batch3", "batch3-graph", "batch3-device", "one-map"])
def test_fused_clahe_equals_clahe_then_run(case, worlds, monkeypatch):
    """Tracker A runs CLAHE on the raw frames (padded rows) itself, tracker B gets the numpy-CLAHE ones; the depth input is the same.
    After every frame: frame info (poses in it) and the complete point lists bit for bit, equalized() and clahe_luts() the numpy ones."""
    cfg, p, _, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case.endswith("graph") else "0")
    g = hip.load()
    B = 3 if case.startswith("batch3") else 1
    if B == 1:
        a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    else:
        a, b = RgbdBatch(g, cfg, p, B), RgbdBatch(g, cfg, p, B)
    try:
        a.set_clahe(True)
        if case == "one-map":
            for t in (a, b):
                t.enable_map(6000); t.enable_observations(60000)
        for f in range(FRAMES):
            raw = _pad(np.stack([frames[s][f][0] for s in range(B)]), 12, 7)
            D = np.stack([frames[s][f][1] for s in range(B)])
            E = np.stack([frames[s][f][2] for s in range(B)])
            if B == 1:
                ia, ib = [a.process(raw[0], D[0])], [b.process(E[0], D[0])]
                pa, pb = [a.points()], [b.points()]
            else:
                if case == "batch3-device":
                    import torch
                    dev = torch.device("cuda", 0)
                    Ld = torch.from_numpy(raw).to(dev); Dd = torch.from_numpy(D.view(np.int16)).to(dev)
                    torch.cuda.synchronize()
                    a.submit_device(Ld.data_ptr(), raw.shape[2], raw.shape[1] * raw.shape[2], Dd.data_ptr(), D.shape[2], D.shape[1] * D.shape[2])
                    ia = a.wait()
                    np.testing.assert_array_equal(Ld.cpu().numpy(), raw, err_msg="the caller's device images were written")
                    np.testing.assert_array_equal(Dd.cpu().numpy().view(np.uint16), D, err_msg="the caller's depth images were written")
                else:
                    ia = a.process(raw, D)
                ib = b.process(E, D)
                pa, pb = [a.points(s) for s in range(B)], [b.points(s) for s in range(B)]
            for s in range(B):
                tag = "%s frame %d sequence %d" % (case, f, s)
                _same_info(ia[s][0], ib[s][0], tag)
                assert ia[s][1] == ib[s][1], tag
                _same_points(pa[s], pb[s], tag)
                np.testing.assert_array_equal(a.equalized(s), E[s], err_msg=tag + " image")
                np.testing.assert_array_equal(a.clahe_luts(s), clahe.clahe_u8(frames[s][f][0])[1], err_msg=tag + " tables")
            if case == "one-map":
                ma, oa = _check_map(a, b, f)
        assert all(fi.status == 1 and fi.n_points >= 150 for fi, _ in ia)          # equal and tracking, not equal and empty
        if case == "one-map":
            assert len(ma["id"]) > 50 and len(oa["id"]) > 200
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_clahe_after_undistortion(worlds, monkeypatch):
    """Raw frames of freiburg1's lens (200 x 640): undistort, then CLAHE on the device == numpy undistort, numpy CLAHE, then run.
    undistorted() still returns the depth image the frame ran on; the image both stages share is the processed one."""
    cfg, p, K, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    cam = uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT)
    und, lens = rectify.undistortion(cam, K, int(cfg.rows), int(cfg.cols)), uc.distorting_maps(cam, K)
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_undistortion(und)
        a.set_clahe(True)
        for f in range(6):
            rawL, rawD = uc.distort_frame(lens, frames[0][f][0], frames[0][f][1])
            L, D = und.apply(rawL, rawD)
            E = cc.clahe_image(L)
            (fa, na), (fb, nb) = a.process(rawL, rawD), b.process(E, D)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            np.testing.assert_array_equal(a.equalized(), E)
            np.testing.assert_array_equal(a.undistorted()[1], D)
        assert fa.status == 1 and fa.n_tracked > 50
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_clahe_behind_color_input(graph, monkeypatch):
    """Grey, then CLAHE on the device == numpy grey, numpy CLAHE, then run.  The grey image is processed in place, so gray() and
    equalized() both return the processed image then."""
    import color_cases as col
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import color
    o = Oracle()
    try:
        cfg, p, _, frames = col.rgbd_world(o, col.RGBD_SEEDS[1])
    finally:
        o.destroy()
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_clahe(True, 4.0, (8, 8))
        a.set_color_input(color.BGRA8)
        for f in range(6):
            c, D, G = frames[f]
            E = cc.clahe_image(G, 4.0)
            assert (E != G).mean() > 0.5
            (fa, na), (fb, nb) = a.process(col.as_format(c, color.BGRA8), D), b.process(E, D)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            np.testing.assert_array_equal(a.equalized(), E)
            np.testing.assert_array_equal(a.gray(), E)
        assert fa.status == 1 and fa.n_tracked > 50
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_second_registration_attempt_reads_the_processed_image_again(monkeypatch):
    """The scenario of test_rgbd_reregistration_paths (icl, stricter landmark minimum, a jump) with CLAHE on: a frame that needs further
    registration attempts is processed once — a second CLAHE of the already processed staging image would change it and with it the
    detector —, and equalized() returns the numpy image afterwards."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    o = Oracle()
    try:
        scene, cfg, p = setup(o, "icl", descriptor=0, max_depth=30.0, seed=41)
        cfg.minimum_number_of_landmarks_to_track = 30
        frames = [(o.render(scene, k)[0], o.render_depth(scene, k, uc.DEPTH_UNIT)) for k in [0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 18]]
    finally:
        o.destroy()
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_clahe(True, 2.0, (8, 8))
        attempts = []
        for f, (L, D) in enumerate(frames):
            E = cc.clahe_image(L, 2.0)
            assert not np.array_equal(cc.clahe_image(E, 2.0), E)              # a second pass would show
            (fa, na), (fb, nb) = a.process(L, D), b.process(E, D)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            np.testing.assert_array_equal(a.equalized(), E, err_msg="frame %d after %d attempts" % (f, fa.track_attempts))
            attempts.append(fa.track_attempts)
        assert max(attempts) >= 2, attempts
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_rgbd_clahe_contract(worlds, monkeypatch):
    cfg, p, _, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    g = hip.load()
    seq = frames[0]
    t, u = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        assert g.lib.vslam_rgbd_set_clahe(None, 1, C.c_double(40.0), 8, 8) == ERR_INVALID
        for call in (t.equalized, t.clahe_luts):                  # off
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE
        for tiles in ((0, 8), (8, 33), (int(cfg.cols), 8)):
            with pytest.raises(VslamError) as e:
                t.set_clahe(True, 40.0, tiles)
            assert e.value.code == ERR_INVALID
        with pytest.raises(VslamError) as e:
            t.set_clahe(True, float("nan"))
        assert e.value.code == ERR_INVALID
        t.set_clahe(True)
        for call in (t.equalized, t.clahe_luts):                  # on, but no frame yet
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE
        with pytest.raises(VslamError) as e:
            t.clahe_luts(1)
        assert e.value.code == ERR_INVALID
        # the two modes exclude each other, in both orders; switching the other one off changes nothing
        with pytest.raises(VslamError) as e:
            t.set_equalization(True)
        assert e.value.code == ERR_STATE and "CLAHE is on" in str(e.value)
        t.set_equalization(False)
        u.set_equalization(True)
        with pytest.raises(VslamError) as e:
            u.set_clahe(True)
        assert e.value.code == ERR_STATE and "global equalisation is on" in str(e.value)
        u.set_clahe(False)
        u.set_equalization(False)
        t.process(seq[0][0], seq[0][1])
        np.testing.assert_array_equal(t.equalized(), seq[0][2])
        t.submit(seq[1][0], seq[1][1])
        for call in (lambda: t.set_clahe(False), lambda: t.set_clahe(True), t.equalized, t.clahe_luts):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "in flight" in str(e.value)
        fi, _ = t.wait()
        assert fi.n_points >= 150
        # the switch survives reset(), the last frame is forgotten
        t.reset()
        with pytest.raises(VslamError) as e:
            t.equalized()
        assert e.value.code == ERR_STATE
        for f in range(3):
            (fa, na), (fb, nb) = t.process(seq[f][0], seq[f][1]), u.process(seq[f][2], seq[f][1])
            _same_info(fa, fb, "after reset frame %d" % f)
        # on then off: as never set
        t.set_clahe(False); t.reset(); u.reset()
        for f in range(3):
            (fa, na), (fb, nb) = t.process(seq[f][2], seq[f][1]), u.process(seq[f][2], seq[f][1])
            _same_info(fa, fb, "off frame %d" % f)
    finally:
        t.destroy(); u.destroy()
    # the host-driven loop does not have the feature and says so; it goes on tracking
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: h.set_clahe(True), lambda: h.set_clahe(False), h.clahe_luts):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
        fi, _ = h.process(seq[0][2], seq[0][1])
        assert fi.n_points > 50
    finally:
        h.destroy()
