"""Colour input in RGB-D mode (vslam_rgbd_set_color_input, csrc/kernels_gray.h): the fused path equal bit for bit to
numpy-grey-then-run for one sequence, under the captured launch sequence, for a batch and for device frames, with the map and the log on,
ahead of the undistortion and of the equalisation, across a frame with several registration attempts, and the contract of the switch."""
import numpy as np
import pytest

import color_cases as cc
import undistort_cases as uc
from test_undistort_gpu import RAW_COLS, RAW_ROWS, SHIFT, _pad, _same_info, _same_points
from vslam_pose_estimation_framework_amd import color, equalize, hip, rectify
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

FRAMES = cc.RGBD_FRAMES
RGB8, BGRA8 = color.RGB8, color.BGRA8


@pytest.fixture(scope="module")
def worlds():
    """Rendered once: the tum configuration at 620 x 188; per world FRAMES frames as (RGB image, depth, numpy grey)."""
    from _oracle import Oracle
    o = Oracle()
    try:
        out = []
        for seed in cc.RGBD_SEEDS:
            cfg, p, K, frames = cc.rgbd_world(o, seed)
            out.append(frames)
    finally:
        o.destroy()
    assert (out[0][0][2] != out[0][0][0][..., 1]).mean() >= 0.8             # the premise: the grey is not a channel passed through
    return cfg, p, K, out


def _check_map(a, b, f):
    np.testing.assert_array_equal(a.point_ids(), b.point_ids())
    ma, mb, oa, ob = a.map(), b.map(), a.observations(), b.observations()
    for k in ma:
        np.testing.assert_array_equal(ma[k], mb[k], err_msg="map %s frame %d" % (k, f))
    for k in oa:
        np.testing.assert_array_equal(oa[k], ob[k], err_msg="log %s frame %d" % (k, f))
    return ma, oa


def _rows_padded(c, extra=12, fill=7):
    """[..., rows, cols, ch] -> [..., rows, ch * cols + extra]: interleaved rows with padding bytes behind them."""
    return _pad(np.ascontiguousarray(c).reshape(c.shape[:-2] + (c.shape[-2] * c.shape[-1],)), extra, fill)


@pytest.mark.gpu
@pytest.mark.parametrize("case,fmt", [("one", RGB8), ("one", BGRA8), ("one-graph", RGB8), ("batch3", BGRA8), ("batch3-graph", RGB8),
                                      ("batch3-device", RGB8), ("batch3-device", BGRA8), ("one-map", RGB8)])
def test_fused_color_equals_gray_then_run(case, fmt, worlds, monkeypatch):
    """Tracker A converts the colour frames itself, tracker B gets the numpy grey; the depth input is the same.  After every frame: frame
    info (poses in it) and the complete point lists bit for bit, gray() the numpy image."""
    cfg, p, _, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case.endswith("graph") else "0")
    g = hip.load()
    B = 3 if case.startswith("batch3") else 1
    if B == 1:
        a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    else:
        a, b = RgbdBatch(g, cfg, p, B), RgbdBatch(g, cfg, p, B)
    rng = np.random.default_rng(fmt)
    try:
        a.set_color_input(fmt)
        if case == "one-map":
            for t in (a, b):
                t.enable_map(6000); t.enable_observations(60000)
        for f in range(FRAMES):
            col = cc.as_format(np.stack([frames[s][f][0] for s in range(B)]), fmt, rng)
            D = np.stack([frames[s][f][1] for s in range(B)])
            G = np.stack([frames[s][f][2] for s in range(B)])
            if B == 1:
                # rows with padding bytes behind them, and the [rows, cols, ch] form, in turn
                ia, ib = [a.process(_rows_padded(col[0]) if f % 2 else col[0], D[0])], [b.process(G[0], D[0])]
                pa, pb = [a.points()], [b.points()]
            else:
                if case == "batch3-device":
                    import torch
                    dev = torch.device("cuda", 0)
                    raw = _rows_padded(col)
                    Ld = torch.from_numpy(raw).to(dev); Dd = torch.from_numpy(D.view(np.int16)).to(dev)
                    torch.cuda.synchronize()
                    a.submit_device(Ld.data_ptr(), raw.shape[2], raw.shape[1] * raw.shape[2], Dd.data_ptr(), D.shape[2], D.shape[1] * D.shape[2])
                    ia = a.wait()
                    np.testing.assert_array_equal(Ld.cpu().numpy(), raw, err_msg="the caller's device images were written")
                    np.testing.assert_array_equal(Dd.cpu().numpy().view(np.uint16), D, err_msg="the caller's depth images were written")
                else:
                    ia = a.process(col if case == "batch3-graph" else _rows_padded(col), D)
                ib = b.process(G, D)
                pa, pb = [a.points(s) for s in range(B)], [b.points(s) for s in range(B)]
            for s in range(B):
                tag = "%s %s frame %d sequence %d" % (case, color.NAMES[fmt], f, s)
                _same_info(ia[s][0], ib[s][0], tag)
                assert ia[s][1] == ib[s][1], tag
                _same_points(pa[s], pb[s], tag)
                np.testing.assert_array_equal(a.gray(s), G[s], err_msg=tag + " image")
            if case == "one-map":
                ma, oa = _check_map(a, b, f)
        assert all(fi.status == 1 and fi.n_tracked > 50 for fi, _ in ia)          # equal and tracking, not equal and empty
        if case == "one-map":
            assert len(ma["id"]) > 50 and len(oa["id"]) > 200
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_color_ahead_of_undistortion(worlds, monkeypatch):
    """Raw colour frames of freiburg1's lens (200 x 640): grey, then undistort on the device == numpy grey, numpy undistort, then run.
    gray() is the raw grey image, undistorted() the pair the frame ran on."""
    cfg, p, K, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    cam = uc.raw_camera(K, uc.FREIBURG1, RAW_ROWS, RAW_COLS, SHIFT)
    und, lens = rectify.undistortion(cam, K, int(cfg.rows), int(cfg.cols)), uc.distorting_maps(cam, K)
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    rng = np.random.default_rng(31)
    try:
        a.set_undistortion(und)
        a.set_color_input(RGB8)
        for f in range(6):
            rawL, rawD = uc.distort_frame(lens, frames[0][f][2], frames[0][f][1])
            rawC = cc.colourise(rawL, rng)
            rawG = color.to_gray_u8(rawC, RGB8)
            L, D = und.apply(rawG, rawD)
            (fa, na), (fb, nb) = a.process(rawC, rawD), b.process(L, D)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            assert a.gray().shape == (RAW_ROWS, RAW_COLS)
            np.testing.assert_array_equal(a.gray(), rawG)
            ui, ud = a.undistorted()
            np.testing.assert_array_equal(ui, L); np.testing.assert_array_equal(ud, D)
        assert fa.status == 1 and fa.n_tracked > 50
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("graph", [0, 1])
def test_color_ahead_of_equalization(graph, worlds, monkeypatch):
    """Grey, then equalise on the device == numpy grey, numpy equalise, then run.  The grey image is equalised in place, so gray() and
    equalized() both return the equalised image then."""
    cfg, p, _, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", str(graph))
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_equalization(True)
        a.set_color_input(BGRA8)
        for f in range(6):
            c, D, G = frames[1][f]
            E = equalize.equalize_hist_u8(G)[0]
            assert (E != G).mean() > 0.5
            (fa, na), (fb, nb) = a.process(cc.as_format(c, BGRA8), D), b.process(E, D)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            np.testing.assert_array_equal(a.equalized(), E)
            np.testing.assert_array_equal(a.gray(), E)
        assert fa.status == 1 and fa.n_tracked > 50
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_second_registration_attempt_reads_the_grey_image_again(monkeypatch):
    """The scenario of test_rgbd_reregistration_paths (icl, a jump) on colour frames (color_cases.reregistration_scenario): a frame that
    needs further registration attempts is converted once, and its attempts read the grey image: the run equals the one on numpy-grey
    frames."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    o = Oracle()
    try:
        cfg, p, frames = cc.reregistration_scenario(o)
    finally:
        o.destroy()
    g = hip.load()
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_color_input(RGB8)
        attempts = []
        for f, (c, D) in enumerate(frames):
            G = color.to_gray_u8(c, RGB8)
            (fa, na), (fb, nb) = a.process(c, D), b.process(G, D)
            _same_info(fa, fb, "frame %d" % f); assert na == nb
            _same_points(a.points(), b.points(), "frame %d" % f)
            np.testing.assert_array_equal(a.gray(), G, err_msg="frame %d after %d attempts" % (f, fa.track_attempts))
            attempts.append(fa.track_attempts)
        assert max(attempts) >= 2, attempts
    finally:
        a.destroy(); b.destroy()


@pytest.mark.gpu
def test_rgbd_color_contract(worlds, monkeypatch):
    cfg, p, _, frames = worlds
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    g = hip.load()
    seq = frames[0]
    t, u = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        assert g.lib.vslam_rgbd_set_color_input(None, RGB8) == ERR_INVALID
        with pytest.raises(VslamError) as e:                       # off
            t.gray()
        assert e.value.code == ERR_STATE
        for bad in (-1, 5):
            with pytest.raises(VslamError) as e:
                t.set_color_input(bad)
            assert e.value.code == ERR_INVALID
        t.set_color_input(RGB8)
        with pytest.raises(VslamError) as e:                       # on, but no frame yet
            t.gray()
        assert e.value.code == ERR_STATE
        with pytest.raises(VslamError) as e:
            t.gray(1)
        assert e.value.code == ERR_INVALID
        with pytest.raises(VslamError) as e:                       # a grey frame's row stride is below channels * cols
            t.process(seq[0][2], seq[0][1])
        assert e.value.code == ERR_INVALID and "row stride" in str(e.value)
        t.process(seq[0][0], seq[0][1])
        np.testing.assert_array_equal(t.gray(), seq[0][2])
        t.submit(seq[1][0], seq[1][1])
        for call in (lambda: t.set_color_input(color.GRAY8), lambda: t.set_color_input(BGRA8), t.gray):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "in flight" in str(e.value)
        fi, _ = t.wait()
        assert fi.n_points > 50
        # the switch survives reset(), the last frame is forgotten
        t.reset()
        with pytest.raises(VslamError) as e:
            t.gray()
        assert e.value.code == ERR_STATE
        for f in range(3):
            (fa, na), (fb, nb) = t.process(seq[f][0], seq[f][1]), u.process(seq[f][2], seq[f][1])
            _same_info(fa, fb, "after reset frame %d" % f)
        np.testing.assert_array_equal(t.gray(), seq[2][2])
        # on then off: as never set
        t.set_color_input(color.GRAY8); t.reset(); u.reset()
        for f in range(3):
            (fa, na), (fb, nb) = t.process(seq[f][2], seq[f][1]), u.process(seq[f][2], seq[f][1])
            _same_info(fa, fb, "off frame %d" % f)
        with pytest.raises(VslamError) as e:
            t.gray()
        assert e.value.code == ERR_STATE
    finally:
        t.destroy(); u.destroy()
    # the host-driven loop does not have the feature and says so; it goes on tracking
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: h.set_color_input(RGB8), lambda: h.set_color_input(color.GRAY8), h.gray):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
        fi, _ = h.process(seq[0][2], seq[0][1])
        assert fi.n_points > 50
    finally:
        h.destroy()
