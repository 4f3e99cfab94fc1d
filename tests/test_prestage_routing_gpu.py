"""Routing of the input stages ("Routing of the input stages"): colour to grey, remap (rectification / undistortion) and
equalisation (global or CLAHE) all on at once, and switched mid-sequence, in both trackers.  Getters only, bit for bit against the numpy
references of the package composed in chain order; tracking results are not judged.

Shapes chosen for the tails the routing can get wrong: processed size 83 x 61 (no multiple of 4 or 16: k_rectify's word-store tail, the
16-byte head and tail of the other kernels), raw size 95 x 70, caller rows of width * channels + 7 bytes that start 3 bytes into their
buffer, CLAHE with tiles (4, 3) and clip 4.0.  Frames are seeded uniform noise, the maps a synthetic radial pair, depth a constant plane."""
import ctypes as C

import numpy as np
import pytest

import map_color_cases as mc
from vslam_pose_estimation_framework_amd import clahe, color, equalize, hip, rectify
from vslam_pose_estimation_framework_amd.capi import DepthParams, RgbdBatch, RgbdTracker

ROWS, COLS, RAW_ROWS, RAW_COLS = 61, 83, 70, 95
EXTRA, OFFSET, FILL = 7, 3, 0xA5
CLIP, TILES = 4.0, (4, 3)
K = np.array([[60.0, 0, 41.5], [0, 60.0, 30.5], [0, 0, 1.0]])
DEPTH_RAW = 1000                        # x 2e-3 m


def _rig():
    """Two raw cameras with radial distortion (95 x 70) in front of the pinhole pair K (83 x 61): the stereo maps and the left camera's
    undistortion."""
    Kraw = np.array([[68.0, 0, 47.0], [0, 68.0, 34.5], [0, 0, 1.0]])
    left = rectify.CameraModel(Kraw, (-0.22, 0.06, 0.0, 0.0, 0.0), RAW_ROWS, RAW_COLS)
    right = rectify.CameraModel(Kraw, (-0.18, 0.04, 0.0, 0.0, 0.0), RAW_ROWS, RAW_COLS)
    P1 = np.concatenate([K, np.zeros((3, 1))], axis=1)
    P2 = P1.copy(); P2[0, 3] = -30.0
    return rectify.Rectification(left, right, np.eye(3), np.eye(3), P1, P2, ROWS, COLS), rectify.undistortion(left, K, ROWS, COLS)


RECT, UND = _rig()


def _config(g):
    cfg = g.default_config("kitti")
    cfg.rows, cfg.cols = ROWS, COLS
    for i in range(9):
        cfg.K[i] = float(K.ravel()[i])
    cfg.baseline_h[0] = -30.0
    cfg.bin_size_pixels = 6
    return cfg


def _chain(img, fmt, maps, mode):
    """The stages in chain order on one image: what each getter must return."""
    out = {}
    if fmt != color.GRAY8:
        img = out["gray"] = color.to_gray_u8(img, fmt)
    if maps is not None:
        img = out["remap"] = rectify.remap_u8(img, *maps)
    if mode == "clahe":
        out["eq"], out["luts"] = clahe.clahe_u8(img, CLIP, TILES)
    else:
        out["eq"], out["hist"] = equalize.equalize_hist_u8(img)[:2]
    return out


def _noise(rng, B, rows, cols, fmt):
    ch = color.channels(fmt)
    return rng.integers(0, 256, (B, rows, cols) + ((ch,) if ch > 1 else ())).astype(np.uint8)


def _strided(px, rows):
    """Images [B, rows, ...] as the caller's buffer: rows of row bytes + EXTRA, the first one OFFSET bytes in, FILL everywhere else.
    (buffer, byte offset of the first image, row stride, stream stride)."""
    B = px.shape[0]
    flat = px.reshape(B, rows, -1)
    stride = flat.shape[2] + EXTRA
    buf = np.full(OFFSET + B * rows * stride, FILL, np.uint8)
    buf[OFFSET:].reshape(B, rows, stride)[..., :flat.shape[2]] = flat
    return buf, OFFSET, stride, rows * stride


def _to_device(buf):
    import torch
    t = torch.from_numpy(buf).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _unchanged(t, buf, what):
    np.testing.assert_array_equal(t.cpu().numpy(), buf, err_msg="the caller's %s device images were written" % what)


# ---- stereo -------------------------------------------------------------------------------------------------------------------------
# (colour format, rectification, slot mode) of the four checked frames: everything on with CLAHE; global equalisation instead; rectification
# off with equalisation still on (the rectified pair's own slabs go); colour off
STEREO_PHASES = [(color.BGR8, True, "clahe"), (color.BGR8, True, "eq"), (color.BGR8, False, "eq"), (color.GRAY8, False, "eq")]


def _stereo_switch(a, state, want):
    fmt, rect, mode = want
    if state is None:
        a.set_color_input(fmt); a.set_rectification(RECT if rect else None)
        a.set_clahe(True, CLIP, TILES) if mode == "clahe" else a.set_equalization(True)
        return
    if mode != state[2]:
        a.set_clahe(False); a.set_equalization(True)
    if rect != state[1]:
        a.set_rectification(RECT if rect else None)
    if fmt != state[0]:
        a.set_color_input(fmt)


def _stereo_submit(a, stage, device, L, R, rows):
    bl, off, stride, stream = _strided(L, rows)
    br = _strided(R, rows)[0]
    if device:
        tl, tr = _to_device(bl), _to_device(br)
        pl, pr = tl.data_ptr() + off, tr.data_ptr() + off
    else:
        pl, pr = bl.ctypes.data + off, br.ctypes.data + off
    args = (a.ctx, C.c_void_p(pl), C.c_void_p(pr), C.c_int32(stride), C.c_size_t(stream))
    if stage:
        a.check(a.fn("frame_begin")(*args, C.c_int(1 if device else 0)))
        a.check(a.fn("frame_finish")(a.ctx))
    else:
        a.check(a.fn("process_device" if device else "process_host")(*args))
    a.synchronize()
    if device:
        _unchanged(tl, bl, "left"); _unchanged(tr, br, "right")


def _stereo_check(a, s, want, tag, tables=True):
    """Every getter that is valid in this phase, stream s, against want[side].  Without rectification the grey pair is written where the
    equalisation works in place: gray_images() is the equalised pair then."""
    for name, get in (("gray", a.gray_images), ("remap", a.rectified_images), ("eq", a.equalized_images)):
        if name in want[0]:
            for side, got in enumerate(get(s)):
                ref = want[side]["eq" if name == "gray" and "remap" not in want[0] else name]
                np.testing.assert_array_equal(got, ref, err_msg="%s %s side %d" % (tag, name, side))
    if tables and "luts" in want[0]:
        np.testing.assert_array_equal(a.clahe_luts(s), np.stack([w["luts"] for w in want]), err_msg=tag + " tables")
    if tables and "hist" in want[0]:
        np.testing.assert_array_equal(a.equalization_histograms(s), np.stack([w["hist"] for w in want]), err_msg=tag + " histogram")


@pytest.mark.gpu
@pytest.mark.parametrize("B,stage,device", [(3, False, False), (3, False, True), (1, True, False), (1, True, True)],
                         ids=["B3-host", "B3-device", "B1-stage-host", "B1-stage-device"])
def test_stereo_chain_and_switches(B, stage, device):
    """Four checked frames, the switches flipped between them (STEREO_PHASES).  B = 3: stream 1 is switched off for the checked frame; two
    frames with every stream on come first in each phase (one per step parity), so that its planes hold a known pair, which must still be
    there afterwards (one exception: a grey host frame is uploaded as one block, so that stream's planes hold what came in, unprocessed)."""
    g = hip.load()
    g.create(_config(g), 0, B)
    rng = np.random.default_rng(1000 + 10 * B + int(device))
    state = None
    try:
        for k, phase in enumerate(STEREO_PHASES):
            fmt, rect, mode = phase
            _stereo_switch(g, state, phase)
            state = phase
            rows, cols = (RAW_ROWS, RAW_COLS) if rect else (ROWS, COLS)
            maps = [(RECT.map_xy_left, RECT.map_a_left), (RECT.map_xy_right, RECT.map_a_right)] if rect else [None, None]
            if B > 1:
                g.set_stream_active(1, True)
                S = [_noise(rng, B, rows, cols, fmt) for _ in range(2)]
                for _ in range(2):
                    _stereo_submit(g, stage, device, S[0], S[1], rows)
                sentinel = [_chain(S[side][1], fmt, maps[side], mode) for side in range(2)]
                _stereo_check(g, 1, sentinel, "phase %d sentinel" % k)
                g.set_stream_active(1, False)
            X = [_noise(rng, B, rows, cols, fmt) for _ in range(2)]
            _stereo_submit(g, stage, device, X[0], X[1], rows)
            for s in range(B):
                tag = "phase %d stream %d" % (k, s)
                if B > 1 and s == 1 and not (fmt == color.GRAY8 and not rect and not device):
                    _stereo_check(g, 1, sentinel, tag + " (switched off)", tables=False)
                elif B > 1 and s == 1:
                    # a grey host frame is copied into upload[parity] as one block, this stream's images with it: no stage touched them
                    _stereo_check(g, 1, [{"eq": X[side][1]} for side in range(2)], tag + " (switched off, as uploaded)", tables=False)
                else:
                    _stereo_check(g, s, [_chain(X[side][s], fmt, maps[side], mode) for side in range(2)], tag)
    finally:
        g.destroy()


# ---- RGB-D --------------------------------------------------------------------------------------------------------------------------
# (colour format, undistortion, slot mode), two frames each: everything on with CLAHE; global equalisation instead; undistortion off (the
# input size changes: the grey image is allocated again and a captured launch sequence dropped)
RGBD_PHASES = [(color.RGBA8, True, "clahe"), (color.RGBA8, True, "eq"), (color.RGBA8, False, "eq")]


def _rgbd_setup(g):
    cfg = _config(g)
    cfg.aligner_minimum_number_of_inliers = 0
    Ki = np.linalg.inv(K)
    return cfg, DepthParams.make(ROWS, COLS, K, Ki, Ki, np.eye(4)[:3], 2e-3, 0.1, 10.0, 1, 1, 6, 0)


def _rgbd_switch(a, state, want):
    fmt, und, mode = want
    if state is None:
        a.set_color_input(fmt); a.set_undistortion(UND if und else None)
        a.set_clahe(True, CLIP, TILES) if mode == "clahe" else a.set_equalization(True)
        return
    if mode != state[2]:
        a.set_clahe(False); a.set_equalization(True)
    if und != state[1]:
        a.set_undistortion(UND if und else None)


def _rgbd_submit(a, B, device, col, D, rows):
    """col [B, rows, cols, 4] in the caller's strided buffer, D [B, rows, cols] dense; waits for the frame."""
    buf, off, stride, stream = _strided(col, rows)
    D = np.ascontiguousarray(D)
    dp = D.ctypes.data_as(C.POINTER(C.c_uint16))
    if device:
        t, td = _to_device(buf), _to_device(D.view(np.int16))
        a.submit_device(t.data_ptr() + off, stride, stream, td.data_ptr(), D.shape[2], D.shape[1] * D.shape[2])
    elif B == 1:
        a._check(a.lib.vslam_rgbd_submit_host(a.h, C.c_void_p(buf.ctypes.data + off), C.c_int32(stride), dp, C.c_int32(D.shape[2])))
    else:
        a._check(a.lib.vslam_rgbd_submit_batch_host(a.h, C.c_void_p(buf.ctypes.data + off), C.c_int32(stride), C.c_size_t(stream), dp, C.c_int32(D.shape[2]),
                                                    C.c_size_t(D.shape[1] * D.shape[2])))
    a.wait()
    if device:
        _unchanged(t, buf, "colour")
        np.testing.assert_array_equal(td.cpu().numpy().view(np.uint16), D, err_msg="the caller's depth images were written")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["one", "one-graph", "batch3-host", "batch3-device"])
def test_rgbd_chain_and_switches(case, monkeypatch):
    """After every frame gray(), undistorted(), equalized() and clahe_luts() against numpy.  The equalisation runs in place in the image the
    detector reads: undistorted()[0] is the processed image while undistorting, gray() is without."""
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case == "one-graph" else "0")
    g = hip.load()
    cfg, p = _rgbd_setup(g)
    B = 3 if case.startswith("batch3") else 1
    device = case == "batch3-device"
    a = RgbdTracker(g, cfg, p) if B == 1 else RgbdBatch(g, cfg, p, B)
    rng = np.random.default_rng(2000 + len(case))
    state, f = None, 0
    sget = (lambda get, s: get()) if B == 1 else (lambda get, s: get(s))
    try:
        for phase in RGBD_PHASES:
            fmt, und, mode = phase
            _rgbd_switch(a, state, phase)
            state = phase
            rows, cols = (RAW_ROWS, RAW_COLS) if und else (ROWS, COLS)
            maps = (UND.map_xy, UND.map_a) if und else None
            for _ in range(2):
                col = _noise(rng, B, rows, cols, fmt)
                D = np.full((B, rows, cols), DEPTH_RAW, np.uint16)
                Dn = rectify.remap_nearest_u16(D[0], *maps) if und else D[0]
                _rgbd_submit(a, B, device, col, D, rows)
                for s in range(B):
                    tag = "%s frame %d sequence %d" % (case, f, s)
                    w = _chain(col[s], fmt, maps, mode)
                    np.testing.assert_array_equal(sget(a.equalized, s), w["eq"], err_msg=tag + " equalized")
                    if und:
                        np.testing.assert_array_equal(sget(a.gray, s), w["gray"], err_msg=tag + " gray")
                        ui, ud = sget(a.undistorted, s)
                        np.testing.assert_array_equal(ui, w["eq"], err_msg=tag + " undistorted image")
                        np.testing.assert_array_equal(ud, Dn, err_msg=tag + " undistorted depth")
                    else:
                        np.testing.assert_array_equal(sget(a.gray, s), w["eq"], err_msg=tag + " gray (in place)")
                    if mode == "clahe":
                        np.testing.assert_array_equal(sget(a.clahe_luts, s), w["luts"], err_msg=tag + " tables")
                f += 1
    finally:
        a.destroy()


@pytest.mark.gpu
def test_rgbd_map_colors_behind_all_stages(monkeypatch):
    """The map and its colours with colour input, undistortion and CLAHE all on.  The noise frames above leave the map empty (4 - 5 points
    a frame), so this case runs on a rendered world at its own size (color_cases.rgbd_world, 620 x 188, behind freiburg1's lens at 640 x
    200, 6 frames).  Tracker b gets the numpy-processed frames: ids and map must agree; b has no colour to sample, so the colours are
    held against color.sample_rgb on the raw colour frame through the undistortion map, at the points of these shared lists."""
    import color_cases as cc
    import undistort_cases as uc
    from _oracle import Oracle
    from test_undistort_gpu import RAW_COLS as LENS_COLS, RAW_ROWS as LENS_ROWS, SHIFT
    o = Oracle()
    try:
        cfg, p, Kw, frames = cc.rgbd_world(o, cc.RGBD_SEEDS[0], 6)
    finally:
        o.destroy()
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    cam = uc.raw_camera(Kw, uc.FREIBURG1, LENS_ROWS, LENS_COLS, SHIFT)
    und, lens = rectify.undistortion(cam, Kw, int(cfg.rows), int(cfg.cols)), uc.distorting_maps(cam, Kw)
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    rng = np.random.default_rng(31)
    rgb, history = np.zeros((0, 3), np.uint8), []
    try:
        a.set_color_input(color.RGBA8); a.set_undistortion(und); a.set_clahe(True, CLIP, TILES)
        a.enable_map(6000); b.enable_map(6000)
        a.enable_map_colors(True)
        for f in range(6):
            rawL, rawD = uc.distort_frame(lens, frames[f][2], frames[f][1])
            rawC = cc.as_format(cc.colourise(rawL, rng), color.RGBA8, rng)
            G = color.to_gray_u8(rawC, color.RGBA8)
            U, D = und.apply(G, rawD)
            E = clahe.clahe_u8(U, CLIP, TILES)[0]
            a.process(rawC, rawD); b.process(E, D)
            np.testing.assert_array_equal(a.gray(), G); np.testing.assert_array_equal(a.equalized(), E)
            np.testing.assert_array_equal(a.undistorted()[1], D)
            np.testing.assert_array_equal(a.point_ids(), b.point_ids(), err_msg="frame %d ids" % f)
            ma, mb = a.map(), b.map()
            for key in ma:
                np.testing.assert_array_equal(ma[key], mb[key], err_msg="frame %d map %s" % (f, key))
            rgb, _ = mc.rgbd_step(rgb, history, a.point_ids(), a.points()["xy"], ma["last_frame"], f, rawC, color.RGBA8, (und.map_xy, und.map_a))
            np.testing.assert_array_equal(a.map_colors(), rgb, err_msg="frame %d colours" % f)
        assert len(rgb) >= 50 and (rgb != 0).any(axis=1).mean() > 0.9, len(rgb)          # equal and filled, not equal and empty
    finally:
        a.destroy(); b.destroy()
