"""Detection masks on the device: vslam_mask_pack_u8 against mask.py bit for bit, detection under static and frame masks against the
checker loop of mask_cases.py (validated against the oracle in test_mask_host.py), invariance to what lies under the mask, identity and
lifetime of the two kinds of mask, and the contract's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mask_cases as mc
from pipeline_compare import compare_frame, create_hip
from vslam_pose_estimation_framework_amd import hip, mask
from vslam_pose_estimation_framework_amd.capi import VslamError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID, ERR_STATE = -1, -5
FRAMES = 8


@pytest.fixture(scope="module")
def api():
    g = hip.load()
    g.create(g.default_config("kitti"), 0, 1)
    yield g
    g.destroy()


# ---- 5. the pack kernel -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_pack_equals_numpy(api, shape):
    rows, cols = shape
    for name in mc.CONTENTS:
        img = mc.content(name, rows, cols)
        for m in mc.MARGINS:
            np.testing.assert_array_equal(api.mask_pack_u8(img, m), mask.pack(img, m), err_msg="%s m=%d" % (name, m))


@pytest.mark.parametrize("rows,cols,stride", [(9, 13, 16), (61, 67, 80)])
def test_pack_strides_phases_and_padding(api, rows, cols, stride):
    for pad in (0, 255):
        for phase in (1, 2, 3):
            raw = np.full(rows * stride + 64 + 16, pad, np.uint8)
            base = (-raw.ctypes.data) % 16 + phase
            view = np.lib.stride_tricks.as_strided(raw[base:], (rows, cols), (stride, 1))
            for name in ("half", "holes", "values"):
                view[...] = mc.content(name, rows, cols, seed=phase)
                assert view.ctypes.data % 16 == phase
                for m in (0, 1, 7):
                    np.testing.assert_array_equal(api.mask_pack_u8(view, m), mask.pack(np.ascontiguousarray(view), m),
                                                  err_msg="%s pad=%d phase=%d m=%d" % (name, pad, phase, m))


def test_pack_image_sizes_and_context_reuse(api):
    img = mc.content("holes", 150, 496, 3) & mc.static_blob(150, 496)
    for m in (0, 5, 28, 64):
        np.testing.assert_array_equal(api.mask_pack_u8(img, m), mask.pack(img, m))
    big = mc.content("holes", 376, 1241, 4) & mc.static_blob(376, 1241)
    first = api.mask_pack_u8(big, 28)
    np.testing.assert_array_equal(first, mask.pack(big, 28))
    # one context twice equals two fresh contexts
    np.testing.assert_array_equal(api.mask_pack_u8(big, 28), first)
    for _ in range(2):
        fresh = hip.load()
        fresh.create(fresh.default_config("kitti"), 0, 1)
        try:
            np.testing.assert_array_equal(fresh.mask_pack_u8(big, 28), first)
        finally:
            fresh.destroy()


def test_pack_refusals_write_nothing(api):
    img = mc.content("half", 9, 70)
    words = np.full((9, 2), 0xA5A5A5A5A5A5A5A5, np.uint64)
    f = api.fn("mask_pack_u8")
    p8, pw = img.ctypes.data_as(C.c_void_p), words.ctypes.data_as(C.c_void_p)
    i32 = C.c_int32
    cases = [(api.ctx, p8, i32(9), i32(70), i32(69), i32(0), pw), (api.ctx, p8, i32(9), i32(70), i32(70), i32(65), pw),
             (api.ctx, p8, i32(9), i32(70), i32(70), i32(-1), pw), (api.ctx, None, i32(9), i32(70), i32(70), i32(0), pw),
             (api.ctx, p8, i32(-9), i32(70), i32(70), i32(0), pw), (None, p8, i32(9), i32(70), i32(70), i32(0), pw)]
    for a in cases:
        assert f(*a) == ERR_INVALID
        assert (words == 0xA5A5A5A5A5A5A5A5).all()
    assert f(api.ctx, p8, i32(9), i32(70), i32(70), i32(0), None) == ERR_INVALID
    assert f(api.ctx, p8, i32(0), i32(70), i32(70), i32(0), pw) == 0 and (words == 0xA5A5A5A5A5A5A5A5).all()
    np.testing.assert_array_equal(api.mask_pack_u8(img, 3), mask.pack(img, 3))       # the context is still usable


# ---- the sequences --------------------------------------------------------------------------------------------------------
class Seq(object):
    def __init__(self, seeds, frames=FRAMES, scale=0.4, speed=None):
        from _oracle import Oracle
        self.o = Oracle()
        self.scenes = [self.o.scene_kitti(scale=scale, seed=s) for s in seeds]
        for sc in self.scenes:
            if speed is not None:
                sc.speed_m = speed
        self.cfg = self.o.config_for_scene(self.scenes[0])
        self.o.create(self.cfg, 0, 1)
        self.rows, self.cols = self.scenes[0].rows, self.scenes[0].cols
        imgs = [[self.o.render(sc, k) for sc in self.scenes] for k in range(frames)]
        self.L = [np.stack([im[0] for im in fr]) for fr in imgs]
        self.R = [np.stack([im[1] for im in fr]) for fr in imgs]
        self.blob = mc.static_blob(self.rows, self.cols)


@pytest.fixture(scope="module")
def seq():
    s = Seq((7, 9, 11))
    yield s
    s.o.destroy()


def frame_masks(seq, k, n, small=False):
    """[n, rows, cols] per side; the right side's rectangle is that of another stream index, so that a swap of sides shows."""
    Lm = np.stack([mc.frame_rect(seq.rows, seq.cols, k, s, small) for s in range(n)])
    Rm = np.stack([mc.frame_rect(seq.rows, seq.cols, k, s + 5, small) for s in range(n)])
    return Lm, Rm


def keep_of(seq, static, frame):
    """bool keep-mask of one side from (mask, margin) pairs or None."""
    return mask.unpack(mask.effective(seq.rows, seq.cols, static, frame), seq.cols)


def submit(g, L, R, stage):
    if not stage:
        g.process_host(L, R)
        return
    g.check(g.fn("frame_begin")(g.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]),
                                C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
    g.check(g.fn("frame_finish")(g.ctx))


# ---- 6. detection under masks equals the checker loop -----------------------------------------------------------------------
def run_detection(seq, n, use_static, use_frame, margin, device=False, stage=False, split=None, off=()):
    """n streams; `off`: frames during which stream 1 is switched off."""
    g = create_hip(seq.cfg, n, split=split)
    checkers = [mc.Checker(seq.o, seq.cfg) for _ in range(n)]
    sL = (seq.blob, margin) if use_static else None
    sR = (np.ascontiguousarray(seq.blob[:, ::-1]), margin) if use_static else None       # another mask on the right side
    try:
        if use_static:
            g.set_detection_mask(sL[0], sR[0], margin)
        for k in range(FRAMES):
            L, R = np.ascontiguousarray(seq.L[k][:n]), np.ascontiguousarray(seq.R[k][:n])
            active = [not (s == 1 and k in off) for s in range(n)]
            if n > 1 and (k in off or k - 1 in off):
                g.set_stream_active(1, active[1])
            fm = frame_masks(seq, k, n) if use_frame else None
            if fm is not None:
                if device:
                    import torch
                    tl, tr = torch.from_numpy(fm[0]).cuda(), torch.from_numpy(fm[1]).cuda()
                    if not active[min(1, n - 1)]:
                        tl[1].fill_(0); tr[1].fill_(0)         # never read: the stream is off
                    before = (tl.clone(), tr.clone())
                    g.set_frame_masks(tl, tr, margin)
                else:
                    g.set_frame_masks(fm[0], fm[1], margin)
            submit(g, L, R, stage)
            for s in range(n):
                if not active[s]:
                    continue
                kL = keep_of(seq, sL, (fm[0][s], margin) if fm is not None else None)
                kR = keep_of(seq, sR, (fm[1][s], margin) if fm is not None else None)
                exp, counts, thr, _ = checkers[s].step((L[s], R[s]), (kL, kR))
                mc.check_detection(g, s, exp, counts, thr, "frame %d stream %d" % (k, s))
                np.testing.assert_array_equal(g.detection_mask(s, 0), mask.pack_bool(kL))
                np.testing.assert_array_equal(g.detection_mask(s, 1), mask.pack_bool(kR))
            if fm is not None and device:
                g.synchronize()
                assert torch.equal(tl, before[0]) and torch.equal(tr, before[1])
    finally:
        g.destroy()


@pytest.mark.parametrize("use_static,use_frame", [(True, False), (False, True), (True, True)], ids=["static", "frame", "both"])
@pytest.mark.parametrize("margin", [0, 5])
def test_detection_one_stream(seq, use_static, use_frame, margin):
    run_detection(seq, 1, use_static, use_frame, margin)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_detection_three_streams_one_switched_off(seq, device):
    run_detection(seq, 3, True, True, 5, device=device, off=(3, 4))
    if not device:
        run_detection(seq, 3, True, False, 0, off=(3, 4))


def test_detection_stage_path(seq):
    run_detection(seq, 1, True, True, 5, stage=True)
    run_detection(seq, 3, True, True, 0, stage=True)


@pytest.mark.parametrize("split", [0, 4])
def test_detection_launch_sequences(seq, split):
    run_detection(seq, 1, True, True, 5, split=split)


# ---- 7. what lies under the mask cannot matter ------------------------------------------------------------------------------
def brief_reach():
    """The BRIEF extractor's reach: the pattern's patch half-width plus the 9 x 9 box sum's 4 (it covers the FAST circle's 3 and the
    3 x 3 suppression's 1 as well)."""
    txt = open(os.path.join(ROOT, "include", "vslam_brief_pattern.h")).read()
    half = int(re.search(r"#define\s+VSLAM_BRIEF_PATCH_HALF\s+(\d+)", txt).group(1))
    fp = open(os.path.join(ROOT, "vslam_pose_estimation_framework_amd", "csrc", "brief_footprint.h")).read()
    assert "VS_FP_ROWS (2 * VSLAM_BRIEF_PATCH_HALF + 1)" in fp
    return half + 4


def orb_reach():
    """The ORB extractor's reach: the steered pattern's radius (the largest tap of the table, one more for the rounding of the rotated
    coordinates) plus the 7 x 7 blur's 3."""
    txt = open(os.path.join(ROOT, "include", "vslam_orb_pattern.h")).read()
    taps = np.array([int(v) for v in re.findall(r"-?\d+", txt.split("VSLAM_ORB_PATTERN_INIT {", 1)[1].split("}\n", 1)[0])]).reshape(-1, 2)
    assert len(taps) == 512
    kernel = open(os.path.join(ROOT, "vslam_pose_estimation_framework_amd", "csrc", "kernels_image.h")).read()
    assert "k_gauss7" in kernel
    return int(np.ceil(np.hypot(taps[:, 0], taps[:, 1]).max())) + 1 + 3


def euroc_grid(cfg, o):
    """The 2 x 2 detector grid of test_pipeline_parity_euroc_grid."""
    d = o.default_config("euroc")
    for name in ("det_rows", "det_cols", "detector_threshold_minimum", "detector_threshold_maximum", "detector_threshold_maximum_change",
                 "bin_size_pixels", "minimum_descriptor_distance_tracking", "maximum_descriptor_distance_tracking",
                 "maximum_reliable_depth_meters", "maximum_depth_meters", "maximum_matching_distance_triangulation",
                 "minimum_track_length_for_landmark_creation", "good_tracking_ratio", "aligner_damping"):
        setattr(cfg, name, getattr(d, name))


@pytest.fixture(scope="module")
def seq_grid():
    s = Seq((7,), scale=0.5, speed=0.3)
    yield s
    s.o.destroy()


@pytest.mark.parametrize("variant,n,use_frame", [("brief", 1, False), ("brief", 1, True), ("brief", 3, True), ("orb", 1, True), ("orb", 3, False), ("grid", 1, True)],
                         ids=["static", "static+frame", "three-streams", "orb", "orb-three-streams", "euroc_grid"])
def test_pixels_under_the_mask_do_not_matter(seq, seq_grid, variant, n, use_frame):
    margin = 28
    assert margin >= (orb_reach() if variant == "orb" else brief_reach())
    if variant == "grid":
        seq = seq_grid
    cfg = seq.cfg.copy()
    cfg.enable_landmark_recovery = 0
    # TRACKING from frame 1 on; the euroc values create landmarks from tracks of length 2, so that configuration cannot be TRACKING before
    # frame 2 with or without a mask (CPU oracle, removed pixels painted grey: seed 7 at scale 0.5, speed 0.3 is TRACKING from frame 2 on)
    first_tracking = 1
    if variant == "orb":
        cfg.descriptor_type = 1         # VSLAM_DESCRIPTOR_ORB
    if variant == "grid":
        euroc_grid(cfg, seq.o)
        first_tracking = 2
    a, b = create_hip(cfg, n), create_hip(cfg, n)
    rng = np.random.default_rng(77)

    def narrow_rect(k, s):
        # 12 x 12 in the upper part of the image: the margin of 28 widens it to 68 x 68
        m = np.ones((seq.rows, seq.cols), np.uint8)
        x0 = (37 * k + 101 * s + seq.cols // 2) % (seq.cols - 12)
        y0 = (11 * k + 29 * s) % (seq.rows // 4)
        m[y0:y0 + 12, x0:x0 + 12] = 0
        return m
    # a much smaller blob than the detection cases': the scenes give ~100 points per frame at this size, and the keep-mask eroded by 28
    # must leave enough of them to track on (on the CPU oracle, with the removed pixels painted grey, the three scenes are TRACKING from
    # frame 1 on with 62 .. 106 points when the masks take 11 % of the image, and lose track at frame 3 when they take 40 %)
    y, x = np.mgrid[0:seq.rows, 0:seq.cols]
    blob = np.where(((x - 0.15 * seq.cols) / (0.04 * seq.cols)) ** 2 + ((y - 0.2 * seq.rows) / (0.12 * seq.rows)) ** 2 <= 1.0, 0, 255).astype(np.uint8)
    try:
        for h in (a, b):
            h.set_detection_mask(blob, blob, margin)
        for k in range(FRAMES):
            L, R = np.ascontiguousarray(seq.L[k][:n]), np.ascontiguousarray(seq.R[k][:n])
            Ln, Rn = L.copy(), R.copy()
            zero = [np.broadcast_to(blob == 0, L.shape).copy(), np.broadcast_to(blob == 0, R.shape).copy()]
            fm = None
            if use_frame:
                fm = [np.stack([narrow_rect(k, s + d) for s in range(n)]) for d in (0, 5)]
                for d in (0, 1):
                    zero[d] |= fm[d] == 0
                for h in (a, b):
                    h.set_frame_masks(fm[0], fm[1], margin)
            Ln[zero[0]] = rng.integers(0, 256, int(zero[0].sum()), dtype=np.uint8)
            Rn[zero[1]] = rng.integers(0, 256, int(zero[1].sum()), dtype=np.uint8)
            assert (Ln != L).any()
            a.process_host(L, R)
            b.process_host(Ln, Rn)
            for s in range(n):
                compare_frame(a, b, s, k, "under the mask", identical=True)
                fi = a.frame_info(s)
                if k >= first_tracking:
                    assert fi.status == 1, (k, s, fi.status)          # VSLAM_TRACKING
                for d in (0, 1):
                    keep = mask.unpack(a.detection_mask(s, d), seq.cols)
                    want = mask.erode(blob != 0, margin) & (mask.erode(fm[d][s] != 0, margin) if fm is not None else True)
                    np.testing.assert_array_equal(keep, want)
                    # no point, and so no landmark (a landmark is created from and carried by a point of the frame), lies on a removed
                    # pixel: with recovery off every point sits on a keypoint of this frame
                    pts = a.points(s)
                    xy = pts["kp"][:, 2 * d:2 * d + 2]
                    assert len(xy) and mask.filter_keypoints(xy, keep).all()
                    with_landmark = pts["meta"][:, 4] > 0             # lm_updates: the point carries a landmark
                    if k >= first_tracking + 1:
                        assert with_landmark.any()
                    assert mask.filter_keypoints(xy[with_landmark], keep).all()
    finally:
        a.destroy()
        b.destroy()


# ---- 8. identity and lifetime ---------------------------------------------------------------------------------------------
def run_plain(seq, n, frames, prepare=None, per_frame=None):
    g = create_hip(seq.cfg, n)
    if prepare:
        prepare(g)
    for k in frames:
        if per_frame:
            per_frame(g, k)
        g.process_host(np.ascontiguousarray(seq.L[k][:n]), np.ascontiguousarray(seq.R[k][:n]))
    return g


def assert_same_run(seq, n, make_a, make_b, frames=range(5)):
    """Two contexts driven frame by frame stay identical bit for bit."""
    a, b = create_hip(seq.cfg, n), create_hip(seq.cfg, n)
    try:
        for k in frames:
            L, R = np.ascontiguousarray(seq.L[k][:n]), np.ascontiguousarray(seq.R[k][:n])
            make_a(a, k)
            make_b(b, k)
            a.process_host(L, R)
            b.process_host(L, R)
            for s in range(n):
                compare_frame(a, b, s, k, identical=True)
    finally:
        a.destroy()
        b.destroy()


def test_all_keep_masks_equal_no_mask(seq):
    keep = np.full((seq.rows, seq.cols), 255, np.uint8)
    keeps = np.stack([keep, keep])

    def with_masks(g, k):
        if k == 0:
            g.set_detection_mask(keep, keep, 7)
        g.set_frame_masks(keeps, keeps, 64)
    assert_same_run(seq, 2, with_masks, lambda g, k: None)


def test_on_then_off_equals_never_on_and_cancel(seq):
    def on_off(g, k):
        if k == 0:
            g.set_detection_mask(seq.blob, None, 3)
            g.set_detection_mask(None, None)
        g.set_frame_masks(frame_masks(seq, k, 1)[0], None, 2)
        g.set_frame_masks(None, None)                       # cancelled before the frame
    assert_same_run(seq, 1, on_off, lambda g, k: None)
    g = run_plain(seq, 1, [0])
    try:
        with pytest.raises(VslamError) as ei:
            g.detection_mask(0, 0)
        assert ei.value.code == ERR_STATE
    finally:
        g.destroy()


def test_static_mask_survives_resets_and_frame_mask_lasts_one_frame(seq):
    fm = frame_masks(seq, 2, 2)

    def a_side(g, k):
        if k == 0:
            g.set_detection_mask(seq.blob, seq.blob, 5)
        if k == 2:
            g.reset()
        if k == 3:
            g.reset_stream(1)
        if k == 4:
            g.set_frame_masks(fm[0], fm[1], 1)

    def b_side(g, k):
        if k in (0, 2):
            if k == 2:
                g.reset()
            g.set_detection_mask(seq.blob, seq.blob, 5)     # set again behind the reset: the same words
        if k == 3:
            g.reset_stream(1)
        if k == 4:
            g.set_frame_masks(fm[0].copy(), fm[1].copy(), 1)
    assert_same_run(seq, 2, a_side, b_side, frames=range(7))
    # the frame after the frame mask equals a static-only checker from the same state
    g = create_hip(seq.cfg, 1)
    chk = mc.Checker(seq.o, seq.cfg)
    try:
        g.set_detection_mask(seq.blob, seq.blob, 0)
        for k in range(4):
            one = frame_masks(seq, k, 1) if k == 1 else None
            if one is not None:
                g.set_frame_masks(one[0], one[1], 0)
            L, R = seq.L[k][:1], seq.R[k][:1]
            g.process_host(np.ascontiguousarray(L), np.ascontiguousarray(R))
            kL = keep_of(seq, (seq.blob, 0), (one[0][0], 0) if one is not None else None)
            kR = keep_of(seq, (seq.blob, 0), (one[1][0], 0) if one is not None else None)
            exp, counts, thr, _ = chk.step((L[0], R[0]), (kL, kR))
            mc.check_detection(g, 0, exp, counts, thr, "frame %d" % k)
            np.testing.assert_array_equal(g.detection_mask(0, 1), mask.pack_bool(kR))
    finally:
        g.destroy()


# ---- 9. behind rectification ----------------------------------------------------------------------------------------------------
def test_masks_behind_rectification():
    """Raw 380 x 500 pairs through a rectifying context with masks in rectified coordinates == the numpy-rectified 360 x 480 pairs through
    a second context with the same masks, bit for bit."""
    import test_rectify_gpu as tr
    from _oracle import Oracle
    o = Oracle()
    scene, cfg = tr._scene_and_config(o)
    maps = [tr._smooth_maps(tr.ROWS, tr.COLS, tr.RAW_ROWS, tr.RAW_COLS, s) for s in (7, 8)]
    rig = tr._Rig(tr.ROWS, tr.COLS, tr.RAW_ROWS, tr.RAW_COLS, maps)
    a, b = create_hip(cfg, 1), create_hip(cfg, 1)
    blob = mc.static_blob(tr.ROWS, tr.COLS)
    try:
        a.set_rectification(rig)
        for h in (a, b):
            h.set_detection_mask(blob, None, 3)
        for k in range(5):
            L, R = o.render(scene, k)
            Lc, Rc = rig.rectify(L, R)
            fm = (mc.frame_rect(tr.ROWS, tr.COLS, k, 0, small=True), mc.frame_rect(tr.ROWS, tr.COLS, k, 5, small=True))
            for h in (a, b):
                h.set_frame_masks(fm[0], fm[1], 2)
            a.process_host(L, R)
            b.process_host(Lc, Rc)
            compare_frame(b, a, 0, k, "behind rectification", identical=True)
            for side in (0, 1):
                want = mask.effective(tr.ROWS, tr.COLS, (blob, 3) if side == 0 else None, (fm[side], 2))
                np.testing.assert_array_equal(a.detection_mask(0, side), want)
                np.testing.assert_array_equal(b.detection_mask(0, side), want)
        assert a.frame_info(0).n_keypoints_left > 50
    finally:
        a.destroy()
        b.destroy()
        o.destroy()


def test_contract_refusals(seq):
    g = create_hip(seq.cfg, 2)
    blob = seq.blob
    p = blob.ctypes.data_as(C.c_void_p)
    i32 = C.c_int32
    try:
        sd, sf, gd = g.fn("set_detection_mask"), g.fn("set_frame_masks"), g.fn("get_detection_mask")
        words = np.full((seq.rows, (seq.cols + 63) // 64), 0x5A, np.uint64)
        pw = words.ctypes.data_as(C.c_void_p)
        assert sd(None, p, p, i32(seq.cols), i32(0)) == ERR_INVALID
        assert sf(None, p, p, i32(seq.cols), C.c_size_t(0), i32(0), C.c_int(0)) == ERR_INVALID
        for stride, margin in ((seq.cols - 1, 0), (seq.cols, -1), (seq.cols, 65)):
            assert sd(g.ctx, p, p, i32(stride), i32(margin)) == ERR_INVALID and g.last_error(g.ctx)
            assert sf(g.ctx, p, p, i32(stride), C.c_size_t(0), i32(margin), C.c_int(0)) == ERR_INVALID and g.last_error(g.ctx)
        g.process_host(np.ascontiguousarray(seq.L[0][:2]), np.ascontiguousarray(seq.R[0][:2]))       # still usable, and nothing was set
        assert gd(g.ctx, C.c_int(0), C.c_int(0), pw) == ERR_STATE
        g.set_detection_mask(blob, None, 0)
        g.process_host(np.ascontiguousarray(seq.L[1][:2]), np.ascontiguousarray(seq.R[1][:2]))
        for stream, side, out in ((2, 0, pw), (-1, 0, pw), (0, 2, pw), (0, 0, None)):
            assert gd(g.ctx, C.c_int(stream), C.c_int(side), out) == ERR_INVALID
        assert (words == 0x5A).all()
        np.testing.assert_array_equal(g.detection_mask(1, 0), mask.pack(blob, 0))
        np.testing.assert_array_equal(g.detection_mask(1, 1), mask.all_keep(seq.rows, seq.cols))     # the unmasked side
        # inside a frame on the stage path
        L, R = np.ascontiguousarray(seq.L[2][:2]), np.ascontiguousarray(seq.R[2][:2])
        g.check(g.fn("frame_begin")(g.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]),
                                    C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
        assert sd(g.ctx, p, p, i32(seq.cols), i32(0)) == ERR_STATE
        assert sf(g.ctx, p, p, i32(seq.cols), C.c_size_t(0), i32(0), C.c_int(0)) == ERR_STATE
        g.check(g.fn("frame_finish")(g.ctx))
        g.set_frame_masks(np.stack([blob, blob]), None, 1)      # accepted again, not sticky
        g.process_host(np.ascontiguousarray(seq.L[3][:2]), np.ascontiguousarray(seq.R[3][:2]))
        assert g.frame_info(0).frame_index >= 0
    finally:
        g.destroy()
