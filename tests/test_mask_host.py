"""Detection masks on the host: mask.py against a scalar restatement, hand-worked cases, and the premises of the GPU cases from the
oracle alone (no GPU)."""
import numpy as np
import pytest

import mask_cases as mc
from vslam_pose_estimation_framework_amd import mask


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "%dx%d" % s)
def test_pack_equals_scalar_restatement(shape):
    rows, cols = shape
    for name in mc.CONTENTS:
        img = mc.content(name, rows, cols)
        for m in mc.MARGINS:
            want = mc.scalar_pack(img, m)
            got = mask.pack(img, m)
            assert got.dtype == np.uint64 and got.shape == (rows, (cols + 63) // 64)
            np.testing.assert_array_equal(got, want, err_msg="%s m=%d" % (name, m))
            keep = mask.unpack(got, cols)
            np.testing.assert_array_equal(keep, mask.erode(img != 0, m))
            np.testing.assert_array_equal(mask.pack_bool(keep), got)


def test_word_seam_and_hand_worked_cases():
    # one zero pixel at column 63 / 64 with m = 1: three columns go, on both sides of the word seam
    for c0 in (63, 64):
        img = np.full((1, 129), 255, np.uint8)
        img[0, c0] = 0
        keep = mask.unpack(mask.pack(img, 1), 129)[0]
        assert sorted(np.flatnonzero(~keep)) == [c0 - 1, c0, c0 + 1]
    w = mask.pack(np.where(np.arange(129) == 63, 0, 255).astype(np.uint8)[None], 1)[0]
    assert int(w[0]) == (1 << 64) - 1 - (1 << 63) - (1 << 62) and int(w[1]) == (1 << 64) - 2 and int(w[2]) == 1
    # m = 64 on a 1 x 129 row with a zero at column 64 clears the whole row
    img = np.full((1, 129), 255, np.uint8)
    img[0, 64] = 0
    assert not mask.pack(img, 64).any()
    assert mask.pack(img, 63)[0].tolist() == [1, 0, 1]
    # all-keep stays all-keep for every margin, and bits beyond cols are 0
    for rows, cols in mc.SHAPES:
        for m in range(0, 65, 9):
            w = mask.pack(np.full((rows, cols), 7, np.uint8), m)
            assert mask.unpack(w, cols).all()
            np.testing.assert_array_equal(w, mask.all_keep(rows, cols))
        tail = cols - 64 * ((cols - 1) // 64)
        assert all(int(x) >> tail == 0 for x in mask.all_keep(rows, cols)[:, -1])


def test_filter_effective_and_refusals():
    keep = np.ones((4, 6), bool)
    keep[2, 5] = False
    xy = np.array([[5, 2], [2, 5 - 2], [0, 0]], np.int16)
    assert mask.filter_keypoints(xy, keep).tolist() == [False, True, True]
    a = mc.content("holes", 9, 70, 1)
    b = mc.content("rect", 9, 70, 2)
    e = mask.effective(9, 70, (a, 2), (b, 0))
    np.testing.assert_array_equal(mask.unpack(e, 70), mask.erode(a != 0, 2) & (b != 0))
    np.testing.assert_array_equal(mask.effective(9, 70), mask.all_keep(9, 70))
    for bad in (-1, 65, 1.5):
        with pytest.raises(ValueError):
            mask.pack(a, bad)
    with pytest.raises(ValueError):
        mask.pack(a.astype(np.int32), 0)
    with pytest.raises(ValueError):
        mask.unpack(e, 200)
    with pytest.raises(ValueError):
        mask.effective(9, 71, (a, 0))


def test_kernel_bit_helpers_against_scalar_loops(tmp_path):
    """tests/cpp/mask_erode_walk.cpp: the host-and-device helpers of csrc/kernels_mask.h (the word erosion by window doubling, the column
    mask, the ballots' bit order) against scalar loops, built and run on the host."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "mask_erode_walk")
    subprocess.check_call([hipcc, "-x", "hip", "-O1", "-std=c++17", "--offload-arch=gfx950", "-o", exe, os.path.join(root, "tests", "cpp", "mask_erode_walk.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and " 0 bad" in out.stdout, out.stdout + out.stderr


def test_tool_flags_and_refusals(tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import run_kitti
    from vslam_pose_estimation_framework_amd import io_formats
    left, right = str(tmp_path / "l.png"), str(tmp_path / "r.png")
    for p in (left, right):
        io_formats.write_png_gray8(p, mc.content("rect", 20, 30))
    a = run_kitti.parse_args(["seq", "--mask", left + "," + right, "--mask-margin", "7", "--frame-masks", str(tmp_path), "--chunks", "3"])
    assert (a.mask, a.mask_margin, a.frame_masks, a.chunks) == (left + "," + right, 7, str(tmp_path), 3)
    a = run_kitti.parse_args(["seq", "--mask", left])
    assert a.mask == left and a.mask_margin == 0 and a.frame_masks is None
    a = run_kitti.parse_args(["seq"])
    assert a.mask is None and a.frame_masks is None
    for argv in (["seq", "--mask-margin", "3"], ["seq", "--mask", left, "--mask-margin", "65"], ["seq", "--mask", left, "--mask-margin", "-1"],
                 ["seq", "--mask", str(tmp_path / "none.png")], ["seq", "--mask", left + "," + right + "," + left], ["seq", "--mask", left + ","],
                 ["seq", "--frame-masks", str(tmp_path / "none")], ["seq", "--mask", left, "--mask-margin", "x"]):
        with pytest.raises(SystemExit):
            run_kitti.parse_args(argv)
    import run_rgbd
    b = run_rgbd.parse_args(["folder", "--mask", left, "--mask-margin", "28", "--undistort", "--clahe"])
    assert (b.mask, b.mask_margin) == (left, 28)
    assert run_rgbd.parse_args(["folder"]).mask is None
    for argv in (["folder", "--mask-margin", "3"], ["folder", "--mask", left, "--mask-margin", "65"], ["folder", "--mask", str(tmp_path / "none.png")]):
        with pytest.raises(SystemExit):
            run_rgbd.parse_args(argv)
    # a mask of another size than the detector's images is refused when it is read
    with pytest.raises(SystemExit):
        run_kitti.DetectionMasks(None, 21, 30, left, 0, None, log=lambda *_: None)
    m = run_kitti.DetectionMasks(None, 20, 30, left, 2, None, log=lambda *_: None)
    assert m.static[1] is None and (m.static[0] == mc.content("rect", 20, 30)).all()


# ---- premises of the GPU cases (test_mask_gpu.py), from the oracle alone ----------------------------------------------------
SEEDS = (7, 9, 11)       # tried: 7, 9, 11 — all three hold every premise
FRAMES = 8


@pytest.mark.parametrize("seed", SEEDS)
def test_checker_loop_and_mask_premises(seed):
    from _oracle import Oracle
    o = Oracle()
    sc = o.scene_kitti(scale=0.4, seed=seed)
    cfg = o.config_for_scene(sc)
    o.create(cfg, 0, 1)
    try:
        rows, cols = sc.rows, sc.cols
        plain, masked = mc.Checker(o, cfg), mc.Checker(o, cfg)
        blob = mc.static_blob(rows, cols)
        assert 0.25 <= np.mean(blob == 0) <= 0.45
        thr_plain, thr_masked, shared_word = [], [], False
        all_keep = np.ones((rows, cols), bool)
        for k in range(FRAMES):
            L, R = o.render(sc, k)
            o.process_host(L, R)
            # the checker with an all-keep mask reproduces the unmasked oracle pipeline
            exp, counts, thr, _ = plain.step((L, R), (all_keep, all_keep))
            mc.check_detection(o, 0, exp, counts, thr, "seed %d frame %d" % (seed, k))
            thr_plain.append(thr)
            keep = (blob != 0) & (mc.frame_rect(rows, cols, k) != 0)
            expm, _, thrm, removed = masked.step((L, R), (keep, keep))
            thr_masked.append(thrm)
            if k == 0:
                on_removed = sum(len(r) for r in removed) / float(sum(counts))
                assert on_removed >= 0.20, on_removed
            for side in (0, 1):     # a removed keypoint in a word that also holds a kept one
                kept_words = set((int(y), int(x) // 64) for x, y in expm[side][0])
                shared_word = shared_word or any((int(y), int(x) // 64) in kept_words for x, y in removed[side])
        assert thr_plain[:4] != thr_masked[:4], (thr_plain, thr_masked)
        assert shared_word
    finally:
        o.destroy()
