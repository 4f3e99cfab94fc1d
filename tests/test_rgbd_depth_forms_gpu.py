"""The launch forms of the space map that only the device-resident RGB-D loop issues (csrc/rgbd_device.h enqueue_first_attempt), each with
inputs on which a wrong form gives a wrong map — premises in tests/test_rgbd_depth_forms_host.py and asserted here from the same runs:

  offset camera     not plain: k_depth_min / _pick / _write ungated, rearm = 1, batched through blockIdx.z; 96 k of 99 k destinations filled
                    from another pixel, 26 k .. 59 k destinations whose winning depth GROWS from one frame to the next
  crossing camera   plain: k_depth_direct runs, finds its sources on other pixels and raises `cross`; the gated passes recompute the image on
                    their token grid of min(rows, 4) row blocks; one stream of the batch has no depth on frame 0 — its gate stays shut while
                    its neighbours' open —; reset() clears `cross` and must find the z-buffer armed
  strip walk        the registered camera on 24 and on 48 streams: rows = 188 > max(8, 4096 / B) = 170 / 85, k_depth_direct's workgroups take
                    a second (and third) row of their strip (the __syncthreads pair inside its row loop); the same with the gates forced open

The product is compared with the checker loop (tests/rgbd_loop.py over the oracle) as test_rgbd_tracker_matches_the_checker_loop does —
counters and point lists exact, camera coordinates bit for bit, pose to 1e-4 — and product with product bit for bit."""
import numpy as np
import pytest

import depth_cases as dc
import undistort_cases as uc
from vslam_pose_estimation_framework_amd import hip, rectify
from vslam_pose_estimation_framework_amd.capi import RgbdBatch, RgbdTracker

pytestmark = pytest.mark.gpu

_alone = {}


def _record(t, frames):
    out = []
    for L, D in frames:
        fi, nt = t.process(L, D)
        out.append((dc.info_tuple(fi, nt), t.points()))
    return out


def _single(g, kind, seed, zero_first=False):
    """The sequence run alone under the default launch path, once per process (callers set no switch before the first call for a key)."""
    key = (kind, seed, zero_first)
    if key not in _alone:
        run = dc.checker_run(kind, seed, zero_first)
        t = RgbdTracker(g, run["cfg"], run["p"])
        try:
            _alone[key] = _record(t, run["frames"])
        finally:
            t.destroy()
    return _alone[key]


def _against_checker(g, kind, seed, tag):
    """One sequence, frame by frame against the checker loop; returns the product's record."""
    run = dc.checker_run(kind, seed)
    t = RgbdTracker(g, run["cfg"], run["p"])
    rec, from_map = [], 0
    try:
        for k, (L, D) in enumerate(run["frames"]):
            fi, nt = t.process(L, D)
            pts = t.points()
            from_map += dc.assert_frame_equals_checker(run, k, fi, nt, pts, tag)
            rec.append((dc.info_tuple(fi, nt), pts))
        assert fi.status == 1 and fi.n_tracked >= 50 and from_map >= 1000, (tag, fi.status, fi.n_tracked, from_map)
    finally:
        t.destroy()
    return rec


def _batch(g, kind, keys):
    """A batch whose stream i is the sequence keys[i] = (seed, zero_first): every stream == that sequence run alone, bit for bit."""
    runs = [dc.checker_run(kind, seed, zero) for seed, zero in keys]
    want = [_single(g, kind, seed, zero) for seed, zero in keys]
    return runs, want


def _run_batch(g, runs, want, tag):
    B = len(runs)
    b = RgbdBatch(g, runs[0]["cfg"], runs[0]["p"], B)
    try:
        for f in range(dc.LOOP_FRAMES):
            res = b.process(np.stack([r["frames"][f][0] for r in runs]), np.stack([r["frames"][f][1] for r in runs]))
            for s in range(B):
                dc.assert_same_run([(dc.info_tuple(*res[s]), b.points(s))], [want[s][f]], "%s frame %d stream %d" % (tag, f, s))
        assert all(fi.status == 1 and fi.n_tracked >= 50 for fi, _ in res), tag
    finally:
        b.destroy()


@pytest.mark.parametrize("case", ["one", "one-graph", "batch3"])
def test_offset_camera_runs_the_general_passes(case, monkeypatch):
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    assert not dc.is_plain(dc.checker_run("offset", dc.LOOP_SEEDS[0])["p"])
    dc.assert_loop_premises(dc.loop_premises(dc.checker_run("offset", dc.LOOP_SEEDS[0])), "offset")
    if case == "batch3":
        runs, want = _batch(g, "offset", [(s, False) for s in dc.LOOP_SEEDS])
        _run_batch(g, runs, want, "offset batch3")
        return
    alone = _single(g, "offset", dc.LOOP_SEEDS[0])
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if case == "one-graph" else "0")
    rec = _against_checker(g, "offset", dc.LOOP_SEEDS[0], "offset " + case)
    dc.assert_same_run(rec, alone, "offset %s against the direct launches" % case)


@pytest.mark.parametrize("case", ["one", "reset", "batch3-one-gate-shut"])
def test_crossing_camera_opens_the_gate(case, monkeypatch):
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    first = dc.checker_run("crossing", dc.LOOP_SEEDS[0])
    assert dc.is_plain(first["p"])
    dc.assert_loop_premises(dc.loop_premises(first), "crossing")
    if case == "one":
        rec = _against_checker(g, "crossing", dc.LOOP_SEEDS[0], "crossing")
        dc.assert_same_run(rec, _single(g, "crossing", dc.LOOP_SEEDS[0]), "crossing, a second tracker")
    elif case == "reset":
        t = RgbdTracker(g, first["cfg"], first["p"])
        try:
            a = _record(t, first["frames"])
            t.reset()
            b = _record(t, first["frames"])
        finally:
            t.destroy()
        dc.assert_same_run(a, _single(g, "crossing", dc.LOOP_SEEDS[0]), "crossing before reset")
        dc.assert_same_run(b, a, "crossing after reset")
        assert a[-1][1]["xy"].shape[0] >= 100
    else:
        keys = [(dc.LOOP_SEEDS[0], False), (dc.LOOP_SEEDS[1], True), (dc.LOOP_SEEDS[2], False)]
        runs, want = _batch(g, "crossing", keys)
        assert not runs[1]["frames"][0][1].any() and runs[0]["frames"][0][1].any() and runs[2]["frames"][0][1].any()
        _run_batch(g, runs, want, "crossing batch3")


@pytest.mark.parametrize("B", dc.STRIP_BATCHES)
@pytest.mark.parametrize("case", ["direct", "force-cross"])
def test_strip_walk_of_the_direct_pass(case, B, monkeypatch):
    """B = 24: rows 170 .. 187 are written in a workgroup's second step — but no feature lies within 31 px of the border (asserted below: no
    point beyond row 157), so nothing the tracker exports reads them; that batch observes the first step's rows and that the walk does no harm.
    B = 48: 85 row blocks, three steps; every sequence has hundreds of points on rows 85 and up, whose coordinates come from rows of the
    second and third step."""
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    keys = [(dc.LOOP_SEEDS[i % 3], False) for i in range(B)]
    runs, want = _batch(g, "registered", keys)          # the single runs: default path, before the switch below
    row_blocks = max(8, 4096 // B)                      # rgbd_device.h: dgrid.y = min(rows, max(8, 4096 / B))
    assert dc.is_plain(runs[0]["p"]) and runs[0]["p"].rows > row_blocks
    walked = [sum(int((w[1]["xy"][:, 1] >= row_blocks).sum()) for w in want[s]) for s in range(3)]
    assert all(n >= 500 for n in walked) if B == dc.STRIP_BATCHES[1] else all(n == 0 for n in walked), (B, walked)
    if case == "force-cross":
        monkeypatch.setenv("VSLAM_RGBD_DEPTH_FORCE_CROSS", "1")
    _run_batch(g, runs, want, "strip walk %s B=%d" % (case, B))


def test_offset_camera_behind_undistortion(monkeypatch):
    """Raw 200 x 640 frames through vslam_rgbd_set_undistortion, then the offset camera's general passes: == numpy-undistort-then-run."""
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "0")
    g = hip.load()
    run = dc.checker_run("offset", dc.LOOP_SEEDS[0])
    cfg, p = run["cfg"], run["p"]
    K = np.array(list(cfg.K)).reshape(3, 3)
    cam = uc.raw_camera(K, uc.FREIBURG1, 200, 640, (10.0, 6.0))
    und, lens = rectify.undistortion(cam, K, int(cfg.rows), int(cfg.cols)), uc.distorting_maps(cam, K)
    rows, cols = int(cfg.rows), int(cfg.cols)
    u, v = rectify.source_coordinates(und.cam, np.eye(3), np.concatenate([und.K, np.zeros((3, 1))], axis=1), rows, cols)
    vv, uu = np.mgrid[0:rows, 0:cols]
    assert (np.hypot(u - 10.0 - uu, v - 6.0 - vv) > 2.0).mean() > 0.4          # the stage has something to do
    a, b = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        a.set_undistortion(und)
        for f, (L, D) in enumerate(run["frames"]):
            rawL, rawD = uc.distort_frame(lens, L, D)
            uL, uD = und.apply(rawL, rawD)
            ia, ib = a.process(rawL, rawD), b.process(uL, uD)
            dc.assert_same_run([(dc.info_tuple(*ia), a.points())], [(dc.info_tuple(*ib), b.points())], "undistorted frame %d" % f)
            gi, gd = a.undistorted()
            np.testing.assert_array_equal(gi, uL); np.testing.assert_array_equal(gd, uD)
        assert ia[0].status == 1 and ia[0].n_tracked >= 50
    finally:
        a.destroy(); b.destroy()
