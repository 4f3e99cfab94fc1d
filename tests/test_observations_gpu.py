"""The device observation log (vslam_enable_observations / k_obs_append): equal bit for bit to a numpy rebuild from the per-frame point
read-backs, tied to the map's first_frame / last_frame, the same under every launch sequence and on the stage path, no effect on
tracking or on the map, per-stream lifetime, capacity overflow (error bit 16), vslam_get_point_ids, and tools/run_kitti.py
--observations end to end (exact and chunked)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pipeline_compare import create_hip  # noqa: E402

BIG = 1 << 16          # map entries per stream
OBS_BIG = 1 << 18      # log entries per stream: these half-size scenes log well under 200 entries per frame
OBS_FLAG = 16


def _frame_points(api, s):
    """kp and meta of the finished frame through vslam_get_frame_points."""
    cap = int(api.cfg.max_points)
    n = C.c_int32()
    kp = np.zeros((cap, 4), np.int16)
    meta = np.zeros((cap, 6), np.int32)
    api.check(api.fn("get_frame_points")(api.ctx, C.c_int(s), C.c_int(0), C.c_int32(cap), C.byref(n), kp.ctypes.data_as(C.c_void_p),
                                         meta.ctypes.data_as(C.c_void_p), None, None, None))
    k = n.value
    return kp[:k].copy(), meta[:k].copy()


class Rebuild(object):
    """The observation log of one stream rebuilt on the host: the id rule of kernels_map.h on the frame's points
    (vslam_get_frame_points), then one entry (id, frame, kp) per point with an id, in point order."""

    def __init__(self, map_cap=BIG):
        self.map_cap = map_cap
        self.next_id = 0
        self.ids_prev = np.zeros(0, np.int64)
        self.ids = np.zeros(0, np.int64)
        self.id, self.frame, self.kp = [], [], []

    def step(self, api, s):
        f = api.frame_info(s).frame_index - 1
        kp, meta = _frame_points(api, s)
        ids = np.full(len(meta), -1, np.int64)
        for i in range(len(meta)):
            ip, lmup = int(meta[i, 2]), int(meta[i, 4])
            id_ = int(self.ids_prev[ip]) if (f > 0 and 0 <= ip < len(self.ids_prev)) else -1
            if id_ < 0 and lmup > 0 and self.next_id < self.map_cap:
                id_ = self.next_id
                self.next_id += 1
            ids[i] = id_
            if id_ >= 0:
                self.id.append(id_); self.frame.append(f); self.kp.append(kp[i].copy())
        self.ids_prev = self.ids = ids

    def arrays(self):
        return (np.array(self.id, np.int32), np.array(self.frame, np.int32),
                np.array(self.kp, np.int16).reshape(-1, 4))

    def check(self, api, s, tag):
        o = api.observations(s)
        id_, fr, kp = self.arrays()
        n = len(id_)
        assert api.observation_count(s) == n, "%s: %d entries, rebuild %d" % (tag, api.observation_count(s), n)
        assert len(o["id"]) == n, tag
        np.testing.assert_array_equal(o["id"], id_, err_msg=tag)
        np.testing.assert_array_equal(o["frame"], fr, err_msg=tag)
        np.testing.assert_array_equal(o["kp"], kp, err_msg=tag)
        k = n // 2                                    # a read from an entry on returns the tail
        t = api.observations(s, first=k)
        np.testing.assert_array_equal(t["id"], id_[k:], err_msg=tag)
        np.testing.assert_array_equal(t["frame"], fr[k:], err_msg=tag)
        np.testing.assert_array_equal(t["kp"], kp[k:], err_msg=tag)


def _scenes(o, seeds, scale=0.5):
    return [o.scene_kitti(scale=scale, seed=sd) for sd in seeds]


def _images(o, scenes, k):
    imgs = [o.render(sc, k) for sc in scenes]
    return np.stack([im[0] for im in imgs]), np.stack([im[1] for im in imgs])


def _logs_equal(a, b, s, tag):
    oa, ob = a.observations(s), b.observations(s)
    assert len(oa["id"]) == len(ob["id"]), tag
    for k in ("id", "frame", "kp"):
        np.testing.assert_array_equal(oa[k], ob[k], err_msg="%s %s" % (tag, k))


def _maps_equal(a, b, s, tag):
    ma, mb = a.map(s), b.map(s)
    assert len(ma["id"]) == len(mb["id"]), tag
    for k in ("xyz", "first_frame", "last_frame", "updates", "desc"):
        np.testing.assert_array_equal(ma[k], mb[k], err_msg="%s %s" % (tag, k))


def _check_log_against_map(o, m, tag):
    """Every (id, frame) pair at most once; for every id the logged frames are exactly first_frame .. last_frame of map entry id."""
    pairs = o["id"].astype(np.int64) * (1 << 20) + o["frame"]
    assert len(np.unique(pairs)) == len(pairs), "%s: an (id, frame) pair occurs twice" % tag
    assert o["id"].min() >= 0 and o["id"].max() < len(m["id"]), tag
    assert set(o["id"].tolist()) == set(m["id"].tolist()), "%s: ids of the log and of the map differ" % tag
    assert np.all(np.diff(o["frame"]) >= 0), "%s: the log is not sorted by frame" % tag
    order = np.argsort(o["id"], kind="stable")            # the log is sorted by frame, so every id's frames stay ascending
    ids, frames = o["id"][order], o["frame"][order]
    start = np.concatenate([[0], np.flatnonzero(np.diff(ids)) + 1])
    count = np.diff(np.concatenate([start, [len(ids)]]))
    uid = ids[start]
    np.testing.assert_array_equal(frames[start], m["first_frame"][uid], err_msg="%s: first logged frame" % tag)
    np.testing.assert_array_equal(frames[start + count - 1], m["last_frame"][uid], err_msg="%s: last logged frame" % tag)
    np.testing.assert_array_equal(count, m["last_frame"][uid] - m["first_frame"][uid] + 1, err_msg="%s: frames logged per id" % tag)


@pytest.mark.gpu
@pytest.mark.parametrize("seeds", [[21], [31, 32, 33]])
def test_log_equals_rebuild_and_ties_to_the_map(seeds):
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, seeds)
    B = len(seeds)
    g = create_hip(o.config_for_scene(scenes[0]), B)
    try:
        g.enable_map(BIG)
        g.enable_observations(OBS_BIG)
        rb = [Rebuild() for _ in range(B)]
        for k in range(60):
            g.process_host(*_images(o, scenes, k))
            for s in range(B):
                rb[s].step(g, s)
                np.testing.assert_array_equal(g.point_ids(s), rb[s].ids, err_msg="frame %d stream %d: vslam_get_point_ids" % (k, s))
                if k in (19, 39, 59):
                    rb[s].check(g, s, "B=%d frame %d stream %d" % (B, k, s))
        for s in range(B):
            assert g.observation_count(s) > 500
            assert g.frame_info(s).error_flags & (8 | OBS_FLAG) == 0
            _check_log_against_map(g.observations(s), g.map(s), "B=%d stream %d" % (B, s))
    finally:
        g.destroy()


@pytest.mark.gpu
def test_log_same_under_every_launch_sequence_and_does_not_perturb_tracking_or_map():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [41, 42, 43])
    cfg = o.config_for_scene(scenes[0])
    ref = create_hip(cfg, 3)                                   # the library's own launch sequence, map and log on
    plain = create_hip(cfg, 3)                                 # map on, log off
    splits = (0, 4)
    forced = [create_hip(cfg, 3, split=sp) for sp in splits]
    ctxs = [ref] + forced
    try:
        for h in ctxs + [plain]:
            h.enable_map(BIG)
        for h in ctxs:
            h.enable_observations(OBS_BIG)
        for k in range(40):
            L, R = _images(o, scenes, k)
            for h in ctxs + [plain]:
                h.process_host(L, R)
            for s in range(3):
                fa, fb = ref.frame_info(s), plain.frame_info(s)
                assert fa.error_flags & OBS_FLAG == 0
                assert bytes(fa) == bytes(fb), "frame %d stream %d: frame_info differs with the log on" % (k, s)
                pa, pb = ref.points(s), plain.points(s)
                for key in pa:
                    np.testing.assert_array_equal(pa[key], pb[key])
                np.testing.assert_array_equal(ref.point_ids(s), plain.point_ids(s))
        for s in range(3):
            np.testing.assert_array_equal(ref.poses(s, 0, 40), plain.poses(s, 0, 40))
            assert ref.observation_count(s) > 300
            _maps_equal(ref, plain, s, "log on / off, stream %d" % s)
            for sp, h in zip(splits, forced):
                _logs_equal(ref, h, s, "VSLAM_SPLIT=%d stream %d" % (sp, s))
                _maps_equal(ref, h, s, "VSLAM_SPLIT=%d stream %d" % (sp, s))
        with pytest.raises(Exception):
            plain.observation_count(0)                         # no log: VSLAM_ERR_STATE
        with pytest.raises(Exception):
            plain.observations(0)
    finally:
        for h in ctxs + [plain]:
            h.destroy()


@pytest.mark.gpu
def test_log_stage_path_equals_process_host():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [51])
    cfg = o.config_for_scene(scenes[0])
    a, b = create_hip(cfg, 1), create_hip(cfg, 1)
    try:
        for h in (a, b):
            h.enable_map(BIG)
            h.enable_observations(OBS_BIG)
        for k in range(30):
            L, R = _images(o, scenes, k)
            L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
            a.process_host(L, R)
            b.check(b.fn("frame_begin")(b.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]),
                                        C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
            b.check(b.fn("frame_finish")(b.ctx))
            np.testing.assert_array_equal(a.point_ids(0), b.point_ids(0))
        assert a.observation_count(0) > 200
        _logs_equal(a, b, 0, "stage path")
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.gpu
def test_log_lifetime_follows_the_map():
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import capi
    o = Oracle()
    scenes = _scenes(o, [61, 62, 63])
    g = create_hip(o.config_for_scene(scenes[0]), 3)
    try:
        with pytest.raises(capi.VslamError) as ei:             # ids come from the map
            g.enable_observations(OBS_BIG)
        assert ei.value.code == capi.ERR_STATE
        with pytest.raises(capi.VslamError) as ei:             # point ids need the map as well
            g.point_ids(0)
        assert ei.value.code == capi.ERR_STATE
        g.enable_map(BIG)
        with pytest.raises(capi.VslamError) as ei:
            g.enable_observations(-1)
        assert ei.value.code == capi.ERR_INVALID
        # the map runs alone for five frames: a log enabled mid-sequence starts with the next frame
        for k in range(5):
            g.process_host(*_images(o, scenes, k))
        g.enable_observations(OBS_BIG)
        assert [g.observation_count(s) for s in range(3)] == [0, 0, 0]
        for k in range(5, 15):
            g.process_host(*_images(o, scenes, k))
        for s in range(3):
            ob = g.observations(s)
            assert len(ob["id"]) > 0 and ob["frame"].min() == 5 and ob["frame"].max() == 14
        frozen = g.observations(1)
        g.set_stream_active(1, False)
        counts = [g.observation_count(s) for s in range(3)]
        for k in range(15, 25):
            g.process_host(*_images(o, scenes, k))
        o1 = g.observations(1)
        for key in frozen:
            np.testing.assert_array_equal(o1[key], frozen[key])      # a switched-off stream's log does not change
        assert g.observation_count(0) > counts[0] and g.observation_count(2) > counts[2]
        keep0, keep1 = g.observations(0), g.observations(1)
        g.reset_stream(2)
        assert g.observation_count(2) == 0
        for s, kept in ((0, keep0), (1, keep1)):                      # only that stream's log is emptied
            ob = g.observations(s)
            for key in kept:
                np.testing.assert_array_equal(ob[key], kept[key])
        rb = Rebuild()
        for k in range(25, 45):                                       # stream 2 starts a fresh sequence: ids and frames from 0
            L, R = _images(o, scenes, k)
            L[2], R[2] = o.render(scenes[2], k - 25)
            g.process_host(L, R)
            rb.step(g, 2)
        rb.check(g, 2, "after vslam_reset_stream")
        assert g.observations(2)["frame"].max() == 19
        _check_log_against_map(g.observations(2), g.map(2), "after vslam_reset_stream")
        g.reset()
        assert [g.observation_count(s) for s in range(3)] == [0, 0, 0]
        g.enable_observations(0)                                      # capacity 0 turns the log off, the map stays
        with pytest.raises(capi.VslamError) as ei:
            g.observation_count(0)
        assert ei.value.code == capi.ERR_STATE
        assert g.map_size(0) == 0
        g.enable_observations(OBS_BIG)
        g.enable_map(0)                                               # no map, no log
        with pytest.raises(capi.VslamError) as ei:
            g.observation_count(0)
        assert ei.value.code == capi.ERR_STATE
        with pytest.raises(capi.VslamError) as ei:
            g.enable_observations(OBS_BIG)
        assert ei.value.code == capi.ERR_STATE
    finally:
        g.destroy()


@pytest.mark.gpu
def test_log_capacity_overflow():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [71])
    cfg = o.config_for_scene(scenes[0])
    n = 30
    full, small = create_hip(cfg, 1), create_hip(cfg, 1)
    try:
        full.enable_map(BIG)
        full.enable_observations(OBS_BIG)
        images, cum = [], []
        for k in range(n):
            images.append(_images(o, scenes, k))
            full.process_host(*images[k])
            cum.append(full.observation_count(0))      # cumulative unconstrained count after every frame
        of = full.observations(0)
        total = len(of["id"])
        assert total > 500
        cap = int(0.4 * total)
        assert cum[0] <= cap < cum[-1]
        small.enable_map(BIG)
        small.enable_observations(cap)
        for k in range(n):
            small.process_host(*images[k])
            flag = small.frame_info(0).error_flags & OBS_FLAG
            assert bool(flag) == (cum[k] > cap), "frame %d: bit 16 is %d, unconstrained count %d, capacity %d" % (k, flag, cum[k], cap)
            assert small.observation_count(0) == min(cum[k], cap)
        os_ = small.observations(0)
        assert len(os_["id"]) == cap
        for key in ("id", "frame", "kp"):
            np.testing.assert_array_equal(os_[key], of[key][:cap], err_msg=key)
        # the map and the tracking do not see the log's capacity
        _maps_equal(full, small, 0, "capacity %d" % cap)
        np.testing.assert_array_equal(full.poses(0, 0, n), small.poses(0, 0, n))
        np.testing.assert_array_equal(full.point_ids(0), small.point_ids(0))
        pa, pb = full.points(0), small.points(0)
        for key in pa:
            np.testing.assert_array_equal(pa[key], pb[key])
        fa, fs = full.frame_info(0), small.frame_info(0)
        assert fa.error_flags & OBS_FLAG == 0
        assert fs.error_flags == fa.error_flags | OBS_FLAG
    finally:
        full.destroy()
        small.destroy()


def _kitti_folder(o, scene, root, n):
    from vslam_pose_estimation_framework_amd import io_formats as io
    (root / "image_0").mkdir(parents=True)
    (root / "image_1").mkdir(parents=True)
    for k in range(n):
        L, R = o.render(scene, k)
        io.write_png_gray8(str(root / "image_0" / ("%06d.png" % k)), L)
        io.write_png_gray8(str(root / "image_1" / ("%06d.png" % k)), R)
    fx, cx, cy, bx = scene.fx, scene.cx, scene.cy, -scene.fx * scene.baseline_m
    with open(root / "calib.txt", "w") as f:
        f.write("P0: %r 0 %r 0 0 %r %r 0 0 0 1 0\n" % (fx, cx, scene.fy, cy))
        f.write("P1: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (fx, cx, bx, scene.fy, cy))


@pytest.mark.gpu
def test_run_kitti_observations_end_to_end(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import io_formats as io
    from vslam_pose_estimation_framework_amd import sharding
    o = Oracle()
    scene = o.scene_kitti(scale=0.5, seed=9)
    n = 30
    seq = tmp_path / "seq"
    _kitti_folder(o, scene, seq, n)
    out = str(tmp_path / "bundle.npz")
    lines = []
    res = run_kitti.run(str(seq), None, "kitti", log=lambda *a: lines.append(" ".join(str(v) for v in a)), obs_path=out)
    assert res["error_flags"] == 0
    b = io.read_bundle(out)
    # the same images through the API: the bundle holds the context's trajectory, map and log
    ks = io.KittiSequence(str(seq))
    cfg = run_kitti.hip.load().default_config("kitti")
    io.apply_calib(cfg, ks.K, ks.baseline, int(scene.rows), int(scene.cols))
    cfg.max_history_frames = 512
    g = create_hip(cfg, 1)
    try:
        g.enable_map(BIG)
        g.enable_observations(n * int(cfg.max_points))
        for k in range(n):
            g.process_host(*o.render(scene, k))
        m, ob, poses = g.map(0), g.observations(0), g.poses(0, 0, n)
    finally:
        g.destroy()
    assert len(ob["id"]) > 300
    np.testing.assert_array_equal(b["K"], ks.K)
    np.testing.assert_array_equal(b["baseline_h"], ks.baseline)
    np.testing.assert_array_equal(b["poses"], poses.reshape(n, 12))
    for key in ("id", "xyz", "first_frame", "last_frame", "updates", "desc"):
        np.testing.assert_array_equal(b["map"][key], m[key], err_msg=key)
    np.testing.assert_array_equal(b["obs_id"], ob["id"])
    np.testing.assert_array_equal(b["obs_frame"], ob["frame"])
    np.testing.assert_array_equal(b["obs_kp"], ob["kp"])
    rp = res["reprojection"]
    assert rp["observations"] == len(ob["id"]) and rp["landmarks"] == len(m["id"])
    assert np.isfinite(rp["median_px"]) and np.isfinite(rp["p90_px"]) and rp["median_px"] <= rp["p90_px"]
    assert any("reprojection residual norm" in ln for ln in lines) and any("frames without any observation" in ln for ln in lines)
    print("run_kitti --observations exact: %d observations of %d landmarks, residual norm median %.3f px, p90 %.3f px, %d frames without observation"
          % (rp["observations"], rp["landmarks"], rp["median_px"], rp["p90_px"], rp["frames_without_observation"]))
    # frame-sharded: 3 chunks, warm-up duplicates dropped with their observations, global frame numbers
    out_ch = str(tmp_path / "bundle_chunks.npz")
    rc = run_kitti.run(str(seq), None, "kitti", log=lambda *_: None, chunks=3, overlap=3, obs_path=out_ch)
    assert rc["error_flags"] == 0
    bc = io.read_bundle(out_ch)
    mc = bc["map"]
    np.testing.assert_array_equal(mc["xyz"], rc["map"]["xyz"])
    np.testing.assert_array_equal(bc["obs_id"], rc["observations"]["id"])
    np.testing.assert_array_equal(bc["poses"], np.asarray(rc["poses"]).reshape(n, 12))
    assert bc["obs_id"].min() >= 0 and bc["obs_id"].max() < len(mc["id"])             # every observation's landmark is in the map
    assert np.all(bc["obs_frame"] >= mc["first_frame"][bc["obs_id"]]) and np.all(bc["obs_frame"] <= mc["last_frame"][bc["obs_id"]])
    assert bc["obs_frame"].min() >= 0 and bc["obs_frame"].max() < n
    plan, _ = sharding.plan_chunks(n, 3, 3)
    for c, (st, fi, en) in enumerate(plan):                      # every chunk assemble_map keeps landmarks from contributes observations
        if (mc["chunk"] == c).any():
            sel = mc["chunk"][bc["obs_id"]] == c
            assert sel.any(), "chunk %d has landmarks and no observation" % c
            assert bc["obs_frame"][sel].min() >= fi and bc["obs_frame"][sel].max() < en
    assert set(np.unique(mc["chunk"]).tolist()) == {0, 1, 2}
    rq = rc["reprojection"]
    assert np.isfinite(rq["median_px"]) and np.isfinite(rq["p90_px"])
    print("run_kitti --observations --chunks 3 --overlap 3: %d observations of %d landmarks (%d dropped with warm-up duplicates), residual norm "
          "median %.3f px, p90 %.3f px, %d frames without observation"
          % (rq["observations"], rq["landmarks"], rc["observations"]["dropped"], rq["median_px"], rq["p90_px"], rq["frames_without_observation"]))
