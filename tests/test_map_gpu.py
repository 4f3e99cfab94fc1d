"""The device landmark map (vslam_enable_map / k_map_commit): equal bit for bit to a numpy rebuild from the per-frame point read-backs,
the same under every launch sequence and on the stage path, no effect on tracking, per-stream lifetime, capacity overflow, geometry
against the synthetic street canyon, and tools/run_kitti.py --map end to end (exact and chunked)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pipeline_compare import create_hip  # noqa: E402

BIG = 1 << 16
# median distance (m) of the map's reliable landmarks to the nearest surface of the synthetic street canyon (ground y = +1.65 m, walls
# x = +-7 m in the scene frame).  Measured on MI355X: 0.098 m (60 frames), 0.078 m / 0.075 m (30 frames, exact / chunked); DESIGN.md §6b
GEOMETRY_BOUND_M = 0.15


def _frame_points(api, s):
    cap = int(api.cfg.max_points)
    n = C.c_int32()
    meta = np.zeros((cap, 6), np.int32)
    lm = np.zeros((cap, 3), np.float64)
    desc = np.zeros((cap, 64), np.uint8)
    api.check(api.fn("get_frame_points")(api.ctx, C.c_int(s), C.c_int(0), C.c_int32(cap), C.byref(n), None, meta.ctypes.data_as(C.c_void_p),
                                         None, lm.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p)))
    k = n.value
    return meta[:k], lm[:k], desc[:k]


class Rebuild(object):
    """The map of one stream rebuilt from the frame's points (vslam_get_frame_points) with the id rule of kernels_map.h."""

    def __init__(self, cap=BIG):
        self.cap = cap
        self.ids_prev = np.zeros(0, np.int64)
        self.xyz, self.first, self.last, self.upd, self.desc = [], [], [], [], []
        self.refused = False

    def frame(self, api, s):
        f = api.frame_info(s).frame_index - 1
        meta, lm, desc = _frame_points(api, s)
        ids = np.full(len(meta), -1, np.int64)
        self.refused = False
        for i in range(len(meta)):
            ip, lmup = int(meta[i, 2]), int(meta[i, 4])
            id_ = int(self.ids_prev[ip]) if (f > 0 and 0 <= ip < len(self.ids_prev)) else -1
            fresh = False
            if id_ < 0 and lmup > 0:
                if len(self.xyz) < self.cap:
                    id_, fresh = len(self.xyz), True
                    self.xyz.append(None); self.first.append(f); self.last.append(0); self.upd.append(0); self.desc.append(None)
                else:
                    self.refused = True
            ids[i] = id_
            if id_ >= 0:
                self.xyz[id_] = lm[i].copy()
                self.last[id_], self.upd[id_] = f, lmup
                self.desc[id_] = desc[i, :32].copy()
                if fresh:
                    self.first[id_] = f
        self.ids_prev = ids

    def check(self, api, s, tag):
        m = api.map(s)
        n = len(self.xyz)
        assert len(m["id"]) == n, "%s: %d entries, rebuild %d" % (tag, len(m["id"]), n)
        if n == 0:
            return
        np.testing.assert_array_equal(m["xyz"], np.array(self.xyz), err_msg=tag)
        np.testing.assert_array_equal(m["first_frame"], self.first, err_msg=tag)
        np.testing.assert_array_equal(m["last_frame"], self.last, err_msg=tag)
        np.testing.assert_array_equal(m["updates"], self.upd, err_msg=tag)
        np.testing.assert_array_equal(m["desc"], np.array(self.desc), err_msg=tag)
        # a read from an id on returns the tail
        k = n // 2
        t = api.map(s, first=k)
        assert list(t["id"]) == list(range(k, n))
        np.testing.assert_array_equal(t["xyz"], m["xyz"][k:])


def _scenes(o, seeds, scale=0.5):
    return [o.scene_kitti(scale=scale, seed=sd) for sd in seeds]


def _images(o, scenes, k):
    imgs = [o.render(sc, k) for sc in scenes]
    return np.stack([im[0] for im in imgs]), np.stack([im[1] for im in imgs])


def _maps_equal(a, b, s, tag):
    ma, mb = a.map(s), b.map(s)
    assert len(ma["id"]) == len(mb["id"]), tag
    for k in ("xyz", "first_frame", "last_frame", "updates", "desc"):
        np.testing.assert_array_equal(ma[k], mb[k], err_msg="%s %s" % (tag, k))


@pytest.mark.gpu
@pytest.mark.parametrize("seeds", [[21], [31, 32, 33]])
def test_map_equals_rebuild(seeds):
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, seeds)
    B = len(seeds)
    g = create_hip(o.config_for_scene(scenes[0]), B)
    try:
        g.enable_map(BIG)
        rb = [Rebuild() for _ in range(B)]
        for k in range(60):
            g.process_host(*_images(o, scenes, k))
            for s in range(B):
                rb[s].frame(g, s)
                if k in (19, 39, 59):
                    rb[s].check(g, s, "B=%d frame %d stream %d" % (B, k, s))
        for s in range(B):
            assert g.map_size(s) > 100
            assert g.frame_info(s).error_flags & 8 == 0
    finally:
        g.destroy()


@pytest.mark.gpu
def test_map_same_under_every_launch_sequence_and_does_not_perturb_tracking():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [41, 42, 43])
    cfg = o.config_for_scene(scenes[0])
    ref = create_hip(cfg, 3)                                   # the library's own launch sequence, map on
    plain = create_hip(cfg, 3)                                 # never enables the map
    splits = (0, 4)
    forced = [create_hip(cfg, 3, split=sp) for sp in splits]
    ctxs = [ref] + forced
    try:
        for h in ctxs:
            h.enable_map(BIG)
        for k in range(40):
            L, R = _images(o, scenes, k)
            for h in ctxs + [plain]:
                h.process_host(L, R)
            for s in range(3):
                fa, fb = ref.frame_info(s), plain.frame_info(s)
                assert bytes(fa) == bytes(fb), "frame %d stream %d: frame_info differs with the map on" % (k, s)
                pa, pb = ref.points(s), plain.points(s)
                for key in pa:
                    np.testing.assert_array_equal(pa[key], pb[key])
        for s in range(3):
            np.testing.assert_array_equal(ref.poses(s, 0, 40), plain.poses(s, 0, 40))
            assert ref.map_size(s) > 50
            for sp, h in zip(splits, forced):
                _maps_equal(ref, h, s, "VSLAM_SPLIT=%d stream %d" % (sp, s))
        with pytest.raises(Exception):
            plain.map_size(0)                                  # no map: VSLAM_ERR_STATE
    finally:
        for h in ctxs + [plain]:
            h.destroy()


@pytest.mark.gpu
def test_map_stage_path_equals_process_host():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [51])
    cfg = o.config_for_scene(scenes[0])
    a, b = create_hip(cfg, 1), create_hip(cfg, 1)
    try:
        a.enable_map(BIG)
        b.enable_map(BIG)
        for k in range(30):
            L, R = _images(o, scenes, k)
            L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
            a.process_host(L, R)
            b.check(b.fn("frame_begin")(b.ctx, L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.c_int32(L.shape[2]),
                                        C.c_size_t(L.shape[1] * L.shape[2]), C.c_int(0)))
            b.check(b.fn("frame_finish")(b.ctx))
        assert a.map_size(0) > 50
        _maps_equal(a, b, 0, "stage path")
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.gpu
def test_map_reset_and_inactive_streams():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [61, 62, 63])
    g = create_hip(o.config_for_scene(scenes[0]), 3)
    try:
        g.enable_map(BIG)
        for k in range(15):
            g.process_host(*_images(o, scenes, k))
        frozen = g.map(1)
        assert len(frozen["id"]) > 0
        g.set_stream_active(1, False)
        sizes = [g.map_size(s) for s in range(3)]
        for k in range(15, 25):
            g.process_host(*_images(o, scenes, k))
        m1 = g.map(1)
        for key in frozen:
            np.testing.assert_array_equal(m1[key], frozen[key])      # a switched-off stream's map does not change
        assert g.map_size(0) > sizes[0] and g.map_size(2) > sizes[2]
        keep0, keep1 = g.map(0), g.map(1)
        g.reset_stream(2)
        assert g.map_size(2) == 0
        for s, kept in ((0, keep0), (1, keep1)):                      # only that stream's map is emptied
            m = g.map(s)
            for key in kept:
                np.testing.assert_array_equal(m[key], kept[key])
        rb = Rebuild()
        for k in range(25, 45):                                       # stream 2 starts a fresh sequence: ids from 0, frames from 0
            L, R = _images(o, scenes, k)
            L[2], R[2] = o.render(scenes[2], k - 25)
            g.process_host(L, R)
            rb.frame(g, 2)
        rb.check(g, 2, "after vslam_reset_stream")
        assert g.map(2)["last_frame"].max() == 19                     # frame indices restart with the stream
        g.reset()
        assert [g.map_size(s) for s in range(3)] == [0, 0, 0]
    finally:
        g.destroy()


@pytest.mark.gpu
def test_map_capacity_overflow():
    from _oracle import Oracle
    o = Oracle()
    scenes = _scenes(o, [71])
    cfg = o.config_for_scene(scenes[0])
    full, small = create_hip(cfg, 1), create_hip(cfg, 1)
    cap = 40
    try:
        full.enable_map(BIG)
        small.enable_map(cap)
        rb = Rebuild(cap)
        overflow_frame = None
        for k in range(30):
            L, R = _images(o, scenes, k)
            full.process_host(L, R)
            small.process_host(L, R)
            rb.frame(small, 0)
            flag = small.frame_info(0).error_flags & 8
            if overflow_frame is None and full.map_size(0) > cap:
                overflow_frame = k
                assert flag, "frame %d: bit 8 missing in the overflow frame" % k
            elif overflow_frame is None:
                assert not flag, "frame %d: bit 8 before the overflow" % k
            assert flag or not rb.refused, "frame %d refused an entry without bit 8" % k
        assert overflow_frame is not None
        assert small.map_size(0) == cap
        rb.check(small, 0, "capacity %d" % cap)
        mf, ms = full.map(0), small.map(0)
        for key in ("xyz", "first_frame", "last_frame", "updates", "desc"):
            np.testing.assert_array_equal(ms[key], mf[key][:cap], err_msg=key)
        assert full.frame_info(0).error_flags & 8 == 0
    finally:
        full.destroy()
        small.destroy()


def surface_distance(xyz_scene, scene):
    """Distance of scene-frame points to the nearest surface of the street canyon (tools/synth/synth_scene.h)."""
    d_ground = np.abs(xyz_scene[:, 1] - scene.cam_height_m)
    d_wall = np.minimum(np.abs(xyz_scene[:, 0] - scene.wall_half_m), np.abs(xyz_scene[:, 0] + scene.wall_half_m))
    return np.minimum(d_ground, d_wall)


def map_geometry(m, poses, gt0, scene, max_depth):
    """Median surface distance of the landmarks within max_depth of the camera of their last update, in the scene frame (gt0:
    camera-to-scene pose of frame 0, where the tracker's world starts)."""
    X = np.asarray(m["xyz"])
    P = np.asarray(poses).reshape(-1, 3, 4)[np.asarray(m["last_frame"])]
    d = X - P[:, :, 3]
    z = np.einsum("nij,ni->nj", P[:, :, :3], d)[:, 2]
    keep = (z > 0) & (z < max_depth)
    Xs = X[keep] @ gt0[:, :3].T + gt0[:, 3]
    return float(np.median(surface_distance(Xs, scene))), int(keep.sum())


@pytest.mark.gpu
def test_map_geometry_street_canyon():
    from _oracle import Oracle
    o = Oracle()
    scene = o.scene_kitti(scale=0.5, seed=81)
    cfg = o.config_for_scene(scene)
    g = create_hip(cfg, 1)
    n = 60
    try:
        g.enable_map(BIG)
        for k in range(n):
            g.process_host(*o.render(scene, k))
        med, cnt = map_geometry(g.map(0), g.poses(0, 0, n), np.array(o.gt_pose(scene, 0)), scene, cfg.maximum_reliable_depth_meters)
        print("street canyon: median surface distance %.4f m over %d reliable landmarks" % (med, cnt))
        assert cnt > 100
        assert med < GEOMETRY_BOUND_M
    finally:
        g.destroy()


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
def test_run_kitti_map_end_to_end(tmp_path):
    import run_kitti
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import io_formats as io
    o = Oracle()
    scene = o.scene_kitti(scale=0.5, seed=9)
    n = 30
    seq = tmp_path / "seq"
    _kitti_folder(o, scene, seq, n)
    gt0 = np.array(o.gt_pose(scene, 0))
    out = str(tmp_path / "map.ply")
    res = run_kitti.run(str(seq), None, "kitti", log=lambda *_: None, map_path=out)
    assert res["error_flags"] == 0
    ply = io.read_ply(out)
    # the same images through the API: the PLY holds the context's map
    ks = io.KittiSequence(str(seq))
    cfg = run_kitti.hip.load().default_config("kitti")
    io.apply_calib(cfg, ks.K, ks.baseline, int(scene.rows), int(scene.cols))
    cfg.max_history_frames = 512
    g = create_hip(cfg, 1)
    try:
        g.enable_map(BIG)
        for k in range(n):
            g.process_host(*o.render(scene, k))
        m = g.map(0)
        poses = g.poses(0, 0, n)
    finally:
        g.destroy()
    np.testing.assert_array_equal(ply["xyz"], m["xyz"])
    for key in ("id", "first_frame", "last_frame", "updates"):
        np.testing.assert_array_equal(ply[key], m[key])
    med, cnt = map_geometry(m, poses, gt0, scene, cfg.maximum_reliable_depth_meters)
    assert cnt > 50 and med < GEOMETRY_BOUND_M
    # frame-sharded: 3 chunks, warm-up duplicates dropped, global frame numbers, the same geometry bound in the first chunk's world
    out_ch = str(tmp_path / "map_chunks.ply")
    rc = run_kitti.run(str(seq), None, "kitti", log=lambda *_: None, chunks=3, overlap=3, map_path=out_ch)
    assert rc["error_flags"] == 0
    pc = io.read_ply(out_ch)
    np.testing.assert_array_equal(pc["xyz"], rc["map"]["xyz"])
    assert list(pc["id"]) == list(range(len(pc["id"])))
    assert pc["first_frame"].min() >= 0 and pc["last_frame"].max() < n
    assert np.all(pc["first_frame"] <= pc["last_frame"])
    assert (pc["first_frame"] >= 10).any() and (pc["first_frame"] >= 20).any()      # every chunk contributes
    med_c, cnt_c = map_geometry(pc, rc["poses"], gt0, scene, cfg.maximum_reliable_depth_meters)
    print("run_kitti --map: exact %.4f m (%d), chunked %.4f m (%d)" % (med, cnt, med_c, cnt_c))
    assert cnt_c > 50 and med_c < GEOMETRY_BOUND_M
