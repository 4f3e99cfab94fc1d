"""The landmark map and the observation log of the device-resident RGB-D loop (vslam_rgbd_enable_map / _enable_observations,
csrc/kernels_rgbd_map.h) against the checker loop tests/rgbd_loop.py over the CPU oracle, which keeps every landmark with
its coordinates and measurements (RgbdTracker.landmarks): ids, map entries and log entries of the product must be the checker's, frame
by frame — the first check of k_rgbd_landmarks' coordinates against anything.  Then re-registration, the batch, capacity, lifetime, and
tools/run_rgbd.py --map --observations end to end."""
import os
import sys

import numpy as np
import pytest

from rgbd_loop import RgbdTracker as PyLoop
from test_rgbd_mode import YAML, setup
from vslam_pose_estimation_framework_amd import hip
from vslam_pose_estimation_framework_amd.capi import ERR_INVALID, ERR_STATE, RgbdBatch, RgbdTracker, VslamError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FRAMES = 12
MAP_BIG, OBS_BIG = 4000, 40000
MAP_FLAG, OBS_FLAG = 8, 16
# landmark coordinates, product against checker: both run the same landmark_update arithmetic in fp64 (the product's on the device), the
# figure test_rgbd_mode.py uses for camera coordinates.  Relative to the landmark's norm.
XYZ_RTOL = 1e-12
CASES = [("tum", 1, None, 26), ("tum", 0, 25.0, 31), ("icl", 1, None, 29), ("xtion", 1, None, 37)]


def premises(ref, info, seen):
    """What keeps the equalities below from holding vacuously, counted on the checker loop after one frame (asserted here and, without a
    GPU, in test_rgbd_map_host.py): recovered points on a track with a landmark, points whose predecessor is a temporary point."""
    cur = ref.frames[-1]
    a, r = info["n_after_prune"], info["n_recovered"]
    seen["recovered_with_id"] += sum(1 for q in cur.points[a:a + r] if q.origin.landmark is not None)
    if len(ref.frames) > 1:
        temps = set(id(q) for q in ref.frames[-2].temps)
        seen["temporary_predecessor"] += sum(1 for q in cur.points if q.previous is not None and id(q.previous) in temps)


class Expect(object):
    """The checker's side: what ids, map and log must be after every frame of an unconstrained run that had map and log on from frame 0."""

    def __init__(self):
        self.created, self.desc_last, self.log = [], {}, []
        self.compared = 0

    def step(self, ref):
        cur = ref.frames[-1]
        while len(self.created) < len(ref.landmarks):        # appended by this frame's _updatePoints
            self.created.append(cur.index)
        index = {id(lm): k for k, lm in enumerate(ref.landmarks)}
        ids = []
        for q in cur.points:
            lm = q.origin.landmark
            k = index[id(lm)] if lm is not None else -1
            ids.append(k)
            if k >= 0:
                updated = q.landmark is lm                    # Landmark::Landmark walked over it / Landmark::update consumed it this frame
                if updated:
                    self.desc_last[k] = q.desc
                self.log.append((k, cur.index, q.xy, q.cam, updated))
        return np.array(ids, np.int32).reshape(-1)

    def check(self, prod, stream, ref, ids, tag):
        got = prod.point_ids(stream)
        np.testing.assert_array_equal(got, ids, err_msg="%s: point ids" % (tag,))
        assert prod.map_size(stream) == len(ref.landmarks), (tag, prod.map_size(stream), len(ref.landmarks))
        m = prod.map(stream)
        worst = 0.0
        for k, lm in enumerate(ref.landmarks):
            assert m["updates"][k] == lm.updates, (tag, k, m["updates"][k], lm.updates)
            assert m["last_frame"][k] == max(f for f, _ in lm.meas), (tag, k)
            assert m["first_frame"][k] == self.created[k], (tag, k)
            np.testing.assert_array_equal(m["desc"][k], self.desc_last[k], err_msg="%s: descriptor of landmark %d" % (tag, k))
            worst = max(worst, np.linalg.norm(m["xyz"][k] - lm.world) / np.linalg.norm(lm.world))
            self.compared += 1
        print("%s: %d landmarks, largest |xyz - checker| / |checker| = %.3e" % (tag, len(ref.landmarks), worst))
        assert worst <= XYZ_RTOL, (tag, worst)
        # the log: count, order (frame, then point order), keypoint and camera coordinates bit for bit
        assert prod.observation_count(stream) == len(self.log), (tag, prod.observation_count(stream), len(self.log))
        ob = prod.observations(stream)
        np.testing.assert_array_equal(ob["id"], np.array([e[0] for e in self.log], np.int32).reshape(-1), err_msg=str(tag))
        np.testing.assert_array_equal(ob["frame"], np.array([e[1] for e in self.log], np.int32).reshape(-1), err_msg=str(tag))
        want_xy = np.array([e[2] for e in self.log], np.float32).reshape(-1, 2)
        want_cam = np.array([e[3] for e in self.log], np.float64).reshape(-1, 3)
        assert ob["xy"].dtype == np.float32 and ob["cam"].dtype == np.float64
        np.testing.assert_array_equal(ob["xy"].view(np.uint32), want_xy.view(np.uint32), err_msg="%s: xy" % (tag,))
        if len(want_cam):
            print("%s: largest |cam - checker| in the log = %.3e m" % (tag, np.max(np.abs(ob["cam"] - want_cam))))
        np.testing.assert_array_equal(ob["cam"].view(np.uint64), want_cam.view(np.uint64), err_msg="%s: cam" % (tag,))
        # ... and the product's own lists (the contract: RgbdList::xy / cam of the labelled points)
        pts = prod.points(stream) if isinstance(prod, RgbdBatch) else prod.points()
        cur = ob["frame"] == ref.frames[-1].index
        np.testing.assert_array_equal(ob["xy"][cur].view(np.uint32), pts["xy"][ids >= 0].view(np.uint32))
        np.testing.assert_array_equal(ob["cam"][cur].view(np.uint64), pts["cam"][ids >= 0].view(np.uint64))
        return m, ob

    def check_final(self, m, ob, ref, tag):
        pairs = ob["id"].astype(np.int64) * 100000 + ob["frame"]
        assert len(np.unique(pairs)) == len(pairs), tag                     # every (id, frame) once
        assert np.all(np.diff(ob["frame"]) >= 0), tag
        for k, lm in enumerate(ref.landmarks):
            sel = ob["id"] == k
            fr = ob["frame"][sel]
            assert len(fr) and fr.min() == m["first_frame"][k] and fr.max() == m["last_frame"][k], (tag, k, fr, m["first_frame"][k], m["last_frame"][k])
            # the measurements Landmark::update consumed, from the creating frame on, are the log of that landmark (updated points)
            upd = np.array([e[4] for e in self.log], bool)[sel]
            meas = sorted([(f, c) for f, c in lm.meas if f >= m["first_frame"][k]], key=lambda e: e[0])
            assert [f for f, _ in meas] == list(fr[upd]), (tag, k)
            np.testing.assert_array_equal(np.array([c for _, c in meas]).view(np.uint64), ob["cam"][sel][upd].view(np.uint64))
        assert self.compared > 0 and len(self.log) > 0


def _render(o, scene, ks):
    return [(o.render(scene, k)[0], o.render_depth(scene, k, 2e-3)) for k in ks]


@pytest.mark.gpu
@pytest.mark.parametrize("which,descriptor,max_depth,seed", CASES)
def test_map_and_log_equal_the_checker_loop(which, descriptor, max_depth, seed, monkeypatch):
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = setup(o, which, descriptor=descriptor, max_depth=max_depth, seed=seed)
    o.create(cfg, 0, 1)
    g = hip.load()
    ref = PyLoop(o, cfg, p)
    prod = RgbdTracker(g, cfg, p)
    ex = Expect()
    try:
        prod.enable_map(MAP_BIG)
        prod.enable_observations(OBS_BIG)
        seen = dict(recovered_with_id=0, temporary_predecessor=0)
        for k, (L, D) in enumerate(_render(o, scene, range(FRAMES))):
            info = ref.process(L, D)
            fi, _ = prod.process(L, D)
            assert fi.error_flags == 0 and fi.n_points == info["n_points"]
            premises(ref, info, seen)
            ids = ex.step(ref)
            m, ob = ex.check(prod, 0, ref, ids, (which, descriptor, k))
        ex.check_final(m, ob, ref, (which, descriptor))
        assert len(ref.landmarks) >= 50 and seen["recovered_with_id"] > 0, (len(ref.landmarks), seen)
        assert (seen["temporary_predecessor"] > 0) == bool(YAML[which]["tri"]), seen
        assert (m["last_frame"] < FRAMES - 1).any()                        # a landmark whose track ended: the case the map exists for
        assert ex.compared >= len(ref.landmarks)                           # every landmark was compared (nothing above is conditional)
        # tail reads: only what is new
        half = len(m["id"]) // 2
        tail = prod.map(0, first=half)
        np.testing.assert_array_equal(tail["id"], m["id"][half:]); np.testing.assert_array_equal(tail["xyz"], m["xyz"][half:])
        otail = prod.observations(0, first=len(ob["id"]) - 7)
        np.testing.assert_array_equal(otail["cam"], ob["cam"][-7:]); np.testing.assert_array_equal(otail["id"], ob["id"][-7:])
    finally:
        prod.destroy(); g.destroy(); o.destroy()


@pytest.mark.gpu
def test_map_and_log_across_reregistration_and_break(monkeypatch):
    """The scenario of test_rgbd_reregistration_paths (icl, stricter landmark minimum, a jump): frames with two and three registration
    attempts and a breakTrack — the same equalities, and every frame committed and logged once."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = setup(o, "icl", descriptor=0, max_depth=30.0, seed=41)
    cfg.minimum_number_of_landmarks_to_track = 30
    o.create(cfg, 0, 1)
    g = hip.load()
    ref = PyLoop(o, cfg, p)
    prod = RgbdTracker(g, cfg, p)
    ex = Expect()
    try:
        prod.enable_map(MAP_BIG)
        prod.enable_observations(OBS_BIG)
        attempts, broken, counts, maps = [], 0, [], []
        for k, (L, D) in enumerate(_render(o, scene, [0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 18])):
            info = ref.process(L, D)
            fi, _ = prod.process(L, D)
            assert fi.track_attempts == info["track_attempts"] and fi.track_broken == info["track_broken"] and fi.error_flags == 0
            attempts.append(fi.track_attempts); broken += fi.track_broken
            ids = ex.step(ref)
            m, ob = ex.check(prod, 0, ref, ids, ("reregistration", k, fi.track_attempts))
            counts.append(len(ob["id"])); maps.append(m)
        ex.check_final(m, ob, ref, "reregistration")
        assert 2 in attempts and 3 in attempts and broken >= 1, attempts
        assert len(ref.landmarks) >= 50
        # breakTrack ends every track: the landmarks of the frames before it outlive them, entry for entry
        k3 = attempts.index(3)
        assert len(maps[k3 - 1]["id"]) >= 50 and (m["last_frame"] < k3).all()
        _same({k: v[:len(maps[k3 - 1]["id"])] for k, v in m.items()}, maps[k3 - 1], MAP_KEYS, "map across breakTrack")
        assert counts[k3:] == [counts[k3 - 1]] * (len(counts) - k3)          # nothing is logged for tracks without a landmark
    finally:
        prod.destroy(); g.destroy(); o.destroy()


def _info_tuple(fi, nt):
    out = []
    for name, _ in fi._fields_:
        v = getattr(fi, name)
        if hasattr(v, "__len__"):
            v = tuple(v)
        if name == "error_flags":
            v = v & ~(MAP_FLAG | OBS_FLAG)
        out.append(v)
    return tuple(out) + (nt,)


def _same(a, b, keys, tag):
    assert sorted(a) == sorted(b)
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (tag, k)
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg="%s %s" % (tag, k))


MAP_KEYS = ("id", "xyz", "first_frame", "last_frame", "updates", "desc")
OBS_KEYS = ("id", "frame", "xy", "cam")


@pytest.mark.gpu
def test_batch_streams_equal_single_sequences(monkeypatch):
    """Three sequences in one context, the middle one jumps (two more registration attempts, breakTrack) while the others track on: every
    stream's ids, map and log bit-identical to the same sequence run alone."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    g = hip.load()
    n, B = 10, 3
    worlds = []
    for i in range(B):
        scene, cfg, p = setup(o, "tum", descriptor=1, seed=101 + 13 * i)
        scene.speed_m = scene.speed_m * (0.7 + 0.15 * i)
        worlds.append(_render(o, scene, list(range(n)) if i != 1 else [0, 1, 2, 3, 4, 20, 21, 22, 23, 24]))
    alone = []
    for frames in worlds:
        t = RgbdTracker(g, cfg, p)
        t.enable_map(MAP_BIG); t.enable_observations(OBS_BIG)
        ids = []
        for L, D in frames:
            t.process(L, D)
            ids.append(t.point_ids())
        alone.append((ids, t.map(), t.observations()))
        t.destroy()
    batch = RgbdBatch(g, cfg, p, B)
    try:
        batch.enable_map(MAP_BIG); batch.enable_observations(OBS_BIG)
        attempts = set()
        for f in range(n):
            res = batch.process(np.stack([worlds[i][f][0] for i in range(B)]), np.stack([worlds[i][f][1] for i in range(B)]))
            for i, (fi, _) in enumerate(res):
                attempts.add((i, fi.track_attempts))
                assert fi.error_flags == 0
                np.testing.assert_array_equal(batch.point_ids(i), alone[i][0][f], err_msg="frame %d sequence %d" % (f, i))
        assert (1, 3) in attempts and (0, 3) not in attempts and (2, 3) not in attempts, attempts
        for i in range(B):
            assert len(alone[i][1]["id"]) >= 50 and len(alone[i][2]["id"]) > 200
            _same(batch.map(i), alone[i][1], MAP_KEYS, "map of sequence %d" % i)
            _same(batch.observations(i), alone[i][2], OBS_KEYS, "log of sequence %d" % i)
    finally:
        batch.destroy(); o.destroy()


@pytest.mark.gpu
def test_map_and_log_do_not_perturb_the_tracker(monkeypatch):
    """Map + log on, the map only, both off; direct launches and the captured launch sequence (VSLAM_RGBD_GRAPH): poses, frame info (apart
    from bits 8 / 16) and the point lists identical over the run, the map identical between the two launch paths."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = setup(o, "tum", descriptor=1, seed=53)
    g = hip.load()
    frames = _render(o, scene, range(10))
    runs = {}
    for graph in ("0", "1"):
        monkeypatch.setenv("VSLAM_RGBD_GRAPH", graph)
        for mode in ("off", "map", "map+log"):
            t = RgbdTracker(g, cfg, p)
            try:
                if mode != "off":
                    t.enable_map(MAP_BIG)
                if mode == "map+log":
                    t.enable_observations(OBS_BIG)
                rec = []
                for L, D in frames:
                    fi, nt = t.process(L, D)
                    rec.append((_info_tuple(fi, nt), t.points()))
                runs[graph, mode] = (rec, t.map() if mode != "off" else None, t.observations() if mode == "map+log" else None)
            finally:
                t.destroy()
    base = runs["0", "off"][0]
    for key, (rec, m, ob) in runs.items():
        for k, ((ia, pa), (ib, pb)) in enumerate(zip(base, rec)):
            assert ia == ib, (key, k)
            _same(pa, pb, ("xy", "cam", "meta", "desc"), "%s frame %d" % (key, k))
    _same(runs["0", "map"][1], runs["1", "map"][1], MAP_KEYS, "map, graph 0 / 1")
    _same(runs["0", "map+log"][1], runs["1", "map+log"][1], MAP_KEYS, "map under the log, graph 0 / 1")
    _same(runs["0", "map"][1], runs["0", "map+log"][1], MAP_KEYS, "map with / without the log")
    _same(runs["0", "map+log"][2], runs["1", "map+log"][2], OBS_KEYS, "log, graph 0 / 1")
    assert len(runs["0", "map"][1]["id"]) >= 50 and len(runs["0", "map+log"][2]["id"]) > 200


@pytest.mark.gpu
def test_map_and_log_capacity(monkeypatch):
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = setup(o, "tum", descriptor=1, seed=59)
    g = hip.load()
    frames = _render(o, scene, range(FRAMES))
    full = RgbdTracker(g, cfg, p)
    small_map, small_log = RgbdTracker(g, cfg, p), RgbdTracker(g, cfg, p)
    try:
        full.enable_map(MAP_BIG); full.enable_observations(OBS_BIG)
        ids_full, cum_obs, infos, pts = [], [], [], []
        for L, D in frames:
            fi, nt = full.process(L, D)
            assert fi.error_flags == 0
            ids_full.append(full.point_ids()); cum_obs.append(full.observation_count()); infos.append(_info_tuple(fi, nt)); pts.append(full.points())
        mf, of = full.map(), full.observations()
        n_map, n_obs = len(mf["id"]), len(of["id"])
        assert n_map >= 50 and n_obs > 200
        # ---- the map at 40 %: ids below the capacity are handed out exactly as before, every later landmark is refused for its track's life
        cap = int(0.4 * n_map)
        small_map.enable_map(cap); small_map.enable_observations(OBS_BIG)
        refused_frames = 0
        for k, (L, D) in enumerate(frames):
            fi, nt = small_map.process(L, D)
            want_ids = np.where(ids_full[k] < cap, ids_full[k], -1)
            np.testing.assert_array_equal(small_map.point_ids(), want_ids, err_msg="frame %d" % k)
            refused = bool((ids_full[k] >= cap).any())          # (every labelled point of the full run was created or updated in its frame)
            assert bool(fi.error_flags & MAP_FLAG) == refused, "frame %d: bit 8 is %d, refused %d" % (k, fi.error_flags & MAP_FLAG, refused)
            assert fi.error_flags & ~MAP_FLAG == 0
            assert _info_tuple(fi, nt) == infos[k], k             # later frames are still tracked, and as before
            refused_frames += refused
        assert 0 < refused_frames < FRAMES
        ms = small_map.map()
        assert len(ms["id"]) == cap == small_map.map_size()
        _same(ms, {k: v[:cap] for k, v in mf.items()}, MAP_KEYS, "map at capacity %d" % cap)
        keep = of["id"] < cap
        _same(small_map.observations(), {k: v[keep] for k, v in of.items()}, OBS_KEYS, "log under the small map")
        # ---- the log at 40 %: exactly the first `capacity` entries; bit 16 in exactly the frames that dropped one
        ocap = int(0.4 * n_obs)
        assert cum_obs[0] <= ocap < cum_obs[-1]
        small_log.enable_map(MAP_BIG); small_log.enable_observations(ocap)
        for k, (L, D) in enumerate(frames):
            fi, nt = small_log.process(L, D)
            assert bool(fi.error_flags & OBS_FLAG) == (cum_obs[k] > ocap), "frame %d: bit 16 is %d, unconstrained count %d, capacity %d" % (
                k, fi.error_flags & OBS_FLAG, cum_obs[k], ocap)
            assert fi.error_flags & ~OBS_FLAG == 0
            assert small_log.observation_count() == min(cum_obs[k], ocap)
            assert _info_tuple(fi, nt) == infos[k], k
            np.testing.assert_array_equal(small_log.point_ids(), ids_full[k])
            _same(small_log.points(), pts[k], ("xy", "cam", "meta", "desc"), "points, frame %d" % k)
        _same(small_log.observations(), {k: v[:ocap] for k, v in of.items()}, OBS_KEYS, "log at capacity %d" % ocap)
        _same(small_log.map(), mf, MAP_KEYS, "map under the small log")
    finally:
        full.destroy(); small_map.destroy(); small_log.destroy(); o.destroy()


@pytest.mark.gpu
def test_map_and_log_lifetime_and_errors(monkeypatch):
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene, cfg, p = setup(o, "tum", descriptor=1, seed=61)
    g = hip.load()
    frames = _render(o, scene, range(10))
    t = RgbdTracker(g, cfg, p)
    first = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: t.enable_observations(OBS_BIG), lambda: t.map_size(), lambda: t.point_ids(), lambda: t.observation_count()):
            with pytest.raises(VslamError) as e:          # the log needs the map; the getters need what they read
                call()
            assert e.value.code == ERR_STATE
        with pytest.raises(VslamError) as e:
            t.enable_map(-1)
        assert e.value.code == ERR_INVALID
        t.enable_map(MAP_BIG)
        with pytest.raises(VslamError) as e:
            t.observation_count()
        assert e.value.code == ERR_STATE
        with pytest.raises(VslamError) as e:
            t.enable_observations(-1)
        assert e.value.code == ERR_INVALID
        n = g.lib.vslam_rgbd_get_map(t.h, 5, 0, 0, None, None, None, None)
        assert n == ERR_INVALID
        assert t.map_size() == 0 and len(t.point_ids()) == 0
        # the reference run: map and log on from frame 0
        first.enable_map(MAP_BIG); first.enable_observations(OBS_BIG)
        ids_first = []
        for L, D in frames:
            first.process(L, D)
            ids_first.append(first.point_ids())
        m0, o0 = first.map(), first.observations()
        # the map alone for four frames, then the log: enabled mid-sequence it starts with the next frame
        for L, D in frames[:4]:
            t.process(L, D)
        t.enable_observations(OBS_BIG)
        assert t.observation_count() == 0
        t.submit(*frames[4])
        for call in (lambda: t.map_size(), lambda: t.map(), lambda: t.observation_count(), lambda: t.observations(), lambda: t.point_ids(),
                     lambda: t.enable_map(MAP_BIG), lambda: t.enable_observations(OBS_BIG)):
            with pytest.raises(VslamError) as e:          # a frame is in flight
                call()
            assert e.value.code == ERR_STATE
        t.wait()
        for L, D in frames[5:]:
            t.process(L, D)
        _same(t.map(), m0, MAP_KEYS, "map, log enabled later")
        late = o0["frame"] >= 4
        _same(t.observations(), {k: v[late] for k, v in o0.items()}, OBS_KEYS, "log enabled after frame 3")
        # reset: both cleared and still enabled, ids from 0 again — the same sequence gives the same map and log
        t.reset()
        assert t.map_size() == 0 and t.observation_count() == 0 and len(t.point_ids()) == 0
        for k, (L, D) in enumerate(frames):
            t.process(L, D)
            np.testing.assert_array_equal(t.point_ids(), ids_first[k])
        _same(t.map(), m0, MAP_KEYS, "map after reset")
        _same(t.observations(), o0, OBS_KEYS, "log after reset")
        # the map enabled mid-sequence: tracks that already carry a landmark get an id at their next update, first_frame = that frame
        t.reset()
        t.enable_map(0)                                     # map and log off
        for call in (lambda: t.map_size(), lambda: t.observation_count(), lambda: t.enable_observations(OBS_BIG)):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE
        for L, D in frames[:5]:
            t.process(L, D)
        t.enable_map(MAP_BIG); t.enable_observations(OBS_BIG)
        assert t.map_size() == 0
        fi, _ = t.process(*frames[5])
        ids, pts = t.point_ids(), t.points()
        has_lm = pts["meta"][:, 2] > 0
        np.testing.assert_array_equal(ids >= 0, has_lm)     # every point whose landmark was updated in this frame, old tracks included
        assert has_lm.sum() > 30 and (pts["meta"][has_lm, 1] > 2).any()
        np.testing.assert_array_equal(ids[has_lm], np.arange(has_lm.sum()))
        m = t.map()
        assert (m["first_frame"] == 5).all() and (m["last_frame"] == 5).all()
        np.testing.assert_array_equal(m["updates"], pts["meta"][has_lm, 2])
        ob = t.observations()
        assert (ob["frame"] == 5).all() and len(ob["id"]) == has_lm.sum()
        # the entries are what the run with the map on from the start holds for the same landmarks after frame 5 (first_frame apart)
        ref5 = RgbdTracker(g, cfg, p)
        try:
            ref5.enable_map(MAP_BIG)
            for L, D in frames[:6]:
                ref5.process(L, D)
            r5, rid = ref5.map(), ref5.point_ids()
            np.testing.assert_array_equal(rid >= 0, has_lm)
            np.testing.assert_array_equal(m["xyz"].view(np.uint64), r5["xyz"][rid[has_lm]].view(np.uint64))
            np.testing.assert_array_equal(m["desc"], r5["desc"][rid[has_lm]])
        finally:
            ref5.destroy()
        t.enable_observations(0)                            # the log off, the map stays
        assert t.map_size() == len(m["id"])
        with pytest.raises(VslamError) as e:
            t.observation_count()
        assert e.value.code == ERR_STATE
    finally:
        t.destroy(); first.destroy()
    # the host-driven loop does not have the feature
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1")
    h = RgbdTracker(g, cfg, p)
    try:
        for call in (lambda: h.enable_map(MAP_BIG), lambda: h.enable_observations(OBS_BIG), lambda: h.map_size(), lambda: h.point_ids()):
            with pytest.raises(VslamError) as e:
                call()
            assert e.value.code == ERR_STATE and "host-driven loop" in str(e.value)
        h.process(*frames[0])                               # and goes on tracking
    finally:
        h.destroy(); o.destroy()


def _write_tum_folder(root, o, scene, n, unit, skew=0.004):
    """tests/test_run_rgbd.py's helper: a TUM RGB-D folder rendered from the synthetic scene."""
    from vslam_pose_estimation_framework_amd import io_formats as io
    (root / "rgb").mkdir(parents=True); (root / "depth").mkdir()
    rgb_lines, dep_lines, gt_lines, frames = ["# color images", "# timestamp filename"], ["# depth maps"], ["# ground truth trajectory", "# timestamp tx ty tz qx qy qz qw"], []
    for k in range(n):
        L = o.render(scene, k)[0]
        D = o.render_depth(scene, k, unit)
        t = 1305031100.0 + k / 30.0
        io.write_png(str(root / "rgb" / ("%.6f.png" % t)), np.stack([L, L, L], axis=2))
        io.write_png(str(root / "depth" / ("%.6f.png" % (t + skew))), D)
        rgb_lines.append("%.6f rgb/%.6f.png" % (t, t)); dep_lines.append("%.6f depth/%.6f.png" % (t + skew, t + skew))
        T = np.array(o.gt_pose(scene, k)).reshape(3, 4)
        q = io.rotation_to_quaternion(T[:, :3])
        gt_lines.append("%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f" % ((t, T[0, 3], T[1, 3], T[2, 3]) + tuple(q)))
        frames.append((L, D))
    (root / "rgb.txt").write_text("\n".join(rgb_lines) + "\n")
    (root / "depth.txt").write_text("\n".join(dep_lines) + "\n")
    (root / "groundtruth.txt").write_text("\n".join(gt_lines) + "\n")
    return frames


@pytest.mark.gpu
def test_run_rgbd_map_and_observations_end_to_end(tmp_path, monkeypatch):
    """tools/run_rgbd.py --map --observations on a rendered TUM folder: the PLY is the API's map, the bundle the API's log (exact round
    trip), the residual figures are printed and returned.  Asserted: at least 95 % of the observations project in front of their camera
    (w > 0).  The pixel and depth medians are reported, not asserted."""
    import run_rgbd
    from _oracle import Oracle
    from vslam_pose_estimation_framework_amd import evaluation, io_formats
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    scene = o.scene_kitti(scale=0.5, seed=13)
    scene.speed_m = 0.25; scene.sway_m = 0.4
    n, unit = 14, 2e-3
    frames = _write_tum_folder(tmp_path / "seq", o, scene, n, unit)
    intr = "%r,%r,%r,%r" % (scene.fx, scene.fy, scene.cx, scene.cy)
    ply, npz = str(tmp_path / "map.ply"), str(tmp_path / "bundle.npz")
    lines = []
    res = run_rgbd.run(str(tmp_path / "seq"), "tum", intr, unit, None, depth_scale=4.0, log=lines.append, map_path=ply, obs_path=npz)
    assert res["frames"] == n and res["error_flags"] == 0
    g = hip.load()
    K = np.array([[scene.fx, 0, scene.cx], [0, scene.fy, scene.cy], [0, 0, 1.0]])
    cfg, p = run_rgbd.configure(g, "tum", scene.rows, scene.cols, K, unit, 1, 0, 4.0)
    tr = RgbdTracker(g, cfg, p)
    try:
        tr.enable_map(MAP_BIG); tr.enable_observations(OBS_BIG)
        poses = [np.array(tr.process(L, D)[0].camera_left_to_world) for L, D in frames]
        m, ob = tr.map(), tr.observations()
    finally:
        tr.destroy(); o.destroy()
    assert len(m["id"]) >= 50 and len(ob["id"]) > 200
    cloud = io_formats.read_ply(ply)
    np.testing.assert_array_equal(cloud["xyz"].view(np.uint64), m["xyz"].view(np.uint64))
    for k in ("id", "first_frame", "last_frame", "updates"):
        np.testing.assert_array_equal(cloud[k], m[k])
    b = io_formats.read_bundle_rgbd(npz)
    np.testing.assert_array_equal(b["K"], K)
    np.testing.assert_array_equal(b["poses"], np.array(poses).reshape(n, 12))
    _same(b["map"], m, MAP_KEYS, "bundle map")
    _same({k: b["obs_" + k] for k in OBS_KEYS}, ob, OBS_KEYS, "bundle log")
    _same(res["map"], m, MAP_KEYS, "returned map")
    _same(res["observations"], ob, OBS_KEYS, "returned log")
    rp = res["reprojection"]
    r, valid = evaluation.reprojection_residuals_uvd(K, b["poses"], m["xyz"], ob["id"], ob["frame"], ob["xy"], ob["cam"])
    assert rp["observations"] == len(ob["id"]) and rp["landmarks"] == len(m["id"]) and rp["valid"] == int(valid.sum())
    assert valid.mean() >= 0.95, valid.mean()
    assert rp["median_px"] == float(np.median(np.linalg.norm(r[valid, :2], axis=1))) and rp["median_depth_m"] == float(np.median(np.abs(r[valid, 2])))
    assert rp["p90_px"] is not None and rp["p90_depth_m"] is not None
    assert any("residuals against the map" in ln and "px" in ln and " m" in ln for ln in lines), lines
    print("run_rgbd residuals: %d observations of %d landmarks, pixel norm median %.3f px / p90 %.3f px, depth median %.4f m / p90 %.4f m" % (
        rp["observations"], rp["landmarks"], rp["median_px"], rp["p90_px"], rp["median_depth_m"], rp["p90_depth_m"]))
