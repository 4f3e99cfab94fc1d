"""Motion models of the RGB-D tracker on the GPU: the device loop (direct and captured, VSLAM_RGBD_GRAPH=1), a batch of 3 and the
host-driven loop (VSLAM_RGBD_HOST=1) against the checker loop with the models restated (motion_cases.motion_loop over the CPU oracle),
as test_rgbd_mode.py compares: counters and lists exact, pose within 1e-4.  xtion runs under its own model, CAMERA_ODOMETRY."""
import ctypes as C

import numpy as np
import pytest

import motion_cases as mc
from test_rgbd_mode import POSE_RTOL, setup
from vslam_pose_estimation_framework_amd import hip
from vslam_pose_estimation_framework_amd.capi import (ERR_INVALID, ERR_STATE, MOTION_CAMERA_ODOMETRY as ODO, MOTION_CONSTANT_VELOCITY as CV, MOTION_NONE as NONE,
                                                      RgbdBatch, RgbdTracker, VslamError, _p)

pytestmark = pytest.mark.gpu

N = 12
FIELDS = (("status", "status"), ("n_keypoints", "n_keypoints_left"), ("n_tracked", "n_tracked"), ("n_lost", "n_lost"), ("n_tracked_landmarks", "n_tracked_landmarks"),
          ("aligner_ran", "aligner_ran"), ("n_inliers", "n_inliers"), ("aligner_iterations", "aligner_iterations"), ("n_after_prune", "n_after_prune"),
          ("n_recovered", "n_recovered"), ("n_active_landmarks", "n_active_landmarks"), ("n_new", "n_new_stereo"), ("n_points", "n_points"),
          ("window_pixels", "window_pixels"), ("track_attempts", "track_attempts"), ("fallback", "fallback"), ("track_broken", "track_broken"),
          ("status_at_start", "status_at_start"))
# which configuration, scene seed, model, limit, blank frames, wrong guess (frame, heading error in rad) — the CPU premise scenarios of
# test_motion_host.py, and xtion under its own model
SCENARIOS = {
    "tum-blank6": ("tum", 26, ODO, 0, (6,), None),
    "tum-blank6-limit2": ("tum", 33, ODO, 2, (6,), None),
    "tum-blank1": ("tum", 40, ODO, 0, (1,), None),
    "tum-wrong6-limit2": ("tum", 40, ODO, 2, (), (6, 0.25)),
    "tum-none": ("tum", 26, NONE, 0, (), None),
    "xtion": ("xtion", 26, ODO, 0, (), None),
    "xtion-blank6-limit2": ("xtion", 26, ODO, 2, (6,), None),
}
_reference = {}


def reference(name):
    """The scenario once on the checker loop over the oracle: (cfg, params, frames, guesses, [per frame: info, point list])."""
    if name not in _reference:
        from _oracle import Oracle
        which, seed, model, limit, blank, wrong = SCENARIOS[name]
        o = Oracle()
        try:
            scene, cfg, p = setup(o, which, seed=seed)
            o.create(cfg, 0, 1)
            frames = mc.rgbd_frames(o, scene, N, blank)
            guesses = mc.gt_guesses(o, scene, list(range(N)))
            if wrong is not None:
                guesses = mc.with_wrong_guess(guesses, wrong[0], wrong[1])
            loop = mc.motion_loop(o, cfg, p, model, limit)
            rec = []
            for k, (L, D) in enumerate(frames):
                loop.set_guess(guesses[k])
                info = dict(loop.process(L, D))
                cur = loop.frames[-1]
                prevlist = (loop.frames[-2].points + loop.frames[-2].temps) if k else []
                pts = [(q.xy.copy(), q.desc.copy(), np.array(q.cam), prevlist.index(q.previous) if q.previous is not None else -1, q.track_len,
                        q.landmark.updates if q.landmark is not None else 0, int(q.unreliable)) for q in cur.points]
                rec.append((info, pts))
        finally:
            o.destroy()
        _reference[name] = (cfg, p, frames, guesses, rec, model, limit)
    return _reference[name]


def check_frame(where, fi, n_temp, pts, want):
    a, cur = want
    for name, field in FIELDS:
        assert a[name] == getattr(fi, field), (where, name, a[name], getattr(fi, field))
    assert a["thresholds"] == list(fi.thresholds)[:len(a["thresholds"])] and a["n_temporary"] == n_temp, where
    assert a["tau_track"] == fi.tau_track, where
    To, Tg = a["pose"], np.array(fi.camera_left_to_world).reshape(3, 4)
    assert np.linalg.norm(Tg - To) / np.linalg.norm(To) <= POSE_RTOL, (where, Tg, To)
    assert np.abs(np.array(fi.previous_to_current).reshape(3, 4) - a["prior"]).max() <= 1e-9, where
    assert len(pts["xy"]) == len(cur), where
    for i, (xy, desc, cam, prev, tlen, upd, unrel) in enumerate(cur):
        assert np.array_equal(pts["xy"][i].view(np.uint32), xy.view(np.uint32)), (where, i)
        np.testing.assert_array_equal(pts["desc"][i], desc)
        np.testing.assert_allclose(pts["cam"][i], cam, rtol=1e-12, atol=0)
        assert tuple(pts["meta"][i]) == (prev, tlen, upd, unrel), (where, i, tuple(pts["meta"][i]), (prev, tlen, upd, unrel))


@pytest.mark.parametrize("impl", ["device", "graph", "host"])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_rgbd_motion_models_match_the_checker_loop(name, impl, monkeypatch):
    monkeypatch.setenv("VSLAM_RGBD_HOST", "1" if impl == "host" else "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1" if impl == "graph" else "0")
    cfg, p, frames, guesses, rec, model, limit = reference(name)
    g = hip.load().create(cfg, 0, 1)
    prod = RgbdTracker(g, cfg, p)
    try:
        prod.set_motion_model(model, limit)
        assert prod.motion_model() == (model, limit)
        taken = 0
        for k, (L, D) in enumerate(frames):
            prod.set_pose_guess(guesses[k])
            fi, n_temp = prod.process(L, D)
            check_frame((name, impl, k), fi, n_temp, prod.points(), rec[k])
            assert fi.track_broken == 0 or model != ODO
            taken += fi.fallback
            if name == "tum-wrong6-limit2" and k in (6, 7):
                # the run's own report: frame 6 tracks no landmark and returns on the guess; frame 7, whose prior carries the same wrong
                # guess as its previous one, reaches the third attempt: _fallbackEstimate in the place of breakTrack, behind the aligner
                want = (1, 0, 1, 0) if k == 6 else (3, 1, 1, 0)
                assert (fi.track_attempts, fi.aligner_ran, fi.fallback, fi.track_broken) == want, (k, fi.track_attempts, fi.aligner_ran, fi.fallback, fi.track_broken)
        if SCENARIOS[name][4] or SCENARIOS[name][5]:
            assert taken >= 1          # the blank frame's pose came from the guess
        if name == "tum-blank6":       # permanent dead reckoning under the prune rule
            assert all(r[0]["fallback"] == 1 and r[0]["n_tracked_landmarks"] == 0 for r in rec[6:])
        if name.endswith("limit2"):
            assert any(r[0]["status"] == 0 for r in rec[7:]) and rec[-1][0]["status"] == 1 and rec[-1][0]["n_tracked_landmarks"] > 0
    finally:
        prod.destroy(); g.destroy()


def test_rgbd_batch_of_three_with_map_and_log(monkeypatch):
    """Three sequences of one camera in one context under CAMERA_ODOMETRY with limit 2 and a blank frame 6, the map and the log on, guesses
    as one host array and, from frame 8 on, as a device array: every stream equals its own sequence on the checker loop."""
    import torch
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    monkeypatch.setenv("VSLAM_RGBD_GRAPH", "1")
    o = Oracle()
    seeds = (26, 33, 40)
    try:
        seqs, gts, loops = [], [], []
        for seed in seeds:
            scene, cfg, p = setup(o, "tum", seed=seed)
            o.create(cfg, 0, 1)
            seqs.append(mc.rgbd_frames(o, scene, N, (6,)))
            gts.append(mc.gt_guesses(o, scene, list(range(N))))
            loops.append(mc.motion_loop(o, cfg, p, ODO, 2))
        g = hip.load().create(cfg, 0, 1)
        batch = RgbdBatch(g, cfg, p, 3)
        try:
            batch.set_motion_model(ODO, 2)
            batch.enable_map(4000); batch.enable_observations(20000)
            for k in range(N):
                G = np.stack([gts[s][k] for s in range(3)])
                if k < 8:
                    batch.set_pose_guesses(G)
                else:
                    Gd = torch.from_numpy(G).to(torch.device("cuda", 0))
                    torch.cuda.synchronize()
                    batch.set_pose_guesses_device(Gd.data_ptr())
                infos = batch.process(np.stack([seqs[s][k][0] for s in range(3)]), np.stack([seqs[s][k][1] for s in range(3)]))
                for s in range(3):
                    loops[s].set_guess(gts[s][k])
                    a = dict(loops[s].process(*seqs[s][k]))
                    cur = loops[s].frames[-1]
                    prevlist = (loops[s].frames[-2].points + loops[s].frames[-2].temps) if k else []
                    pts = [(q.xy.copy(), q.desc.copy(), np.array(q.cam), prevlist.index(q.previous) if q.previous is not None else -1, q.track_len,
                            q.landmark.updates if q.landmark is not None else 0, int(q.unreliable)) for q in cur.points]
                    check_frame(("batch", s, k), infos[s][0], infos[s][1], batch.points(s), (a, pts))
            assert all(batch.map_size(s) > 0 for s in range(3))
        finally:
            batch.destroy(); g.destroy()
    finally:
        o.destroy()


def test_rgbd_motion_contract(monkeypatch):
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene, cfg, p = setup(o, "tum", seed=26)
        frames = mc.rgbd_frames(o, scene, 3)
    finally:
        o.destroy()
    g = hip.load().create(cfg, 0, 1)
    T = mc.identity()
    for host in ("0", "1"):
        monkeypatch.setenv("VSLAM_RGBD_HOST", host)
        t = RgbdTracker(g, cfg, p)
        lib = t.lib
        try:
            assert t.motion_model() == (CV, 0)
            for model, limit in ((-1, 0), (3, 0), (ODO, -1), (NONE, 1), (CV, 2)):
                assert lib.vslam_rgbd_set_motion_model(t.h, C.c_int(model), C.c_int32(limit)) == ERR_INVALID
            assert lib.vslam_rgbd_set_motion_model(None, C.c_int(0), C.c_int32(0)) == ERR_INVALID
            assert lib.vslam_rgbd_set_pose_guess(t.h, C.c_int32(0), None) == ERR_INVALID
            assert lib.vslam_rgbd_set_pose_guess(t.h, C.c_int32(1), _p(T, C.c_double)) == ERR_INVALID
            assert lib.vslam_rgbd_set_pose_guess(t.h, C.c_int32(-1), _p(T, C.c_double)) == ERR_INVALID
            assert lib.vslam_rgbd_set_pose_guesses(t.h, None, C.c_int(0)) == ERR_INVALID
            assert lib.vslam_rgbd_set_pose_guess(None, C.c_int32(0), _p(T, C.c_double)) == ERR_INVALID
            assert t.motion_model() == (CV, 0)
            t.set_motion_model(ODO, 2)
            t.submit(*frames[0])
            assert lib.vslam_rgbd_set_motion_model(t.h, C.c_int(NONE), C.c_int32(0)) == ERR_STATE
            assert lib.vslam_rgbd_set_pose_guess(t.h, C.c_int32(0), _p(T, C.c_double)) == ERR_STATE
            t.wait()
            if host == "0":      # a device array, then a host guess: whichever was set last holds (the host copy waits for the queue's)
                import torch
                Gd = torch.from_numpy(mc.translation(0.0, 0.0, 9.0)).to(torch.device("cuda", 0))
                torch.cuda.synchronize()
                t.set_pose_guesses_device(Gd.data_ptr())
            t.set_pose_guess(mc.translation(0.0, 0.0, 0.25))
            fi, _ = t.process(*frames[1])
            assert fi.track_broken == 0
            if fi.fallback:      # the pose is the guess's: the prior is the one the host guess gives
                assert list(fi.previous_to_current) == list(mc.translation(0.0, 0.0, -0.25))
            assert np.linalg.norm(np.array(fi.camera_left_to_world)[[3, 7, 11]]) < 1.0      # never the 9 m of the device array
            t.reset()
            assert t.motion_model() == (ODO, 2)          # the model survives a reset
            t.set_motion_model(CV)
            fi, _ = t.process(*frames[0])
            assert list(fi.previous_to_current) == list(T)
        finally:
            t.destroy()
    g.destroy()


def test_rgbd_default_is_untouched(monkeypatch):
    """Constant velocity set explicitly, and odometry switched back before frame 0 with a guess stored, equal an untouched tracker."""
    from _oracle import Oracle
    monkeypatch.setenv("VSLAM_RGBD_HOST", "0")
    o = Oracle()
    try:
        scene, cfg, p = setup(o, "tum", seed=33)
        frames = mc.rgbd_frames(o, scene, 6)
    finally:
        o.destroy()
    g = hip.load().create(cfg, 0, 1)
    trackers = [RgbdTracker(g, cfg, p) for _ in range(3)]
    try:
        trackers[1].set_motion_model(CV)
        trackers[2].set_motion_model(ODO, 2); trackers[2].set_motion_model(CV); trackers[2].set_pose_guess(mc.translation(1.0, 2.0, 3.0))
        for L, D in frames:
            out = [t.process(L, D) for t in trackers]
            assert bytes(out[0][0]) == bytes(out[1][0]) == bytes(out[2][0]) and out[0][1] == out[1][1] == out[2][1]
            pts = [t.points() for t in trackers]
            for key in ("xy", "cam", "meta", "desc"):
                np.testing.assert_array_equal(pts[0][key], pts[1][key]); np.testing.assert_array_equal(pts[0][key], pts[2][key])
    finally:
        for t in trackers:
            t.destroy()
        g.destroy()
