"""Shared pieces of the motion-model tests (test_motion_host.py, test_motion_gpu.py, test_motion_rgbd_gpu.py, test_run_motion.py): the
prior's reference arithmetic and its error bound, the hand cases, random rigid transforms, ground-truth pose guesses of the synthetic
scenes, the stereo scenarios (a drop-out gap, a blank pair, a wrong guess, a ghosted pair), the runner that holds the fused stereo path
against host_tracker.PoseTracker3D (the only piece that needs a GPU; it loads the library when called), and the RGB-D checker loop with
the three models restated."""
import math

import numpy as np

U = 2.0 ** -53          # unit round-off of float64

GAP_FRAMES = list(range(0, 6)) + list(range(10, 16))      # frames 0..5 then 10..15: a four-frame drop-out


def identity():
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


def to44(T, dtype=np.float64):
    M = np.zeros((4, 4), dtype)
    M[:3, :] = np.asarray(T, dtype).reshape(3, 4)
    M[3, 3] = 1
    return M


def prior_reference(guess, guess_prev):
    """inverse(guess) * guess_prev in extended precision (numpy longdouble), rounded to float64, and the elementwise bound
    8 * 2^-53 * (|A| |B|) on what the float64 evaluation may differ from it, with A = inverse(guess) = [R^T | -R^T t] as computed and
    B = guess_prev, both as 4 x 4 homogeneous matrices: the bound of two three-term dot products and one subtraction."""
    g = np.asarray(guess, np.float64).reshape(-1, 3, 4)
    p = np.asarray(guess_prev, np.float64).reshape(-1, 3, 4)
    out = np.zeros_like(g)
    bound = np.zeros_like(g)
    for i in range(len(g)):
        R, t = g[i, :, :3].astype(np.longdouble), g[i, :, 3].astype(np.longdouble)
        Rp, tp = p[i, :, :3].astype(np.longdouble), p[i, :, 3].astype(np.longdouble)
        out[i, :, :3] = (R.T @ Rp).astype(np.float64)
        out[i, :, 3] = (R.T @ tp - R.T @ t).astype(np.float64)
        A = np.abs(np.linalg.inv(to44(g[i])))
        bound[i] = 8 * U * (A @ np.abs(to44(p[i])))[:3, :]
    return out.reshape(-1, 12), bound.reshape(-1, 12)


def translation(x, y, z):
    T = identity()
    T[3], T[7], T[11] = x, y, z
    return T


def rot_z90(x=0.0, y=0.0, z=0.0):
    """90 degrees about z (entries 0 and +-1 only) with a translation: every product is exact."""
    return np.array([0, -1, 0, x, 1, 0, 0, y, 0, 0, 1, z], np.float64)


def hand_cases():
    """(guess, guess_prev, expected inverse(guess) * guess_prev), all exactly representable: a float64 evaluation in any order gives
    these bits."""
    cases = []
    # dyadic pure translations: prior = guess_prev - guess
    cases.append((translation(0.5, -0.25, 4.0), translation(0.25, 0.125, 3.0), translation(-0.25, 0.375, -1.0)))
    cases.append((translation(1024.0, 0.0, -2048.5), translation(0.0, 0.0, 0.0), translation(-1024.0, 0.0, 2048.5)))
    # a 90 degree rotation: R^T (t_prev - t) with R^T = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], rotation part R^T * I
    cases.append((rot_z90(1.0, 2.0, 3.0), translation(2.0, 4.0, 8.0), np.array([0, 1, 0, 2.0, -1, 0, 0, -1.0, 0, 0, 1, 5.0], np.float64)))
    # guess == guess_prev: identity
    cases.append((rot_z90(3.0, -1.5, 0.75), rot_z90(3.0, -1.5, 0.75), identity()))
    cases.append((translation(7.0, 8.0, 9.0), translation(7.0, 8.0, 9.0), identity()))
    return cases


def random_rigid(rng, n, t_max=1000.0):
    """n rigid transforms [n, 12]: rotations from random unit quaternions, translations uniform in +-t_max metres."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    T = np.zeros((n, 3, 4), np.float64)
    T[:, :, :3] = R
    T[:, :, 3] = rng.uniform(-t_max, t_max, size=(n, 3))
    return T.reshape(n, 12)


def gt_guesses(oracle, scene, frames):
    """camera_left_to_world of every frame relative to the first one, as an odometry source would report it: float64 [len(frames), 12]."""
    first = np.linalg.inv(to44(oracle.gt_pose(scene, frames[0])))
    return np.stack([(first @ to44(oracle.gt_pose(scene, k)))[:3, :].reshape(12) for k in frames])


def with_noise(guesses, sigma_m, seed):
    """The guesses with Gaussian noise of sigma_m metres on every translation but the first."""
    g = np.array(guesses, np.float64).reshape(-1, 3, 4).copy()
    g[1:, :, 3] += np.random.default_rng(seed).normal(scale=sigma_m, size=(len(g) - 1, 3))
    return g.reshape(-1, 12)


def with_wrong_guess(guesses, k, angle_rad):
    """Frame k's guess turned by angle_rad about the camera's y axis (a heading error of the odometry)."""
    g = np.array(guesses, np.float64).reshape(-1, 3, 4).copy()
    c, s = math.cos(angle_rad), math.sin(angle_rad)
    g[k, :, :3] = g[k, :, :3] @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return g.reshape(-1, 12)


def render_sequence(oracle, scene, frames, blank=()):
    """[(left, right)] of the frames; positions listed in `blank` are all-zero pairs (a covered lens: no keypoint)."""
    out = []
    for i, k in enumerate(frames):
        L, R = oracle.render(scene, k)
        if i in blank:
            L, R = np.zeros_like(L), np.zeros_like(R)
        out.append((L, R))
    return out


def with_ghost_pair(oracle, scene, frames, k, weight=0.5, ghost_seed_offset=100):
    """The rendered sequence with position k's pair blended, at `weight`, with the same frame of another scene (a reflection on the
    lens): enough of the previous frame's points still match for the registration to run, too few of them agree for the aligner."""
    seq = render_sequence(oracle, scene, frames)
    ghost = oracle.scene_kitti(scale=0.4, seed=int(scene.seed) + ghost_seed_offset)
    ghost.rows, ghost.cols, ghost.fx, ghost.fy, ghost.cx, ghost.cy = scene.rows, scene.cols, scene.fx, scene.fy, scene.cx, scene.cy
    other = oracle.render(ghost, frames[k])
    seq[k] = tuple(((1 - weight) * a.astype(np.float64) + weight * b.astype(np.float64)).astype(np.uint8) for a, b in zip(seq[k], other))
    return seq


def position_error(pose12, gt_rel12):
    return float(np.linalg.norm(np.asarray(pose12, np.float64).reshape(3, 4)[:, 3] - np.asarray(gt_rel12, np.float64).reshape(3, 4)[:, 3]))


def decision(fi, previous_pose):
    """Which of the CAMERA_ODOMETRY decisions a frame's report shows, or None: 'guess_only' (Tracking, no tracked landmarks: the pose is
    the guess's, no aligner), 'third_attempt' (Tracking, the third attempt failed: _fallbackEstimate in the place of breakTrack),
    'localizing_fallback' (Localizing fallback whose pose moved with the guess)."""
    from vslam_pose_estimation_framework_amd.capi import LOCALIZING, TRACKING
    if not fi.fallback or fi.track_broken:
        return None
    if fi.status_at_start == TRACKING:
        if fi.track_attempts == 3:
            return "third_attempt"
        return "guess_only" if not fi.aligner_ran else None
    if fi.status_at_start == LOCALIZING and previous_pose is not None and list(fi.camera_left_to_world) != list(previous_pose):
        return "localizing_fallback"
    return None


# ---- the fused stereo path against host_tracker.PoseTracker3D over the stage entries (GPU) --------------------------------------------
INFO_FIELDS = ("status", "status_at_start", "n_keypoints_left", "n_keypoints_right", "n_tracked", "n_lost", "n_tracked_landmarks", "aligner_ran",
               "n_after_prune", "n_recovered", "n_active_landmarks", "n_new_stereo", "n_points", "window_pixels", "track_attempts", "tau_track")
ALIGNER_FIELDS = ("n_inliers", "n_outliers", "aligner_iterations", "aligner_converged", "total_error")      # of a frame whose last attempt ran the aligner


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run_stereo(oracle, scenes, frames, model, guesses=None, limit=0, blank=(), inactive=None, device_guesses=False, device_images=False,
               host_tracker_check=True, sequences=None):
    """len(scenes) streams of one fused context, frame by frame, each stream beside a PoseTracker3D with the same model over the stage
    entries of a one-stream context of its own: frame report, points, pose and prior bit for bit.  guesses: per stream [len(frames), 12]
    or None; blank: frame positions rendered black (sequences: the image pairs per stream, in the place of the rendered ones); inactive: {stream: positions at which the stream is switched off}.  On every frame
    whose pose is the guess's the prior must be the stand-alone entry's output and the pose previous * inverse(prior).  Returns, per
    stream, one record per processed frame: dict(pos, fi, decision, prior_pose)."""
    from vslam_pose_estimation_framework_amd import hip, host_tracker
    from vslam_pose_estimation_framework_amd.capi import MOTION_CAMERA_ODOMETRY
    B = len(scenes)
    inactive = inactive or {}
    cfg = oracle.config_for_scene(scenes[0])
    rows, cols = cfg.rows, cfg.cols
    fused = hip.load().create(cfg, 0, B)
    staged, trackers = [], []
    records = [[] for _ in range(B)]
    keep = []                                      # device buffers of the frame in flight
    try:
        fused.set_motion_model(model, limit)
        assert fused.motion_model() == (model, limit)
        if host_tracker_check:
            for s in range(B):
                api = hip.load().create(cfg, 0, 1)
                staged.append(api)
                trackers.append(host_tracker.PoseTracker3D(api, motion_model=model, dead_reckoning_limit=limit))
        seqs = sequences if sequences is not None else [render_sequence(oracle, sc, frames, blank) for sc in scenes]
        last_guess = [identity() for _ in range(B)]
        prev_pose = [None] * B
        was_active = [True] * B
        for i in range(len(frames)):
            active = [i not in inactive.get(s, ()) for s in range(B)]
            for s in range(B):
                if active[s] != was_active[s]:
                    fused.set_stream_active(s, active[s])
            was_active = active
            frozen = {s: fused.pose_guess(s) for s in range(B) if not active[s]}
            L = np.stack([seqs[s][i][0] for s in range(B)])
            R = np.stack([seqs[s][i][1] for s in range(B)])
            if guesses is not None:
                G = np.stack([guesses[s][i] for s in range(B)])
                if device_guesses:
                    import torch
                    Gd = torch.from_numpy(G).to(torch.device("cuda", 0))
                    torch.cuda.synchronize()
                    keep.append(Gd)
                    fused.set_pose_guesses_device(Gd.data_ptr())
                elif B == 1:
                    fused.set_pose_guess(G[0], 0)
                else:
                    fused.set_pose_guesses(G)
            if device_images:
                import torch
                Ld, Rd = torch.from_numpy(L).to(torch.device("cuda", 0)), torch.from_numpy(R).to(torch.device("cuda", 0))
                torch.cuda.synchronize()
                keep.extend([Ld, Rd])
                fused.process_device(Ld.data_ptr(), Rd.data_ptr(), cols, rows * cols)
            else:
                fused.process_host(L, R)
            fused.synchronize()
            del keep[:]
            for s in range(B):
                if not active[s]:
                    after = fused.pose_guess(s)
                    assert np.array_equal(_bits(frozen[s][0]), _bits(after[0])) and np.array_equal(_bits(frozen[s][1]), _bits(after[1])), (i, s)
                    continue
                ff = fused.frame_info(s)
                where = (i, s)
                if host_tracker_check:
                    t = trackers[s]
                    if guesses is not None:
                        t.set_guess(guesses[s][i])
                    fs = t.compute(seqs[s][i][0], seqs[s][i][1])
                    for name in INFO_FIELDS + (ALIGNER_FIELDS if ff.aligner_ran else ()):
                        assert getattr(fs, name) == getattr(ff, name), (where, name, getattr(fs, name), getattr(ff, name))
                    assert (t.fallback, t.track_broken) == (ff.fallback, ff.track_broken), (where, t.fallback, t.track_broken, ff.fallback, ff.track_broken)
                    assert np.array_equal(_bits(list(fs.camera_left_to_world)), _bits(list(ff.camera_left_to_world))), where
                    assert np.array_equal(_bits(list(fs.previous_to_current)), _bits(list(ff.previous_to_current))), where
                    ps, pf = staged[s].points(0), fused.points(s)
                    for key in ("kp", "meta", "cam", "lm"):
                        np.testing.assert_array_equal(ps[key], pf[key], err_msg=repr((where, key)))
                d = decision(ff, prev_pose[s])
                if model == MOTION_CAMERA_ODOMETRY and ff.fallback:
                    # the pose was taken from the guess: prior == the entry's output, pose == previous * inverse(prior)
                    g = guesses[s][i] if guesses is not None else identity()
                    want = fused.motion_prior(g, last_guess[s])[0]
                    assert np.array_equal(_bits(want), _bits(list(ff.previous_to_current))), (where, want, list(ff.previous_to_current))
                    pose = host_tracker._mul(list(prev_pose[s]), host_tracker._inverse([float(v) for v in want]))
                    assert np.array_equal(_bits(pose), _bits(list(ff.camera_left_to_world))), where
                if guesses is not None:
                    last_guess[s] = np.array(guesses[s][i], np.float64)
                    g_now, g_prev = fused.pose_guess(s)
                    assert np.array_equal(_bits(g_now), _bits(last_guess[s])), where
                    if model == MOTION_CAMERA_ODOMETRY:
                        assert np.array_equal(_bits(g_prev), _bits(last_guess[s])), where
                records[s].append(dict(pos=i, fi=ff, decision=d, previous_pose=prev_pose[s]))
                prev_pose[s] = list(ff.camera_left_to_world)
        return records
    finally:
        for api in staged:
            api.destroy()
        fused.destroy()


# ---- the RGB-D checker loop with the three motion models (rgbd_loop.py itself stays as it is) ------------------------------------------
def _eye34():
    return np.hstack([np.eye(3), np.zeros((3, 1))])


def motion_loop(api, cfg, params, model=0, limit=0):
    """rgbd_loop.RgbdTracker restated with Parameters::MotionModel (pose_tracker_3d.cpp:40-66, 316-341, 405-417, 551-566) and the
    dead-reckoning limit: set_guess(T) hands over the next frame's external pose."""
    import rgbd_loop
    from vslam_pose_estimation_framework_amd import host_tracker
    NONE, ODOMETRY = 1, 2

    class MotionLoop(rgbd_loop.RgbdTracker):
        def __init__(self):
            super().__init__(api, cfg, params)
            self.guess, self.guess_prev = _eye34(), _eye34()
            self.dr_count, self.moved = 0, False

        def set_guess(self, T):
            self.guess = np.array(T, np.float64).reshape(3, 4).copy()

        def process(self, left, depth):
            self.moved = False
            if model == NONE:
                self.prior = _eye34()
            elif model == ODOMETRY:
                if self.frames:          # _context->currentFrame(); float64 in the order of the device function: inverse, then product
                    self.prior = np.array(host_tracker._mul(host_tracker._inverse(list(self.guess.reshape(12))), list(self.guess_prev.reshape(12)))).reshape(3, 4)
                self.guess_prev = self.guess.copy()
            return super().process(left, depth)

        def accept(self, cur, prev):
            before = self.info.get("fallback", 0)
            super().accept(cur, prev)
            self.moved = self.info.get("fallback", 0) == before

        def fallback(self, cur, prev):          # :551-566
            if model != ODOMETRY:
                return super().fallback(cur, prev)
            cur.set_pose(rgbd_loop._mul(prev.c2w, rgbd_loop._inv(self.prior)))      # :555-559, the prior kept
            self.info["fallback"] = 1

        def register_recursive(self, cur, prev, left, depth, recursion):
            if model != ODOMETRY:
                return super().register_recursive(cur, prev, left, depth, recursion)
            c = self.cfg
            rel = rgbd_loop._div(float(self.n_tracked_landmarks), float(self.n_lm_prev))
            if self.n_tracked_landmarks == 0 or rel < 0.1:
                self.fallback(cur, prev)            # :323-328 the guess, :333-336 _fallbackEstimate: the same pose
                return
            r = self.align(cur, True)
            if r["n_inliers"] > c.minimum_number_of_landmarks_to_track:
                self.accept(cur, prev)
            elif recursion < 2:
                if self.win < c.maximum_projection_tracking_distance_pixels:
                    self.win += 1
                self.initialize(left, depth, first=False); self.track(cur, prev, False); self.register_recursive(cur, prev, left, depth, recursion + 1)
            else:
                self.fallback(cur, prev)            # :408-411

        def compute(self, cur):                 # called right behind the status switch: where the frame closes
            self.dr_count = 0 if self.moved else self.dr_count + 1
            if limit > 0 and self.dr_count >= limit and self.status == rgbd_loop.TRACKING:
                self.status = rgbd_loop.LOCALIZING
            return super().compute(cur)

    return MotionLoop()


def rgbd_frames(oracle, scene, n, blank=(), unit_m=2e-3):
    """[(image, depth)] of frames 0 .. n-1; positions in `blank` are a black image over its true depth (a covered lens)."""
    out = []
    for k in range(n):
        L, _ = oracle.render(scene, k)
        if k in blank:
            L = np.zeros_like(L)
        out.append((L, oracle.render_depth(scene, k, unit_m)))
    return out
