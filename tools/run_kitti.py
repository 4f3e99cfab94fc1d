#!/usr/bin/env python3
"""Run the MI355X front end on a KITTI odometry folder and write the trajectory (the I/O formats
either side of the hot path; executables/test_stereo_frontend.cpp:106-111,256-312 of the reference is the template).

    python tools/run_kitti.py <sequence dir with image_0/ image_1/ calib.txt [times.txt]> [--out traj.txt]
                              [--format kitti|tum] [--gt poses.txt] [--max-frames N] [--config kitti|euroc]
                              [--chunks B [--overlap 6]]   frame-sharded mode: B chunks side by side (approximate at the seams)
    python tools/run_kitti.py <EuRoC dir with mav0/cam0 mav0/cam1> --format tum --out traj.txt   (ground truth found in mav0/)
    python tools/run_kitti.py <EuRoC dir> --rectify --format tum --out traj.txt   raw images: rectified on the GPU from mav0/cam{0,1}/sensor.yaml
    python tools/run_kitti.py <sequence dir> --equalize   (or -eh, the reference's spelling) cv::equalizeHist on every image, on the GPU,
                              behind --rectify and ahead of the detector: dim, low-contrast sequences; also with --chunks, --map, --observations
    python tools/run_kitti.py <sequence dir> --clahe [CLIP] [--clahe-tiles X,Y]   cv::CLAHE on every image, on the GPU, in the place of --equalize
                              (not together with it; clip limit 40.0 and 8,8 tiles by default): unevenly lit sequences; also with --rectify,
                              --color, --chunks, --map, --observations
    python tools/run_kitti.py <sequence dir with image_2/ image_3/> --color   the odometry benchmark's colour cameras with their own calibration
                              (P2 / P3 of calib.txt); the RGB frames are converted to grey on the GPU; also with --chunks, --equalize, --map, --observations
    python tools/run_kitti.py <sequence dir> --map map.ply   the landmark map as well (binary PLY: x y z id first_frame last_frame updates)
    python tools/run_kitti.py <sequence dir> --observations bundle.npz   trajectory + landmark map + which landmark was seen in which
                              frame at which pixels, in one file (io_formats.read_bundle); implies the map; also with --chunks
    python tools/run_kitti.py <sequence dir with image_2/ image_3/> --color --map map.ply --map-color   a coloured cloud: red green blue per
                              landmark (its left keypoint's pixel at the last update, sampled on the GPU); map_rgb in the --observations bundle
    python tools/run_kitti.py <sequence dir> --motion-model odometry --odometry poses.txt [--dead-reckoning-limit N]   the reference's
                              CAMERA_ODOMETRY model: every frame starts from the motion an external pose source reports (a KITTI pose file, line k
                              for frame k, or a TUM trajectory associated by time stamp; camera frame) and dead-reckons on it where the images
                              fail, in the place of a broken track; N > 0 localizes again after N such frames in a row.  --motion-model none
                              starts every frame from identity.  Also with --chunks: every chunk gets its own frames' poses
    python tools/run_kitti.py <sequence dir> --mask LEFT.png[,RIGHT.png] [--mask-margin N] [--frame-masks DIR]   detection masks (8-bit PNGs at
                              the processed size, the rectified one under --rectify; zero = no keypoints there, N = 0 .. 64 widens every
                              masked region by N pixels): --mask for the whole run (the bonnet, overlays, vignetted corners), --frame-masks
                              a folder that mirrors the two image folders file name for file name (moving objects from a segmentation
                              network; a missing file: no mask for that frame).  Also with --chunks (every chunk its own frame's mask),
                              --rectify, --color, --equalize / --clahe, --map, --observations
    python tools/run_kitti.py <sequence dir> --rectify --mask-invalid [N]   with --rectify: no keypoints on rectified pixels whose source lies partly
                              outside the raw image (the seam between picture and black fill); the masks of both sides are computed from
                              the rectification maps on the GPU (vslam_set_rectification_mask), N = 0 .. 64 widens them.  Also with --chunks,
                              --mask, --frame-masks, --map, --observations

The sequence runs in exact mode (one stream, whole sequence, bit-for-bit the reference port's arithmetic); images are
uploaded frame by frame through vslam_process_host.  With --gt (KITTI 3x4 rows) the ATE-RMSE after rigid alignment is
printed, as trajectory_analyzer.cpp:212-284 computes it."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from vslam_pose_estimation_framework_amd import color as color_mod, downscale as downscale_mod, evaluation, hip, io_formats, smooth as smooth_mod  # noqa: E402


MAP_ENTRIES_PER_FRAME = 200     # map capacity per stream and processed frame (a KITTI frame creates ~30-60 landmarks)


def run_chunked(api, cfg, seq, n, n_chunks, overlap, device, log, rect=None, want_map=False, want_obs=False, equalize=False, color=False, clahe=None, clahe_tiles=(8, 8),
                map_color=False, motion_model=0, dead_reckoning_limit=0, guesses=None, masks=None, mask_invalid=None, downscale=None, smooth=None):
    """Frame-sharded mode (bench.py's headline mode) on a recorded sequence: `n_chunks` contiguous chunks, each
    started `overlap` frames early, run side by side as the streams of one context; the chunk trajectories are chained at the seams
    (sharding.assemble_trajectory).  Approximate at the seams — DESIGN.md section 9 has the accuracy study."""
    from vslam_pose_estimation_framework_amd import sharding
    plan, _ = sharding.plan_chunks(n, n_chunks, overlap)
    steps = max(e - s for (s, f, e) in plan)
    cfg.max_history_frames = steps + 2
    api.create(cfg, device, len(plan))
    if rect is not None:
        api.set_rectification(rect)
    if downscale is not None:
        api.set_downscale(*downscale)
    if mask_invalid is not None:
        api.set_rectification_mask(True, mask_invalid)
    if smooth is not None:
        api.set_smoothing(*smooth)
    if equalize:
        api.set_equalization(True)
    if clahe is not None:
        api.set_clahe(True, clahe, clahe_tiles)
    if color:
        api.set_color_input(color_mod.RGB8)
    if want_map:
        api.enable_map(MAP_ENTRIES_PER_FRAME * steps)
    if map_color:
        api.enable_map_colors(True)
    if want_obs:
        api.enable_observations(steps * int(cfg.max_points))      # a frame logs at most max_points entries: the log cannot overflow
    api.set_motion_model(motion_model, dead_reckoning_limit)
    if masks is not None:
        masks.set_static(api)
    rows, cols = downscale[1:] if downscale is not None else (rect.raw_rows, rect.raw_cols) if rect is not None else (int(cfg.rows), int(cfg.cols))
    Lb = np.zeros((len(plan), rows, cols) + ((3,) if color else ()), np.uint8)
    Rb = np.zeros_like(Lb)
    live = [True] * len(plan)
    for k in range(steps):
        for c, (st, fi, en) in enumerate(plan):
            if st + k < en:
                Lb[c], Rb[c] = seq.pair(st + k)
            elif live[c]:
                api.set_stream_active(c, False)
                live[c] = False
        if guesses is not None:      # every chunk its own frame's pose (a chunk that has ended is switched off: its entry is not read)
            api.set_pose_guesses(np.stack([guesses[min(st + k, en - 1)] for (st, fi, en) in plan]))
        if masks is not None:        # every chunk its own frame's mask (a chunk that has ended is switched off: its mask is not read)
            masks.set_frame(api, [st + k if st + k < en else None for (st, fi, en) in plan])
        api.process_host(Lb, Rb)
        if k % 20 == 19 or k == steps - 1:
            log("step %5d of %d (%d chunks side by side)" % (k + 1, steps, sum(live)))
    api.synchronize()
    flags = 0
    for c in range(len(plan)):
        flags |= api.frame_info(c).error_flags
    chunks = [api.poses(c, 0, en - st) for c, (st, fi, en) in enumerate(plan)]
    maps = [api.map(c) for c in range(len(plan))] if want_map else None
    if map_color:
        for c, m in enumerate(maps):
            m["rgb"] = api.map_colors(c)
    lm_map = sharding.assemble_map(maps, chunks, plan) if want_map else None
    obs = sharding.assemble_observations(maps, [api.observations(c) for c in range(len(plan))], plan) if want_obs else None
    return np.asarray(sharding.assemble_trajectory(chunks, plan)).reshape(n, 12), flags, lm_map, obs


def run(seq_dir, out_path=None, fmt="kitti", gt_path=None, max_frames=0, which="kitti", device=0, log=print, layout="kitti", asl_gt=None,
        chunks=0, overlap=6, rectify=False, map_path=None, obs_path=None, equalize=False, color=False, clahe=None, clahe_tiles=(8, 8), map_color=False,
        motion_model="constant-velocity", odometry=None, dead_reckoning_limit=0, mask=None, mask_margin=0, frame_masks=None, mask_invalid=None,
        downscale=1, smooth=None):
    smooth = smooth_mod.argument(smooth, SystemExit)
    check_mask_args(mask, mask_margin, frame_masks, SystemExit, mask_invalid, rectify)
    check_downscale_arg(downscale, SystemExit)
    check_motion_args(motion_model, odometry, dead_reckoning_limit, SystemExit)
    if map_color and not (color and (map_path or obs_path)):
        raise SystemExit("--map-color needs --color and --map or --observations")
    euroc = layout == "euroc" or os.path.isdir(os.path.join(seq_dir, "mav0"))
    if color and euroc:
        raise SystemExit("--color: an ASL / EuRoC folder holds grey images (it takes a KITTI odometry folder with image_2/ and image_3/)")
    if color and not os.path.isdir(os.path.join(seq_dir, "image_2")):
        raise SystemExit("--color: no image_2/ and image_3/ under %s" % seq_dir)
    if rectify and not euroc:
        raise SystemExit("--rectify: a KITTI odometry folder is already rectified (it takes raw EuRoC / ASL folders with sensor.yaml)")
    seq = io_formats.EurocSequence(seq_dir) if euroc else io_formats.KittiSequence(seq_dir, color=color)
    n = len(seq) if max_frames <= 0 else min(len(seq), max_frames)
    if n == 0:
        raise SystemExit("no images under %s" % seq_dir)
    left, right = seq.pair(0)
    api = hip.load()
    cfg = api.default_config("euroc" if euroc and which == "kitti" else which)
    rect = None
    ds = None                          # (factor, full rows, full cols) under --downscale
    if downscale != 1:
        try:
            downscale_mod.output_size(left.shape[0], left.shape[1], downscale)
        except ValueError as e:
            raise SystemExit("--downscale: %s" % e)
        ds = (int(downscale), int(left.shape[0]), int(left.shape[1]))
    if rectify:
        from vslam_pose_estimation_framework_amd import rectify as rectify_mod
        raw = seq.raw_calibration()
        if raw is None:
            raise SystemExit("--rectify: no mav0/cam0/sensor.yaml and mav0/cam1/sensor.yaml under %s" % seq_dir)
        if (raw[0].rows, raw[0].cols) != left.shape[:2]:
            raise SystemExit("--rectify: sensor.yaml says %dx%d, the images are %dx%d" % (raw[0].rows, raw[0].cols, left.shape[0], left.shape[1]))
        if ds is not None:             # the raw cameras of the reduced images: the maps are built over them
            raw = tuple(rectify_mod.CameraModel(downscale_mod.scale_intrinsics(c.K, ds[0]), c.dist, c.rows // ds[0], c.cols // ds[0]) for c in raw[:2]) + tuple(raw[2:])
        rect = rectify_mod.rectification(*raw)
        rectify_mod.apply_to_config(cfg, rect)
        log("rectifying on the GPU: raw %dx%d -> %dx%d, f %.3f px, baseline %.4f m" % (
            rect.raw_rows, rect.raw_cols, rect.rows, rect.cols, rect.P1[0, 0], -rect.P2[0, 3] / rect.P1[0, 0]))
        if mask_invalid is not None:
            log("validity masks from the rectification maps on the GPU: %.1f / %.1f %% of the left / right pixels have every tap inside the raw image, margin %d px" % (
                100.0 * float(rectify_mod.validity(rect.map_xy_left, rect.map_a_left, rect.raw_rows, rect.raw_cols).mean()),
                100.0 * float(rectify_mod.validity(rect.map_xy_right, rect.map_a_right, rect.raw_rows, rect.raw_cols).mean()), mask_invalid))
    elif euroc:
        cal = seq.calibration()       # a rectified export may carry its P0 / P1; otherwise the EuRoC values of the default config
        if cal is not None:
            io_formats.apply_calib(cfg, cal[0], cal[1], left.shape[0], left.shape[1])
        else:
            cfg.rows, cfg.cols = int(left.shape[0]), int(left.shape[1])
            try:
                raw = seq.raw_calibration()
            except (ValueError, KeyError):
                raw = None
            if raw is not None and (np.any(raw[0].dist != 0) or np.any(raw[1].dist != 0)):
                log("note: sensor.yaml describes distorted raw cameras and there is no calib.txt; --rectify rectifies them on the GPU")
    else:
        io_formats.apply_calib(cfg, seq.K, seq.baseline, left.shape[0], left.shape[1])
    if ds is not None:
        if rect is None:
            downscale_mod.apply_to_config(cfg, ds[0])
        log("downscaling on the GPU by %d: %dx%d -> %dx%d, ahead of %s; calibration scaled (f %.3f px, c %.3f %.3f)" % (
            ds[0], ds[1], ds[2], ds[1] // ds[0], ds[2] // ds[0], "the rectification" if rect is not None else "the detector", cfg.K[0], cfg.K[2], cfg.K[5]))
    if smooth is not None:
        log("smoothing on the GPU (%s %d x %d on every image, ahead of %s)" % (
            "Gaussian" if smooth[0] == smooth_mod.GAUSSIAN else "median", smooth[1], smooth[1], "the equalisation" if equalize else "CLAHE" if clahe is not None else "the detector"))
    if color:
        log("colour cameras (image_2 / image_3, calibration P2 / P3): RGB -> grey on the GPU, ahead of %s" % ("the equalisation" if equalize else "CLAHE" if clahe is not None else "the detector"))
    if equalize:
        log("equalising histograms on the GPU (cv::equalizeHist on every image%s)" % (", behind the rectification" if rect is not None else ""))
    if clahe is not None:
        log("CLAHE on the GPU (cv::CLAHE, clip limit %g, %d x %d tiles, on every image%s)" % (clahe, clahe_tiles[0], clahe_tiles[1], ", behind the rectification" if rect is not None else ""))
    guesses = None
    if odometry:
        guesses, own = io_formats.read_pose_guesses(odometry, seq.times[:n])
        log("motion model camera odometry: %d of %d frames have a pose of their own in %s%s" % (
            int(own.sum()), n, odometry, ", dead-reckoning limit %d" % dead_reckoning_limit if dead_reckoning_limit else ""))
    model = MOTION_MODELS[motion_model]
    masks = DetectionMasks(seq, int(cfg.rows), int(cfg.cols), mask, mask_margin, frame_masks, log) if (mask or frame_masks) else None
    t0 = time.perf_counter()
    flags = 0
    tracking = 0
    dead_reckoned = 0
    want_map = bool(map_path or obs_path)        # the log's ids are the map's
    obs = None
    if chunks > 1:
        poses, flags, lm_map, obs = run_chunked(api, cfg, seq, n, chunks, overlap, device, log, rect, want_map=want_map, want_obs=bool(obs_path),
                                                equalize=equalize, color=color, clahe=clahe, clahe_tiles=clahe_tiles, map_color=map_color,
                                                motion_model=model, dead_reckoning_limit=dead_reckoning_limit, guesses=guesses, masks=masks, mask_invalid=mask_invalid, downscale=ds, smooth=smooth)
        tracking = None
        dead_reckoned = None
    else:
        cfg.max_history_frames = 512
        api.create(cfg, device, 1)
        if rect is not None:
            api.set_rectification(rect)
        if ds is not None:
            api.set_downscale(*ds)
        if mask_invalid is not None:
            api.set_rectification_mask(True, mask_invalid)
        if smooth is not None:
            api.set_smoothing(*smooth)
        if equalize:
            api.set_equalization(True)
        if clahe is not None:
            api.set_clahe(True, clahe, clahe_tiles)
        if color:
            api.set_color_input(color_mod.RGB8)
        if want_map:
            api.enable_map(MAP_ENTRIES_PER_FRAME * n)
        if map_color:
            api.enable_map_colors(True)
        if obs_path:
            api.enable_observations(n * int(cfg.max_points))      # a frame logs at most max_points entries: the log cannot overflow
        api.set_motion_model(model, dead_reckoning_limit)
        if masks is not None:
            masks.set_static(api)
        for k in range(n):
            if k:
                left, right = seq.pair(k)
            if guesses is not None and own[k]:
                api.set_pose_guess(guesses[k], 0)
            if masks is not None:
                masks.set_frame(api, [k])
            api.process_host(left, right)
            fi = api.frame_info(0)
            flags |= fi.error_flags
            tracking += int(fi.status == 1)
            dead_reckoned += int(model == 2 and fi.fallback == 1)
            if k % 100 == 99 or k == n - 1:
                log("frame %6d  status %s  points %5d  tracked %5d  inliers %5d" % (
                    k, "tracking" if fi.status == 1 else "localizing", fi.n_points, fi.n_tracked, fi.n_inliers))
        poses = api.poses(0, 0, n)
        lm_map = api.map(0) if want_map else None
        if map_color:
            lm_map["rgb"] = api.map_colors(0)
        obs = api.observations(0) if obs_path else None
    dt = time.perf_counter() - t0
    K, baseline_h = np.array(cfg.K, np.float64).reshape(3, 3), np.array(cfg.baseline_h, np.float64)
    api.destroy()
    log("%d frames in %.2f s (%.1f frames/s incl. PNG decode and upload), error flags %d" % (n, dt, n / dt, flags))
    if out_path:
        if fmt == "tum":
            io_formats.write_trajectory_tum(out_path, poses, seq.times[:n])
        else:
            io_formats.write_trajectory_kitti(out_path, poses)
        log("trajectory (%s) -> %s" % (fmt, out_path))
    result = {"frames": n, "seconds": dt, "error_flags": flags, "poses": poses, "tracking_frames": tracking}     # tracking_frames: exact mode only
    if model == 2:
        result["dead_reckoned_frames"] = dead_reckoned     # frames whose pose was taken from the odometry (exact mode only)
        if dead_reckoned:
            log("%d frames took their pose from the odometry" % dead_reckoned)
    if map_path:
        if flags & 8:
            log("warning: the landmark map ran out of capacity (error flag 8): landmarks created after that are missing")
        io_formats.write_ply(map_path, lm_map["xyz"], lm_map.get("rgb"), id=lm_map["id"], first_frame=lm_map["first_frame"], last_frame=lm_map["last_frame"],
                             updates=lm_map["updates"])
        log("landmark map: %d landmarks -> %s" % (len(lm_map["id"]), map_path))
        result["map"] = lm_map
    if want_map and not map_path:
        if flags & 8:
            log("warning: the landmark map ran out of capacity (error flag 8): landmarks created after that are missing")
        result["map"] = lm_map
    if obs_path:
        io_formats.write_bundle(obs_path, K, baseline_h, poses, lm_map, obs)
        res, valid = evaluation.reprojection_residuals(K, baseline_h, poses, lm_map["xyz"], obs["id"], obs["frame"], obs["kp"])
        norm = np.linalg.norm(res[valid], axis=1)
        empty = n - len(np.unique(obs["frame"]))
        result["observations"] = obs
        result["reprojection"] = {"observations": int(len(obs["id"])), "landmarks": int(len(lm_map["id"])), "valid": int(valid.sum()),
                                  "median_px": float(np.median(norm)) if len(norm) else None,
                                  "p90_px": float(np.percentile(norm, 90)) if len(norm) else None, "frames_without_observation": int(empty)}
        log("observations: %d of %d landmarks -> %s%s" % (len(obs["id"]), len(lm_map["id"]), obs_path,
                                                        "  (%d dropped with warm-up duplicates)" % obs["dropped"] if "dropped" in obs else ""))
        log("frames without any observation: %d of %d" % (empty, n))
        if len(norm):
            log("reprojection residual norm (xL, y, xR) against the map: median %.3f px, 90th percentile %.3f px over %d observations" % (
                result["reprojection"]["median_px"], result["reprojection"]["p90_px"], len(norm)))
    if gt_path:
        gt = io_formats.read_trajectory_kitti(gt_path)[:n]
        result["ate_rmse_aligned"] = evaluation.ate_rmse(poses[:len(gt)], gt)
        log("ATE-RMSE after rigid alignment: %.4f m over %d frames" % (result["ate_rmse_aligned"], len(gt)))
    asl = asl_gt or (seq.ground_truth_path if euroc else None)
    if asl and out_path and fmt == "tum":
        r = evaluation.trajectory_analyzer(out_path, asl)     # executables/trajectory_analyzer.cpp: -tum <out> -asl <ground truth>
        result["trajectory_analyzer"] = {k: r[k] for k in ("correspondences", "raw_rmse", "optimal_rmse")}
        log("trajectory_analyzer: %d interpolated positions, raw RMSE %.4f m, optimal RMSE %.4f m" % (r["correspondences"], r["raw_rmse"], r["optimal_rmse"]))
    return result


class DetectionMasks(object):
    """--mask / --mask-margin / --frame-masks: the static masks (read once) and each frame's masks, looked up under the folder that
    mirrors the sequence's two image folders."""

    def __init__(self, seq, rows, cols, mask, margin, frame_dir, log=print):
        self.seq, self.rows, self.cols, self.margin, self.frame_dir = seq, rows, cols, int(margin), frame_dir
        self.static = None
        if mask:
            paths = mask.split(",")
            self.static = [self._read(p) for p in paths] + [None] * (2 - len(paths))
            log("detection mask: %s, margin %d px" % (" / ".join(paths), self.margin))
        if frame_dir:
            log("per-frame detection masks from %s, margin %d px" % (frame_dir, self.margin))

    def _read(self, path):
        m = io_formats.read_png_gray8(path)
        if m.shape != (self.rows, self.cols):
            raise SystemExit("mask %s is %dx%d, the detector works on %dx%d images" % (path, m.shape[0], m.shape[1], self.rows, self.cols))
        return m

    def relative(self, k):
        """Where frame k's two images lie under the sequence folder, so where its masks lie under --frame-masks."""
        s = self.seq
        if isinstance(s, io_formats.EurocSequence):
            return os.path.join("cam0", "data", s.left[k]), os.path.join("cam1", "data", s.right[k])
        return tuple(os.path.join(d, s.names[k]) for d in s.dirs)

    def set_static(self, api):
        if self.static is not None:
            api.set_detection_mask(self.static[0], self.static[1], self.margin)

    def set_frame(self, api, frames):
        """frames: the frame index of every stream's next frame (None: the stream has ended).  A side for which no stream has a file gets
        no mask; a stream without a file among streams with one gets an all-keep mask."""
        if not self.frame_dir:
            return
        sides = [None, None]
        for c, k in enumerate(frames):
            if k is None:
                continue
            for d, rel in enumerate(self.relative(k)):
                path = os.path.join(self.frame_dir, rel)
                if os.path.exists(path):
                    if sides[d] is None:
                        sides[d] = np.full((len(frames), self.rows, self.cols), 255, np.uint8)
                    sides[d][c] = self._read(path)
        if sides[0] is not None or sides[1] is not None:
            api.set_frame_masks(sides[0], sides[1], self.margin)


def check_mask_args(mask, mask_margin, frame_masks, error, mask_invalid=None, rectify=True):
    """What --mask, --mask-margin and --frame-masks allow together (tools/run_rgbd.py takes the first two)."""
    if mask_margin < 0 or mask_margin > 64:
        raise error("--mask-margin: a whole number of pixels in 0 .. 64")
    if mask_margin and not (mask or frame_masks):
        raise error("--mask-margin needs --mask or --frame-masks")
    if mask is not None:
        paths = mask.split(",")
        if len(paths) > 2 or not all(paths):
            raise error("--mask LEFT.png[,RIGHT.png]")
        for p in paths:
            if not os.path.isfile(p):
                raise error("--mask: no such file: %s" % p)
    if frame_masks is not None and not os.path.isdir(frame_masks):
        raise error("--frame-masks: no such folder: %s" % frame_masks)
    if mask_invalid is not None and not rectify:
        raise error("--mask-invalid needs --rectify: the validity masks come from the rectification maps")
    if mask_invalid is not None and (mask_invalid < 0 or mask_invalid > 64):
        raise error("--mask-invalid: a whole number of pixels in 0 .. 64")


MOTION_MODELS = {"constant-velocity": 0, "none": 1, "odometry": 2}     # enum vslam_motion_model


def check_downscale_arg(downscale, error):
    if isinstance(downscale, bool) or not isinstance(downscale, int) or downscale < 1 or downscale > 4:
        raise error("--downscale: a whole factor in 1 .. 4 (1: off)")


def check_motion_args(motion_model, odometry, dead_reckoning_limit, error):
    """What --motion-model, --odometry and --dead-reckoning-limit allow together (tools/run_rgbd.py takes the same flags)."""
    if motion_model not in MOTION_MODELS:
        raise error("--motion-model: one of %s" % ", ".join(sorted(MOTION_MODELS)))
    if motion_model == "odometry" and not odometry:
        raise error("--motion-model odometry needs --odometry FILE (a KITTI pose file or a TUM trajectory)")
    if odometry and motion_model != "odometry":
        raise error("--odometry is read under --motion-model odometry only")
    if dead_reckoning_limit < 0 or (dead_reckoning_limit and motion_model != "odometry"):
        raise error("--dead-reckoning-limit N >= 0 needs --motion-model odometry")


def _tiles(text):
    """--clahe-tiles X,Y -> (X, Y)"""
    try:
        x, y = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected X,Y (two integers)")
    return x, y


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("sequence")
    ap.add_argument("--out", default=None)
    ap.add_argument("--format", choices=("kitti", "tum"), default="kitti")
    ap.add_argument("--gt", default=None)
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--config", choices=("kitti", "euroc"), default="kitti")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--chunks", type=int, default=0, help="frame-sharded mode: cut the sequence into this many chunks and run them side by side (0 / 1: exact mode, one stream)")
    ap.add_argument("--overlap", type=int, default=6, help="warm-up frames per chunk in frame-sharded mode")
    ap.add_argument("--layout", choices=("kitti", "euroc"), default="kitti", help="folder layout (a folder with mav0/ is taken as EuRoC / ASL)")
    ap.add_argument("--asl-gt", default=None, help="ASL ground-truth csv for the trajectory_analyzer step (needs --format tum --out)")
    ap.add_argument("--rectify", action="store_true", help="EuRoC / ASL folder of raw images: undistort and rectify them on the GPU from mav0/cam{0,1}/sensor.yaml")
    ap.add_argument("--map", default=None, help="write the landmark map (every landmark of the run, world frame) to this binary PLY file")
    ap.add_argument("--observations", default=None, help="write trajectory, landmark map and the landmark observation log (id, frame, xL yL xR yR) "
                    "to this .npz bundle (io_formats.read_bundle); implies the map")
    ap.add_argument("--equalize", "-eh", action="store_true", help="equalise every image's histogram on the GPU ahead of the detector "
                    "(the reference's -equalize-histogram / -eh): dim or low-contrast sequences")
    ap.add_argument("--clahe", nargs="?", type=float, const=40.0, default=None, metavar="CLIP", help="contrast-limited adaptive histogram equalisation "
                    "(cv::CLAHE) of every image on the GPU ahead of the detector, clip limit CLIP (40.0 without a value): dim or unevenly lit "
                    "sequences; not together with --equalize")
    ap.add_argument("--clahe-tiles", type=_tiles, default=(8, 8), metavar="X,Y", help="the tile grid of --clahe (8,8)")
    ap.add_argument("--color", action="store_true", help="a KITTI odometry folder's colour cameras (image_2 / image_3 with the calibration of P2 / P3); "
                    "the frames are converted to grey on the GPU")
    ap.add_argument("--map-color", action="store_true", help="with --color and --map / --observations: the colour of every landmark (its left keypoint's "
                    "pixel at the last update, sampled on the GPU) as red green blue in the PLY and map_rgb in the bundle")
    ap.add_argument("--motion-model", choices=sorted(MOTION_MODELS), default="constant-velocity", help="the prior every frame starts with: the last "
                    "refined motion (the default), identity (none), or the motion an external pose source reports (odometry, with --odometry)")
    ap.add_argument("--odometry", default=None, metavar="FILE", help="--motion-model odometry: camera_left_to_world per frame, a KITTI pose file (line k "
                    "for frame k) or a TUM trajectory (associated by time stamp)")
    ap.add_argument("--dead-reckoning-limit", type=int, default=0, metavar="N", help="--motion-model odometry: localize again after N frames in a row "
                    "whose pose was taken from the odometry (0: never)")
    ap.add_argument("--mask", default=None, metavar="LEFT.png[,RIGHT.png]", help="detection masks for the whole run: 8-bit PNGs at the processed size, "
                    "zero = no keypoints on that pixel (the bonnet, overlays, vignetted corners); one file masks the left image only")
    ap.add_argument("--mask-margin", type=int, default=0, metavar="N", help="widen every masked region of --mask / --frame-masks by N pixels (0 .. 64)")
    ap.add_argument("--mask-invalid", nargs="?", type=int, const=0, default=None, metavar="N", help="with --rectify: no keypoints on pixels whose source lies "
                    "partly outside the raw image (the seam between picture and black fill), computed from the maps on the GPU, both sides; N widens it (0 .. 64)")
    ap.add_argument("--smooth", default=None, metavar="MODE[:K]", help="smooth every grey image on the GPU ahead of the equalisation and the detector: "
                    "gaussian[:3|5|7] (default gaussian:5) or median[:3|5] (default median:3)")
    ap.add_argument("--downscale", type=int, default=1, metavar="N", help="reduce every image by the whole factor N (2, 3 or 4) on the GPU ahead of everything but "
                    "the colour conversion: rounded block averages; the folder's calibration is scaled and the tracker runs at the reduced size "
                    "(masks are given at that size); combines with every other switch")
    ap.add_argument("--frame-masks", default=None, metavar="DIR", help="per-frame detection masks: a folder that mirrors the sequence's two image folders "
                    "file name for file name; a missing file means no mask for that frame")
    a = ap.parse_args(argv)
    try:
        check_mask_args(a.mask, a.mask_margin, a.frame_masks, ValueError, a.mask_invalid, a.rectify)
        check_downscale_arg(a.downscale, ValueError)
        smooth_mod.argument(a.smooth, ValueError)
        check_motion_args(a.motion_model, a.odometry, a.dead_reckoning_limit, ValueError)
    except ValueError as e:
        ap.error(str(e))
    if a.clahe is not None and a.equalize:
        ap.error("--clahe and --equalize exclude each other: one equalisation ahead of the detector")
    if a.map_color and not (a.color and (a.map or a.observations)):
        ap.error("--map-color needs --color and --map or --observations")
    return a


def main(argv=None):
    a = parse_args(argv)
    run(a.sequence, a.out, a.format, a.gt, a.max_frames, a.config, a.device, layout=a.layout, asl_gt=a.asl_gt, chunks=a.chunks, overlap=a.overlap,
        rectify=a.rectify, map_path=a.map, obs_path=a.observations, equalize=a.equalize, color=a.color, clahe=a.clahe, clahe_tiles=a.clahe_tiles,
        map_color=a.map_color, motion_model=a.motion_model, odometry=a.odometry, dead_reckoning_limit=a.dead_reckoning_limit,
        mask=a.mask, mask_margin=a.mask_margin, frame_masks=a.frame_masks, mask_invalid=a.mask_invalid, downscale=a.downscale, smooth=a.smooth)


if __name__ == "__main__":
    main()
