#!/usr/bin/env python3
"""Run the MI355X RGB-D front end (vslam_rgbd_*: PoseTracker3D with DepthFramePointGenerator + UVDAligner) on a TUM RGB-D folder — the layout
the TUM benchmark and ICL-NUIM ship (`rgb.txt`, `depth.txt`, `rgb/`, `depth/`, optional `groundtruth.txt`) — and write the trajectory in the
reference's TUM format (WorldMap::writeTrajectoryTUM, world_map.cpp:222-258).

    python tools/run_rgbd.py <folder> [--config icl|tum|xtion] [--intrinsics freiburg1|freiburg2|freiburg3|icl|fx,fy,cx,cy]
                             [--depth-unit 0.0002] [--out traj.txt] [--max-frames N] [--descriptor ORB|BRIEF] [--detector FAST|ORB]
                             [--map map.ply] [--observations bundle.npz] [--undistort [k1,k2,p1,p2[,k3]]] [--equalize | -eh] [--color [--map-color]]
                             [--clahe [CLIP]] [--clahe-tiles X,Y] [--motion-model constant-velocity|none|odometry] [--odometry FILE]
                             [--dead-reckoning-limit N] [--bilateral [SIGMA_COLOR,SIGMA_SPACE]] [--mask MASK.png] [--frame-masks DIR] [--mask-margin N] [--mask-invalid [N]]

--config picks the values of configurations/configuration_{icl,tum,xtion}.yaml the path reads (table below: detector grid and thresholds,
tracking windows and descriptor distances, depth limits, bin size, triangulation of points without depth, landmark / aligner settings); the
camera comes from --intrinsics (the depth image is registered to the colour image in these data sets: one camera matrix, identity offset).
Colour images are converted like cv::imread(IMREAD_GRAYSCALE).  With a groundtruth.txt in the folder (or --gt) and --out, the reference's
trajectory_analyzer (executables/trajectory_analyzer.cpp, restated in evaluation.py) reports the RMSE after its alignment.
--map writes every landmark of the run (world frame) as a binary PLY (x y z id first_frame last_frame updates); --observations writes
trajectory + landmark map + which landmark was seen in which frame at which pixel and depth into one .npz (io_formats.read_bundle_rgbd;
implies the map) and reports the residuals of the log against map and trajectory.  Both need the device-resident loop.
--detector ORB runs the reference's OrbDetector (cv::ORB as detector: float keypoints of up to eight pyramid levels) on the device-resident
loop as well, so it combines with every flag below but the masks: --mask, --frame-masks and --mask-invalid are refused with the library's
message (cv::ORB::detect resizes its mask per pyramid level; the library has no restatement of that).
--undistort takes the folder's frames as RAW ones of a camera with radial-tangential lens distortion and undoes it on the GPU ahead of the
detector (vslam_rgbd_set_undistortion: image bilinear, depth nearest, one map for both — the depth images are registered to the colour
camera); without a value the coefficients are io_formats.TUM_DISTORTION[--intrinsics].  The output camera is --intrinsics' pinhole
camera at the raw size; trajectory, map and observations are then in undistorted coordinates.  Device-resident loop only.
--equalize (or -eh, the reference's spelling) equalises the intensity image's histogram on the GPU (cv::equalizeHist; the depth image is
untouched), behind --undistort and ahead of the detector: dim or low-contrast sequences.  Device-resident loop only.
--clahe [CLIP] runs cv::CLAHE (clip limit CLIP, 40.0 without a value; --clahe-tiles X,Y, 8,8 by default) on the intensity image in the place of
--equalize (not together with it): unevenly lit sequences.  Device-resident loop only.
--color hands the colour frames over as decoded and converts them to grey on the GPU (vslam_rgbd_set_color_input: the same integers as the
host conversion without the flag), ahead of --undistort and --equalize.  Device-resident loop only.
--map-color (with --color and --map / --observations) samples every landmark's colour on the GPU (vslam_rgbd_enable_map_colors: the pixel of
its point at the last update, through the --undistort map when that is on): red green blue in the PLY, map_rgb in the bundle.
--motion-model odometry --odometry FILE starts every frame from the motion an external pose source reports (the reference's CAMERA_ODOMETRY,
configuration_xtion.yaml's own model; FILE: a TUM trajectory associated by time stamp, or a KITTI pose file, in the camera's frame) and
dead-reckons on it where the images fail, in the place of a broken track; --dead-reckoning-limit N localizes again after N such frames in a
row (without it one failed frame means dead reckoning for good: DESIGN.md 6j).  --motion-model none starts every frame from identity.  Both
loops.
--bilateral [SIGMA_COLOR,SIGMA_SPACE] smooths every depth image with the reference's bilateral filter on the GPU ahead of the space map
(vslam_rgbd_set_bilateral: enable_bilateral_filtering, cv::bilateralFilter on the depth in metres; 2,2 without a value), behind --undistort:
noisy depth streams.  The intensity image is untouched, so it combines with --color, --equalize and --clahe.  Device-resident loop only.
--frame-masks DIR gives every frame a mask of its own (vslam_rgbd_set_frame_masks): a folder of 8-bit PNGs at the processed size named like
the frames' files under rgb/; a missing file means no mask for that frame.  --mask-margin applies to --mask and --frame-masks.
--mask-invalid [N] (with --undistort) keeps keypoints off the pixels whose source lies partly outside the raw frame, the seam between picture
and black fill (vslam_rgbd_set_undistortion_mask: computed from the maps on the GPU); N = 0 .. 64 widens it.  Both compose with --mask,
--map and --observations.  Device-resident loop only.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from vslam_pose_estimation_framework_amd import color as color_mod, downscale as downscale_mod, evaluation, hip, io_formats, smooth as smooth_mod  # noqa: E402
from vslam_pose_estimation_framework_amd.capi import DepthParams, RgbdTracker, VslamError  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from run_kitti import MOTION_MODELS, check_motion_args  # noqa: E402  (--motion-model / --odometry / --dead-reckoning-limit: one set of rules)

MAP_ENTRIES_PER_FRAME = 200     # map capacity per processed frame, as tools/run_kitti.py chooses it

# configurations/configuration_{icl,tum,xtion}.yaml: base_framepoint_generation / depth_framepoint_generation / tracking / landmark values
YAML = {
    "icl": dict(thr=(5, 100), max_change=1.0, grid=(2, 2), win=(5, 25), desc=(25, 50), depth=(2.5, 10.0, 0.001), bin=25, tri=0,
                lm_err=0.5, min_lm=10, tunnel=0.5, good=0.25, delta_move=(0.0, 0.0), kernel=5),
    "tum": dict(thr=(10, 100), max_change=0.5, grid=(1, 1), win=(10, 50), desc=(40, 40), depth=(2.5, 10.0, 0.1), bin=15, tri=1,
                lm_err=1.0, min_lm=5, tunnel=0.75, good=0.25, delta_move=(0.001, 0.01), kernel=10),
    "xtion": dict(thr=(10, 100), max_change=0.5, grid=(1, 1), win=(5, 10), desc=(25, 50), depth=(2.5, 8.0, 0.1), bin=10, tri=1,
                  lm_err=4.0, min_lm=25, tunnel=0.75, good=0.5, delta_move=(0.001, 0.01), kernel=10),
}


def configure(api, which, rows, cols, K, depth_unit, descriptor=1, detector=0, depth_scale=1.0):
    """vslam_config + vslam_depth_params with `which` configuration's values; depth_scale multiplies the three metric depth limits (the
    synthetic street scenes of the tests are larger than a room)."""
    y = YAML[which]
    cfg = api.default_config("kitti")
    cfg.rows, cfg.cols = int(rows), int(cols)
    for i in range(9):
        cfg.K[i] = float(np.asarray(K).reshape(9)[i])
    cfg.baseline_h[0] = -float(K[0][0]) * 0.1        # unused in this mode (one camera); vslam_create wants a valid stereo baseline
    cfg.det_rows, cfg.det_cols = y["grid"]
    cfg.detector_threshold_minimum, cfg.detector_threshold_maximum = y["thr"]
    cfg.detector_threshold_maximum_change = y["max_change"]; cfg.target_number_of_keypoints_tolerance = 0.1
    cfg.minimum_projection_tracking_distance_pixels, cfg.maximum_projection_tracking_distance_pixels = y["win"]
    cfg.minimum_descriptor_distance_tracking, cfg.maximum_descriptor_distance_tracking = y["desc"]
    cfg.maximum_reliable_depth_meters = y["depth"][0] * depth_scale; cfg.maximum_depth_meters = y["depth"][1] * depth_scale
    cfg.minimum_depth_meters = y["depth"][2]
    cfg.enable_keypoint_binning = 1; cfg.bin_size_pixels = y["bin"]
    cfg.minimum_track_length_for_landmark_creation = 2; cfg.minimum_number_of_landmarks_to_track = y["min_lm"]
    cfg.tunnel_vision_ratio = y["tunnel"]; cfg.good_tracking_ratio = y["good"]
    cfg.minimum_delta_angular_for_movement, cfg.minimum_delta_translational_for_movement = y["delta_move"]
    cfg.aligner_error_delta_for_convergence = 1e-5; cfg.aligner_maximum_error_kernel = y["kernel"]; cfg.aligner_damping = 0
    cfg.aligner_maximum_number_of_iterations = 1000; cfg.aligner_minimum_number_of_inliers = 0
    cfg.landmark_maximum_error_squared_meters = y["lm_err"]
    cfg.enable_landmark_recovery = 1
    cfg.descriptor_type = descriptor
    K = np.asarray(K, np.float64).reshape(3, 3)
    p = DepthParams.make(rows, cols, K, np.linalg.inv(K), np.linalg.inv(K), np.eye(4)[:3], depth_unit, y["depth"][2], y["depth"][1] * depth_scale,
                         y["tri"], 1, y["bin"], descriptor, detector)
    return cfg, p


def distortion_of(undistort, intrinsics):
    """--undistort's value -> the five coefficients (k1, k2, p1, p2, k3), or None without the flag.  "" (the flag alone): the table's
    coefficients of a named --intrinsics.  A string "k1,k2,p1,p2[,k3]" or a sequence of 4 or 5 numbers: those."""
    if undistort is None:
        return None
    if isinstance(undistort, str):
        if undistort.strip() == "":
            if intrinsics not in io_formats.TUM_DISTORTION:
                raise SystemExit("--undistort without coefficients needs a named --intrinsics (%s); give k1,k2,p1,p2[,k3]" % ", ".join(sorted(io_formats.TUM_DISTORTION)))
            return tuple(io_formats.TUM_DISTORTION[intrinsics])
        try:
            undistort = [float(v) for v in undistort.split(",")]
        except ValueError:
            raise SystemExit("--undistort: expected k1,k2,p1,p2[,k3], got %r" % (undistort,))
    d = [float(v) for v in undistort]
    if len(d) not in (4, 5):
        raise SystemExit("--undistort: 4 or 5 coefficients (k1,k2,p1,p2[,k3]), got %d" % len(d))
    return tuple(d + [0.0] * (5 - len(d)))


def run(folder, which="tum", intrinsics="freiburg1", depth_unit=io_formats.TUM_DEPTH_UNIT_M, out_path=None, max_frames=0, descriptor=1, detector=0,
        gt_path=None, device=0, depth_scale=1.0, log=print, map_path=None, obs_path=None, undistort=None, equalize=False, color=False, clahe=None, clahe_tiles=(8, 8),
        map_color=False, motion_model="constant-velocity", odometry=None, dead_reckoning_limit=0, bilateral=None, mask=None, mask_margin=0,
        frame_masks=None, mask_invalid=None, downscale=1, smooth=None):
    check_mask_args(mask, mask_margin, SystemExit, frame_masks, mask_invalid, undistort)
    smooth = smooth_mod.argument(smooth, SystemExit)
    if isinstance(downscale, bool) or not isinstance(downscale, int) or downscale < 1 or downscale > 4:
        raise SystemExit("--downscale: a whole factor in 1 .. 4 (1: off)")
    check_motion_args(motion_model, odometry, dead_reckoning_limit, SystemExit)
    if map_color and not (color and (map_path or obs_path)):
        raise SystemExit("--map-color needs --color and --map or --observations")
    seq = io_formats.TumRgbdSequence(folder)
    n = len(seq) if max_frames <= 0 else min(len(seq), max_frames)
    if n == 0:
        raise SystemExit("no associated rgb / depth pairs under %s" % folder)
    fx, fy, cx, cy = io_formats.TUM_INTRINSICS[intrinsics] if intrinsics in io_formats.TUM_INTRINSICS else [float(v) for v in intrinsics.split(",")]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    fmt = color_mod.GRAY8
    if color:
        gray, fmt, depth = seq.frame_color(0)        # `gray`: the intensity image as it is handed over, [rows, cols, 3 | 4] here
    else:
        gray, depth = seq.frame(0)
    api = hip.load()
    full_rows, full_cols = int(gray.shape[0]), int(gray.shape[1])
    rows, cols = full_rows, full_cols
    if downscale != 1:                           # the camera of the reduced frames: tracker, depth parameters and undistortion maps are built on it
        try:
            rows, cols = downscale_mod.output_size(full_rows, full_cols, downscale)
        except ValueError as e:
            raise SystemExit("--downscale: %s" % e)
        K = downscale_mod.scale_intrinsics(K, downscale)
    cfg, p = configure(api, which, rows, cols, K, depth_unit, descriptor, detector, depth_scale)
    dist = distortion_of(undistort, intrinsics)
    if dist is None and any(io_formats.TUM_DISTORTION.get(intrinsics, ())):
        log("note: the %s camera has lens distortion (k1 %g, k2 %g, ...) and the frames are used as they are; --undistort undoes it on the GPU" % (
            intrinsics, io_formats.TUM_DISTORTION[intrinsics][0], io_formats.TUM_DISTORTION[intrinsics][1]))
    if dist is not None and not any(dist):
        log("--undistort: all distortion coefficients are zero, there is nothing to undo")
        dist = None
    guesses = own = None
    if odometry:
        guesses, own = io_formats.read_pose_guesses(odometry, seq.times[:n])
        log("motion model camera odometry: %d of %d frames have a pose of their own in %s%s" % (
            int(own.sum()), n, odometry, ", dead-reckoning limit %d" % dead_reckoning_limit if dead_reckoning_limit else ""))
    tr = RgbdTracker(api, cfg, p, device)
    poses, flags, tracking, dead_reckoned = [], 0, 0, 0

    def refusable(set_mask):                     # --detector ORB takes no mask: the run ends with the library's own words
        try:
            set_mask()
        except VslamError as e:
            if detector != 1:
                raise
            raise SystemExit(str(e))
    want_map = bool(map_path or obs_path)        # the log's ids are the map's
    lm_map = obs = None
    t0 = time.perf_counter()
    try:
        if dist is not None:
            from vslam_pose_estimation_framework_amd import rectify
            und = rectify.undistortion(rectify.CameraModel(K, dist, rows, cols))
            tr.set_undistortion(und)
            log("undistorting on the GPU: %dx%d, k1 %g k2 %g p1 %g p2 %g k3 %g, %.1f %% of the pixels have a source inside the raw frame" % (
                (und.rows, und.cols) + tuple(dist) + (100.0 * float(np.mean(rectify.remap_nearest_u16(np.ones((und.raw_rows, und.raw_cols), np.uint16), und.map_xy, und.map_a))),)))
        if downscale != 1:
            tr.set_downscale(downscale, full_rows, full_cols)
            log("downscaling on the GPU by %d: %dx%d -> %dx%d (image: rounded block averages; depth: lower median of the valid values), ahead of %s; "
                "calibration scaled (f %.3f px, c %.3f %.3f)" % (downscale, full_rows, full_cols, rows, cols, "the undistortion" if dist is not None else "the detector",
                                                               K[0, 0], K[0, 2], K[1, 2]))
        if fmt != color_mod.GRAY8:
            tr.set_color_input(fmt)
            log("colour frames (%s): converted to grey on the GPU, ahead of %s" % (color_mod.NAMES[fmt], "the undistortion" if dist is not None else "the detector"))
        elif color:
            log("--color: the folder's images are grey already, nothing to convert")
        if smooth is not None:
            tr.set_smoothing(*smooth)
            log("smoothing on the GPU (%s %d x %d on every intensity image, ahead of %s; the depth image is untouched)" % (
                "Gaussian" if smooth[0] == smooth_mod.GAUSSIAN else "median", smooth[1], smooth[1], "the equalisation" if equalize else "CLAHE" if clahe is not None else "the detector"))
        if equalize:
            tr.set_equalization(True)
            log("equalising histograms on the GPU (cv::equalizeHist on every intensity image%s)" % (", behind the undistortion" if dist is not None else ""))
        if clahe is not None:
            tr.set_clahe(True, clahe, clahe_tiles)
            log("CLAHE on the GPU (cv::CLAHE, clip limit %g, %d x %d tiles, on every intensity image%s)" % (clahe, clahe_tiles[0], clahe_tiles[1], ", behind the undistortion" if dist is not None else ""))
        if bilateral is not None:
            tr.set_bilateral(True, bilateral[0], bilateral[1])
            log("bilateral filter on the GPU (cv::bilateralFilter on every depth image in metres, sigma colour %g, sigma space %g%s)" % (
                tr.get_bilateral()[1:] + (", behind the undistortion" if dist is not None else "",)))
        if mask:
            mk = io_formats.read_png_gray8(mask)
            if mk.shape != (int(cfg.rows), int(cfg.cols)):
                raise SystemExit("--mask: %s is %dx%d, the detector works on %dx%d images" % (mask, mk.shape[0], mk.shape[1], cfg.rows, cfg.cols))
            refusable(lambda: tr.set_detection_mask(mk, mask_margin))
            log("detection mask: %s, margin %d px (no keypoints on its zero pixels, every re-registration attempt included)" % (mask, mask_margin))
        if mask_invalid is not None:
            if dist is None:
                raise SystemExit("--mask-invalid: nothing is undistorted, there are no maps to take a validity mask from")
            refusable(lambda: tr.set_undistortion_mask(True, mask_invalid))
            log("validity mask from the undistortion maps on the GPU: %.1f %% of the pixels have every tap inside the raw frame, margin %d px" % (
                100.0 * float(rectify.validity(und.map_xy, und.map_a, und.raw_rows, und.raw_cols).mean()), mask_invalid))
        if frame_masks:
            log("frame masks: %s, margin %d px (a PNG named like the frame's rgb file; a frame without one has none)" % (frame_masks, mask_margin))
        masked_frames = 0
        tr.set_motion_model(MOTION_MODELS[motion_model], dead_reckoning_limit)
        if want_map:
            tr.enable_map(MAP_ENTRIES_PER_FRAME * n)
        if map_color and fmt == color_mod.GRAY8:
            log("--map-color: the folder's images are grey, the map stays without colours")
            map_color = False
        if map_color:
            tr.enable_map_colors(True)
        if obs_path:
            tr.enable_observations(n * int(cfg.max_points))      # a frame logs at most max_points entries: the log cannot overflow
        for k in range(n):
            if k:
                if color:
                    gray, fmt_k, depth = seq.frame_color(k)
                    if fmt_k != fmt:
                        raise SystemExit("--color: frame %d is %s, the sequence began as %s" % (k, color_mod.NAMES[fmt_k], color_mod.NAMES[fmt]))
                else:
                    gray, depth = seq.frame(k)
            if guesses is not None and own[k]:
                tr.set_pose_guess(guesses[k])
            if frame_masks:
                mpath = os.path.join(frame_masks, os.path.basename(seq.rgb[k]))
                if os.path.isfile(mpath):
                    mk = io_formats.read_png_gray8(mpath)
                    if mk.shape != (int(cfg.rows), int(cfg.cols)):
                        raise SystemExit("--frame-masks: %s is %dx%d, the detector works on %dx%d images" % (mpath, mk.shape[0], mk.shape[1], cfg.rows, cfg.cols))
                    refusable(lambda: tr.set_frame_mask(mk, mask_margin))
                    masked_frames += 1
            fi, n_temp = tr.process(gray, depth)
            dead_reckoned += int(motion_model == "odometry" and fi.fallback == 1)
            poses.append(np.array(fi.camera_left_to_world))
            flags |= fi.error_flags
            tracking += int(fi.status == 1)
            if k % 100 == 99 or k == n - 1:
                log("frame %6d  status %s  points %5d (+%d temporary)  tracked %5d  inliers %5d  landmarks %5d" % (
                    k, "tracking" if fi.status == 1 else "localizing", fi.n_points, n_temp, fi.n_tracked, fi.n_inliers, fi.n_active_landmarks))
        if want_map:
            lm_map = tr.map(0)
            if map_color:
                lm_map["rgb"] = tr.map_colors(0)
        if obs_path:
            obs = tr.observations(0)
    finally:
        tr.destroy()
    dt = time.perf_counter() - t0
    poses = np.array(poses).reshape(-1, 3, 4)
    log("%d frames in %.2f s (%.1f frames/s incl. PNG decode and upload), error flags %d" % (n, dt, n / dt, flags))
    result = {"frames": n, "seconds": dt, "error_flags": flags, "poses": poses, "times": seq.times[:n], "tracking_frames": tracking}
    if frame_masks:
        result["masked_frames"] = masked_frames
        log("%d of %d frames had a mask of their own" % (masked_frames, n))
    if motion_model == "odometry":
        result["dead_reckoned_frames"] = dead_reckoned     # frames whose pose was taken from the odometry
        if dead_reckoned:
            log("%d frames took their pose from the odometry" % dead_reckoned)
    if want_map:
        if flags & 8:
            log("warning: the landmark map ran out of capacity (error flag 8): landmarks created after that are missing")
        result["map"] = lm_map
    if map_path:
        io_formats.write_ply(map_path, lm_map["xyz"], lm_map.get("rgb"), id=lm_map["id"], first_frame=lm_map["first_frame"], last_frame=lm_map["last_frame"],
                             updates=lm_map["updates"])
        log("landmark map: %d landmarks -> %s" % (len(lm_map["id"]), map_path))
    if obs_path:
        io_formats.write_bundle_rgbd(obs_path, K, poses, lm_map, obs)
        res, valid = evaluation.reprojection_residuals_uvd(K, poses, lm_map["xyz"], obs["id"], obs["frame"], obs["xy"], obs["cam"])
        px, dz = np.linalg.norm(res[valid, :2], axis=1), np.abs(res[valid, 2])
        pct = lambda v, q: float(np.percentile(v, q)) if len(v) else None      # noqa: E731
        result["observations"] = obs
        result["reprojection"] = {"observations": int(len(obs["id"])), "landmarks": int(len(lm_map["id"])), "valid": int(valid.sum()),
                                  "median_px": pct(px, 50), "p90_px": pct(px, 90), "median_depth_m": pct(dz, 50), "p90_depth_m": pct(dz, 90)}
        log("observations: %d of %d landmarks -> %s%s" % (len(obs["id"]), len(lm_map["id"]), obs_path,
                                                          " (error flag 16: the log ran out of capacity)" if flags & 16 else ""))
        if len(px):
            log("residuals against the map over %d observations: pixel norm median %.3f px, 90th percentile %.3f px; depth median %.4f m, "
                "90th percentile %.4f m" % (len(px), result["reprojection"]["median_px"], result["reprojection"]["p90_px"],
                                            result["reprojection"]["median_depth_m"], result["reprojection"]["p90_depth_m"]))
    if out_path:
        io_formats.write_trajectory_tum(out_path, poses, seq.times[:n])
        log("trajectory (tum) -> %s" % out_path)
        gt = gt_path or seq.ground_truth_path
        if gt:
            # executables/trajectory_analyzer.cpp's pipeline (time-stamp interpolation :152-205, start-point shift + 100 robust rounds :212-284)
            # with the ground truth read from the benchmark's own `timestamp tx ty tz qx qy qz qw` file instead of an ASL csv
            t_s, p_s = evaluation.read_trajectory_tum(out_path)
            rows = io_formats.read_tum_list(gt)
            t_g = np.array([t for t, _ in rows]); p_g = np.array([[float(v) for v in a[:3]] for _, a in rows]).reshape(-1, 3)
            meas, ref = evaluation.interpolate_correspondences(t_s, p_s, t_g, p_g)
            if len(meas):
                T, _ = evaluation.align_robust_icp(meas, ref)
                moved = meas @ T[:3, :3].T + T[:3, 3]
                result["trajectory_analyzer"] = {"correspondences": len(meas), "raw_rmse": evaluation.rmse(meas, ref), "optimal_rmse": evaluation.rmse(moved, ref)}
                log("trajectory_analyzer: %d interpolated positions, raw RMSE %.4f m, optimal RMSE %.4f m" % (
                    len(meas), result["trajectory_analyzer"]["raw_rmse"], result["trajectory_analyzer"]["optimal_rmse"]))
    return result


def _tiles(text):
    """--clahe-tiles X,Y -> (X, Y)"""
    try:
        x, y = (int(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected X,Y (two integers)")
    return x, y


def _sigmas(text):
    """--bilateral SIGMA_COLOR,SIGMA_SPACE -> (sigma_color, sigma_space)"""
    try:
        sc, ss = (float(v) for v in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError("expected SIGMA_COLOR,SIGMA_SPACE (two numbers)")
    if not (sc >= 0 and ss >= 0 and sc < float("inf") and ss < float("inf")):
        raise argparse.ArgumentTypeError("sigmas must be finite and not negative (0 selects the reference's 2)")
    return sc, ss


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("folder")
    ap.add_argument("--config", choices=sorted(YAML), default="tum")
    ap.add_argument("--intrinsics", default="freiburg1")
    ap.add_argument("--depth-unit", type=float, default=io_formats.TUM_DEPTH_UNIT_M, help="metres per depth count (TUM / ICL: 1/5000)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--gt", default=None)
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--descriptor", choices=("ORB", "BRIEF"), default="ORB", help='the configurations say "ORB-256": cv::ORB::create() as extractor')
    ap.add_argument("--detector", choices=("FAST", "ORB"), default="FAST")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--map", default=None, help="write the landmark map (every landmark of the run, world frame) to this binary PLY file")
    ap.add_argument("--observations", default=None, help="write trajectory, landmark map and the landmark observation log (id, frame, x y, camera "
                    "coordinates) to this .npz bundle (io_formats.read_bundle_rgbd); implies the map")
    ap.add_argument("--undistort", nargs="?", const="", default=None, metavar="k1,k2,p1,p2[,k3]", help="the frames are raw: undo this radial-tangential "
                    "lens distortion on the GPU ahead of the detector; without a value: the coefficients that belong to a named --intrinsics")
    ap.add_argument("--equalize", "-eh", action="store_true", help="equalise every intensity image's histogram on the GPU ahead of the detector "
                    "(the reference's -equalize-histogram / -eh): dim or low-contrast sequences")
    ap.add_argument("--clahe", nargs="?", type=float, const=40.0, default=None, metavar="CLIP", help="contrast-limited adaptive histogram equalisation "
                    "(cv::CLAHE) of every intensity image on the GPU ahead of the detector, clip limit CLIP (40.0 without a value): dim or unevenly "
                    "lit sequences; not together with --equalize")
    ap.add_argument("--clahe-tiles", type=_tiles, default=(8, 8), metavar="X,Y", help="the tile grid of --clahe (8,8)")
    ap.add_argument("--color", action="store_true", help="hand the colour frames over as decoded and convert them to grey on the GPU, ahead of "
                    "--undistort and --equalize (without it: converted on the host, frame by frame)")
    ap.add_argument("--map-color", action="store_true", help="with --color and --map / --observations: the colour of every landmark (the pixel of its "
                    "point at the last update, sampled on the GPU) as red green blue in the PLY and map_rgb in the bundle")
    ap.add_argument("--bilateral", nargs="?", type=_sigmas, const=(2.0, 2.0), default=None, metavar="SIGMA_COLOR,SIGMA_SPACE", help="smooth every depth "
                    "image with the reference's bilateral filter (enable_bilateral_filtering) on the GPU ahead of the space map; 2,2 without a value")
    argv = list(sys.argv[1:] if argv is None else argv)
    for i in range(len(argv) - 1):          # "--undistort -0.28,0.07,0,0": argparse would read the negative list as an option
        if argv[i] == "--undistort" and argv[i + 1][:1] == "-" and argv[i + 1][1:2] in "0123456789.":
            argv[i:i + 2] = ["--undistort=" + argv[i + 1]]
            break
    ap.add_argument("--motion-model", choices=sorted(MOTION_MODELS), default="constant-velocity", help="the prior every frame starts with: the last "
                    "refined motion (the default), identity (none), or the motion an external pose source reports (odometry, with --odometry; "
                    "configuration_xtion.yaml's own model)")
    ap.add_argument("--odometry", default=None, metavar="FILE", help="--motion-model odometry: camera_left_to_world per frame, a TUM trajectory "
                    "(associated by time stamp) or a KITTI pose file (line k for frame k)")
    ap.add_argument("--dead-reckoning-limit", type=int, default=0, metavar="N", help="--motion-model odometry: localize again after N frames in a row "
                    "whose pose was taken from the odometry (0: never)")
    ap.add_argument("--mask", default=None, metavar="MASK.png", help="detection mask for the whole run: an 8-bit PNG at the processed size (the undistorted "
                    "one under --undistort), zero = no keypoints on that pixel (the robot's own body, overlays, vignetted corners)")
    ap.add_argument("--mask-margin", type=int, default=0, metavar="N", help="widen every masked region of --mask and --frame-masks by N pixels (0 .. 64)")
    ap.add_argument("--smooth", default=None, metavar="MODE[:K]", help="smooth every intensity image on the GPU ahead of the equalisation and the detector: "
                    "gaussian[:3|5|7] (default gaussian:5) or median[:3|5] (default median:3); the depth image is untouched")
    ap.add_argument("--downscale", type=int, default=1, metavar="N", help="reduce every image and depth image by the whole factor N (2, 3 or 4) on the GPU ahead "
                    "of everything but the colour conversion: rounded block averages, and for depth the lower median of a block's valid values; the "
                    "intrinsics are scaled and the tracker runs at the reduced size (masks are given at that size); combines with every other switch")
    ap.add_argument("--frame-masks", default=None, metavar="DIR", help="a mask per frame (a segmentation network's output): a folder of 8-bit PNGs at the "
                    "processed size, named like the frames' files under rgb/; a frame without a file has no mask of its own")
    ap.add_argument("--mask-invalid", nargs="?", type=int, const=0, default=None, metavar="N", help="with --undistort: no keypoints on pixels whose source "
                    "lies partly outside the raw frame (the seam between picture and black fill), computed from the maps on the GPU; N widens it (0 .. 64)")
    a = ap.parse_args(argv)
    try:
        check_mask_args(a.mask, a.mask_margin, ValueError, a.frame_masks, a.mask_invalid, a.undistort)
        check_motion_args(a.motion_model, a.odometry, a.dead_reckoning_limit, ValueError)
        smooth_mod.argument(a.smooth, ValueError)
    except ValueError as e:
        ap.error(str(e))
    if a.downscale < 1 or a.downscale > 4:
        ap.error("--downscale: a whole factor in 1 .. 4 (1: off)")
    if a.clahe is not None and a.equalize:
        ap.error("--clahe and --equalize exclude each other: one equalisation ahead of the detector")
    if a.map_color and not (a.color and (a.map or a.observations)):
        ap.error("--map-color needs --color and --map or --observations")
    return a


def check_mask_args(mask, mask_margin, error, frame_masks=None, mask_invalid=None, undistort=None):
    """What --mask, --frame-masks, --mask-margin and --mask-invalid allow together."""
    if mask_margin < 0 or mask_margin > 64:
        raise error("--mask-margin: a whole number of pixels in 0 .. 64")
    if mask_margin and not mask and not frame_masks:
        raise error("--mask-margin needs --mask or --frame-masks")
    if mask is not None and not os.path.isfile(mask):
        raise error("--mask: no such file: %s" % mask)
    if frame_masks is not None and not os.path.isdir(frame_masks):
        raise error("--frame-masks: no such folder: %s" % frame_masks)
    if mask_invalid is not None and undistort is None:
        raise error("--mask-invalid needs --undistort: the validity mask comes from the undistortion maps")
    if mask_invalid is not None and (mask_invalid < 0 or mask_invalid > 64):
        raise error("--mask-invalid: a whole number of pixels in 0 .. 64")


def main(argv=None):
    a = parse_args(argv)
    run(a.folder, a.config, a.intrinsics, a.depth_unit, a.out, a.max_frames, 1 if a.descriptor == "ORB" else 0, 1 if a.detector == "ORB" else 0, a.gt, a.device,
        map_path=a.map, obs_path=a.observations, undistort=a.undistort, equalize=a.equalize, color=a.color, clahe=a.clahe, clahe_tiles=a.clahe_tiles, motion_model=a.motion_model, odometry=a.odometry,
        dead_reckoning_limit=a.dead_reckoning_limit,
        map_color=a.map_color, bilateral=a.bilateral, mask=a.mask, mask_margin=a.mask_margin, frame_masks=a.frame_masks, mask_invalid=a.mask_invalid, downscale=a.downscale, smooth=a.smooth)


if __name__ == "__main__":
    main()
