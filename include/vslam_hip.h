/* vslam_hip.h — C ABI of the MI355X-native ProSLAM front end (libvslam_hip.so).
 *
 * Drop-in boundary for the per-frame hot path of Ssellu/vslam-pose-estimation-framework
 * (a ProSLAM fork).  The reference has no FFI: its plug points are C++ virtuals wired in
 * SLAMAssembly::_createStereoTracker (src/system/slam_assembly.cpp:61-76).  Each entry
 * point below names the reference interface it replaces (paths relative to the reference
 * repository root).  The header-only C++ shim that subclasses the reference classes and
 * forwards to these calls is shim/proslam_hip_plugin.h; INTEGRATION.md shows the two lines
 * a maintainer changes.
 *
 * Conventions
 *   - plain C, no exceptions, no callbacks; every call returns 0 (VSLAM_OK) or a negative
 *     vslam_status; vslam_last_error() gives the text (reference: std::runtime_error thrown
 *     at stereo_framepoint_generator.cpp:30-33,75-78,139-142,468-471, caught in app.cpp:128).
 *   - a context owns `n_streams` independent sequences ("streams": whole KITTI sequences
 *     or chunks of one).  Every per-frame call processes ONE stereo pair per stream, all
 *     streams in the same kernels (grid dimension = stream).  n_streams = 1 is the literal
 *     drop-in for the reference's single tracker.
 *   - images: 8-bit grayscale, row-major, `stride` bytes per row
 *     (reference: Frame::intensityImageLeft/Right, CV_8UC1, src/types/frame.h:114-119).
 *   - transforms: double[12], row-major 3x4 [R|t] (reference: TransformMatrix3D,
 *     src/types/definitions.h:62).
 *   - descriptors: 32 bytes (256 bit), Hamming norm (definitions.h:45-49).
 *   - a context is single-caller (reference: one caller thread, app.cpp:96).
 */
#ifndef VSLAM_HIP_H
#define VSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSLAM_MAX_REGIONS 16      /* detector grid cells (det_rows*det_cols)          */
#define VSLAM_DESC_BYTES 32       /* SRRG_PROSLAM_DESCRIPTOR_SIZE_BITS=256            */
#define VSLAM_MAX_EPI 8           /* maximum_epipolar_search_offset_pixels upper bound */

typedef enum {
  VSLAM_OK = 0,
  VSLAM_ERR_INVALID = -1,   /* bad argument / null frame (reference: runtime_error)          */
  VSLAM_ERR_NO_DEVICE = -2, /* HIP device or kernel image missing: the product path never   */
                            /* falls back to a CPU implementation                           */
  VSLAM_ERR_HIP = -3,       /* a HIP runtime call failed                                    */
  VSLAM_ERR_CAPACITY = -4,  /* an output array of the caller, or the scratch buffers of a stand-alone entry, are too
                               small.  Overflow of a context's device-resident buffers inside vslam_process_* / the
                               stage calls is NOT a return code: processing continues on the truncated lists and the
                               frame's vslam_frame_info.error_flags reports it per stream (bit 0 keypoints, bit 1 points,
                               bit 2 history, bit 3 landmark map, bit 4 observation log) */
  VSLAM_ERR_STATE = -5      /* call sequence violated (e.g. track before frame_begin)       */
} vslam_status;

typedef enum { VSLAM_LOCALIZING = 0, VSLAM_TRACKING = 1 } vslam_tracker_status; /* Frame::Status */

/* All parameters the hot path reads.  Names follow the reference's YAML keys
 * (configurations/configuration_kitti.yaml:49-134, src/types/parameters.h:64-330). */
typedef struct vslam_config {
  /* camera (src/types/camera.h): left == right intrinsics for a rectified pair.  With vslam_set_rectification the
     context takes raw pairs and these describe the RECTIFIED pair the maps produce (rows x cols, K = P1, baseline from P2) */
  int32_t rows, cols;
  double K[9];          /* cameraMatrix(), row-major                                        */
  double baseline_h[3]; /* Camera::baselineHomogeneous() of the right camera: (-fx*B, 0, 0) */

  /* base_framepoint_generation */
  int32_t det_rows, det_cols;            /* number_of_detectors_vertical / _horizontal      */
  int32_t detector_threshold_minimum;    /* FAST thresholds (parameters.h:176-177)           */
  int32_t detector_threshold_maximum;
  double detector_threshold_maximum_change;
  double target_number_of_keypoints_tolerance;
  int32_t bin_size_pixels;
  int32_t enable_keypoint_binning;
  int32_t minimum_projection_tracking_distance_pixels;
  int32_t maximum_projection_tracking_distance_pixels;
  double minimum_descriptor_distance_tracking;
  double maximum_descriptor_distance_tracking;
  double maximum_reliable_depth_meters;
  double maximum_depth_meters;
  double minimum_depth_meters;

  /* stereo_framepoint_generation */
  double maximum_matching_distance_triangulation;
  double minimum_disparity_pixels;
  int32_t maximum_epipolar_search_offset_pixels;

  /* tracking (PoseTracker3DParameters) */
  int32_t minimum_track_length_for_landmark_creation;
  int32_t minimum_number_of_landmarks_to_track;
  double tunnel_vision_ratio;
  double good_tracking_ratio;
  int32_t enable_landmark_recovery;
  double minimum_delta_angular_for_movement;
  double minimum_delta_translational_for_movement;

  /* tracking.aligner (AlignerParameters) */
  double aligner_error_delta_for_convergence;
  double aligner_maximum_error_kernel;
  double aligner_damping;
  int32_t aligner_maximum_number_of_iterations;
  int32_t aligner_minimum_number_of_inliers;

  /* landmark (LandmarkParameters, parameters.h:97-112) */
  double landmark_maximum_error_squared_meters;
  int32_t landmark_maximum_number_of_iterations;

  /* capacities of the device-resident buffers (no reference counterpart: std::vector grows) */
  int32_t max_keypoints;       /* per image, 64..65535                                        */
  int32_t max_points;          /* framepoints per frame                                       */
  int32_t max_history_frames;  /* frames of per-point history kept for landmark refinement     */

  /* descriptor extractor (base_framepoint_generator.cpp:184-224): 0 = BRIEF-32 (descriptor_type "BRIEF",
   * configuration_kitti.yaml:60; 28 px border), 1 = ORB (cv::ORB::create() used as extractor on the detector's FAST
   * keypoints: descriptor_type "ORB" and every unknown string, e.g. configuration_euroc.yaml:52 "ORB-256"; rBRIEF at
   * level 0 of the 7x7 Gaussian-blurred image, steered by KeyPoint::angle = -1 as FAST leaves it, 31 px border) */
  int32_t descriptor_type;
} vslam_config;
#define VSLAM_DESCRIPTOR_BRIEF 0
#define VSLAM_DESCRIPTOR_ORB 1

/* Per-frame, per-stream report: the scalars PoseTracker3D / SLAMAssembly read back from the
 * plug-ins (pose_tracker_3d.cpp:111,132,242-248,361; slam_assembly.cpp:644-742). */
typedef struct vslam_frame_info {
  int32_t frame_index;         /* frames processed by this stream so far (this one included)  */
  int32_t status;              /* tracker status AFTER the frame (vslam_tracker_status)       */
  int32_t status_at_start;     /* status the frame was created with                           */
  int32_t n_keypoints_left, n_keypoints_right;   /* after the descriptor border filter        */
  int32_t n_detected_left, n_detected_right;     /* raw FAST detections (controller input); behind a detection mask: the masked counts */
  int32_t thresholds[VSLAM_MAX_REGIONS];         /* detector thresholds AFTER adjust          */
  int32_t track_attempts;      /* 1 + recursive re-registrations (pose_tracker_3d.cpp:300)    */
  int32_t n_tracked;           /* points linked by the final track() call                     */
  int32_t n_lost;              /* lost list of the final track() call                         */
  int32_t n_tracked_landmarks; /* numberOfTrackedLandmarks()                                  */
  int32_t aligner_ran;         /* StereoUVAligner::converge() was called on the final points  */
  int32_t aligner_iterations;  /* oneRound() calls of that converge()                         */
  int32_t aligner_converged;   /* hasSystemConverged()                                        */
  int32_t n_inliers, n_outliers;
  double total_error;          /* totalError()                                                */
  int32_t n_after_prune;       /* points surviving _prunePoints                               */
  int32_t n_recovered;         /* points added by recoverPoints                               */
  int32_t n_active_landmarks;  /* _number_of_active_landmarks                                 */
  int32_t n_new_stereo;        /* points appended by compute()                                */
  int32_t n_points;            /* frame->points().size() at the end of the frame              */
  int32_t track_broken;        /* breakTrack() happened                                       */
  int32_t fallback;            /* _fallbackEstimate() was used                                */
  int32_t window_pixels;       /* _projection_tracking_distance_pixels after the frame        */
  int32_t error_flags;         /* bit0 keypoint capacity, bit1 point capacity, bit2 history,  */
                               /* bit3 (value 8) landmark map capacity (vslam_enable_map)     */
                               /* bit4 (value 16) observation log capacity (vslam_enable_observations) */
  double tau_track;            /* _current_descriptor_distance_tracking after the frame       */
  double tau_triangulation;    /* _current_maximum_descriptor_distance_triangulation          */
  double camera_left_to_world[12];  /* frame pose (robotToWorld with identity robot offset)   */
  double previous_to_current[12];   /* motion prior kept for the next frame                   */
} vslam_frame_info;

typedef struct vslam_ctx vslam_ctx;

/* ---- lifetime --------------------------------------------------------------------------
 * Replaces: new StereoFramePointGenerator(params) + setCameraLeft/Right + configure(),
 *           new StereoUVAligner(params) + setMaximum/MinimumReliableDepthMeters + configure(),
 *           PoseTracker3D::configure()   (slam_assembly.cpp:61-76, pose_tracker_3d.cpp:11-21).
 * `device` is the HIP device ordinal.  Fails with VSLAM_ERR_NO_DEVICE when no GPU is usable. */
int vslam_create(const vslam_config* cfg, int device, int n_streams, vslam_ctx** out);
void vslam_destroy(vslam_ctx* ctx);
const char* vslam_last_error(const vslam_ctx* ctx); /* ctx may be NULL: last create() error */
void vslam_default_config_kitti(vslam_config* cfg); /* configuration_kitti.yaml values, KITTI-00 calib */
void vslam_default_config_euroc(vslam_config* cfg); /* configuration_euroc.yaml values                */
/* Restart every stream as a fresh sequence (PoseTracker3D::configure, WorldMap::clear). */
int vslam_reset(vslam_ctx* ctx);
/* Exact mode with whole sequences of different lengths per stream: a stream whose sequence has ended is
 * switched off — every kernel skips it, its last frame's state, report and pose log stay readable — while the other
 * streams of the context carry on; vslam_reset_stream restarts ONE stream as a fresh sequence (a new PoseTracker3D /
 * generator / aligner / WorldMap: pose_tracker_3d.cpp:11-21) so that a stream can work through a queue of sequences.
 * vslam_set_stream_active synchronises the context; vslam_reset_stream is asynchronous (queued between two frames on the
 * context's HIP streams).  Neither may be called between vslam_frame_begin and the end of that frame.
 * The images passed for an inactive stream are ignored (the pointer arithmetic still reserves its slot). */
int vslam_set_stream_active(vslam_ctx* ctx, int stream, int active);
int vslam_reset_stream(vslam_ctx* ctx, int stream);
int vslam_reset_streams(vslam_ctx* ctx, int32_t n, const int32_t* streams);   /* several streams, one launch per state half */
/* Use the caller's HIP stream (hipStream_t passed as void*) for all work of this context. */
int vslam_set_hip_stream(vslam_ctx* ctx, void* hip_stream);

/* ---- whole-frame entry point -------------------------------------------------------------
 * Replaces PoseTracker3D::compute() (pose_tracker_3d.cpp:32-222) for every stream of the
 * context: initialize -> track -> StereoUVAligner -> prune -> recoverPoints -> landmark
 * update -> compute, with the tracker's control logic evaluated on the device.  Asynchronous
 * on the context stream; no host synchronisation.
 *   left/right: n_streams images each; image s starts at base + s*image_stride_bytes.
 *   *_device variant: pointers are device memory (inputs already resident in HBM).
 *   host variant: pointers are host memory, copied to the device first (hipMemcpyAsync on the image stream: one
 *     copy per side when the images are back to back, else one per image; pinned memory makes it truly asynchronous).
 *     The buffers must stay valid and unchanged until the copy has run (vslam_synchronize, or any read-back call). */
int vslam_process_device(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right,
                         int32_t row_stride_bytes, size_t image_stride_bytes);
int vslam_process_host(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right,
                       int32_t row_stride_bytes, size_t image_stride_bytes);
/* ---- rectification of raw, distorted stereo pairs (opt-in) ---------------------------------------------------------------
 * A context gets one rig, shared by all its streams, as two fixed-point remap maps per side at the RECTIFIED size (cfg rows x cols),
 * in the format cv::convertMaps(..., CV_16SC2) / initUndistortRectifyMap(..., CV_16SC2) produce [recalled], so a caller that has
 * OpenCV passes its own maps unchanged:
 *   map_xy: int16 [rows][cols][2] = (ix >> 5, iy >> 5), ix = rint(32 u), iy = rint(32 v), (u, v) the source coordinate in the raw image
 *   map_a : uint16 [rows][cols]   = (iy & 31) * 32 + (ix & 31); values >= 1024 are rejected (VSLAM_ERR_INVALID)
 * Interpolation is cv::remap INTER_LINEAR, BORDER_CONSTANT 0 [recalled], in integers: ax = a & 31, ay = a >> 5,
 *   w00 = (32-ax)(32-ay)*32, w01 = ax(32-ay)*32, w10 = (32-ax)ay*32, w11 = ax*ay*32 (sum 32768),
 *   p_ij = raw[y0+i][x0+j] inside the raw image, else 0;  out = (sum w*p + 16384) >> 15.
 * While rectification is set, vslam_process_host, vslam_process_device and vslam_frame_begin take RAW images of raw_rows x raw_cols
 * (row stride >= raw_cols); one kernel (k_rectify) rectifies every stream's pair ahead of the detector, on the image queue.  Device
 * images are read by that kernel only: they must stay valid until it has run, not until the frame ends.  Everything downstream
 * reports rectified coordinates (keypoints, views, points, poses of the rectified left camera).  Rectification survives vslam_reset
 * and vslam_reset_stream(s).
 * vslam_set_rectification: all four map pointers NULL turns it off.  Host pointers, copied to the device before the call returns
 *   (it synchronises the context).  VSLAM_ERR_STATE between vslam_frame_begin and the end of that frame.
 * vslam_get_rectified_images: the rectified pair the last submitted frame of `stream` was processed on (rows*cols bytes each, dense);
 *   VSLAM_ERR_STATE when rectification is off or no frame has been submitted since it was set.  Synchronises.
 * vslam_remap_u8: the same remap stand-alone on host images (like vslam_resize_linear_u8): src is rows x cols with row_stride bytes
 *   per row, dst is dst_rows x dst_cols (dense), the maps are dst-sized. */
int vslam_set_rectification(vslam_ctx* ctx, int32_t raw_rows, int32_t raw_cols,
                            const int16_t* map_xy_left, const uint16_t* map_a_left,
                            const int16_t* map_xy_right, const uint16_t* map_a_right);
int vslam_get_rectified_images(vslam_ctx* ctx, int stream, uint8_t* left, uint8_t* right);
int vslam_remap_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride,
                   const int16_t* map_xy, const uint16_t* map_a, int32_t dst_rows, int32_t dst_cols, uint8_t* dst);
/* ---- histogram equalisation of the input pair (opt-in; csrc/kernels_equalize.h) --------------------------------
 * The reference's -equalize-histogram / -eh switch (option_equalize_histogram): cv::equalizeHist on each 8-bit image [recalled]:
 *   h[256] = counts of the rows x cols pixels (row padding is never counted);  i0 = the first v with h[v] != 0;
 *   a constant image (h[i0] == rows*cols) stays as it is;  scale = 255.f / float(rows*cols - h[i0])  (one IEEE single division);
 *   lut[v] = 0 for v <= i0, else min(255, rint(float(h[i0+1] + ... + h[v]) * scale))  (one single multiply, ties to even);  out = lut[in].
 * Images of up to 2^24 pixels (the counts are then exact in float), else VSLAM_ERR_INVALID.
 * Order: rectify (when set), then equalise, then detect — the rectified pair is equalised, as in the reference's node.  Two kernels
 * (k_hist_u8, k_equalize_apply) per frame on the queue of the image pipeline, under the fused entries and the stage path alike.  The
 * equalised pair lives in the context's own input slabs: host images are equalised in place there, device images are READ by the two
 * kernels only and never written.  A switched-off stream is neither read nor written.
 * vslam_set_equalization: on != 0 turns it on (its own allocations), 0 turns it off and frees them; nothing is launched while off.
 *   Synchronises the context.  VSLAM_ERR_STATE between vslam_frame_begin and the end of that frame.  The switch survives vslam_reset and
 *   vslam_reset_stream(s).
 * vslam_get_equalized_images: the equalised pair the last submitted frame of `stream` was processed on (rows*cols bytes each, dense);
 *   VSLAM_ERR_STATE when equalisation is off or no frame has been submitted since it was set.  Synchronises.  With rectification on as
 *   well, vslam_get_rectified_images still returns the rectified (not yet equalised) pair: it is kept in slabs of its own.
 * vslam_get_equalization_histograms: uint32 [2][256], the counts of that frame's left and right image; the same errors.  The table is
 *   zeroed whole every frame, so the rows of a switched-off stream read zero.
 * vslam_equalize_hist_u8: the same two kernels stand-alone on one host image: src is rows x cols with row_stride bytes per row (any
 *   alignment), dst is dense, hist256 (may be NULL) receives the counts.  rows or cols 0: VSLAM_OK, nothing written.  VSLAM_ERR_INVALID:
 *   null src / dst, negative size, row_stride < cols, more than 2^24 pixels; the context stays usable. */
int vslam_set_equalization(vslam_ctx* ctx, int on);
int vslam_get_equalized_images(vslam_ctx* ctx, int stream, uint8_t* left, uint8_t* right);
int vslam_get_equalization_histograms(vslam_ctx* ctx, int stream, uint32_t* hist512);
int vslam_equalize_hist_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride,
                           uint8_t* dst /* dense */, uint32_t* hist256 /* may be NULL */);
/* ---- CLAHE of the input pair: the second mode of the equalisation slot (opt-in; csrc/kernels_clahe.h) -------------------
 * cv::createCLAHE(clip_limit, Size(tiles_x, tiles_y))->apply [recalled], bit-exact against the numpy restatement in clahe.py: per-tile
 * counts of the image extended to whole tiles (BORDER_REFLECT_101), clipped at max((int)(clip_limit * tile_area / 256), 1) with the
 * excess spread over the bins, one table per tile, and every pixel blended from the four tables around it.  clip_limit <= 0: no clipping.
 * Same place and same placement as global equalisation (behind colour conversion and rectification, ahead of the detector; host images
 * in place in the context's slabs, device images read only), two kernels (k_clahe_lut, k_clahe_apply) per frame on the queue of the
 * image pipeline, under the fused entries and the stage path alike.  A switched-off stream is neither read nor written.
 * vslam_set_clahe: on != 0 turns it on (its own allocations; again with other arguments: they replace the earlier ones), 0 turns it off
 *   and frees them; nothing is launched while off.  Synchronises the context.  VSLAM_ERR_STATE between vslam_frame_begin and the end of
 *   that frame, and while global equalisation is on; vslam_set_equalization(ctx, 1) returns VSLAM_ERR_STATE while CLAHE is on (switching
 *   either one OFF while the other is on is accepted and changes nothing).  VSLAM_ERR_INVALID: tiles_x or tiles_y outside
 *   1 .. VSLAM_CLAHE_MAX_TILES, cols <= tiles_x or rows <= tiles_y (the reflected border would leave the image), more than 2^24 pixels,
 *   clip_limit not finite.  The switch survives vslam_reset and vslam_reset_stream(s).
 * vslam_get_equalized_images returns the CLAHE pair in this mode; vslam_get_equalization_histograms returns VSLAM_ERR_STATE.
 * vslam_get_clahe_luts: uint8 [2][tiles_y][tiles_x][256], the tables of the left and right image of the last submitted frame of
 *   `stream`, with the errors of vslam_get_equalized_images (VSLAM_ERR_STATE also under global equalisation).  Synchronises.
 * vslam_clahe_u8: the same two kernels stand-alone on one host image: src is rows x cols with row_stride bytes per row, dst with
 *   dst_row_stride (bytes beyond cols in a row are neither read nor written), each at any alignment — the device copies keep the
 *   caller's alignment mod 16; dst == src (with equal strides) works in place, otherwise the two must not overlap.  luts (may be NULL)
 *   receives [tiles_y][tiles_x][256].  VSLAM_ERR_INVALID, nothing written: the refusals of vslam_set_clahe, null src / dst, a stride
 *   below cols; the context stays usable. */
#define VSLAM_CLAHE_MAX_TILES 32
int vslam_set_clahe(vslam_ctx* ctx, int on, double clip_limit, int tiles_x, int tiles_y);
int vslam_get_clahe_luts(vslam_ctx* ctx, int stream, uint8_t* luts);
int vslam_clahe_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, double clip_limit, int32_t tiles_x,
                   int32_t tiles_y, uint8_t* dst, int32_t dst_row_stride, uint8_t* luts /* may be NULL */);
/* ---- bilateral filtering of the 16-bit depth image (csrc/kernels_bilateral.h) --------------------------------------------
 * The optional first step of DepthFramePointGenerator::_computeDepthMap (depth_framepoint_generator.cpp:415-422,
 * enable_bilateral_filtering): depth to metres as float, cv::bilateralFilter(src, dst, -1, sigma_color, sigma_space), back to 16 bit
 * [recalled], bit-exact against the numpy restatement in bilateral.py, which fixes every order of operations: v = float(raw) *
 * float(depth_scale); radius = max(1, cvRound(sigma_space * 1.5)), sigmas <= 0 count as 1; the taps inside the circle in scan order;
 * BORDER_REFLECT_101; the colour table of 4098 floats over the image's own range (a flat image is returned as it is, its table is zeros);
 * out = clamp(rint(filtered * float(1.0 / depth_scale)), 0, 65535).  Holes (zeros) are pixels like any other, as in the reference.
 * vslam_bilateral_depth_u16: three kernels (k_depth_range, k_bilateral_lut, k_bilateral_apply) on one host image: src is rows x cols
 *   with row_stride ELEMENTS per row, dst with dst_row_stride (elements beyond cols in a row are neither read nor written), each at any
 *   2-byte alignment; dst == src (with equal strides) works in place, otherwise the two must not overlap.  lut4098 (may be NULL)
 *   receives the table.  rows == 0 or cols == 0: VSLAM_OK, nothing written.  VSLAM_ERR_INVALID, nothing written: null src / dst, a
 *   negative size, a stride below cols, depth_scale <= 0 or not finite, a sigma that is not finite, a radius above
 *   VSLAM_BILATERAL_MAX_RADIUS, more than 2^24 pixels; the context stays usable. */
#define VSLAM_BILATERAL_MAX_RADIUS 8
#define VSLAM_BILATERAL_LUT 4098
int vslam_bilateral_depth_u16(vslam_ctx* ctx, const uint16_t* src, int32_t rows, int32_t cols, int32_t row_stride /* elements */,
                              double depth_scale, double sigma_color, double sigma_space, uint16_t* dst, int32_t dst_row_stride,
                              float* lut4098 /* may be NULL */);
/* ---- colour input: interleaved 8-bit colour to grey ahead of everything else (opt-in; csrc/kernels_gray.h) -------------
 * The reference converts a colour frame itself before anything else happens to it (slam_assembly.cpp:392-399, cvtColor CV_BGR2GRAY).
 * One definition, cvtColor on 8-bit images with 14 fractional bits [recalled], all integer:
 *   gray = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14;  alpha is ignored.
 * (Newer OpenCV uses 15 bits, 9798 / 19235 / 3735, and differs on 0.26 % of all colour triples: not built.)
 * Order: colour -> grey -> rectify (when set) -> equalise (when set) -> detect.  One kernel (k_gray_u8) per frame at the head of the image
 * pipeline, on its queue, under the fused entries and the stage path alike.
 * vslam_set_color_input: while format is not VSLAM_PIXEL_GRAY8, vslam_process_host, vslam_process_device and vslam_frame_begin take
 *   interleaved colour images of the size the context otherwise expects (raw_rows x raw_cols while rectification is set, else rows x
 *   cols); row_stride and image_stride are in BYTES, row_stride >= channels * cols (else VSLAM_ERR_INVALID).  Host images are copied to
 *   colour slabs of the context's own; device images are READ by this kernel only (and, while vslam_enable_map_colors is on, once more
 *   behind the frame's last launch: see there) and never written.  The grey pair is written where the
 *   next stage reads.  A switched-off stream is neither read nor written.  Synchronises the context; VSLAM_ERR_STATE between
 *   vslam_frame_begin and the end of that frame; VSLAM_ERR_INVALID for a format outside 0 .. 4.  The switch survives vslam_reset and
 *   vslam_reset_stream(s).  GRAY8 turns it off and frees its allocations; nothing is launched while off.
 * vslam_get_gray_images: the grey pair of the last submitted frame of `stream` at the input size (raw_rows x raw_cols while rectification
 *   is set, else rows x cols; dense); VSLAM_ERR_STATE when the switch is off or no frame has been submitted since it was set.
 *   Synchronises.  With equalisation on and rectification off the pair is equalised in place afterwards: this getter then returns the
 *   equalised pair, like vslam_get_equalized_images.
 * vslam_gray_u8: the kernel stand-alone on one host image: src is rows x cols pixels with row_stride BYTES per row (any alignment), dst is
 *   dense.  rows or cols 0: VSLAM_OK, nothing written.  VSLAM_ERR_INVALID: null src / dst, negative size, row_stride < channels * cols,
 *   format outside 1 .. 4; the context stays usable. */
#define VSLAM_PIXEL_GRAY8 0
#define VSLAM_PIXEL_BGR8 1   /* a cv::Mat CV_8UC3 */
#define VSLAM_PIXEL_RGB8 2   /* a decoded PNG, ROS rgb8 */
#define VSLAM_PIXEL_BGRA8 3
#define VSLAM_PIXEL_RGBA8 4
int vslam_set_color_input(vslam_ctx* ctx, int format);
int vslam_get_gray_images(vslam_ctx* ctx, int stream, uint8_t* left, uint8_t* right);
int vslam_gray_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride_bytes, int format,
                  uint8_t* dst /* dense */);
/* ---- integer-factor reduction of images and depth images (csrc/kernels_downscale.h, downscale.py) ------------------------
 * The project's own definition, all integer.  Factor f is 2, 3 or 4.  A full image of full_rows x full_cols gives full_rows / f x
 * full_cols / f (integer division); the full_rows % f bottom rows and full_cols % f right columns are never read.  Both full sizes lie
 * in 1 .. 32767 and give at least 1 x 1.
 *   8 bit:  out[y][x] = (sum of the f x f block at (f y, f x) + f f / 2) / (f f), round half up.  At f = 2 that is (a + b + c + d + 2) >> 2,
 *           which cv::resize(INTER_AREA) computes at an integer factor of 2 [recalled]; at 3 and 4 OpenCV goes through a float reciprocal
 *           and may differ on ties.  Parity with OpenCV is not pinned.
 *   depth:  the values are never blended (a mix across a depth edge invents a surface, as for the nearest-neighbour depth remap): the v
 *           non-zero values of the block in ascending order, out = the element at index (v - 1) / 2, the lower median; 0 when v == 0.
 * Calibration of the reduced image (the caller's arithmetic, downscale.py: scale_intrinsics / scale_projection; the library does not
 * touch K): output pixel x covers full pixels f x .. f x + f - 1, so fx' = fx / f, fy' = fy / f, cx' = (cx + 0.5) / f - 0.5, cy'
 * likewise, a projection matrix's P[0][3] is divided by f; baseline, distortion coefficients and depth scale are unchanged.
 * vslam_downscale_u8 / vslam_downscale_depth_u16: the kernels (k_downscale_u8, k_downscale_depth_u16) stand-alone on one host image:
 *   src is rows x cols (the FULL size) with row_stride bytes / elements per row, dst is rows / factor x cols / factor with
 *   dst_row_stride, each at any alignment (2-byte for depth); what lies beyond the reduced width in a dst row is neither read nor written.
 *   rows == 0 or cols == 0: VSLAM_OK, nothing written.  VSLAM_ERR_INVALID, nothing written: a factor outside 2 .. 4, null src / dst, a
 *   negative size, row_stride < cols, dst_row_stride < cols / factor, a full size above 32767 or one that gives a 0-row or 0-column
 *   result; the context stays usable.
 * The stage (opt-in, the stereo context): colour -> grey -> DOWNSCALE -> rectify (when set) -> equalise / CLAHE (when set) -> detect.  One
 * kernel (k_downscale_u8) per frame on the image pipeline's queue, all streams and both sides in one launch, under the fused entries and
 * the stage path (vslam_frame_begin) alike.
 * vslam_set_downscale: while factor is not 1, vslam_process_host, vslam_process_device and vslam_frame_begin take images of full_rows x
 *   full_cols — colour images (vslam_set_color_input) of that size too.  full / factor must equal what the next stage expects: raw_rows x
 *   raw_cols while rectification is set (the maps then address the REDUCED raw image; the maps' validity mask needs no change), else the
 *   context's rows x cols; else VSLAM_ERR_INVALID, not sticky, nothing changed.  vslam_set_rectification makes the same check while this
 *   switch is on, so the pair of setters is consistent in either order: with maps whose raw size differs from rows x cols, set the maps
 *   first.  The context is created at the reduced size with the reduced calibration (downscale.py: apply_to_config); the library does
 *   not touch K.  Detection masks stay at the processed size.  Host images are copied to full-size slabs of the stage's own (two
 *   parities); device images are READ by this kernel only (colour ones by k_gray_u8, and by k_map_color while map colours are on) and
 *   never written.  The reduced pair is written where the next stage reads.  A switched-off stream is neither read nor written.
 *   Synchronises the context; VSLAM_ERR_STATE between vslam_frame_begin and the end of that frame; VSLAM_ERR_INVALID for a factor outside
 *   1 .. 4 or a full size outside 1 .. 32767.  The switch survives vslam_reset and vslam_reset_stream(s).  factor 1 (the sizes are then
 *   ignored) turns it off and frees its allocations; nothing is launched or allocated while off.
 *   Map colours under the switch: k_map_color reads the caller's full-size colour image; each tap is the per-channel block average with
 *   the rounding above, through the remap's four taps when rectification is on, each of them such an average.
 * vslam_get_downscale: the switch in force; factor 1, sizes 0 while off.
 * vslam_get_downscaled_images: the reduced pair of the last submitted frame of `stream` (full / factor, dense); VSLAM_ERR_STATE when the
 *   switch is off or no frame has been submitted since it was set.  Synchronises.  With equalisation on and rectification off the pair
 *   is equalised in place afterwards: this getter then returns the equalised pair, like vslam_get_equalized_images.  While the switch is
 *   on, vslam_get_gray_images returns the full-size grey pair, which no later stage touches. */
int vslam_set_downscale(vslam_ctx* ctx, int32_t factor, int32_t full_rows, int32_t full_cols);
int vslam_get_downscale(vslam_ctx* ctx, int32_t* factor, int32_t* full_rows, int32_t* full_cols);
int vslam_get_downscaled_images(vslam_ctx* ctx, int stream, uint8_t* left, uint8_t* right);
/* The same stage in RGB-D mode (the device-resident loop; the vslam_rgbd type is declared with that mode below).  The image: colour ->
 * grey -> DOWNSCALE -> undistort -> equalise / CLAHE -> detect (the ORB detector of that loop included, which sits behind the stage).  The
 * depth image, by the depth rule above: on the space map's queue behind the upload and ahead of the depth undistortion and the bilateral
 * filter, once per frame, inside the captured launch sequence (VSLAM_RGBD_GRAPH=1) as well; toggling drops the captured sequence.
 * vslam_rgbd_set_downscale: as vslam_set_downscale, with vslam_rgbd_set_undistortion in the place of vslam_set_rectification (the same
 *   size check in both setters); the frame entries then take image AND depth image of full_rows x full_cols.  Host frames are copied to
 *   full-size staging of the stage's own; caller device images are only read (depth images of a batch need no dense stream stride while
 *   the switch is on).  VSLAM_ERR_STATE with a frame in flight, and on the host-driven loop (VSLAM_RGBD_HOST=1), which does not get the
 *   feature.  The switch survives vslam_rgbd_reset.
 * vslam_rgbd_get_downscale: the switch in force; factor 1, sizes 0 while off (and on the host-driven loop).
 * vslam_rgbd_get_downscaled: the reduced image and depth image of the last finished frame of `stream` (dense, full / factor; either may
 *   be NULL); VSLAM_ERR_STATE when off, before a frame, after a reset, with a frame in flight.  With equalisation on and undistortion off
 *   the image is equalised in place afterwards and this getter returns the equalised image. */
struct vslam_rgbd;
int vslam_rgbd_set_downscale(struct vslam_rgbd* t, int32_t factor, int32_t full_rows, int32_t full_cols);
int vslam_rgbd_get_downscale(struct vslam_rgbd* t, int32_t* factor, int32_t* full_rows, int32_t* full_cols);
int vslam_rgbd_get_downscaled(struct vslam_rgbd* t, int32_t stream, uint8_t* image /* may be NULL */, uint16_t* depth /* may be NULL */);
int vslam_downscale_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int32_t factor, uint8_t* dst,
                       int32_t dst_row_stride);
int vslam_downscale_depth_u16(vslam_ctx* ctx, const uint16_t* src, int32_t rows, int32_t cols, int32_t row_stride /* elements */,
                              int32_t factor, uint16_t* dst, int32_t dst_row_stride);
/* ---- smoothing of the intensity image: Gaussian and median (opt-in; csrc/kernels_smooth.h, smooth.py) --------------------
 * Noise suppression on the 8-bit grey image ahead of the equalisation slot and the detector.  All integer, bit-exact by definition:
 *   VSLAM_SMOOTH_GAUSSIAN, ksize 3, 5 or 7: taps K in 1/256 — {64,128,64}, {16,64,96,64,16}, {8,28,56,72,56,28,8} —
 *     out = (sum_i sum_j K_i K_j p(y+i-r, x+j-r) + 32768) >> 16, r = ksize / 2, rows and columns reflected without edge duplication
 *     (index -1 -> 1).  This is cv::GaussianBlur(src, dst, Size(k, k), 0) on CV_8UC1 with BORDER_REFLECT_101 [recalled; parity with OpenCV
 *     is not pinned, the integer definition is].  It needs rows > r and cols > r.
 *   VSLAM_SMOOTH_MEDIAN, ksize 3 or 5: element k k / 2 of the sorted k x k window, the border replicated (cv::medianBlur [recalled]); any
 *     size from 1 x 1.
 * The chain: colour -> grey -> downscale -> rectify -> SMOOTH -> equalise / CLAHE -> detect.  The histogram and the CLAHE tables are
 * built from the smoothed pair; masks, FAST, the descriptors, the recovery and the ORB extractor read the smoothed (then equalised) pair;
 * map colours keep sampling the colour source.  One launch (k_smooth) per frame on the image pipeline's queue, all streams and both sides;
 * a switched-off stream is neither read nor written; a caller's device pair is only read.  The stage never works in place.
 * vslam_set_smoothing: mode VSLAM_SMOOTH_OFF frees the stage's buffers (ksize is then ignored).  VSLAM_ERR_INVALID for an unknown mode,
 *   a ksize the mode does not have (nothing changes; the Gaussian's size refusal can only be met through vslam_smooth_u8: a context is
 *   never that small); VSLAM_ERR_STATE inside a frame
 *   of the stage path.  Nothing is allocated or launched while off.  The switch survives vslam_reset.
 * vslam_get_smoothing: the switch in force; ksize 0 while off.
 * vslam_get_smoothed_images: the smoothed pair of the last submitted frame of `stream` (rows x cols, dense), ahead of the equalisation;
 *   VSLAM_ERR_STATE while off, before a frame has run under the switch, after vslam_reset.  Synchronises.  While the switch is on,
 *   vslam_get_rectified_images / _downscaled_images / _gray_images return the pair ahead of the smoothing: no later stage touches it.
 * vslam_smooth_u8: the kernel stand-alone on one host image, dense dst (rows x cols).  rows or cols 0: VSLAM_OK, nothing written.
 *   VSLAM_ERR_INVALID as above, for a null pointer and for row_stride < cols. */
#define VSLAM_SMOOTH_OFF 0
#define VSLAM_SMOOTH_GAUSSIAN 1
#define VSLAM_SMOOTH_MEDIAN 2
int vslam_set_smoothing(vslam_ctx* ctx, int mode, int32_t ksize);
int vslam_get_smoothing(vslam_ctx* ctx, int* mode, int32_t* ksize);
int vslam_get_smoothed_images(vslam_ctx* ctx, int stream, uint8_t* left, uint8_t* right);
int vslam_smooth_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int mode, int32_t ksize, uint8_t* dst);
/* The same stage in RGB-D mode (the device-resident loop): colour -> grey -> downscale -> undistort -> SMOOTH -> equalise / CLAHE ->
 * detect (the ORB detector of that loop included: its pyramid is built from the smoothed, equalised image).  Only the intensity image is
 * smoothed; the depth image is untouched.  Once per frame on the image queue (further registration attempts read the smoothed image
 * again), inside the captured launch sequence (VSLAM_RGBD_GRAPH=1) as well; toggling drops the captured sequence.
 * vslam_rgbd_set_smoothing: as vslam_set_smoothing; VSLAM_ERR_STATE with a frame in flight, and on the host-driven loop
 *   (VSLAM_RGBD_HOST=1), which does not get the stage.  The switch survives vslam_rgbd_reset.
 * vslam_rgbd_get_smoothing: the switch in force; OFF and 0 on the host-driven loop.
 * vslam_rgbd_get_smoothed: the smoothed image of the last finished frame of `stream` (dense); VSLAM_ERR_STATE when off, before a frame,
 *   after a reset, with a frame in flight.  With the equalisation slot on the image is equalised in place afterwards and this getter
 *   returns the equalised image, like vslam_rgbd_get_undistorted. */
int vslam_rgbd_set_smoothing(struct vslam_rgbd* t, int mode, int32_t ksize);
int vslam_rgbd_get_smoothing(struct vslam_rgbd* t, int* mode, int32_t* ksize);
int vslam_rgbd_get_smoothed(struct vslam_rgbd* t, int32_t stream, uint8_t* image);
/* ---- detection masks: keep keypoints off masked pixels (opt-in; csrc/kernels_mask.h, mask.py) ----------------------------
 * cv::Feature2D::detect(image, keypoints, mask) [recalled]: the detector and its non-maximum suppression run on the whole image, and
 * every keypoint whose pixel reads 0 in the mask is dropped afterwards (KeyPointsFilter::runByPixelsMask), ahead of the count the
 * threshold controller sees.  A mask is an 8-bit single-channel image at the processed size (rows x cols of the context: the rectified
 * image's coordinates while rectification is set), row_stride_bytes >= cols per row; non-zero = keep.  `margin` m, 0 .. 64, erodes the
 * keep-mask by the (2m+1) x (2m+1) square (a pixel stays kept only if every pixel within Chebyshev distance m is kept; pixels outside
 * the image count as kept).  Packed form: (cols + 63) / 64 little-endian 64-bit words per row, bit b of word t = column 64 t + b, bits
 * beyond cols 0.  A context holds a static mask (all streams) and a frame mask (per stream, the next frame only) per image side; the
 * effective keep-mask is their AND, each eroded by its own margin, a missing one all-keep.  It is ANDed into the corner words between
 * k_fast_box and k_emit, on the image pipeline's queue, under the fused entries and the stage path alike; nothing is launched,
 * allocated or copied while no mask is set.  A switched-off stream's mask is neither read nor applied.  The mask governs detection only:
 * landmark recovery and projection tracking sample the image wherever a landmark projects.  vslam_frame_info.n_detected_* are the
 * masked counts, which is what the controller used.
 * vslam_set_detection_mask: the static masks; host pointers, copied and packed before the call returns (it synchronises the context).
 *   Either side may be NULL (unmasked); both NULL switches the static mask off and frees it.  Survives vslam_reset and
 *   vslam_reset_stream(s).
 * vslam_set_frame_masks: n_streams masks per side, stream s at side + s * image_stride_bytes, as the images of vslam_process_* are
 *   addressed; either side may be NULL.  Consumed by the next frame (vslam_process_* or vslam_frame_begin).  Host masks (on_device 0)
 *   are copied on the image pipeline's queue by that frame's call and, like device masks (read in place by that frame's kernel, never
 *   written), must stay valid and unchanged until that frame has been synchronised (vslam_synchronize or any getter).  With more than one
 *   stream image_stride_bytes must hold one mask (VSLAM_ERR_INVALID otherwise).  The kernel loads aligned 32-bit words: of a mask whose
 *   rows do not start on a multiple of four bytes, up to 3 bytes either side of every row are read as well (and ignored).  Both NULL
 *   cancels a pending set, and so does vslam_reset.
 * Both: VSLAM_ERR_STATE between vslam_frame_begin and the end of that frame; VSLAM_ERR_INVALID (not sticky, nothing changed) for a
 *   stride below cols or a margin outside 0 .. 64.  Frames of the fused entries that are still queued are no refusal: the static
 *   setter waits for them (it synchronises), the frame-mask setter only records its arguments for the next frame.
 * vslam_get_detection_mask: the effective packed keep-mask (rows * ((cols + 63) / 64) words) the last submitted frame of `stream` used
 *   on `side` (0 left, 1 right).  Synchronises.  VSLAM_ERR_STATE when that frame used no mask at all or the stream was switched off
 *   during it; VSLAM_ERR_INVALID for a bad
 *   stream, side or a null pointer.
 * vslam_mask_pack_u8: the pack kernel stand-alone on one host image of any size up to 32767 x 32767 (any alignment): `words` receives
 *   rows * ((cols + 63) / 64) words.  rows or cols 0: VSLAM_OK, nothing written.  VSLAM_ERR_INVALID, nothing written: null src / words, a
 *   negative size, a stride below cols, a margin outside 0 .. 64; the context stays usable.
 * The rectification maps' validity mask (k_map_valid in csrc/kernels_mask.h).  k_rectify fills every tap outside the raw
 * image with 0, and FAST fires along the seam between picture and fill.  An output pixel is VALID iff every tap of non-zero weight of
 * its map entry (x0, y0), ax = a & 31, ay = (a >> 5) & 31 lies inside the raw image:
 *   x0 >= 0 and x0 + (ax > 0) <= raw_cols - 1 and y0 >= 0 and y0 + (ay > 0) <= raw_rows - 1
 * (integers; not defined by the remap's result: a missing tap of weight <= 2/1024 rounds away).  Packed and eroded like any mask.
 * vslam_set_rectification_mask: on != 0: the validity words of both sides, computed once from the maps the context holds, become part
 *   of the context-wide keep-mask: static mask AND validity, per side, wherever the static mask applies (both launch sequences, the
 *   stage entries, composed with frame masks); vslam_get_detection_mask returns the words including them, with validity as the only
 *   mask as well.  New maps (vslam_set_rectification) recompute the words, switching rectification off switches this off; it survives
 *   vslam_reset.  VSLAM_ERR_STATE without rectification maps or inside a frame, VSLAM_ERR_INVALID for a margin outside 0 .. 64; nothing
 *   is changed by a refused call.  While off nothing is allocated or launched.  Synchronises the context.
 * vslam_get_rectification_mask: the switch and its margin (0, 0 while off).
 * vslam_map_validity_mask: the kernel stand-alone on one dense host map of rows x cols entries (map_xy [rows][cols][2], map_a [rows]
 *   [cols]) over a raw image of raw_rows x raw_cols: `words` receives rows * ((cols + 63) / 64) words.  VSLAM_ERR_INVALID, nothing
 *   written: a size outside 1 .. 32767, a margin outside 0 .. 64, a null pointer, a map_a value >= 1024; the context stays usable.
 * Not built: masks in the shim (the reference's generator has no mask argument), masks for the stand-alone vslam_fast_detect /
 * vslam_orb_detect entries, validity masks for fisheye maps (the maps themselves are refused). */
#define VSLAM_MASK_MAX_MARGIN 64
int vslam_set_detection_mask(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t row_stride_bytes, int32_t margin);
int vslam_set_frame_masks(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right, int32_t row_stride_bytes, size_t image_stride_bytes,
                          int32_t margin, int on_device);
int vslam_get_detection_mask(vslam_ctx* ctx, int stream, int side, uint64_t* words);
int vslam_mask_pack_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride_bytes, int32_t margin,
                       uint64_t* words);
int vslam_set_rectification_mask(vslam_ctx* ctx, int on, int32_t margin);
int vslam_get_rectification_mask(vslam_ctx* ctx, int* on, int32_t* margin);
int vslam_map_validity_mask(vslam_ctx* ctx, const int16_t* map_xy, const uint16_t* map_a, int32_t rows, int32_t cols, int32_t raw_rows,
                            int32_t raw_cols, int32_t margin, uint64_t* words);
/* Block until all queued work of the context is done; returns the sticky HIP error state (VSLAM_ERR_HIP once a runtime
 * call has failed, else VSLAM_OK; capacity overflows are reported in vslam_frame_info.error_flags, see VSLAM_ERR_CAPACITY). */
int vslam_synchronize(vslam_ctx* ctx);

/* ---- stage entry points (the reference's plug-in virtuals, one call each) ------------------
 * These drive the same device code as vslam_process_* but leave the control flow to the
 * caller (the shim's PoseTracker3D keeps the reference's own logic). All act on every stream. */

/* StereoFramePointGenerator::initialize(frame, extract_features=true)
 * (stereo_framepoint_generator.cpp:73-133): FAST per detector region + threshold controller
 * (base_framepoint_generator.cpp:355-459), BRIEF-32, triangulation-distance rule, feature
 * stores.  Frame::status() of the new frame is the tracker status held in the context. */
int vslam_frame_begin(vslam_ctx* ctx, const uint8_t* left, const uint8_t* right,
                      int32_t row_stride_bytes, size_t image_stride_bytes, int on_device);
/* Second half of the two-call form of vslam_process_*: everything PoseTracker3D::compute does after
 * initialize() (track .. compute), evaluated on the device.  vslam_frame_begin + vslam_frame_finish ==
 * vslam_process_*. */
int vslam_frame_finish(vslam_ctx* ctx);
/* initialize(frame, extract_features=false): rebuild both feature stores (…:128-132). */
int vslam_frame_restore(vslam_ctx* ctx);
/* StereoFramePointGenerator::track (…:464-681) using the tracker state held in the context
 * (prior, window, descriptor distance; setters below). */
int vslam_track(vslam_ctx* ctx, int by_appearance);
/* StereoUVAligner::initialize + converge (stereouv_aligner.cpp:10-69,210-264). */
int vslam_align(vslam_ctx* ctx, int enable_inverse_depth_as_information);
/* PoseTracker3D::_prunePoints + recoverPoints (pose_tracker_3d.cpp:437-472,
 * stereo_framepoint_generator.cpp:683-869). */
int vslam_prune_recover(vslam_ctx* ctx);
/* PoseTracker3D::_updatePoints incl. Landmark create/update (pose_tracker_3d.cpp:475-520,
 * landmark.cpp:8-33,66-167). */
int vslam_update_points(vslam_ctx* ctx);
/* StereoFramePointGenerator::compute (…:135-462). */
int vslam_stereo_new(vslam_ctx* ctx);
int vslam_compute(vslam_ctx* ctx);          /* vslam_update_points + vslam_stereo_new in ONE launch (the shim's compute())  */
/* Tracker-owned state the reference pokes through setters
 * (setProjectionTrackingDistancePixels, setMaximumDescriptorDistanceTracking,
 * base_framepoint_generator.h:166-167; Frame::setRobotToWorld; Frame::setStatus). */
int vslam_set_tracker_state(vslam_ctx* ctx, int stream, int status, const double prior[12],
                            int window_pixels, double tau_track);
int vslam_set_pose(vslam_ctx* ctx, int stream, const double camera_left_to_world[12]);

/* ---- motion models (Parameters::MotionModel, src/types/parameters.h:17-19; pose_tracker_3d.cpp:40-66) ----------------------------
 * The prior a frame of vslam_process_* / vslam_frame_finish starts with.  VSLAM_MOTION_CONSTANT_VELOCITY (the default) keeps the last
 * refined motion and launches nothing new.  VSLAM_MOTION_NONE starts every frame from identity.  VSLAM_MOTION_CAMERA_ODOMETRY takes
 * inverse(guess) * guess_previous from the external pose handed over with every frame (vslam_set_pose_guess*), computed on the device
 * ahead of everything that reads the prior; under it the registration never breaks the track and never retries by appearance with
 * an identity prior: without tracked landmarks, on the third attempt, and in every fallback, the frame's pose is previous *
 * inverse(prior) and the prior is kept (:316-341, :405-417, :551-566).  Such a frame reports fallback = 1 and track_broken = 0.
 * Every stream holds a guess and the previous frame's guess (camera_left_to_world, 3 x 4 row-major), identity after vslam_create,
 * vslam_reset and vslam_reset_stream(s); a frame for which no guess was set re-uses the last one.  Guesses are in the frame of the left
 * camera: a caller with poses of a robot base composes cameraToRobot itself.
 * vslam_set_motion_model: dead_reckoning_limit N > 0 (CAMERA_ODOMETRY only; no reference counterpart): after N
 *   consecutive frames whose pose is not an accepted aligner result a Tracking stream localizes again at the end of the frame, pose
 *   and prior untouched; 0 is off.  Synchronises the context.  VSLAM_ERR_STATE inside a frame; VSLAM_ERR_INVALID (not sticky): unknown
 *   model, negative limit, a limit with another model.  The model survives vslam_reset and vslam_reset_stream(s).  The stage entries
 *   (vslam_track ..) leave the model to their caller, which owns the control flow and sets the prior (vslam_set_tracker_state).
 * vslam_set_pose_guess: the guess of one stream's next frame; host-side, applied at the head of the next frame.
 * vslam_set_pose_guesses: those of all streams, [n_streams][12]; a stream that is switched off when the frame starts is neither read nor
 *   written.  on_device != 0: T is device memory, read on the context's queue at the head of the next frame without a host
 *   synchronisation; the caller keeps it alive and unchanged until that frame is finished.  A guess set for one stream afterwards
 *   takes precedence for that stream.  The array applies to every stream that is active at that frame, one restarted by
 *   vslam_reset_stream(s) in between included; vslam_reset_stream(s) drops only what was set for that stream on the host.
 *   Both: VSLAM_ERR_STATE inside a frame, VSLAM_ERR_INVALID for a bad stream or a null pointer.  Under another model a guess is
 *   stored and ignored: under VSLAM_MOTION_NONE in the stream state; under VSLAM_MOTION_CONSTANT_VELOCITY on the host alone, where
 *   nothing is launched, copied or allocated for it — host guesses wait for the first frame under another model, a device array ends
 *   with the next frame.
 * vslam_get_pose_guess: guess and guess_previous of `stream` as the last frame left them (either may be NULL).  Synchronises.
 * vslam_motion_prior: out[i] = inverse(guess[i]) * guess_previous[i] for n transforms, the arithmetic of the frame start stand-alone. */
typedef enum { VSLAM_MOTION_CONSTANT_VELOCITY = 0, VSLAM_MOTION_NONE = 1, VSLAM_MOTION_CAMERA_ODOMETRY = 2 } vslam_motion_model;
int vslam_set_motion_model(vslam_ctx* ctx, int model, int32_t dead_reckoning_limit);
int vslam_get_motion_model(vslam_ctx* ctx, int* model, int32_t* dead_reckoning_limit);
int vslam_set_pose_guess(vslam_ctx* ctx, int stream, const double camera_left_to_world[12]);
int vslam_set_pose_guesses(vslam_ctx* ctx, const double* camera_left_to_world /* [n_streams][12] */, int on_device);
int vslam_get_pose_guess(vslam_ctx* ctx, int stream, double guess[12], double guess_previous[12]);
int vslam_motion_prior(vslam_ctx* ctx, int32_t n, const double* guess /* [n][12] */, const double* guess_previous /* [n][12] */,
                       double* out /* [n][12] */);

/* ---- readback (synchronises the context stream) -------------------------------------------- */
int vslam_get_frame_info(vslam_ctx* ctx, int stream, vslam_frame_info* out);
/* Frame::keypointsLeft/Right + descriptorsLeft/Right (frame.h:64-67).  xy = (x,y) int16 pairs
 * (FAST keypoints are integer pixels), score = KeyPoint::response, desc = n*32 bytes.
 * Order: image row-major.  Any output pointer may be NULL.  cap = capacity in keypoints. */
int vslam_get_keypoints(vslam_ctx* ctx, int stream, int side, int32_t cap, int32_t* n,
                        int16_t* xy, int32_t* score, uint8_t* desc);
/* Frame::points() of the current frame (frame.h:88-89) as SoA.
 *   kp   : n*4 int16 (xL,yL,xR,yR)              FramePoint::keypointLeft/Right().pt
 *   meta : n*6 int32 (hamming_LR, epipolar_offset, previous_index, track_length,
 *                      landmark_updates, disparity)
 *   cam  : n*3 double  cameraCoordinatesLeft()
 *   lm   : n*3 double  landmark()->coordinates() (world), valid where landmark_updates>0
 *   chi  : n double    StereoUVAligner::errors() of the point (-1 if none), inl: inliers() */
int vslam_get_points(vslam_ctx* ctx, int stream, int32_t cap, int32_t* n, int16_t* kp,
                     int32_t* meta, double* cam, double* lm);
int vslam_get_aligner_result(vslam_ctx* ctx, int stream, int32_t cap, int32_t* n, double* chi,
                             uint8_t* inlier, double T[12], double H[36]);
/* Stage-granular read-backs for a host that keeps the reference's object model (shim/proslam_hip_plugin.h).
 * vslam_get_track_result: what the last vslam_track left — out4 = (index in frame_previous->points(), left feature,
 *   right feature, Hamming L-R) per tracked point in the order of the previous points (feature = index in the row-major
 *   keypoint list of vslam_get_keypoints), lost = indices of the previous points on the lost list
 *   (stereo_framepoint_generator.cpp:659-665).  cap bounds both lists.
 * vslam_get_frame_points: as vslam_get_points, plus the 64 descriptor bytes (left | right) of every point; in_progress = 1
 *   reads the frame the stage calls are assembling (after vslam_prune_recover: survivors of _prunePoints followed by the
 *   recovered points), 0 the finished frame. */
int vslam_get_track_result(vslam_ctx* ctx, int stream, int32_t cap, int32_t* n_tracked, int32_t* out4, int32_t* n_lost,
                           int32_t* lost);
int vslam_get_frame_points(vslam_ctx* ctx, int stream, int in_progress, int32_t cap, int32_t* n, int16_t* kp, int32_t* meta,
                           double* cam, double* lm, uint8_t* desc);
/* ---- landmark map (opt-in; WorldMap::landmarks(), world_map.cpp:74-77, world_map.h:116) --------------------------------------
 * Every landmark a stream creates is kept on the device for the rest of its sequence, indexed by a dense id, as WorldMap::_landmarks
 * keeps it by Landmark::identifier().  Open loop only: no local maps, merging or relocalization.
 * Id rule, per stream and frame, in the order of the frame's points (vslam_get_points):
 *   id = the predecessor's id           if the point has a predecessor (meta previous_index >= 0) that carries an id;
 *   else the stream's next id           if the point carries a landmark (landmark_updates > 0);
 *   else none.
 * Ids start at 0 and follow point order within a frame (Landmark::identifier() of a fresh reference process, by intent).  Entry `id`:
 *   xyz  : 3 double   Landmark::coordinates() (world) after its last update
 *   info : 3 int32    first_frame (the frame that created it), last_frame (its last update, _last_update), updates (landmark_updates
 *                     then, Landmark::_number_of_updates); frame indices are 0-based per stream, as in vslam_get_poses
 *   desc : 32 bytes   left descriptor of the last update (the last entry of Landmark::_descriptors)
 * One kernel behind every frame of vslam_process_* / vslam_frame_finish writes them; the stage calls of the shim (vslam_track ..
 * vslam_compute) and the RGB-D tracker do not.  A context without a map launches nothing for it.
 * vslam_enable_map: allocates `capacity_per_stream` entries per stream and clears every map (a map enabled mid-sequence starts with the
 *   landmarks of the next frame); 0 frees the store and turns the map off.  Synchronises; VSLAM_ERR_STATE inside a frame.  When a
 *   stream's map is full, landmarks created after that get no entry for their whole life, and the frame that refused one reports
 *   error_flags bit 3 (value 8).
 * vslam_reset clears every map, vslam_reset_stream(s) the affected streams' maps; a stream switched off by vslam_set_stream_active
 *   keeps its map unchanged.
 * vslam_get_map_size: entries of `stream`'s map.  vslam_get_map: entries first_id .. first_id + n - 1, n = min(cap, size - first_id)
 *   (a caller fetches what is new since its last call); any output pointer may be NULL.  Both synchronise, VSLAM_ERR_STATE without a
 *   map. */
int vslam_enable_map(vslam_ctx* ctx, int32_t capacity_per_stream);
int vslam_get_map_size(vslam_ctx* ctx, int stream, int32_t* n);
int vslam_get_map(vslam_ctx* ctx, int stream, int32_t first_id, int32_t cap, int32_t* n, double* xyz,
                  int32_t* info /* first_frame, last_frame, updates per entry */, uint8_t* desc);
/* ---- the map's colours (opt-in, on top of the landmark map and colour input; csrc/kernels_map_color.h) ----------------
 * Every map entry gets the colour of its landmark's LEFT keypoint (xL, yL) in the frame's left colour image at the landmark's last update
 * (the frames in which the entry's last_frame is written), as (r, g, b) whatever the input's channel order; alpha is ignored.  While
 * rectification is set the keypoint lies in the rectified image and the colour image is the raw one: each colour plane is then remapped
 * through the left map with vslam_remap_u8's integer arithmetic at that pixel (four taps, taps outside the raw image count as 0).  One
 * kernel (k_map_color) directly behind the map's on the frame queue, on vslam_process_* / vslam_frame_finish.  Integer arithmetic only.
 * vslam_enable_map_colors: needs the map and a colour format (VSLAM_ERR_STATE without either, and inside a frame); synchronises.  Enabled
 *   between frames of a running sequence, an entry reads (0, 0, 0) until its next update; an entry the map refused (capacity) has no
 *   colour.  0 frees the store; so do vslam_enable_map (any capacity: ids start over) and vslam_set_color_input(ctx, VSLAM_PIXEL_GRAY8).
 *   The colours follow the map through vslam_reset and vslam_reset_stream(s); a switched-off stream is neither read nor written.
 *   LIFETIME of device images while the switch is on: the caller's LEFT image passed to vslam_process_device / vslam_frame_begin is read
 *   again behind the frame's last launch, so it must stay valid and unchanged until that frame has ended (vslam_synchronize or any
 *   read-back); host images are copied and may be reused at once, as before.
 * vslam_get_map_colors: rgb of entries first_id .. first_id + n - 1, n = min(cap, size - first_id), like vslam_get_map; rgb may be NULL.
 *   Synchronises; VSLAM_ERR_STATE while the switch is off.
 * vslam_sample_color_u8: the gather stand-alone on one host image (rows x cols pixels, row_stride BYTES per row, any alignment) at n integer
 *   pixels xy = (x, y): direct when both maps are NULL (a pixel outside the image gives (0, 0, 0)), else through the map pair (map_rows x
 *   map_cols, dense, vslam_set_rectification's format; a pixel outside the map gives (0, 0, 0)).  n == 0: VSLAM_OK, nothing written.
 *   VSLAM_ERR_INVALID: null pointers, negative sizes, row_stride < channels * cols, format outside 1 .. 4, one map without the other, a
 *   map_a entry >= 1024; the context stays usable. */
int vslam_enable_map_colors(vslam_ctx* ctx, int on);
int vslam_get_map_colors(vslam_ctx* ctx, int stream, int32_t first_id, int32_t cap, int32_t* n, uint8_t* rgb /* [cap][3] */);
int vslam_sample_color_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride_bytes, int format,
                          const int16_t* map_xy, const uint16_t* map_a, int32_t map_rows, int32_t map_cols, /* both NULL: direct */
                          const int16_t* xy /* [n][2] */, int32_t n, uint8_t* rgb /* [n][3] */);
/* ---- landmark observations (opt-in, on top of the landmark map) -------------------------------------------------------------
 * Which landmark was seen in which frame at which pixels: with vslam_get_poses and vslam_get_map, the input of a mapping or
 * bundle-adjustment back end, written on the device without a host round trip per frame.
 * Rule, per stream and frame: once the frame's map ids are final, every point that carries an id appends one entry to the stream's
 * log, in the order of the frame's points (vslam_get_points).  Entry (16 bytes on the device):
 *   id    : int32      the landmark's map id (entry `id` of vslam_get_map)
 *   frame : int32      0-based per stream, as in vslam_get_poses and the map's first_frame / last_frame
 *   kp    : 4 int16    xL, yL, xR, yR: the point's keypoints, the values vslam_get_points reports as kp
 * The log is sorted by frame, then by point order, and is deterministic.  A landmark's observations start with the frame that
 * created its map entry (first_frame) and end with last_frame: the earlier points of its track, from before
 * minimum_track_length_for_landmark_creation was reached, carry no id and are NOT logged.
 * One kernel behind the map's writes them, on vslam_process_* / vslam_frame_finish; the stage calls of the shim and the RGB-D
 * tracker do not.  A context without a log launches and allocates nothing for it.
 * vslam_enable_observations: allocates `capacity_per_stream` entries per stream and clears every log (a log enabled mid-sequence
 *   starts with the next frame); 0 frees the store and turns the log off.  Synchronises.  VSLAM_ERR_STATE without a map
 *   (vslam_enable_map first) and inside a frame, VSLAM_ERR_INVALID for a negative capacity.  Once a stream's log is full, later
 *   entries are dropped (the log holds exactly the first `capacity` entries), and every frame that dropped one reports error_flags
 *   bit 4 (value 16).
 * The log follows the map: vslam_reset clears every log, vslam_reset_stream(s) the affected streams' logs, a stream switched off by
 *   vslam_set_stream_active keeps its log unchanged; vslam_enable_map(ctx, 0) turns the log off as well, and vslam_enable_map with a
 *   new capacity (ids start at 0 again) clears every log.
 * vslam_get_observation_count: entries of `stream`'s log.  vslam_get_observations: entries first .. first + n - 1,
 *   n = min(cap, count - first) (a caller fetches what is new since its last call); id_frame receives (id, frame) pairs; any output
 *   pointer may be NULL.  Both synchronise, VSLAM_ERR_STATE without a log.
 * vslam_get_point_ids: the map id, or -1, of every point of the finished frame, in vslam_get_points order (e.g. for a viewer that
 *   colours tracks).  Needs the map only, not the log; synchronises; VSLAM_ERR_CAPACITY when cap < n. */
int vslam_enable_observations(vslam_ctx* ctx, int32_t capacity_per_stream);
int vslam_get_observation_count(vslam_ctx* ctx, int stream, int32_t* n);
int vslam_get_observations(vslam_ctx* ctx, int stream, int32_t first, int32_t cap, int32_t* n,
                           int32_t* id_frame /* n*2: id, frame */, int16_t* kp /* n*4: xL, yL, xR, yR */);
int vslam_get_point_ids(vslam_ctx* ctx, int stream, int32_t cap, int32_t* n, int32_t* ids);
/* Pinned (page-locked) host memory.  Host images handed to vslam_process_host / vslam_frame_begin from ordinary (pageable) memory
 * are staged through a pinned buffer of the context first (one memcpy per image, ~30 us per 467 KB); images that already live in
 * memory from vslam_host_alloc (e.g. the cv::Mat a loader decodes into, constructed on such a buffer) are copied to the device
 * directly and asynchronously. */
int vslam_host_alloc(void** out, size_t bytes);
void vslam_host_free(void* p);

/* ---- stage views: zero-copy read-back for a host that keeps the reference's object model --------------------------------------
 * The reference's tracker reads its plug-ins' results after every virtual call (pose_tracker_3d.cpp:32-222: keypoints after
 * initialize(), the tracked list after track(), errors()/inliers() after converge(), Frame::points() after recoverPoints() and
 * compute()).  A vslam_view_* call packs exactly the live elements of that stage's results into a pinned host buffer owned by the
 * context (one small kernel, the GPU writes host memory directly) and synchronises the stream's frame queue ONCE; the pointers it
 * returns stay valid until the next vslam_view_* call on the context (one report buffer per context); the keypoint arrays (coordinates,
 * scores, descriptors) have a region of their own that only the next frame's keypoint report rewrites, so they may still be copied after
 * vslam_track has been LAUNCHED (the shim copies descriptor rows while the device tracks).  Same data, same order and same meaning as the
 * vslam_get_* calls above, which copy array by array. */
typedef struct vslam_keypoints_view {
  int32_t n[2];                /* left, right                                           */
  const int16_t* xy[2];        /* n * (x, y), image row-major                           */
  const uint8_t* score[2];     /* n FAST scores (KeyPoint::response)                    */
  const uint8_t* desc[2];      /* n * 32 descriptor bytes                               */
} vslam_keypoints_view;
typedef struct vslam_track_view {
  int32_t n_tracked, n_lost, n_tracked_landmarks;
  const int32_t* tracked4;     /* as vslam_get_track_result out4                        */
  const int32_t* lost;
} vslam_track_view;
typedef struct vslam_aligner_view {
  int32_t n, n_inliers, n_outliers, iterations, converged;
  double total_error;
  const double* chi;           /* StereoUVAligner::errors()                             */
  const uint8_t* inlier;       /* StereoUVAligner::inliers()                            */
  double T[12], H[36];
} vslam_aligner_view;
typedef struct vslam_points_view {
  int32_t n;
  int32_t first_full;          /* meta / cam / desc are filled for points first_full .. n-1: 0 for the finished frame; for the frame in
                                  assembly (in_progress = 1) the number of survivors of the prune — those are objects the caller already
                                  holds, only the recovered points behind them are new                                                  */
  const int16_t* kp;           /* n * (xL, yL, xR, yR), every point                     */
  const int32_t* meta;         /* n * 6, the layout of vslam_get_points                 */
  const double* cam;           /* n * 3                                                 */
  const uint8_t* desc;         /* n * 64 (left | right); in_progress = 1 only, else NULL (the finished frame's new points carry the
                                  descriptors of the caller's own features)             */
  vslam_frame_info info;       /* the stream's report as of this stage                  */
  /* in-kernel chronometers of the stream, accumulated seconds (the tracker-side five of vslam_get_timers) */
  double seconds_tracking, seconds_pose_optimization, seconds_point_recovery, seconds_landmark_optimization, seconds_point_triangulation;
} vslam_points_view;
int vslam_view_keypoints(vslam_ctx* ctx, int stream, vslam_keypoints_view* out);            /* after vslam_frame_begin    */
/* The same with desc[] = NULL, as soon as the detector has written coordinates and scores (the descriptors are still being computed): a
 * caller builds its cv::KeyPoint lists meanwhile and fetches the descriptors with vslam_view_keypoints afterwards.  One-stream contexts
 * inside a frame; anywhere else it is vslam_view_keypoints. */
int vslam_view_keypoints_xy(vslam_ctx* ctx, int stream, vslam_keypoints_view* out);
int vslam_view_track(vslam_ctx* ctx, int stream, vslam_track_view* out);                    /* after vslam_track          */
int vslam_view_aligner(vslam_ctx* ctx, int stream, vslam_aligner_view* out);                /* after vslam_align          */
int vslam_view_points(vslam_ctx* ctx, int stream, int in_progress, vslam_points_view* out); /* after vslam_prune_recover (1) / vslam_stereo_new (0) */
/* StereoUVAligner::_weights_translation as the stream's last initialize() left it (stereouv_aligner.cpp:22,57-61): the
 * vector is a MEMBER of the aligner, `resize(n, 1)` keeps the elements it already holds, and they are rewritten only while
 * enable_inverse_depth_as_information is set — so Localizing frames (flag off, pose_tracker_3d.cpp:124) reuse the weights the
 * last Tracking frame left at the same indices.  n = the vector's size. */
int vslam_get_aligner_weights(vslam_ctx* ctx, int stream, int32_t cap, int32_t* n, double* weight);
/* The 8 chronometers SLAMAssembly::printReport prints (slam_assembly.cpp:703-742), seconds of
 * device time accumulated per stage over all streams (HIP events): keypoint_detection,
 * descriptor_extraction, point_triangulation, tracking, track_creation, pose_optimization,
 * landmark_optimization, point_recovery. */
int vslam_get_timers(vslam_ctx* ctx, double seconds[8]);
int vslam_enable_timers(vslam_ctx* ctx, int on);
/* Per-kernel device time (HIP events on the context stream, recorded while timers are enabled):
 * accumulated milliseconds and launch counts of k_fast_box, k_emit, k_brief, k_track_candidates, k_frame (its
 * phase launches together, counted once), k_recover_brief, slot 6 (reserved, always 0: it timed k_update_landmarks,
 * a kernel no launch sequence uses any more), k_stereo_dist.
 * Used by bench.py for the roofline of the dominant kernel.  Synchronises; vslam_enable_timers(ctx,1)
 * clears the accumulators.  Stage path of a one-stream context (vslam_frame_begin): the image pipeline is timed by three events
 * instead of two per kernel, so k_fast_box's figure covers k_emit as well (ms[0] + ms[1] = keypoint detection either way) and
 * k_stereo_dist is not timed. */
int vslam_get_kernel_times(vslam_ctx* ctx, double ms[8], int32_t launches[8]);

/* ---- stand-alone kernels (unit parity, and the reference's optional knnMatch block) -------- */
/* cv::FastFeatureDetector::detect on one ROI (base_framepoint_generator.cpp:12-25,367):
 * FAST-9/16, non-max suppression, output row-major, coordinates relative to the ROI. */
int vslam_fast_detect(vslam_ctx* ctx, const uint8_t* image_host, int32_t rows, int32_t cols,
                      int32_t stride, int32_t roi_x, int32_t roi_y, int32_t roi_w, int32_t roi_h,
                      int32_t threshold, int32_t cap, int32_t* n, int16_t* xy, int32_t* score);
/* _descriptor_extractor->compute (base_framepoint_generator.cpp:431-438): BRIEF-32 at given
 * integer keypoints; keypoints closer than 28 px to the border are removed (keep[i]=0). */
int vslam_brief_describe(vslam_ctx* ctx, const uint8_t* image_host, int32_t rows, int32_t cols,
                         int32_t stride, int32_t n, const int16_t* xy, uint8_t* keep, uint8_t* desc);
/* matcher->knnMatch(query, train, k=2) of the use_matches block (stereo_framepoint_generator.cpp:168-206); the matcher type
 * selects the norm (:175-197).  norm: 0 = NORM_HAMMING on the bits (BRUTEFORCE_HAMMING), 1 = NORM_L2 on the bytes converted
 * to float (convertTo(CV_32F) + BRUTEFORCE), 2 = NORM_L1 (BRUTEFORCE_L1), 3 = squared L2 (BRUTEFORCE_SL2).
 * idx: nq*2 int32 (-1 if fewer than 2 train rows), dist: nq*2 float. Ties -> lowest index. */
int vslam_knn2(vslam_ctx* ctx, int norm, int32_t nq, const uint8_t* query, int32_t nt,
               const uint8_t* train, int32_t* idx, float* dist);
/* StereoUVAligner on caller-provided correspondences (stereouv_aligner.cpp:72-264):
 * moving n*3, fixed n*4, omega n, weight n. */
int vslam_align_points(vslam_ctx* ctx, int32_t n, const double* moving, const double* fixed,
                       const double* omega, const double* weight, const double T_init[12],
                       double T_out[12], double* chi, uint8_t* inlier, int32_t* n_inliers,
                       double* total_error, int32_t* iterations, double H_out[36]);

/* The translation weights over a sequence of StereoUVAligner::initialize calls on ONE aligner object
 * (stereouv_aligner.cpp:22,57-61), for known-answer tests: call k has n[k] measurements with depths depth[off_k ..]
 * (off_k = n[0] + .. + n[k-1]) and the flag inverse_depth[k]; out receives the n[k] weights in effect after call k.
 * Runs the weight rule of the fused tracker's aligner (maximum_reliable_depth_meters of ctx's config). */
int vslam_aligner_weights(vslam_ctx* ctx, int32_t n_calls, const int32_t* n, const int32_t* inverse_depth,
                          const double* depth, double* out);

/* UVDAligner (RGB-D mode, uvd_aligner.cpp:72-232) on caller-provided correspondences: moving n*3 (previous camera
 * coordinates), fixed n*3 (u, v, depth), omega_uv n and omega_depth n (the diagonal of the information matrix:
 * uvd_aligner.cpp:28-61 sets (1 + landmark updates) and 10x that, or 0 for unreliable depth), weight n (translation
 * weight).  Same solver, damping, convergence rule and outputs as vslam_align_points; inlier-only rounds need more
 * than 100 inliers (uvd_aligner.cpp:211).  SURVEY.md 8f row 4, first half. */
int vslam_align_points_uvd(vslam_ctx* ctx, int32_t n, const double* moving, const double* fixed_uvd,
                           const double* omega_uv, const double* omega_depth, const double* weight,
                           const double T_init[12], double T_out[12], double* chi, uint8_t* inlier,
                           int32_t* n_inliers, double* total_error, int32_t* iterations, double H_out[36]);
/* StereoFramePointGenerator::track (stereo_framepoint_generator.cpp:464-681, with
 * IntensityFeatureMatcher::getMatchingFeatureInRectangularRegion, intensity_feature_matcher.cpp:81-148) on
 * caller-provided data, for known-answer tests: nP previous points (left-camera coordinates n*3, left / right
 * descriptors n*32, epipolar offsets), motion prior T, window d, the feature sets of the current images as
 * (row, col) pairs + descriptors (one feature per pixel).  Geometry (rows, cols, K, baseline) from ctx's config.
 * out4 = (previous index, left feature, right feature, L-R distance) per tracked point in the order of the
 * previous points, cap nP; lost = indices of the previous points that go to the lost list, cap nP. */
int vslam_track_match(vslam_ctx* ctx, const double T[12], int32_t d, double tau_track, double tau_tri,
                      int32_t by_appearance, int32_t nP, const double* cam, const uint8_t* prev_desc_left,
                      const uint8_t* prev_desc_right, const int32_t* epipolar_offset, int32_t nL,
                      const int32_t* rc_left, const uint8_t* desc_left, int32_t nR, const int32_t* rc_right,
                      const uint8_t* desc_right, int32_t* n_tracked, int32_t* out4, int32_t* n_lost, int32_t* lost);

/* StereoFramePointGenerator::compute (stereo_framepoint_generator.cpp:135-462: epipolar sweep over the configured
 * offsets, ordering constraint, minimum disparity, bin competition if enabled in ctx's config) on caller-provided
 * feature sets ((row, col) pairs + descriptors, one feature per pixel), for known-answer tests.
 * out4 = (left feature, right feature, L-R distance, epipolar offset) per new framepoint in emission order. */
int vslam_stereo_match(vslam_ctx* ctx, double tau_tri, int32_t nL, const int32_t* rc_left, const uint8_t* desc_left,
                       int32_t nR, const int32_t* rc_right, const uint8_t* desc_right, int32_t cap, int32_t* n_out,
                       int32_t* out4);

/* StereoFramePointGenerator::recoverPoints (stereo_framepoint_generator.cpp:683-869) on caller-provided data, for known-answer
 * tests: n lost points (landmark flag, landmark world coordinates n*3, last left / right descriptors n*32), the frame's
 * world_to_camera_left and both images (ctx's image size, geometry, depth and disparity limits, descriptor type).  Per lost point
 * in list order: projection into both cameras (:704-745), depth and 5 * keypoint.size border gates (:746-764), descriptors at the
 * rounded projections, the three descriptor gates and the minimum disparity (:773-842).  Outputs (cap n) in list order:
 * rec_index = position in the lost list, rec_xy4 = (xL, yL, xR, yR), rec_dist = left-right distance, rec_desc = left | right
 * descriptor (64 B), rec_xyz = triangulated left-camera coordinates (:871-895). */
int vslam_stereo_recover(vslam_ctx* ctx, const uint8_t* image_left, const uint8_t* image_right, int32_t row_stride,
                         const double world_to_camera[12], int32_t n, const uint8_t* has_landmark, const double* landmark_world,
                         const uint8_t* prev_desc_left, const uint8_t* prev_desc_right, double tau_track, double tau_tri,
                         int32_t* n_recovered, int32_t* rec_index, int32_t* rec_xy4, int32_t* rec_dist, uint8_t* rec_desc,
                         double* rec_xyz);

/* Landmark::update (types/landmark.cpp:66-167) for n landmarks, stand-alone (the fused tracker runs the same refinement inside
 * its frame kernel): landmark i owns the measurements offsets[i] .. offsets[i+1]-1 in the caller's order, the LAST one being
 * the new observation; measurement m was taken in frame frame_of[m] (pose tables world_to_camera / camera_to_world, 3x4 each)
 * at left-camera coordinates cam[m] with information 1 / cam[m].z (landmark.h:22-36).  Gauss-Newton on the world position
 * with the saturated kernel (landmark_maximum_error_squared_meters, landmark_maximum_number_of_iterations of ctx's config),
 * 3x3 full-pivot LU; on convergence the estimate is taken if it has more inliers than the landmark had updates, reset to the
 * mean of the measurements if inliers < outliers, kept otherwise.  world (n*3) and updates (n) are read and written. */
int vslam_landmark_update(vslam_ctx* ctx, int32_t n, const int32_t* offsets, const int32_t* frame_of, int32_t n_frames,
                          const double* world_to_camera, const double* camera_to_world, const double* cam, double* world,
                          int32_t* updates);

/* ---- RGB-D components: the pieces of DepthFramePointGenerator, stand-alone -----------------
 * Not wired into the fused stereo tracker; same role as vslam_align_points_uvd (the RGB-D aligner): the kernels a
 * depth-mode shim calls, each checked against the oracle and an independent fixture. */
typedef struct vslam_depth_params {
  int32_t rows, cols;
  double K_left[9];             /* _camera_left->cameraMatrix(), row-major                                        */
  double K_left_inverse[9];     /* its inverse as the caller's linear algebra gives it (Eigen .inverse() upstream) */
  double K_right_inverse[9];    /* inverse of the depth camera's matrix (depth_framepoint_generator.cpp:443)      */
  double right_to_left[12];     /* _camera_left->robotToCamera()*_camera_right->cameraToRobot() (:446), 3x4       */
  double depth_scale_factor_intensity_to_meters;       /* parameters.h:251 (1e-3)                               */
  double minimum_depth_meters, maximum_depth_meters;    /* parameters.h:197-198                                   */
  int32_t enable_point_triangulation;                   /* parameters.h:256                                       */
  int32_t enable_keypoint_binning, bin_size_pixels;     /* base generator parameters                              */
  int32_t descriptor_type;                              /* extractor of recoverPoints: VSLAM_DESCRIPTOR_BRIEF / _ORB (the RGB-D
                                                           configurations say "ORB-256", i.e. cv::ORB::create())   */
  int32_t detector_type;                                /* vslam_rgbd_*: VSLAM_DETECTOR_FAST (every shipped configuration) or
                                                           VSLAM_DETECTOR_ORB = OrbDetector, cv::ORB::create(5000, 1.2, 8, 31, 0, 2,
                                                           HARRIS_SCORE, 31, threshold) per detector region
                                                           (base_framepoint_generator.cpp:52-70, :242-247; parameters.cpp:341)  */
} vslam_depth_params;
#define VSLAM_DETECTOR_FAST 0
#define VSLAM_DETECTOR_ORB 1

/* DepthFramePointGenerator::_computeDepthMap (depth_framepoint_generator.cpp:410-485) behind its optional bilateral
 * filter (that step is vslam_bilateral_depth_u16 / vslam_rgbd_set_bilateral below; this entry maps the image it is given): every non-zero u16 depth pixel is back-projected through K_right_inverse, moved into the left camera,
 * projected with K_left and z-buffered (strict "stored float > new double", scan order) into the rows x cols x 3 float
 * space map, initialised to (0, 0, maximum_depth); row_map / col_map receive the winning source pixel (-1: none).
 * depth: host image, row stride in ELEMENTS.  Outputs may be NULL; the map also stays resident in the context for
 * vslam_depth_compute. */
int vslam_depth_space_map(vslam_ctx* ctx, const vslam_depth_params* p, const uint16_t* depth, int32_t row_stride,
                          float* space_map, int16_t* row_map, int16_t* col_map);

/* DepthFramePointGenerator::compute (:45-164) on caller-provided features: rc_features = nF (row, col) pairs in the
 * feature vector's order (row-major sorted), rc_tracked = nT (row, col) of the framepoints the frame already holds
 * (tracked / recovered: they own their bin).  space_map: host map (rows*cols*3 floats) or NULL = the one the last
 * vslam_depth_space_map call left in the context.  New points (measured depth) come back in emission order — bin grid
 * row-major when binning is on (lower depth wins an untracked bin, first wins ties), feature order otherwise — as
 * feature index + left-camera coordinates; temporary points (depth >= maximum and triangulation enabled, :84-96) in
 * feature order with the coordinates K_left_inverse * (col*max, row*max, max).  cap bounds both lists. */
int vslam_depth_compute(vslam_ctx* ctx, const vslam_depth_params* p, const float* space_map, int32_t nF,
                        const int32_t* rc_features, int32_t nT, const int32_t* rc_tracked, int32_t cap, int32_t* n_new,
                        int32_t* new_feature, double* new_xyz, int32_t* n_temporary, int32_t* temporary_feature,
                        double* temporary_xyz);

/* DepthFramePointGenerator::track (:166-287) on caller-provided data: the previous frame's points followed by its
 * temporary points (:181-184) as left-camera coordinates cam (nP*3), left descriptors (nP*32) and flags (bit 0: has a
 * landmark, bit 1: hasUnreliableDepth); the motion prior T (previous -> current camera), the search window d, the
 * descriptor threshold tau (minimum_descriptor_distance_tracking in the reference) and the search mode; the current left
 * features as (row, col) pairs + descriptors (one feature per pixel); the space map as in vslam_depth_compute.
 * Outputs, all in the order of the previous points (the greedy, order-dependent outcome of the serial loop, reproduced
 * exactly): out2 = (previous index, left feature) of the tracked points with their measured coordinates xyz; temp2 = the
 * same pairs for matches on pixels without depth (temporary points, triangulation enabled); lost = previous points that go
 * to the lost list (:281-284).  Every list has room for nP entries. */
int vslam_depth_track(vslam_ctx* ctx, const vslam_depth_params* p, const float* space_map, const double T[12], int32_t d,
                      double tau, int32_t by_appearance, int32_t nP, const double* cam, const uint8_t* previous_desc,
                      const uint8_t* previous_flags, int32_t nL, const int32_t* rc_left, const uint8_t* desc_left,
                      int32_t* n_tracked, int32_t* out2, double* xyz, int32_t* n_temporary, int32_t* temp2, int32_t* n_lost,
                      int32_t* lost, int32_t* n_tracked_landmarks);

/* DepthFramePointGenerator::recoverPoints (:289-407) on caller-provided data: the lost points' landmarks in world
 * coordinates (n*3; has_landmark[i] = 0 skips the point as :305 does), their last left descriptors (n*32), the frame's
 * world_to_camera_left (3x4), the LEFT intensity image (host, u8) and the keypoint size (7 for FAST; the search border is
 * 5*size + 1 px).  A landmark is recovered when it projects into the image, its pixel (rint of the projection) has a
 * measured depth in [minimum, maximum), the projection keeps the border and BRIEF at the projection — the ROI origin is
 * the rounded corner, cv::Rect_<float> -> cv::Rect — is within tau of the previous descriptor.  Outputs in the order of
 * the lost list, room for n entries each: rec_index (position in the lost list), rec_xy (the new keypoint: the sub-pixel
 * projection as the reference's float arithmetic leaves it), rec_desc, rec_xyz (the space-map entry).  A projection whose
 * rounded pixel falls outside the map (x == cols or y == rows: an out-of-bounds read upstream) is skipped. */
int vslam_depth_recover(vslam_ctx* ctx, const vslam_depth_params* p, const float* space_map, const uint8_t* image_left,
                        int32_t row_stride, const double world_to_camera_left[12], int32_t n, const uint8_t* has_landmark,
                        const double* landmark_world, const uint8_t* previous_desc, float keypoint_size, double tau,
                        int32_t* n_recovered, int32_t* rec_index, float* rec_xy, uint8_t* rec_desc, double* rec_xyz);

/* BaseFramePointGenerator::getPointInCamera (base_framepoint_generator.cpp:461-494) for n point pairs: midpoint
 * triangulation of a previous / current image point pair under the motion T (previous -> current camera); the 3x2
 * least-squares problem is solved through its singular value decomposition (minimum-norm for a rank-deficient pair).
 * xy_*: n*2 floats; out: n*3 doubles.  Floating point: agrees with the reference's JacobiSVD to rounding (tests: 1e-9). */
int vslam_point_in_camera(vslam_ctx* ctx, int32_t n, const float* xy_previous, const float* xy_current,
                          const double T[12], const double K[9], double* out);

/* ---- ORB as descriptor extractor (second half; base_framepoint_generator.cpp:190-196,219-224) -------
 * cv::ORB::create()->compute(image, keypoints, descriptors) on provided keypoints, restated [recalled, OpenCV 3.x orb.cpp
 * detectAndCompute with useProvidedKeypoints]: keypoints closer than 31 px to the border are removed, the image (level 0:
 * FAST keypoints carry octave 0) is blurred with GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) — 8-bit fixed-point
 * separable filter, kernel round(256 k) = {18, 34, 49, 55, 49, 34, 18}, result (sum + 2^15) >> 16 — and every keypoint gets
 * 256 steered tests I(c + R p1) < I(c + R p2), R = rotation by KeyPoint::angle (degrees; float arithmetic, cvRound), bit k
 * of byte i = test 8i + k.  The 256 pairs are REPO-DEFINED (include/vslam_orb_pattern.h; OpenCV's bit_pattern_31_ is not
 * in the reference tree).  vslam_gaussian_blur7_u8: host image in, host image out (dense, cols bytes per row); rows, cols >= 4
 * (one reflection per border).
 * vslam_orb_describe: n integer keypoints xy with one angle for all (FAST: -1), keep[i] = 0 for removed keypoints. */
int vslam_gaussian_blur7_u8(vslam_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t row_stride, uint8_t* blurred);

/* ---- the descriptor test pairs are DATA ------------------------------------------------------------------------------------
 * BRIEF-32 and ORB each compare 256 fixed pixel pairs.  OpenCV's tables (xfeatures2d generated_32.i; features2d orb.cpp
 * bit_pattern_31_) are not in the reference tree, so this library ships tables of its own (include/vslam_brief_pattern.h,
 * vslam_orb_pattern.h): same construction, different numbers — descriptors are NOT bit-compatible with an OpenCV build until
 * the caller passes OpenCV's tables in.  An integration that has them (shim/proslam_hip_plugin.h: HipContext::brief_pattern /
 * orb_pattern) calls these once before the first frame; maps, relocalization data and Hamming thresholds tuned on OpenCV
 * descriptors then keep their meaning.
 *   BRIEF pair i = {y1, x1, y2, x2}: bit i (byte i / 8, MSB first) = box9x9(p + (x1, y1)) < box9x9(p + (x2, y2)); |.| <= 24.
 *   ORB   pair i = {x1, y1, x2, y2}: bit i (byte i / 8, LSB first) = I(c + R (x1, y1)) < I(c + R (x2, y2)); |x|, |y| <= 15, the
 *   31 x 31 patch (OpenCV's bit_pattern_31_, whose points reach radius 17.7, fits).
 * The tables live in the device's constant memory: the setting holds for every context on `device` in this process.  Call
 * them while no frame is in flight.  vslam_get_*_pattern returns the table in effect (256 * 4 bytes). */
int vslam_set_brief_pattern(int device, const int8_t* pairs_y1x1y2x2 /* 256 * 4 */);
int vslam_set_orb_pattern(int device, const int8_t* pairs_x1y1x2y2 /* 256 * 4 */);
int vslam_get_brief_pattern(int device, int8_t* pairs_out /* 256 * 4 */);
int vslam_get_orb_pattern(int device, int8_t* pairs_out /* 256 * 4 */);
int vslam_orb_describe(vslam_ctx* ctx, const uint8_t* image_host, int32_t rows, int32_t cols, int32_t stride, int32_t n,
                       const int16_t* xy, float angle_degrees, uint8_t* keep, uint8_t* desc);

/* ---- RGB-D mode end to end: PoseTracker3D with DepthFramePointGenerator + UVDAligner ---------------
 * (slam_assembly.cpp _createDepthTracker; configuration_{icl,tum,xtion}.yaml).  Two implementations inside the library, same results
 * frame by frame: the device-resident loop (csrc/kernels_rgbd.h + csrc/rgbd_device.h, the default: framepoints, temporary points,
 * landmarks, history and the tracker's scalars live in HBM; a frame is two copies in, one launch sequence on two HIP streams and one
 * 1 KB state block out) and the host-driven loop over the stand-alone entry points above (csrc/rgbd_tracker.h: VSLAM_RGBD_HOST=1 in the
 * environment of vslam_rgbd_create), kept as the cross-check.  Both serve p->detector_type = VSLAM_DETECTOR_FAST and _ORB: with the
 * OrbDetector the device-resident loop runs every region's pyramid, FAST, the two retainBest selects, Harris and angles, the extractor
 * (ORB::compute on the keypoint's own level and angle, or BRIEF at level 0) and a feature store of float keypoints on the frame's queue
 * (csrc/kernels_rgbd_orb.h), so batches, the captured launch sequence, the map, the log, map colours and every input
 * stage below work with it; the detection masks alone are refused in that mode (VSLAM_ERR_STATE, the context stays usable).  A detector
 * grid above 2 x 2 with the OrbDetector (regions of different sizes) selects the host-driven loop.  One sequence per object, any detector
 * grid (configuration_icl.yaml: 2 x 2).  cfg carries the tracker / aligner / landmark / detector values, p the depth camera
 * (p->descriptor_type selects the extractor: the RGB-D configurations say "ORB-256").  A frame that fails (capacity, HIP error) leaves
 * the tracker refusing further frames until vslam_rgbd_reset (the reference throws out of compute() and the run ends, app.cpp:128).
 * vslam_rgbd_process_host = PoseTracker3D::compute for one frame: left = 8-bit image, depth = 16-bit depth image (row
 * strides in bytes / in elements).  vslam_rgbd_get_frame_info fills the counters that exist in this mode (n_keypoints_left,
 * n_detected_left, thresholds[region], track_attempts, n_tracked, n_lost, n_tracked_landmarks, aligner_*, n_inliers, n_after_prune,
 * n_recovered, n_active_landmarks, n_new_stereo = new points with measured depth, n_points, window_pixels, tau_track, status,
 * poses) and the number of temporary points of the frame.  vslam_rgbd_get_points: Frame::points() as xy (float: recovered
 * points sit at sub-pixel projections), cam, meta = (index of the predecessor in the previous frame's points followed by its
 * temporary points or -1, track length, landmark updates or 0, hasUnreliableDepth), 32 descriptor bytes. */
typedef struct vslam_rgbd vslam_rgbd;
int vslam_rgbd_create(const vslam_config* cfg, const vslam_depth_params* p, int device, vslam_rgbd** out);
void vslam_rgbd_destroy(vslam_rgbd* t);
int vslam_rgbd_reset(vslam_rgbd* t);
const char* vslam_rgbd_last_error(const vslam_rgbd* t);
int vslam_rgbd_process_host(vslam_rgbd* t, const uint8_t* left, int32_t left_row_stride, const uint16_t* depth, int32_t depth_row_stride);
/* vslam_rgbd_process_host in two halves: submit copies the frame in and enqueues its kernels, wait returns its status (after it the frame's
 * info and points can be read; between submit and wait the getters return VSLAM_ERR_STATE: the frame in flight is rewriting the lists they
 * would copy).  One frame in flight per tracker.  Several trackers — one sequence each, HIP streams of their own — overlap
 * on the GPU when their frames are submitted before any of them is waited for (tests/validation/rgbd_bench.py --trackers). */
int vslam_rgbd_submit_host(vslam_rgbd* t, const uint8_t* left, int32_t left_row_stride, const uint16_t* depth, int32_t depth_row_stride);
int vslam_rgbd_wait(vslam_rgbd* t);
/* Several sequences in ONE context (device-resident loop only): n_streams independent sequences of the same camera and configuration advance
 * together, one frame each per call — the launch sequence of a frame serves all of them (one workgroup per sequence in its single-workgroup
 * kernels, a grid dimension in the wide ones), so a step costs the time of its slowest sequence (tests/validation/rgbd_batch.py).  Images: n_streams
 * images `left_stream_stride` bytes apart, depth images `depth_stream_stride` ELEMENTS apart.  A sequence that needs another registration attempt
 * gets it without disturbing the others.  Results per sequence through the *_stream getters. */
int vslam_rgbd_create_batch(const vslam_config* cfg, const vslam_depth_params* p, int device, int32_t n_streams, vslam_rgbd** out);
int vslam_rgbd_process_batch_host(vslam_rgbd* t, const uint8_t* left, int32_t left_row_stride, size_t left_stream_stride, const uint16_t* depth,
                                  int32_t depth_row_stride, size_t depth_stream_stride);
int vslam_rgbd_submit_batch_host(vslam_rgbd* t, const uint8_t* left, int32_t left_row_stride, size_t left_stream_stride, const uint16_t* depth,
                                 int32_t depth_row_stride, size_t depth_stream_stride);   /* then vslam_rgbd_wait */
/* the same with images that are already in HBM (device pointers; the caller orders their producer before this call on the device, e.g.
 * by a device synchronisation): nothing is copied.  Depth images dense per sequence (depth_stream_stride == rows * depth_row_stride). */
int vslam_rgbd_submit_batch_device(vslam_rgbd* t, const uint8_t* left_device, int32_t left_row_stride, size_t left_stream_stride,
                                   const uint16_t* depth_device, int32_t depth_row_stride, size_t depth_stream_stride);
int vslam_rgbd_get_frame_info_stream(vslam_rgbd* t, int32_t stream, vslam_frame_info* out, int32_t* n_temporary);
int vslam_rgbd_get_points_stream(vslam_rgbd* t, int32_t stream, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc);
int vslam_rgbd_get_frame_info(vslam_rgbd* t, vslam_frame_info* out, int32_t* n_temporary);
int vslam_rgbd_get_points(vslam_rgbd* t, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc);
/* The landmark map and the observation log of this mode (opt-in; csrc/kernels_rgbd_map.h): the contract of vslam_enable_map /
 * vslam_enable_observations restated for this tracker's data, one sequence or a batch.  Identity is the track: a point whose predecessor
 * carries an id takes it, else a point whose landmark was created or updated this frame takes the next id (dense from 0 after enabling or
 * vslam_rgbd_reset, in point order: id k is the k-th landmark the reference creates), else -1.  Map entry: world coordinates, info3 =
 * (first_frame, last_frame, updates), the 32 descriptor bytes of the point at the last update; rewritten exactly in the frames that created
 * or updated the landmark.  Observation entry, one per point with an id, in point order: id_frame2 = (id, frame), xy (the keypoint, float)
 * and cam (the point's camera coordinates, the measurement Landmark::update consumed), both bit for bit what vslam_rgbd_get_points reports;
 * a landmark's entries start with the frame that created its map entry.  Frames are 0-based per sequence.  A full map refuses later
 * landmarks for their track's life and sets bit 8 of that frame's error_flags; a full log keeps the first `capacity` entries and sets bit
 * 16 in every frame that dropped one; neither stops the tracker.  vslam_rgbd_reset clears both and leaves them enabled; capacity 0 turns
 * the store off (vslam_rgbd_enable_map(0): map and log); the log needs the map (VSLAM_ERR_STATE otherwise).  Enabling between frames of a
 * running sequence is allowed: tracks that already carry a landmark get an id at their next update.  With a frame in flight (between
 * submit and wait) every call here returns VSLAM_ERR_STATE; so does every call on the host-driven loop (VSLAM_RGBD_HOST=1),
 * which does not have the feature.  Any output pointer may be NULL; first_id / first read only what is new;
 * vslam_rgbd_get_point_ids: the finished frame's ids in vslam_rgbd_get_points order (needs the map only). */
int vslam_rgbd_enable_map(vslam_rgbd* t, int32_t capacity_per_stream);
int vslam_rgbd_get_map_size(vslam_rgbd* t, int32_t stream, int32_t* n);
int vslam_rgbd_get_map(vslam_rgbd* t, int32_t stream, int32_t first_id, int32_t cap, int32_t* n, double* xyz, int32_t* info3, uint8_t* desc);
int vslam_rgbd_enable_observations(vslam_rgbd* t, int32_t capacity_per_stream);
int vslam_rgbd_get_observation_count(vslam_rgbd* t, int32_t stream, int32_t* n);
int vslam_rgbd_get_observations(vslam_rgbd* t, int32_t stream, int32_t first, int32_t cap, int32_t* n, int32_t* id_frame2, float* xy, double* cam);
int vslam_rgbd_get_point_ids(vslam_rgbd* t, int32_t stream, int32_t cap, int32_t* n, int32_t* ids);
/* The map's colours in this mode (opt-in; the definition above vslam_enable_map_colors): the colour of the pixel of RgbdList::xy — a float,
 * rounded half to even in float32 and clamped to the image first — in the frame's colour image, written exactly in the frames that create
 * or update the entry (when its row is written), through the undistortion map when undistortion is on.  One kernel directly behind the
 * map's on the same queue, once per frame (after the last registration attempt), inside the captured launch sequence as well.
 * vslam_rgbd_enable_map_colors: VSLAM_ERR_STATE without the map or a colour format, with a frame in flight, and on the host-driven loop;
 *   0 frees the store, and so do vslam_rgbd_enable_map and vslam_rgbd_set_color_input(t, VSLAM_PIXEL_GRAY8); vslam_rgbd_reset clears
 *   the colours with the map and leaves them enabled.  LIFETIME: a host frame is coloured from the tracker's staged copy; a DEVICE frame
 *   (vslam_rgbd_submit_batch_device) is read again by this kernel, so the caller's image must stay valid and unchanged until vslam_rgbd_wait
 *   has returned (the frame's last registration attempt, and with it this kernel, may run inside vslam_rgbd_wait).
 * vslam_rgbd_get_map_colors: like vslam_rgbd_get_map; VSLAM_ERR_STATE while the switch is off. */
int vslam_rgbd_enable_map_colors(vslam_rgbd* t, int on);
int vslam_rgbd_get_map_colors(vslam_rgbd* t, int32_t stream, int32_t first_id, int32_t cap, int32_t* n, uint8_t* rgb /* [cap][3] */);
/* Undistortion of raw frames in this mode (opt-in; csrc/kernels_undistort.h): the counterpart of vslam_set_rectification for
 * one camera with a depth image registered to it (TUM, Kinect / RealSense streams).  One map pair in vslam_set_rectification's format at
 * the tracker's rows x cols serves image and depth.  The image is remapped like vslam_remap_u8 (bilinear, the same kernel); the depth
 * image takes the NEAREST raw pixel of the 1/32-px coordinate, ties up — depth is never blended across an edge:
 *   x = x0 + ((a & 31) >> 4), y = y0 + (((a >> 5) & 31) >> 4), out = raw[y][x] inside the raw image, else 0 (0 = no measurement).
 * While set, vslam_rgbd_process_host, _submit_host, _submit_batch_host and _submit_batch_device take RAW frames of raw_rows x raw_cols (row
 * strides >= raw_cols; device depth images of a batch need not be dense); two kernels undistort every sequence's frame ahead of the
 * detector and of the space map, each on the queue of its consumer.  Device images are read by those two kernels only.  Everything
 * downstream reports undistorted coordinates.  The maps survive vslam_rgbd_reset.
 * vslam_rgbd_set_undistortion: host pointers, copied before the call returns; both NULL turns it off and frees the storage.
 *   VSLAM_ERR_INVALID: one map only, map_a >= 1024, raw size outside 1 .. 32767.  VSLAM_ERR_STATE: a frame in flight, or the host-driven
 *   loop (VSLAM_RGBD_HOST=1), which does not have the feature.
 * vslam_rgbd_get_undistorted: the image (rows*cols bytes) and depth image (rows*cols uint16) the last finished frame of `stream` was
 *   processed on, dense; either pointer may be NULL.  VSLAM_ERR_STATE when off, before a frame, or with a frame in flight.
 * vslam_remap_nearest_u16: the depth remap stand-alone on a host image, the counterpart of vslam_remap_u8 (src rows x cols <= 32767 with
 *   row_stride elements per row, dst and the maps dst_rows x dst_cols, dense). */
int vslam_rgbd_set_undistortion(vslam_rgbd* t, int32_t raw_rows, int32_t raw_cols, const int16_t* map_xy, const uint16_t* map_a);
int vslam_rgbd_get_undistorted(vslam_rgbd* t, int32_t stream, uint8_t* image, uint16_t* depth);
/* Histogram equalisation in this mode (opt-in; the definition above vslam_set_equalization): the intensity image only, the depth image is
 * untouched (slam_assembly.cpp:406-409).  On the image queue, behind the undistortion of the image when that is on and ahead of the
 * detector, once per frame (further registration attempts read the equalised image again), inside the captured launch sequence as well.
 * A caller's device image is read only: it is equalised into an image of the tracker's own.  The switch survives vslam_rgbd_reset.
 * vslam_rgbd_set_equalization: VSLAM_ERR_STATE with a frame in flight, or on the host-driven loop (VSLAM_RGBD_HOST=1),
 *   which does not have the feature; VSLAM_ERR_INVALID above 2^24 pixels.
 * vslam_rgbd_get_equalized: the image (rows*cols bytes, dense) the last finished frame of `stream` was processed on; VSLAM_ERR_STATE
 *   when off, before a frame, or with a frame in flight. */
int vslam_rgbd_set_equalization(vslam_rgbd* t, int on);
int vslam_rgbd_get_equalized(vslam_rgbd* t, int32_t stream, uint8_t* image);
/* CLAHE in this mode (opt-in; the definition above vslam_set_clahe): the second mode of the same slot — the intensity image only, the same
 * place on the image queue, once per frame, inside the captured launch sequence (toggling drops it); a caller's device image is read only.
 * The switch survives vslam_rgbd_reset.
 * vslam_rgbd_set_clahe: VSLAM_ERR_STATE with a frame in flight, on the host-driven loop, or while global equalisation is on
 *   (vslam_rgbd_set_equalization(t, 1) likewise while CLAHE is on; switching either one OFF while the other is on changes nothing);
 *   VSLAM_ERR_INVALID as vslam_set_clahe.
 * vslam_rgbd_get_equalized returns the processed image in this mode.
 * vslam_rgbd_get_clahe_luts: uint8 [tiles_y][tiles_x][256] of the last finished frame of `stream`, with the errors of
 *   vslam_rgbd_get_equalized. */
int vslam_rgbd_set_clahe(vslam_rgbd* t, int on, double clip_limit, int tiles_x, int tiles_y);
int vslam_rgbd_get_clahe_luts(vslam_rgbd* t, int32_t stream, uint8_t* luts);
/* Bilateral filtering of the depth image in this mode (opt-in; the definition above vslam_bilateral_depth_u16; the reference's
 * enable_bilateral_filtering with its sigmas 2, 2): the three kernels run on the space map's queue behind the depth upload and the depth
 * undistortion and ahead of the map's first kernel, once per frame (further registration attempts reuse the map), inside the captured
 * launch sequence as well (toggling drops it).  They write an image of the tracker's own, which the space map reads instead: a caller's
 * device depth image is read only, and vslam_rgbd_get_undistorted keeps returning the unfiltered depth.  depth_scale is
 * depth_scale_factor_intensity_to_meters.  The switch survives vslam_rgbd_reset.  Nothing is launched or allocated while it is off.
 * vslam_rgbd_set_bilateral: a sigma of 0 selects the reference's 2.  VSLAM_ERR_STATE with a frame in flight, or on the host-driven loop
 *   (VSLAM_RGBD_HOST=1), which does not have the feature; VSLAM_ERR_INVALID for a negative or non-finite sigma, a
 *   radius above VSLAM_BILATERAL_MAX_RADIUS, a depth scale <= 0 or more than 2^24 pixels.
 * vslam_rgbd_get_bilateral: the switch and the sigmas in force (any pointer may be NULL).
 * vslam_rgbd_get_filtered_depth: the depth image (rows*cols uint16, dense) the last finished frame of `stream` was mapped from, and its
 *   table (4098 floats); either may be NULL.  VSLAM_ERR_STATE when off, before a frame, after vslam_rgbd_reset, or with a frame in flight. */
int vslam_rgbd_set_bilateral(vslam_rgbd* t, int on, double sigma_color, double sigma_space);
int vslam_rgbd_get_bilateral(vslam_rgbd* t, int* on, double* sigma_color, double* sigma_space);
int vslam_rgbd_get_filtered_depth(vslam_rgbd* t, int32_t stream, uint16_t* depth, float* lut4098);
/* Detection masks in this mode (opt-in; the definition above vslam_set_detection_mask; csrc/kernels_mask.h): one
 * 8-bit image at the processed size (the undistorted image's coordinates while undistortion is set), shared by every sequence of a batch.
 * Its eroded packed words are ANDed into the corner words between k_fast_box and k_emit of EVERY attempt of a frame, re-registration
 * attempts included, inside the captured launch sequence as well; nothing is launched while it is off.  n_detected_left of the frame
 * report is the masked count.  The effective keep-mask of sequence s is (static mask AND undistortion validity AND frame mask of s),
 * each eroded by its own margin, a missing one all-keep.
 * With p->detector_type = VSLAM_DETECTOR_ORB no mask is built: cv::ORB::detect resizes its mask for every pyramid level and the library
 * has no restatement of that.  The three setters return VSLAM_ERR_STATE with a message that says so (switching a mask off is accepted),
 * nothing changes and the next frame runs as if the call had not been made.
 * vslam_rgbd_set_detection_mask: host pointer, copied and packed before the call returns; NULL switches the mask off and frees it.  The
 *   mask survives vslam_rgbd_reset.  VSLAM_ERR_STATE with a frame in flight (between submit and wait), or on the host-driven loop
 *   (VSLAM_RGBD_HOST=1), which does not have the feature; VSLAM_ERR_INVALID (nothing changed) for a stride below cols
 *   or a margin outside 0 .. 64.
 * vslam_rgbd_get_detection_mask: the packed keep-mask (rows * ((cols + 63) / 64) words) the last finished frame used; VSLAM_ERR_STATE
 *   when off, before a frame, after vslam_rgbd_reset, or with a frame in flight.  These are the context-wide words: the static mask
 *   AND the undistortion maps' validity (below); with validity as the only mask the call succeeds.
 * vslam_rgbd_set_frame_masks: one mask per sequence of the batch for the NEXT submit only (a frame without a set behaves as if the call
 *   did not exist): sequence s at masks + s * image_stride_bytes; NULL cancels a pending set.  "The next submit" is the next one that
 *   is accepted: a submit refused for its arguments or its state (a frame in flight, a failed tracker) changes nothing and the set goes
 *   on waiting; a submit that fails after it was accepted (VSLAM_ERR_HIP) drops the set with its frame.  That submit copies host masks
 *   (on_device 0) on the frame's queue; device masks are read in place by its one k_mask_pack launch and never written.  The launch
 *   runs on the tracker's own queue and waits for no other stream: whatever wrote the device masks must have finished before the
 *   submit call (synchronise the producing stream first, as for the images of vslam_rgbd_submit_batch_device), and they must stay as
 *   they are until that launch has run: vslam_rgbd_wait is the bound.  The launch packs and erodes every sequence's mask and ANDs the
 *   context-wide words in, into effective words [B][rows][TX], ahead of the first detection; k_mask_apply ANDs a sequence's words into
 *   its corner words in every attempt of that frame.  Under VSLAM_RGBD_GRAPH=1 the pack launch stays outside the captured sequence,
 *   which is captured again when a frame with masks follows one without, or the reverse.  VSLAM_ERR_STATE with a frame in flight or on
 *   the host-driven loop; VSLAM_ERR_INVALID for a stride below cols, a margin outside 0 .. 64, or, with more than one sequence, an
 *   image stride smaller than one mask.  No refusal is sticky, and a refused call changes nothing.  vslam_rgbd_reset drops a pending set.
 * vslam_rgbd_get_frame_detection_mask: the effective words the last finished frame of `stream` used (the context-wide words when it had
 *   no frame mask); VSLAM_ERR_STATE when that frame used no mask of any kind, before a frame, after vslam_rgbd_reset, or with a frame
 *   in flight.
 * vslam_rgbd_set_undistortion_mask / vslam_rgbd_get_undistortion_mask: the undistortion maps' validity as part of the context-wide
 *   keep-mask, as vslam_set_rectification_mask defines it: computed once per call and per new maps (vslam_rgbd_set_undistortion), off
 *   with the maps, kept over vslam_rgbd_reset.  VSLAM_ERR_STATE without maps, with a frame in flight, or on the host-driven loop;
 *   VSLAM_ERR_INVALID for a margin outside 0 .. 64. */
int vslam_rgbd_set_detection_mask(vslam_rgbd* t, const uint8_t* mask, int32_t row_stride_bytes, int32_t margin);
int vslam_rgbd_get_detection_mask(vslam_rgbd* t, uint64_t* words);
int vslam_rgbd_set_frame_masks(vslam_rgbd* t, const uint8_t* masks, int32_t row_stride_bytes, size_t image_stride_bytes, int32_t margin,
                               int on_device);
int vslam_rgbd_get_frame_detection_mask(vslam_rgbd* t, int32_t stream, uint64_t* words);
int vslam_rgbd_set_undistortion_mask(vslam_rgbd* t, int on, int32_t margin);
int vslam_rgbd_get_undistortion_mask(vslam_rgbd* t, int* on, int32_t* margin);
/* Colour input in this mode (opt-in; the definition and the VSLAM_PIXEL_* formats above vslam_set_color_input): while the format is not
 * VSLAM_PIXEL_GRAY8 the intensity image of every process / submit / batch entry, host or device, is interleaved colour at the size the
 * tracker otherwise expects; its row and stream strides are in BYTES (row stride >= channels * cols).  The depth image is untouched.
 * k_gray_u8 runs on the image queue ahead of the undistortion, the equalisation and the detector, once per frame (further registration
 * attempts read the grey image again), inside the captured launch sequence as well.  A caller's device image is read only.  The switch
 * survives vslam_rgbd_reset.
 * vslam_rgbd_set_color_input: VSLAM_ERR_STATE with a frame in flight, or on the host-driven loop (VSLAM_RGBD_HOST=1),
 *   which does not have the feature; VSLAM_ERR_INVALID for a format outside 0 .. 4.
 * vslam_rgbd_get_gray: the grey image (dense, at the input size: the raw size while undistortion maps are set) of the last finished
 *   frame of `stream`; VSLAM_ERR_STATE when off, before a frame, after vslam_rgbd_reset, or with a frame in flight.  With equalisation on
 *   and undistortion off the image is equalised in place afterwards, and this getter returns it so. */
int vslam_rgbd_set_color_input(vslam_rgbd* t, int format);
int vslam_rgbd_get_gray(vslam_rgbd* t, int32_t stream, uint8_t* image);

/* Motion models in this mode (opt-in; the definition above vslam_set_motion_model): the device loop computes the prior inside the frame's
 * launch sequence (captured or not), once per frame; the host-driven loop through vslam_motion_prior.  VSLAM_ERR_STATE with a frame in
 * flight (between submit and wait), VSLAM_ERR_INVALID as for the stereo calls.  The device form of vslam_rgbd_set_pose_guesses is copied
 * on the tracker's queue at the call (no host synchronisation; VSLAM_ERR_STATE on the host-driven loop); a host guess set after it waits
 * for that copy, so whichever was set last holds.  A guess is kept until the next one is set, under every model.  The model survives
 * vslam_rgbd_reset, the guesses do not. */
int vslam_rgbd_set_motion_model(vslam_rgbd* t, int model, int32_t dead_reckoning_limit);
int vslam_rgbd_get_motion_model(vslam_rgbd* t, int* model, int32_t* dead_reckoning_limit);
int vslam_rgbd_set_pose_guess(vslam_rgbd* t, int32_t stream, const double camera_left_to_world[12]);
int vslam_rgbd_set_pose_guesses(vslam_rgbd* t, const double* camera_left_to_world /* [n_streams][12] */, int on_device);
int vslam_remap_nearest_u16(vslam_ctx* ctx, const uint16_t* src, int32_t rows, int32_t cols, int32_t row_stride,
                            const int16_t* map_xy, const uint16_t* map_a, int32_t dst_rows, int32_t dst_cols, uint16_t* dst);

/* ---- OrbDetector components (first half; base_framepoint_generator.cpp:52-70) ----------------------
 * The reference's OrbDetector is cv::ORB::create(5000, 1.2, 8, 31, 0, 2, HARRIS_SCORE, 31, threshold) used as a DETECTOR
 * (descriptors still come from the configured extractor).  OpenCV is not in the reference tree: the published algorithm
 * (features2d/src/orb.cpp computeKeyPoints, imgproc resize) is restated [recalled]; parity is pinned against the
 * repo's independent numpy restatement only. */

/* cv::resize(src, dst, dsize, 0, 0, INTER_LINEAR) for 8-bit single channel: 11-bit fixed-point bilinear weights,
 * horizontal pass in 32-bit, vertical pass ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.  Host images. */
int vslam_resize_linear_u8(vslam_ctx* ctx, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride,
                           uint8_t* dst, int32_t dst_rows, int32_t dst_cols);

/* HarrisResponses (block 7, k = 0.04) and ICAngles (half patch 15, fastAtan2) of orb.cpp at n integer pixel positions
 * (xy: n*2 int16, at least 16 px from the border): response n floats, angle n floats (degrees). */
int vslam_harris_angle(vslam_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t row_stride, int32_t n,
                       const int16_t* xy, float* response, float* angle);

/* ORB::detect with HARRIS_SCORE, firstLevel 0, no mask: pyramid by successive INTER_LINEAR resizes, FAST-9/16 + NMS per
 * level, 31 px border filter, retainBest(2 n_level) on the FAST score, Harris response, retainBest(n_level), intensity
 * centroid angle, coordinates scaled back to level 0.  retainBest keeps every keypoint whose response ties the n-th
 * (as KeyPointsFilter does); within a level the keypoints stay in row-major order (std::nth_element leaves the order
 * unspecified upstream).  out: 6 floats per keypoint (x, y, size, angle, response, octave), levels in ascending order. */
int vslam_orb_detect(vslam_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t row_stride,
                     int32_t nfeatures, float scale_factor, int32_t nlevels, int32_t edge_threshold, int32_t patch_size,
                     int32_t fast_threshold, int32_t cap, int32_t* n, float* keypoints);

/* cv::ORB::create()->compute() on keypoints that carry an octave and an angle — what BaseFramePointGenerator::computeDescriptors
 * (base_framepoint_generator.cpp:431-438) does with an OrbDetector's keypoints when the extractor is ORB [recalled: orb.cpp
 * detectAndCompute with useProvidedKeypoints]: runByImageBorder(31) on the level-0 coordinates (Rect::contains rounds the float point), a
 * pyramid up to the highest octave present (level l from level l-1, INTER_LINEAR, cvRound(cols / scale) x cvRound(rows / scale), scale =
 * (float)pow(scale_factor, l)), GaussianBlur 7x7 sigma 2 per level, 256 tests steered by the keypoint's own angle around
 * (cvRound(x / scale), cvRound(y / scale)) of its level.  keypoints: n x 6 floats as vslam_orb_detect writes them.  keep[i] = 0: removed
 * (border filter; also a keypoint whose pattern would leave its level, which an OrbDetector never produces). */
int vslam_orb_describe_keypoints(vslam_ctx* ctx, const uint8_t* image, int32_t rows, int32_t cols, int32_t row_stride, int32_t n,
                                 const float* keypoints, float scale_factor, uint8_t* keep, uint8_t* descriptors);

/* ---- multi-GPU: trajectory assembly ---------------------------------------------------------
 * No reference counterpart (single process).  The pose all-gather is issued by the host
 * launcher through RCCL (torch.distributed backend "nccl"); these helpers pack/unpack. */
int vslam_get_poses(vslam_ctx* ctx, int stream, int32_t first_frame, int32_t n_frames,
                    double* camera_left_to_world /* n_frames*12 */);
/* Same, for ALL streams, into DEVICE memory (dst[stream][frame][12], asynchronous on the context
 * stream): the send buffer of the RCCL all-gather. */
int vslam_copy_poses_device(vslam_ctx* ctx, int32_t first_frame, int32_t n_frames, double* dst_device);

/* ---- multi-GPU: the pose all-gather itself, on RCCL, for callers that are not Python ---------------
 * One process per GPU.  Rank 0 asks for a unique id (128 bytes, ncclUniqueId) and hands it to the other ranks by whatever
 * channel launched them (MPI, a file, torch.distributed's store); every rank then joins with vslam_comm_init.  RCCL
 * (librccl.so) is loaded on first use: a single-GPU user of the library never needs it.
 * vslam_allgather_poses: send_device holds this rank's count doubles (e.g. [streams][frames][12] as vslam_copy_poses_device
 * leaves them), recv_device receives nranks * count doubles ordered by rank; one ncclAllGather (xGMI on one node), queued
 * on hip_stream (NULL: the default stream), asynchronous — synchronise the stream before reading. */
typedef struct vslam_comm vslam_comm;
#define VSLAM_COMM_ID_BYTES 128
/* Local precondition of vslam_comm_init (librccl.so loadable with the expected symbols, the device selectable): every rank
 * calls it and the ranks agree on the result over the launcher's channel BEFORE anyone enters the collective
 * ncclCommInitRank — a rank that cannot take part must not leave its peers waiting in it. */
int vslam_comm_available(int device);
int vslam_comm_unique_id(uint8_t id[VSLAM_COMM_ID_BYTES]);
int vslam_comm_init(int rank, int nranks, const uint8_t id[VSLAM_COMM_ID_BYTES], int device, vslam_comm** out);
int vslam_allgather_poses(vslam_comm* comm, const double* send_device, double* recv_device, size_t count, void* hip_stream);
void vslam_comm_destroy(vslam_comm* comm);
const char* vslam_comm_last_error(void);

/* The pose (camera_left_to_world) of the frame every stream processed last, into DEVICE memory dst[stream][12],
 * asynchronous on the context stream: one row block of the all-gather's send buffer per step. */
int vslam_copy_current_poses_device(vslam_ctx* ctx, double* dst_device);

#ifdef __cplusplus
}
#endif
#endif /* VSLAM_HIP_H */
