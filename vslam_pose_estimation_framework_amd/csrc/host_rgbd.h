// host_rgbd.h — RGB-D mode behind vslam_rgbd_*.  Host code, included by vslam_hip.hip after the context, the frame path and the
// stand-alone entries (the host-driven loop calls them).
#pragma once
// Two implementations behind the same entry points: the device-resident loop (csrc/rgbd_device.h + kernels_rgbd.h; the default) and the
// host-driven loop over the library's own stand-alone entry points (csrc/rgbd_tracker.h; VSLAM_RGBD_HOST=1), kept as the cross-check.
// Both serve detector_type FAST and ORB.
#include "rgbd_tracker.h"
#include "rgbd_device.h"
struct vslam_rgbd {
  bool on_host = false, host_pending = false;
  int host_rc = 0;
  vs_rgbd::Tracker t;
  vs_rgbd::DeviceTracker d;
  std::string& err() { return on_host ? t.err : d.err; }
};
static thread_local std::string g_rgbd_error;
VS_API const char* vslam_rgbd_last_error(const vslam_rgbd* r) { return r ? (r->on_host ? r->t.err.c_str() : r->d.err.c_str()) : g_rgbd_error.c_str(); }
static int rgbd_create(const vslam_config* cfg, const vslam_depth_params* p, int device, int n_streams, vslam_rgbd** out) {
  if (!cfg || !p || !out) { g_rgbd_error = "vslam_rgbd_create: null argument"; return VSLAM_ERR_INVALID; }
  vslam_rgbd* r = new vslam_rgbd;
  if (const char* e = std::getenv("VSLAM_RGBD_HOST")) r->on_host = std::atoi(e) != 0;
  // detector_type ORB: the device-resident loop runs the OrbDetector on its own queue (kernels_rgbd_orb.h) for detector grids whose regions
  // all have one size (up to 2 x 2: every shipped configuration); a larger grid keeps the host-driven loop, with its refusals
  if (p->detector_type == VSLAM_DETECTOR_ORB) { if (!vs_rgbd::DeviceTracker::orb_grid_supported(*cfg)) r->on_host = true; }
  else if (p->detector_type != VSLAM_DETECTOR_FAST) { g_rgbd_error = "vslam_rgbd_create: unknown detector_type"; delete r; return VSLAM_ERR_INVALID; }
  if (r->on_host && n_streams != 1) { g_rgbd_error = "vslam_rgbd_create_batch: the host-driven loop (VSLAM_RGBD_HOST=1, detector_type ORB on a grid above 2 x 2) tracks one sequence per object"; delete r; return VSLAM_ERR_INVALID; }
  const int rc = r->on_host ? r->t.create(*cfg, *p, device) : r->d.create(*cfg, *p, device, n_streams);
  if (rc != VSLAM_OK) { g_rgbd_error = r->err(); delete r; return rc; }
  *out = r;
  return VSLAM_OK;
}
VS_API int vslam_rgbd_create(const vslam_config* cfg, const vslam_depth_params* p, int device, vslam_rgbd** out) { return rgbd_create(cfg, p, device, 1, out); }
VS_API int vslam_rgbd_create_batch(const vslam_config* cfg, const vslam_depth_params* p, int device, int32_t n_streams, vslam_rgbd** out) {
  return rgbd_create(cfg, p, device, n_streams, out);
}
VS_API void vslam_rgbd_destroy(vslam_rgbd* r) { delete r; }
VS_API int vslam_rgbd_reset(vslam_rgbd* r) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) { r->t.reset(); return VSLAM_OK; }
  return r->d.reset();
}
// what every entry that takes a frame checks first; the message lands in the loop's own error string
static int rgbd_frame_args_ok(vslam_rgbd* r, const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride) {
  if (!left || !depth) { r->err() = "called with empty frame"; return VSLAM_ERR_INVALID; }   // depth_framepoint_generator.cpp:48-50
  const int cols = r->on_host ? r->t.cfg.cols : r->d.in_cols();     // the raw width while undistortion maps are set
  const int wb = r->on_host ? cols : r->d.in_bytes();               // channels * width of a colour frame (vslam_rgbd_set_color_input)
  if (lstride < wb || dstride < cols) { r->err() = "row stride smaller than image width"; return VSLAM_ERR_INVALID; }
  return VSLAM_OK;
}
VS_API int vslam_rgbd_process_host(vslam_rgbd* r, const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride) {
  if (!r) return VSLAM_ERR_INVALID;
  if (int rc = rgbd_frame_args_ok(r, left, lstride, depth, dstride)) return rc;
  return r->on_host ? r->t.process(left, lstride, depth, dstride) : r->d.process(left, lstride, depth, dstride);
}
VS_API int vslam_rgbd_submit_host(vslam_rgbd* r, const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride) {
  if (!r) return VSLAM_ERR_INVALID;
  if (int rc = rgbd_frame_args_ok(r, left, lstride, depth, dstride)) return rc;
  if (r->on_host) { r->host_rc = r->t.process(left, lstride, depth, dstride); r->host_pending = true; return r->host_rc; }   // the host-driven loop has nothing to overlap
  return r->d.submit(left, lstride, depth, dstride);
}
VS_API int vslam_rgbd_wait(vslam_rgbd* r) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) {
    if (!r->host_pending) { r->t.err = "RGB-D tracker: no frame in flight"; return VSLAM_ERR_STATE; }
    r->host_pending = false;
    return r->host_rc;
  }
  return r->d.wait();
}
VS_API int vslam_rgbd_submit_batch_host(vslam_rgbd* r, const uint8_t* left, int32_t lstride, size_t left_stream_stride, const uint16_t* depth, int32_t dstride,
                                        size_t depth_stream_stride) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) { r->t.err = "batch entry points need the device-resident loop"; return VSLAM_ERR_STATE; }
  if (int rc = rgbd_frame_args_ok(r, left, lstride, depth, dstride)) return rc;
  return r->d.submit(left, lstride, depth, dstride, left_stream_stride, depth_stream_stride);
}
VS_API int vslam_rgbd_process_batch_host(vslam_rgbd* r, const uint8_t* left, int32_t lstride, size_t left_stream_stride, const uint16_t* depth, int32_t dstride,
                                         size_t depth_stream_stride) {
  const int rc = vslam_rgbd_submit_batch_host(r, left, lstride, left_stream_stride, depth, dstride, depth_stream_stride);
  return rc != VSLAM_OK ? rc : vslam_rgbd_wait(r);
}
VS_API int vslam_rgbd_submit_batch_device(vslam_rgbd* r, const uint8_t* left, int32_t lstride, size_t left_stream_stride, const uint16_t* depth, int32_t dstride,
                                          size_t depth_stream_stride) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) { r->t.err = "device images need the device-resident loop"; return VSLAM_ERR_STATE; }
  if (int rc = rgbd_frame_args_ok(r, left, lstride, depth, dstride)) return rc;
  return r->d.submit(left, lstride, depth, dstride, left_stream_stride, depth_stream_stride, true);
}
VS_API int vslam_rgbd_get_frame_info(vslam_rgbd* r, vslam_frame_info* out, int32_t* n_temporary) {
  if (!r || !out) return VSLAM_ERR_INVALID;
  if (r->on_host) { *out = r->t.info; if (n_temporary) *n_temporary = r->t.n_temporary; return VSLAM_OK; }
  if (int rc = r->d.readable(0)) return rc;
  *out = r->d.host.info;
  if (n_temporary) *n_temporary = r->d.host.n_temporary;
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_points(vslam_rgbd* r, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc) {
  if (!r || !n) return VSLAM_ERR_INVALID;
  if (!r->on_host) return r->d.get_points(0, cap, n, xy, cam, meta4, desc);
  if (r->t.info.frame_index == 0) { *n = 0; return VSLAM_OK; }
  const vs_rgbd::Fr& f = r->t.current();
  *n = (int32_t)f.points.size();
  if (*n > cap) { r->t.err = "point output capacity too small"; return VSLAM_ERR_CAPACITY; }
  for (int i = 0; i < *n; ++i) {
    const vs_rgbd::Pt& q = r->t.point(f.points[i]);
    if (xy) { xy[2 * i] = q.xy[0]; xy[2 * i + 1] = q.xy[1]; }
    if (cam) for (int k = 0; k < 3; ++k) cam[3 * i + k] = q.cam[k];
    if (meta4) { meta4[4 * i] = r->t.previous_index(q); meta4[4 * i + 1] = q.track_len; meta4[4 * i + 2] = q.landmark >= 0 ? r->t.landmarks()[q.landmark].updates : 0; meta4[4 * i + 3] = q.unreliable ? 1 : 0; }
    if (desc) std::memcpy(desc + (size_t)32 * i, q.desc, 32);
  }
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_frame_info_stream(vslam_rgbd* r, int32_t stream, vslam_frame_info* out, int32_t* n_temporary) {
  if (!r || !out) return VSLAM_ERR_INVALID;
  if (r->on_host) return stream == 0 ? vslam_rgbd_get_frame_info(r, out, n_temporary) : VSLAM_ERR_INVALID;
  if (int rc = r->d.readable(stream)) return rc;
  *out = r->d.hosts[stream].info;
  if (n_temporary) *n_temporary = r->d.hosts[stream].n_temporary;
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_points_stream(vslam_rgbd* r, int32_t stream, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc) {
  if (!r || !n) return VSLAM_ERR_INVALID;
  if (r->on_host) return stream == 0 ? vslam_rgbd_get_points(r, cap, n, xy, cam, meta4, desc) : VSLAM_ERR_INVALID;
  return r->d.get_points(stream, cap, n, xy, cam, meta4, desc);
}
// ---- the RGB-D landmark map and observation log (kernels_rgbd_map.h): the device-resident loop only ----
static int rgbd_map_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) keeps no landmark map or observation log; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_enable_map(vslam_rgbd* r, int32_t cap) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_enable_map") : r->d.enable_map(cap);
}
VS_API int vslam_rgbd_get_map_size(vslam_rgbd* r, int32_t stream, int32_t* n) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) return rgbd_map_host_refusal(r, "vslam_rgbd_get_map_size");
  if (!n) { r->d.err = "vslam_rgbd_get_map_size: null output"; return VSLAM_ERR_INVALID; }
  return r->d.map_ready(stream, false, n);
}
VS_API int vslam_rgbd_get_map(vslam_rgbd* r, int32_t stream, int32_t first_id, int32_t cap, int32_t* n, double* xyz, int32_t* info3, uint8_t* desc) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_get_map") : r->d.get_map(stream, first_id, cap, n, xyz, info3, desc);
}
VS_API int vslam_rgbd_enable_observations(vslam_rgbd* r, int32_t cap) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_enable_observations") : r->d.enable_observations(cap);
}
VS_API int vslam_rgbd_get_observation_count(vslam_rgbd* r, int32_t stream, int32_t* n) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) return rgbd_map_host_refusal(r, "vslam_rgbd_get_observation_count");
  if (!n) { r->d.err = "vslam_rgbd_get_observation_count: null output"; return VSLAM_ERR_INVALID; }
  return r->d.map_ready(stream, true, n);
}
VS_API int vslam_rgbd_get_observations(vslam_rgbd* r, int32_t stream, int32_t first, int32_t cap, int32_t* n, int32_t* id_frame2, float* xy, double* cam) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_get_observations") : r->d.get_observations(stream, first, cap, n, id_frame2, xy, cam);
}
VS_API int vslam_rgbd_get_point_ids(vslam_rgbd* r, int32_t stream, int32_t cap, int32_t* n, int32_t* ids) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_get_point_ids") : r->d.get_point_ids(stream, cap, n, ids);
}
VS_API int vslam_rgbd_enable_map_colors(vslam_rgbd* r, int on) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_enable_map_colors") : r->d.enable_map_colors(on);
}
VS_API int vslam_rgbd_get_map_colors(vslam_rgbd* r, int32_t stream, int32_t first_id, int32_t cap, int32_t* n, uint8_t* rgb) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_map_host_refusal(r, "vslam_rgbd_get_map_colors") : r->d.get_map_colors(stream, first_id, cap, n, rgb);
}
// ---- undistortion of raw frames (kernels_undistort.h): the device-resident loop only ----
static int rgbd_undistort_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) takes undistorted frames only; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_undistortion(vslam_rgbd* r, int32_t raw_rows, int32_t raw_cols, const int16_t* map_xy, const uint16_t* map_a) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_undistort_host_refusal(r, "vslam_rgbd_set_undistortion") : r->d.set_undistortion(raw_rows, raw_cols, map_xy, map_a);
}
VS_API int vslam_rgbd_get_undistorted(vslam_rgbd* r, int32_t stream, uint8_t* image, uint16_t* depth) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_undistort_host_refusal(r, "vslam_rgbd_get_undistorted") : r->d.get_undistorted(stream, image, depth);
}
// ---- histogram equalisation of the intensity image (kernels_equalize.h): the device-resident loop only ----
static int rgbd_equalize_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) does not equalise; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_equalization(vslam_rgbd* r, int on) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_equalize_host_refusal(r, "vslam_rgbd_set_equalization") : r->d.set_equalization(on);
}
VS_API int vslam_rgbd_get_equalized(vslam_rgbd* r, int32_t stream, uint8_t* image) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_equalize_host_refusal(r, "vslam_rgbd_get_equalized") : r->d.get_equalized(stream, image);
}
// ---- the static detection mask (kernels_mask.h): the device-resident loop only ----
static int rgbd_mask_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) takes no detection mask; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_detection_mask(vslam_rgbd* r, const uint8_t* mask, int32_t row_stride, int32_t margin) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_mask_host_refusal(r, "vslam_rgbd_set_detection_mask") : r->d.set_detection_mask(mask, row_stride, margin);
}
VS_API int vslam_rgbd_set_frame_masks(vslam_rgbd* r, const uint8_t* masks, int32_t row_stride, size_t image_stride, int32_t margin, int on_device) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_mask_host_refusal(r, "vslam_rgbd_set_frame_masks") : r->d.set_frame_masks(masks, row_stride, image_stride, margin, on_device != 0);
}
VS_API int vslam_rgbd_get_frame_detection_mask(vslam_rgbd* r, int32_t stream, uint64_t* words) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_mask_host_refusal(r, "vslam_rgbd_get_frame_detection_mask") : r->d.get_frame_detection_mask(stream, words);
}
VS_API int vslam_rgbd_set_undistortion_mask(vslam_rgbd* r, int on, int32_t margin) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_mask_host_refusal(r, "vslam_rgbd_set_undistortion_mask") : r->d.set_undistortion_mask(on, margin);
}
VS_API int vslam_rgbd_get_undistortion_mask(vslam_rgbd* r, int* on, int32_t* margin) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) { if (on) *on = 0; if (margin) *margin = 0; return VSLAM_OK; }
  return r->d.get_undistortion_mask(on, margin);
}
VS_API int vslam_rgbd_get_detection_mask(vslam_rgbd* r, uint64_t* words) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_mask_host_refusal(r, "vslam_rgbd_get_detection_mask") : r->d.get_detection_mask(words);
}
// ---- CLAHE of the intensity image, the equalisation slot's second mode (kernels_clahe.h): the device-resident loop only ----
VS_API int vslam_rgbd_set_clahe(vslam_rgbd* r, int on, double clip_limit, int tiles_x, int tiles_y) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_equalize_host_refusal(r, "vslam_rgbd_set_clahe") : r->d.set_clahe(on, clip_limit, tiles_x, tiles_y);
}
VS_API int vslam_rgbd_get_clahe_luts(vslam_rgbd* r, int32_t stream, uint8_t* luts) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_equalize_host_refusal(r, "vslam_rgbd_get_clahe_luts") : r->d.get_clahe_luts(stream, luts);
}
// ---- bilateral filtering of the depth image (kernels_bilateral.h): the device-resident loop only ----
static int rgbd_bilateral_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) does not filter the depth image; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_bilateral(vslam_rgbd* r, int on, double sigma_color, double sigma_space) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_bilateral_host_refusal(r, "vslam_rgbd_set_bilateral") : r->d.set_bilateral(on, sigma_color, sigma_space);
}
VS_API int vslam_rgbd_get_bilateral(vslam_rgbd* r, int* on, double* sigma_color, double* sigma_space) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) return rgbd_bilateral_host_refusal(r, "vslam_rgbd_get_bilateral");
  return r->d.get_bilateral(on, sigma_color, sigma_space);
}
VS_API int vslam_rgbd_get_filtered_depth(vslam_rgbd* r, int32_t stream, uint16_t* depth, float* lut4098) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_bilateral_host_refusal(r, "vslam_rgbd_get_filtered_depth") : r->d.get_filtered_depth(stream, depth, lut4098);
}
// ---- colour input (kernels_gray.h): the device-resident loop only ----
static int rgbd_color_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) takes grey frames only; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_color_input(vslam_rgbd* r, int format) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_color_host_refusal(r, "vslam_rgbd_set_color_input") : r->d.set_color_input(format);
}
VS_API int vslam_rgbd_get_gray(vslam_rgbd* r, int32_t stream, uint8_t* image) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_color_host_refusal(r, "vslam_rgbd_get_gray") : r->d.get_gray(stream, image);
}

// ---- downscale of the incoming frames (the definition above vslam_downscale_u8) -------------------------------------------
static int rgbd_downscale_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) does not downscale; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_downscale(vslam_rgbd* r, int32_t factor, int32_t full_rows, int32_t full_cols) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_downscale_host_refusal(r, "vslam_rgbd_set_downscale") : r->d.set_downscale(factor, full_rows, full_cols);
}
VS_API int vslam_rgbd_get_downscale(vslam_rgbd* r, int32_t* factor, int32_t* full_rows, int32_t* full_cols) {
  if (!r) return VSLAM_ERR_INVALID;
  if (!r->on_host) { r->d.get_downscale(factor, full_rows, full_cols); return VSLAM_OK; }
  if (factor) *factor = 1;
  if (full_rows) *full_rows = 0;
  if (full_cols) *full_cols = 0;
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_downscaled(vslam_rgbd* r, int32_t stream, uint8_t* image, uint16_t* depth) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_downscale_host_refusal(r, "vslam_rgbd_get_downscaled") : r->d.get_downscaled(stream, image, depth);
}

// ---- smoothing of the intensity image (the definition above vslam_set_smoothing) ------------------------------------------
static int rgbd_smoothing_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1) does not smooth; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
VS_API int vslam_rgbd_set_smoothing(vslam_rgbd* r, int mode, int32_t ksize) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_smoothing_host_refusal(r, "vslam_rgbd_set_smoothing") : r->d.set_smoothing(mode, ksize);
}
VS_API int vslam_rgbd_get_smoothing(vslam_rgbd* r, int* mode, int32_t* ksize) {
  if (!r) return VSLAM_ERR_INVALID;
  if (!r->on_host) { r->d.get_smoothing(mode, ksize); return VSLAM_OK; }
  if (mode) *mode = VSLAM_SMOOTH_OFF;
  if (ksize) *ksize = 0;
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_smoothed(vslam_rgbd* r, int32_t stream, uint8_t* image) {
  if (!r) return VSLAM_ERR_INVALID;
  return r->on_host ? rgbd_smoothing_host_refusal(r, "vslam_rgbd_get_smoothed") : r->d.get_smoothed(stream, image);
}

// ---- motion models (the definition above vslam_set_motion_model) ---------------------------------------------------------
VS_API int vslam_rgbd_set_motion_model(vslam_rgbd* r, int model, int32_t dead_reckoning_limit) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host && r->host_pending) { r->t.err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
  return r->on_host ? r->t.set_motion_model(model, dead_reckoning_limit) : r->d.set_motion_model(model, dead_reckoning_limit);
}
VS_API int vslam_rgbd_get_motion_model(vslam_rgbd* r, int* model, int32_t* dead_reckoning_limit) {
  if (!r) return VSLAM_ERR_INVALID;
  if (model) *model = r->on_host ? r->t.motion_model : r->d.motion_model;
  if (dead_reckoning_limit) *dead_reckoning_limit = r->on_host ? r->t.dead_reckoning_limit : r->d.dead_reckoning_limit;
  return VSLAM_OK;
}
static int rgbd_set_guess(vslam_rgbd* r, int32_t stream, const double* T, bool on_device) {
  if (!r) return VSLAM_ERR_INVALID;
  if (!r->on_host) return r->d.set_pose_guess(stream, T, on_device);
  if (!T) { r->t.err = "vslam_rgbd_set_pose_guess: null pose"; return VSLAM_ERR_INVALID; }
  if (stream > 0) { r->t.err = "stream index out of range"; return VSLAM_ERR_INVALID; }
  if (on_device) { r->t.err = "vslam_rgbd_set_pose_guesses: device memory on the host-driven loop (VSLAM_RGBD_HOST=1)"; return VSLAM_ERR_STATE; }
  if (r->host_pending) { r->t.err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
  std::memcpy(r->t.guess, T, 96);
  return VSLAM_OK;
}
VS_API int vslam_rgbd_set_pose_guess(vslam_rgbd* r, int32_t stream, const double T[12]) {
  if (r && stream < 0) { r->err() = "stream index out of range"; return VSLAM_ERR_INVALID; }
  return rgbd_set_guess(r, stream, T, false);
}
VS_API int vslam_rgbd_set_pose_guesses(vslam_rgbd* r, const double* T, int on_device) { return rgbd_set_guess(r, -1, T, on_device != 0); }
