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
// ---- entries of the device-resident loop only ----------------------------------------------------------------------------------------
// What the host-driven loop lacks, by feature: the phrase of its refusal.
static const char* const RGBD_HOST_NO_MAP = "keeps no landmark map or observation log";       // kernels_rgbd_map.h
static const char* const RGBD_HOST_NO_UNDISTORT = "takes undistorted frames only";            // kernels_undistort.h
static const char* const RGBD_HOST_NO_EQUALIZE = "does not equalise";                         // kernels_equalize.h, kernels_clahe.h
static const char* const RGBD_HOST_NO_MASK = "takes no detection mask";                       // kernels_mask.h
static const char* const RGBD_HOST_NO_BILATERAL = "does not filter the depth image";          // kernels_bilateral.h
static const char* const RGBD_HOST_NO_COLOR = "takes grey frames only";                       // kernels_gray.h
static const char* const RGBD_HOST_NO_DOWNSCALE = "does not downscale";                       // the definition above vslam_downscale_u8; DESIGN.md 6o
static const char* const RGBD_HOST_NO_SMOOTHING = "does not smooth";                          // the definition above vslam_set_smoothing; DESIGN.md 6p
// entry `name`: call(the device-resident tracker), or on the host-driven loop the refusal with `phrase`
template <class Call>
static int rgbd_device_only(vslam_rgbd* r, const char* name, const char* phrase, Call&& call) {
  if (!r) return VSLAM_ERR_INVALID;
  if (!r->on_host) return call(r->d);
  r->t.err = std::string(name) + ": the host-driven loop (VSLAM_RGBD_HOST=1) " + phrase + "; use the device-resident loop";
  return VSLAM_ERR_STATE;
}
using RgbdDev = vs_rgbd::DeviceTracker;
VS_API int vslam_rgbd_enable_map(vslam_rgbd* r, int32_t cap) {
  return rgbd_device_only(r, "vslam_rgbd_enable_map", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.enable_map(cap); });
}
VS_API int vslam_rgbd_get_map_size(vslam_rgbd* r, int32_t stream, int32_t* n) {
  return rgbd_device_only(r, "vslam_rgbd_get_map_size", RGBD_HOST_NO_MAP, [&](RgbdDev& d) {
    if (!n) { d.err = "vslam_rgbd_get_map_size: null output"; return (int)VSLAM_ERR_INVALID; }
    return d.map_ready(stream, false, n);
  });
}
VS_API int vslam_rgbd_get_map(vslam_rgbd* r, int32_t stream, int32_t first_id, int32_t cap, int32_t* n, double* xyz, int32_t* info3, uint8_t* desc) {
  return rgbd_device_only(r, "vslam_rgbd_get_map", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.get_map(stream, first_id, cap, n, xyz, info3, desc); });
}
VS_API int vslam_rgbd_enable_observations(vslam_rgbd* r, int32_t cap) {
  return rgbd_device_only(r, "vslam_rgbd_enable_observations", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.enable_observations(cap); });
}
VS_API int vslam_rgbd_get_observation_count(vslam_rgbd* r, int32_t stream, int32_t* n) {
  return rgbd_device_only(r, "vslam_rgbd_get_observation_count", RGBD_HOST_NO_MAP, [&](RgbdDev& d) {
    if (!n) { d.err = "vslam_rgbd_get_observation_count: null output"; return (int)VSLAM_ERR_INVALID; }
    return d.map_ready(stream, true, n);
  });
}
VS_API int vslam_rgbd_get_observations(vslam_rgbd* r, int32_t stream, int32_t first, int32_t cap, int32_t* n, int32_t* id_frame2, float* xy, double* cam) {
  return rgbd_device_only(r, "vslam_rgbd_get_observations", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.get_observations(stream, first, cap, n, id_frame2, xy, cam); });
}
VS_API int vslam_rgbd_get_point_ids(vslam_rgbd* r, int32_t stream, int32_t cap, int32_t* n, int32_t* ids) {
  return rgbd_device_only(r, "vslam_rgbd_get_point_ids", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.get_point_ids(stream, cap, n, ids); });
}
VS_API int vslam_rgbd_enable_map_colors(vslam_rgbd* r, int on) {
  return rgbd_device_only(r, "vslam_rgbd_enable_map_colors", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.enable_map_colors(on); });
}
VS_API int vslam_rgbd_get_map_colors(vslam_rgbd* r, int32_t stream, int32_t first_id, int32_t cap, int32_t* n, uint8_t* rgb) {
  return rgbd_device_only(r, "vslam_rgbd_get_map_colors", RGBD_HOST_NO_MAP, [&](RgbdDev& d) { return d.get_map_colors(stream, first_id, cap, n, rgb); });
}
VS_API int vslam_rgbd_set_undistortion(vslam_rgbd* r, int32_t raw_rows, int32_t raw_cols, const int16_t* map_xy, const uint16_t* map_a) {
  return rgbd_device_only(r, "vslam_rgbd_set_undistortion", RGBD_HOST_NO_UNDISTORT, [&](RgbdDev& d) { return d.set_undistortion(raw_rows, raw_cols, map_xy, map_a); });
}
VS_API int vslam_rgbd_get_undistorted(vslam_rgbd* r, int32_t stream, uint8_t* image, uint16_t* depth) {
  return rgbd_device_only(r, "vslam_rgbd_get_undistorted", RGBD_HOST_NO_UNDISTORT, [&](RgbdDev& d) { return d.get_undistorted(stream, image, depth); });
}
VS_API int vslam_rgbd_set_equalization(vslam_rgbd* r, int on) {
  return rgbd_device_only(r, "vslam_rgbd_set_equalization", RGBD_HOST_NO_EQUALIZE, [&](RgbdDev& d) { return d.set_equalization(on); });
}
VS_API int vslam_rgbd_get_equalized(vslam_rgbd* r, int32_t stream, uint8_t* image) {
  return rgbd_device_only(r, "vslam_rgbd_get_equalized", RGBD_HOST_NO_EQUALIZE, [&](RgbdDev& d) { return d.get_equalized(stream, image); });
}
VS_API int vslam_rgbd_set_clahe(vslam_rgbd* r, int on, double clip_limit, int tiles_x, int tiles_y) {
  return rgbd_device_only(r, "vslam_rgbd_set_clahe", RGBD_HOST_NO_EQUALIZE, [&](RgbdDev& d) { return d.set_clahe(on, clip_limit, tiles_x, tiles_y); });
}
VS_API int vslam_rgbd_get_clahe_luts(vslam_rgbd* r, int32_t stream, uint8_t* luts) {
  return rgbd_device_only(r, "vslam_rgbd_get_clahe_luts", RGBD_HOST_NO_EQUALIZE, [&](RgbdDev& d) { return d.get_clahe_luts(stream, luts); });
}
VS_API int vslam_rgbd_set_detection_mask(vslam_rgbd* r, const uint8_t* mask, int32_t row_stride, int32_t margin) {
  return rgbd_device_only(r, "vslam_rgbd_set_detection_mask", RGBD_HOST_NO_MASK, [&](RgbdDev& d) { return d.set_detection_mask(mask, row_stride, margin); });
}
VS_API int vslam_rgbd_set_frame_masks(vslam_rgbd* r, const uint8_t* masks, int32_t row_stride, size_t image_stride, int32_t margin, int on_device) {
  return rgbd_device_only(r, "vslam_rgbd_set_frame_masks", RGBD_HOST_NO_MASK, [&](RgbdDev& d) { return d.set_frame_masks(masks, row_stride, image_stride, margin, on_device != 0); });
}
VS_API int vslam_rgbd_get_frame_detection_mask(vslam_rgbd* r, int32_t stream, uint64_t* words) {
  return rgbd_device_only(r, "vslam_rgbd_get_frame_detection_mask", RGBD_HOST_NO_MASK, [&](RgbdDev& d) { return d.get_frame_detection_mask(stream, words); });
}
VS_API int vslam_rgbd_set_undistortion_mask(vslam_rgbd* r, int on, int32_t margin) {
  return rgbd_device_only(r, "vslam_rgbd_set_undistortion_mask", RGBD_HOST_NO_MASK, [&](RgbdDev& d) { return d.set_undistortion_mask(on, margin); });
}
VS_API int vslam_rgbd_get_detection_mask(vslam_rgbd* r, uint64_t* words) {
  return rgbd_device_only(r, "vslam_rgbd_get_detection_mask", RGBD_HOST_NO_MASK, [&](RgbdDev& d) { return d.get_detection_mask(words); });
}
VS_API int vslam_rgbd_set_bilateral(vslam_rgbd* r, int on, double sigma_color, double sigma_space) {
  return rgbd_device_only(r, "vslam_rgbd_set_bilateral", RGBD_HOST_NO_BILATERAL, [&](RgbdDev& d) { return d.set_bilateral(on, sigma_color, sigma_space); });
}
VS_API int vslam_rgbd_get_bilateral(vslam_rgbd* r, int* on, double* sigma_color, double* sigma_space) {
  return rgbd_device_only(r, "vslam_rgbd_get_bilateral", RGBD_HOST_NO_BILATERAL, [&](RgbdDev& d) { return d.get_bilateral(on, sigma_color, sigma_space); });
}
VS_API int vslam_rgbd_get_filtered_depth(vslam_rgbd* r, int32_t stream, uint16_t* depth, float* lut4098) {
  return rgbd_device_only(r, "vslam_rgbd_get_filtered_depth", RGBD_HOST_NO_BILATERAL, [&](RgbdDev& d) { return d.get_filtered_depth(stream, depth, lut4098); });
}
VS_API int vslam_rgbd_set_color_input(vslam_rgbd* r, int format) {
  return rgbd_device_only(r, "vslam_rgbd_set_color_input", RGBD_HOST_NO_COLOR, [&](RgbdDev& d) { return d.set_color_input(format); });
}
VS_API int vslam_rgbd_get_gray(vslam_rgbd* r, int32_t stream, uint8_t* image) {
  return rgbd_device_only(r, "vslam_rgbd_get_gray", RGBD_HOST_NO_COLOR, [&](RgbdDev& d) { return d.get_gray(stream, image); });
}
VS_API int vslam_rgbd_set_downscale(vslam_rgbd* r, int32_t factor, int32_t full_rows, int32_t full_cols) {
  return rgbd_device_only(r, "vslam_rgbd_set_downscale", RGBD_HOST_NO_DOWNSCALE, [&](RgbdDev& d) { return d.set_downscale(factor, full_rows, full_cols); });
}
VS_API int vslam_rgbd_get_downscaled(vslam_rgbd* r, int32_t stream, uint8_t* image, uint16_t* depth) {
  return rgbd_device_only(r, "vslam_rgbd_get_downscaled", RGBD_HOST_NO_DOWNSCALE, [&](RgbdDev& d) { return d.get_downscaled(stream, image, depth); });
}
VS_API int vslam_rgbd_set_smoothing(vslam_rgbd* r, int mode, int32_t ksize) {
  return rgbd_device_only(r, "vslam_rgbd_set_smoothing", RGBD_HOST_NO_SMOOTHING, [&](RgbdDev& d) { return d.set_smoothing(mode, ksize); });
}
VS_API int vslam_rgbd_get_smoothed(vslam_rgbd* r, int32_t stream, uint8_t* image) {
  return rgbd_device_only(r, "vslam_rgbd_get_smoothed", RGBD_HOST_NO_SMOOTHING, [&](RgbdDev& d) { return d.get_smoothed(stream, image); });
}
// the switches' getters: on the host-driven loop every switch reads as off
VS_API int vslam_rgbd_get_undistortion_mask(vslam_rgbd* r, int* on, int32_t* margin) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) { if (on) *on = 0; if (margin) *margin = 0; return VSLAM_OK; }
  return r->d.get_undistortion_mask(on, margin);
}
VS_API int vslam_rgbd_get_downscale(vslam_rgbd* r, int32_t* factor, int32_t* full_rows, int32_t* full_cols) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) DownscaleSwitch().get(factor, full_rows, full_cols); else r->d.get_downscale(factor, full_rows, full_cols);
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_smoothing(vslam_rgbd* r, int* mode, int32_t* ksize) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) SmoothSwitch().get(mode, ksize); else r->d.get_smoothing(mode, ksize);
  return VSLAM_OK;
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
