// host_switches.h — the stereo context's input-stage switches and their getters: rectification (vslam_set_rectification), the equalisation
// slot (vslam_set_equalization, vslam_set_clahe), colour input (vslam_set_color_input), the downscale (vslam_set_downscale) and smoothing
// (vslam_set_smoothing), and the stand-alone vslam_remap_u8; behind them the motion model and the pose guesses of CAMERA_ODOMETRY
// (vslam_set_motion_model, vslam_set_pose_guess*) with launch_motion_prior, the head of the frame's launch sequence, and the detection masks.
// Which slabs the stages own is stage_plan.h's decision: slabs_reconcile is the one function that allocates and frees them, and every
// setter has one shape — check, unchanged? return, drain, change the switch, reconcile, on failure turn that switch off and reconcile
// again.  Should that second reconcile fail as well, slabs_settle turns colour input (with the map's colours) and the equalisation slot off
// too, without a word of its own: the caller learns of the switch it was setting, and the getters of the others show them off.  The checks and what else the switches share with the RGB-D tracker are host_prestage.h; a frame's routing is route_frame in
// host_frame.h.  Host code, included by vslam_hip.hip after host_ctx.h and ahead of host_frame.h.
#pragma once

// ---- the slabs of the input stages ------------------------------------------------------------------
// the switch state that the plan (stage_plan.h) is a function of
static StageSwitches stage_switches(const vslam_ctx* c) {
  StageSwitches s;
  s.channels = c->col.format == VSLAM_PIXEL_GRAY8 ? 0 : gray_channels(c->col.format);
  s.factor = c->ds.factor; s.full_rows = c->ds.full_rows; s.full_cols = c->ds.full_cols;
  s.remap = c->rect.on; s.raw_rows = c->rect.maps.raw_rows; s.raw_cols = c->rect.maps.raw_cols;
  s.smooth = c->sm.mode != VSLAM_SMOOTH_OFF; s.slot = c->eq.on;
  s.rows = c->cfg.c.rows; s.cols = c->cfg.c.cols; s.up_stride = c->up_stride;
  assert(c->up_stream_stride == (size_t)s.rows * s.up_stride);     // the plan's slabs at the processed size have upload[parity]'s strides
  return s;
}
// The context's slabs brought into agreement with the plan; queues idle.  The one place that allocates or frees them.  Colour slabs that go
// or change their size (another format, another size of the frames that come in) take the grey pair's getter with them until the next frame.
static hipError_t slabs_reconcile(vslam_ctx* c) {
  SlabGeom want[SLAB_OWNED];
  stage_slabs(stage_switches(c), want);
  if (!(c->slabs.geo[SLAB_COLOR] == want[SLAB_COLOR])) c->col.have_frame = false;
  return (hipError_t)stage_slabs_reconcile(c->slabs, want, c->B);
}
// Behind a failed reconcile, with the switch that wanted more off again: what is left frees, or puts back a slab that was freed to make room
// (the colour slabs at the size that comes in again, the rectified pair's own).  Should even that fail, colour input and the slot go off
// as well (and with the colour the map's colours, as vslam_set_color_input(GRAY8) does), and then the plan only frees.
static void slabs_settle(vslam_ctx* c) {
  if (slabs_reconcile(c) == hipSuccess) return;
  mapcol_free(c);
  c->col = vslam_ctx::Col();
  c->eq.release();
  (void)slabs_reconcile(c);
}
static int hip_status(vslam_ctx* c, const char* who, hipError_t e) {
  return e == hipSuccess ? VSLAM_OK : fail(c, VSLAM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
}
// What a setter ends in, queues idle and its switch changed: the slabs follow.  When an allocation fails, off() turns that switch off again.
template <class Off>
static int slabs_follow(vslam_ctx* c, const char* who, Off&& off) {
  const hipError_t e = slabs_reconcile(c);
  if (e != hipSuccess) { off(); slabs_settle(c); }
  return hip_status(c, who, e);
}
// slab `id` of step parity `set` as an image pair: SLAB_UPLOAD is upload[set]; a slab of one pair serves both parities
static ImgPlanes slab_planes(const vslam_ctx* c, int id, int set) {
  if (id == SLAB_UPLOAD) return {{c->upload[set][0], c->upload[set][1]}, c->up_stride, c->up_stream_stride};
  const SlabGeom& g = c->slabs.geo[id];
  uint8_t* const* p = c->slabs.p[id][g.pairs == 2 ? set : 0];
  return {{p[0], p[1]}, g.stride, g.stream_stride()};
}
static void rect_off(vslam_ctx* c) {
  c->rect.mem.release();
  c->rect = vslam_ctx::Rect();
}
// both sides of stream s of a pair, rows x cols, dense
static int pair_to_host(vslam_ctx* c, const ImgPlanes& x, int s, int rows, int cols, uint8_t* left, uint8_t* right) {
  for (int k = 0; k < 2; ++k) HIP_TRY(c, planes_to_host(k ? right : left, x, k, s, rows, cols));
  return VSLAM_OK;
}

// ---- rectification of raw input pairs ------------------------------------------------------------
static void mask_valid_free(vslam_ctx* c);                       // the maps' validity mask (below, with the detection masks)
static hipError_t mask_valid_build(vslam_ctx* c, int margin);
VS_API int vslam_set_rectification(vslam_ctx* c, int32_t raw_rows, int32_t raw_cols, const int16_t* xyL, const uint16_t* aL, const int16_t* xyR,
                                   const uint16_t* aR) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_rectification called inside a frame");
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols;
  const int16_t* const xy[2] = {xyL, xyR};
  const uint16_t* const a[2] = {aL, aR};
  bool off = false;
  std::string why;
  if (const int rc = remap_maps_check("vslam_set_rectification", 2, raw_rows, raw_cols, rows, cols, xy, a, &off, &why)) return fail(c, rc, why);
  if (const int rc = remap_downscale_check(VS_CONTEXT_WORDS, c->ds, off, raw_rows, raw_cols, rows, cols, &why)) return fail(c, rc, why);
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old maps and raw slabs
  rect_off(c);
  const bool valid_on = c->dmask.valid_on;       // the maps' validity mask: recomputed from new maps, off with them
  const int valid_margin = c->dmask.valid_margin;
  if (valid_on) { mask_valid_free(c); c->dmask.last = 0; }
  if (off) {                       // the rectified pair's own slabs go; colour frames come in at another size
    if (slabs_reconcile(c) == hipSuccess) return VSLAM_OK;
    slabs_settle(c);
    return fail(c, VSLAM_ERR_HIP, "vslam_set_rectification: colour slabs");
  }
  hipError_t e = remap_maps_upload(c->rect.mem, c->rect.maps, 2, raw_rows, raw_cols, rows, cols, xy, a);
  c->rect.on = e == hipSuccess;
  if (e == hipSuccess) e = slabs_reconcile(c);
  if (e == hipSuccess && valid_on) e = mask_valid_build(c, valid_margin);
  if (e != hipSuccess) { mask_valid_free(c); rect_off(c); slabs_settle(c); }
  return hip_status(c, "vslam_set_rectification", e);
}
VS_API int vslam_get_rectified_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_rectified_images: null output");
  if (!c->rect.on || !c->rect.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_rectified_images: no frame has been rectified since vslam_set_rectification");
  return pair_to_host(c, slab_planes(c, stage_route(stage_switches(c), false).remap.dst, c->last_set), s, c->cfg.c.rows, c->cfg.c.cols, left, right);
}
VS_API int vslam_remap_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, const int16_t* map_xy,
                          const uint16_t* map_a, int32_t drows, int32_t dcols, uint8_t* dst) {
  if (!c) return VSLAM_ERR_INVALID;
  tmp_reset(c);
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (!src || !dst || !map_xy || !map_a || rows < 1 || cols < 1 || row_stride < cols || drows < 1 || dcols < 1)
    return fail(c, VSLAM_ERR_INVALID, "remap: bad argument");
  if (!rect_maps_ok(map_a, (size_t)drows * dcols)) return fail(c, VSLAM_ERR_INVALID, "remap: interpolation table index >= 1024");
  HIP_TRY(c, hipSetDevice(c->device));
  RemapMaps m;
  m.rows = drows; m.cols = dcols; m.raw_rows = rows; m.raw_cols = cols;
  m.stride = (dcols + 3) & ~3;
  std::vector<int16_t> pxy;
  std::vector<uint16_t> pa;
  rect_pad_maps(map_xy, map_a, drows, dcols, m.stride, pxy, pa);
  uint8_t *ds = nullptr, *dd = nullptr;
  hipError_t e = tmp_get(c, (void**)&ds, (size_t)rows * row_stride);
  if (e == hipSuccess) e = tmp_get(c, (void**)&m.xy[0], pxy.size() * 2);
  if (e == hipSuccess) e = tmp_get(c, (void**)&m.a[0], pa.size() * 2);
  if (e == hipSuccess) e = tmp_get(c, (void**)&dd, (size_t)drows * m.stride);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, src, (size_t)(rows - 1) * row_stride + cols, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m.xy[0], pxy.data(), pxy.size() * 2, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m.a[0], pa.data(), pa.size() * 2, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    uint32_t active[VS_MAX_STREAMS / 32];
    active_all(active, 1);
    remap_enqueue(c->stream, m, ImgPlanes{{ds, nullptr}, row_stride, 0}, ImgPlanes{{dd, nullptr}, m.stride, (size_t)drows * m.stride}, 1, 1, active);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy2DAsync(dst, dcols, dd, m.stride, dcols, drows, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, VSLAM_ERR_HIP, hipGetErrorString(e));
  return VSLAM_OK;
}

// ---- the equalisation slot of the input pair: global (kernels_equalize.h) or CLAHE (kernels_clahe.h) ---------------
// geo null: global equalisation, else CLAHE with what clahe_geometry made of the caller's arguments
static int eq_switch(vslam_ctx* c, bool on, const ClaheArgs* geo, double clip_limit) {
  static const char* const names[2] = {"vslam_set_equalization", "vslam_set_clahe"};
  std::string why;
  const bool was_on = c->eq.on;
  const int rc = c->eq.switch_to(on, geo, clip_limit, c->B, 2, names, &why,
                                 [&] { (void)hipSetDevice(c->device); sync_all(c); c->eq.release(); },     // the frames in flight still read the tables and the slabs
                                 [&] { return slabs_reconcile(c); });
  if ((was_on || rc) && !c->eq.on) slabs_settle(c);      // switched off, or back off behind a failure: the pairs ahead of the slot go to upload[parity] again
  return rc ? fail(c, rc, why) : VSLAM_OK;
}
VS_API int vslam_set_equalization(vslam_ctx* c, int on) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_equalization called inside a frame");
  std::string why;
  if (const int rc = equalization_size_check(VS_CONTEXT_WORDS, c->cfg.c.rows, c->cfg.c.cols, &why)) return fail(c, rc, why);
  return eq_switch(c, on != 0, nullptr, 0);
}
VS_API int vslam_set_clahe(vslam_ctx* c, int on, double clip_limit, int tiles_x, int tiles_y) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_clahe called inside a frame");
  ClaheArgs geo;
  std::memset(&geo, 0, sizeof geo);
  const char* why = "";
  if (on && !clahe_geometry(c->cfg.c.rows, c->cfg.c.cols, clip_limit, tiles_x, tiles_y, geo, &why)) return fail(c, VSLAM_ERR_INVALID, std::string("vslam_set_clahe: ") + why);
  return eq_switch(c, on != 0, &geo, clip_limit);
}
static int eq_readable(vslam_ctx* c, int s, const char* who) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (!c->eq.on || !c->eq.have_frame) return fail(c, VSLAM_ERR_STATE, std::string(who) + ": no frame has been equalised since vslam_set_equalization");
  return VSLAM_OK;
}
VS_API int vslam_get_equalized_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  if (int rc = eq_readable(c, s, "vslam_get_equalized_images")) return rc;
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_equalized_images: null output");
  return pair_to_host(c, c->eq.dst, s, c->cfg.c.rows, c->cfg.c.cols, left, right);
}
VS_API int vslam_get_equalization_histograms(vslam_ctx* c, int s, uint32_t* hist512) {
  if (int rc = eq_readable(c, s, "vslam_get_equalization_histograms")) return rc;
  if (c->eq.clahe) return fail(c, VSLAM_ERR_STATE, "vslam_get_equalization_histograms: the context runs CLAHE, which keeps tables per tile (vslam_get_clahe_luts)");
  if (!hist512) return fail(c, VSLAM_ERR_INVALID, "vslam_get_equalization_histograms: null output");
  HIP_TRY(c, c->eq.hist_to_host(hist512, s));
  return VSLAM_OK;
}
VS_API int vslam_get_clahe_luts(vslam_ctx* c, int s, uint8_t* luts) {
  if (int rc = eq_readable(c, s, "vslam_get_clahe_luts")) return rc;
  if (!c->eq.clahe) return fail(c, VSLAM_ERR_STATE, "vslam_get_clahe_luts: the context runs global equalisation, not CLAHE");
  if (!luts) return fail(c, VSLAM_ERR_INVALID, "vslam_get_clahe_luts: null output");
  HIP_TRY(c, c->eq.luts_to_host(luts, s));
  return VSLAM_OK;
}

// ---- colour input (kernels_gray.h) ---------------------------------------------------------------
VS_API int vslam_set_color_input(vslam_ctx* c, int format) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_color_input called inside a frame");
  std::string why;
  if (const int rc = color_format_check(VS_CONTEXT_WORDS, format, &why)) return fail(c, rc, why);
  if (format == c->col.format) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the slabs
  if (format == VSLAM_PIXEL_GRAY8) mapcol_free(c);     // no colour left to sample
  c->col = vslam_ctx::Col();
  c->col.format = format;
  return slabs_follow(c, "vslam_set_color_input", [&] { c->col = vslam_ctx::Col(); });
}
VS_API int vslam_get_gray_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (c->col.format == VSLAM_PIXEL_GRAY8 || !c->col.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_gray_images: no frame has been converted since vslam_set_color_input");
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_gray_images: null output");
  return pair_to_host(c, c->pre.gray, s, c->pre.in_rows, c->pre.in_cols, left, right);
}

// ---- integer-factor reduction of the incoming frames (kernels_downscale.h) ----------------------------------------
VS_API int vslam_set_downscale(vslam_ctx* c, int32_t factor, int32_t full_rows, int32_t full_cols) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_downscale called inside a frame");
  const bool remap = c->rect.on;
  std::string why;
  if (const int rc = downscale_check(VS_CONTEXT_WORDS, factor, full_rows, full_cols, remap, remap ? c->rect.maps.raw_rows : c->cfg.c.rows,
                                     remap ? c->rect.maps.raw_cols : c->cfg.c.cols, &why)) return fail(c, rc, why);
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (c->ds.is(factor, full_rows, full_cols)) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the slabs
  c->ds = vslam_ctx::Ds();
  if (factor != 1) { c->ds.factor = factor; c->ds.full_rows = full_rows; c->ds.full_cols = full_cols; }     // colour frames come in at the new size, too
  return slabs_follow(c, "vslam_set_downscale", [&] { c->ds = vslam_ctx::Ds(); });
}
VS_API int vslam_get_downscale(vslam_ctx* c, int32_t* factor, int32_t* full_rows, int32_t* full_cols) {
  if (!c) return VSLAM_ERR_INVALID;
  c->ds.get(factor, full_rows, full_cols);
  return VSLAM_OK;
}
VS_API int vslam_get_downscaled_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (c->ds.factor == 1 || !c->ds.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_downscaled_images: no frame has been downscaled since vslam_set_downscale");
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_downscaled_images: null output");
  return pair_to_host(c, c->pre.reduced, s, c->pre.red_rows, c->pre.red_cols, left, right);
}

// ---- smoothing of the grey pair ahead of the equalisation slot (kernels_smooth.h) ------------------------------------
VS_API int vslam_set_smoothing(vslam_ctx* c, int mode, int32_t ksize) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_smoothing called inside a frame");
  std::string why;
  if (mode != VSLAM_SMOOTH_OFF)
    if (const int rc = smooth_check("vslam_set_smoothing", mode, ksize, c->cfg.c.rows, c->cfg.c.cols, &why)) return fail(c, rc, why);
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (c->sm.is(mode, ksize)) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the slabs
  c->sm = vslam_ctx::Sm();         // from one mode to another the plan is the same: the slabs stay
  if (mode != VSLAM_SMOOTH_OFF) { c->sm.mode = mode; c->sm.ksize = ksize; }
  return slabs_follow(c, "vslam_set_smoothing", [&] { c->sm = vslam_ctx::Sm(); });
}
VS_API int vslam_get_smoothing(vslam_ctx* c, int* mode, int32_t* ksize) {
  if (!c) return VSLAM_ERR_INVALID;
  c->sm.get(mode, ksize);
  return VSLAM_OK;
}
VS_API int vslam_get_smoothed_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (!c->sm.mode || !c->sm.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_smoothed_images: no frame has been smoothed since vslam_set_smoothing / vslam_reset");
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_smoothed_images: null output");
  return pair_to_host(c, c->pre.smoothed, s, c->cfg.c.rows, c->cfg.c.cols, left, right);
}

// ---- motion models and the pose guesses of CAMERA_ODOMETRY (kernels_motion.h) --------------------------------------
VS_API int vslam_set_motion_model(vslam_ctx* c, int model, int32_t dead_reckoning_limit) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_motion_model called inside a frame");
  if (model < VSLAM_MOTION_CONSTANT_VELOCITY || model > VSLAM_MOTION_CAMERA_ODOMETRY) return fail(c, VSLAM_ERR_INVALID, "vslam_set_motion_model: unknown motion model");
  if (dead_reckoning_limit < 0) return fail(c, VSLAM_ERR_INVALID, "vslam_set_motion_model: negative dead_reckoning_limit");
  if (dead_reckoning_limit > 0 && model != VSLAM_MOTION_CAMERA_ODOMETRY) return fail(c, VSLAM_ERR_INVALID, "vslam_set_motion_model: dead_reckoning_limit needs VSLAM_MOTION_CAMERA_ODOMETRY");
  if (model == c->cfg.motion_model && dead_reckoning_limit == c->cfg.dead_reckoning_limit) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the configuration's device copy
  c->cfg.motion_model = model; c->cfg.dead_reckoning_limit = dead_reckoning_limit;
  HIP_TRY(c, hipMemcpy(c->d_cfg, &c->cfg, sizeof(DevCfg), hipMemcpyHostToDevice));
  return VSLAM_OK;
}
VS_API int vslam_get_motion_model(vslam_ctx* c, int* model, int32_t* dead_reckoning_limit) {
  if (!c) return VSLAM_ERR_INVALID;
  if (model) *model = c->cfg.motion_model;
  if (dead_reckoning_limit) *dead_reckoning_limit = c->cfg.dead_reckoning_limit;
  return VSLAM_OK;
}
// the host side of the guesses set one stream at a time or as a host array, with the first one
static void guess_host_ready(vslam_ctx* c) {
  vslam_ctx::Guess& g = c->guess;
  if (g.mask.empty()) { g.host.assign((size_t)c->B * 12, 0.0); g.mask.assign((size_t)c->B, 0); }
}
// their device copy and its pinned staging, with the first frame that hands them over (never under CONSTANT_VELOCITY)
static int guess_store_ready(vslam_ctx* c) {
  vslam_ctx::Guess& g = c->guess;
  if (g.d_host) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipError_t e = g.mem.alloc(&g.d_host, (size_t)c->B * 12);
  if (e == hipSuccess) e = g.mem.alloc(&g.d_mask, (size_t)c->B);
  for (int q = 0; q < 2 && e == hipSuccess; ++q) {
    void* h = nullptr;
    e = hipHostMalloc(&h, (size_t)c->B * (12 * sizeof(double) + sizeof(int32_t)), hipHostMallocDefault);
    if (e == hipSuccess) { g.pin[q] = (unsigned char*)h; e = hipEventCreateWithFlags(&g.pin_ev[q], hipEventDisableTiming); }
  }
  if (e != hipSuccess) {
    g.mem.release(); g.d_host = nullptr; g.d_mask = nullptr;
    for (int q = 0; q < 2; ++q) { if (g.pin[q]) (void)hipHostFree(g.pin[q]); if (g.pin_ev[q]) (void)hipEventDestroy(g.pin_ev[q]); g.pin[q] = nullptr; g.pin_ev[q] = nullptr; }
    return fail(c, VSLAM_ERR_HIP, std::string("pose guess store: ") + hipGetErrorString(e));
  }
  return VSLAM_OK;
}
VS_API int vslam_set_pose_guess(vslam_ctx* c, int s, const double T[12]) {
  if (int rc = check_stream_index(c, s)) return rc;
  if (!T) return fail(c, VSLAM_ERR_INVALID, "vslam_set_pose_guess: null pose");
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_pose_guess called inside a frame");
  guess_host_ready(c);
  std::memcpy(&c->guess.host[(size_t)s * 12], T, 12 * sizeof(double));
  c->guess.mask[s] = 1; c->guess.any = true;
  return VSLAM_OK;
}
VS_API int vslam_set_pose_guesses(vslam_ctx* c, const double* T, int on_device) {
  if (!c) return VSLAM_ERR_INVALID;
  if (!T) return fail(c, VSLAM_ERR_INVALID, "vslam_set_pose_guesses: null array");
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_pose_guesses called inside a frame");
  guess_host_ready(c);
  vslam_ctx::Guess& g = c->guess;
  if (on_device) {                 // supersedes what was set before it, stream by stream or as a host array
    g.dev = T; std::fill(g.mask.begin(), g.mask.end(), 0); g.any = false;
    return VSLAM_OK;
  }
  std::memcpy(g.host.data(), T, (size_t)c->B * 12 * sizeof(double));
  std::fill(g.mask.begin(), g.mask.end(), 1);
  g.dev = nullptr; g.any = true;
  return VSLAM_OK;
}
// Head of the frame's launch sequence, on the queue the candidate kernel runs on.  Under CONSTANT_VELOCITY nothing is launched, copied or
// allocated: host guesses stay where they are (the first frame under another model hands them over), a device array ends with the frame.  The host's guesses leave from pinned staging, two buffers in turn: a buffer is refilled once the copy that last read it is done.
static int launch_motion_prior(vslam_ctx* c) {
  vslam_ctx::Guess& g = c->guess;
  if (c->cfg.motion_model == VSLAM_MOTION_CONSTANT_VELOCITY) { g.dev = nullptr; return VSLAM_OK; }
  GuessSrc src = {g.dev, nullptr, nullptr};
  if (g.any) {
    if (int rc = guess_store_ready(c)) return rc;
    const int q = g.turn;
    g.turn ^= 1;
    if (g.pin_used[q]) HIP_TRY(c, hipEventSynchronize(g.pin_ev[q]));
    const size_t nb = g.host.size() * sizeof(double), mb = g.mask.size() * sizeof(int32_t);
    std::memcpy(g.pin[q], g.host.data(), nb);
    std::memcpy(g.pin[q] + nb, g.mask.data(), mb);
    HIP_TRY(c, hipMemcpyAsync(g.d_host, g.pin[q], nb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(g.d_mask, g.pin[q] + nb, mb, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipEventRecord(g.pin_ev[q], c->stream));
    g.pin_used[q] = true;
    src.host = g.d_host; src.mask = g.d_mask;
  }
  hipLaunchKernelGGL(k_motion_prior, dim3((c->B + 63) / 64), dim3(64), 0, c->stream, c->buf, c->B, c->cfg.motion_model, src);
  HIP_TRY(c, hipGetLastError());
  guess_drop_pending(c);
  return VSLAM_OK;
}
// ---- detection masks (kernels_mask.h) ------------------------------------------------------------------------------
static hipError_t mask_static_sync(vslam_ctx* c) {
  vslam_ctx::DetMask& q = c->dmask;
  return mask_static_combine(c->stream, 2, (size_t)c->cfg.c.rows * c->cfg.TX, q.user, q.valid, q.comb_mem, q.comb, q.stat);
}
static void mask_static_free(vslam_ctx* c) {
  c->dmask.user_mem.release();
  c->dmask.user[0] = c->dmask.user[1] = nullptr;
  (void)mask_static_sync(c);     // what is left: the validity words, or nothing
}
static void mask_valid_free(vslam_ctx* c) {
  c->dmask.valid_mem.release();
  c->dmask.valid[0] = c->dmask.valid[1] = nullptr;
  c->dmask.valid_on = false; c->dmask.valid_margin = 0;
  (void)mask_static_sync(c);
}
// the validity words of the maps the context holds (queues idle, rectification on)
static hipError_t mask_valid_build(vslam_ctx* c, int margin) {
  vslam_ctx::DetMask& q = c->dmask;
  hipError_t e = mask_valid_words(c->stream, c->rect.maps, 2, margin, (size_t)c->cfg.c.rows * c->cfg.TX, q.valid_mem, q.valid);
  if (e == hipSuccess) { q.valid_on = true; q.valid_margin = margin; e = mask_static_sync(c); }
  return e;
}
VS_API int vslam_set_rectification_mask(vslam_ctx* c, int on, int32_t margin) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_rectification_mask called inside a frame");
  std::string why;
  if (on) if (const int rc = mask_margin_check("vslam_set_rectification_mask", margin, &why)) return fail(c, rc, why);
  if (on && !c->rect.on) return fail(c, VSLAM_ERR_STATE, "vslam_set_rectification_mask: no rectification maps are set (vslam_set_rectification)");
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (!on && !c->dmask.valid_on) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old words
  c->dmask.last = 0;               // no frame has run under the new setting
  if (!on) { mask_valid_free(c); return VSLAM_OK; }
  const hipError_t e = mask_valid_build(c, margin);
  if (e != hipSuccess) mask_valid_free(c);
  return hip_status(c, "vslam_set_rectification_mask", e);
}
VS_API int vslam_get_rectification_mask(vslam_ctx* c, int* on, int32_t* margin) {
  if (!c) return VSLAM_ERR_INVALID;
  if (on) *on = c->dmask.valid_on ? 1 : 0;
  if (margin) *margin = c->dmask.valid_on ? c->dmask.valid_margin : 0;
  return VSLAM_OK;
}
VS_API int vslam_set_detection_mask(vslam_ctx* c, const uint8_t* left, const uint8_t* right, int32_t row_stride, int32_t margin) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_detection_mask called inside a frame");
  const bool off = !left && !right;
  std::string why;
  if (!off) if (const int rc = mask_args_check("vslam_set_detection_mask", c->cfg.c.cols, row_stride, margin, &why)) return fail(c, rc, why);
  if (c->sticky != VSLAM_OK) return c->sticky;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old words
  mask_static_free(c);
  c->dmask.last = 0;               // no frame has run under the new setting
  if (off) return VSLAM_OK;
  const uint8_t* const src[2] = {left, right};
  hipError_t e = mask_static_upload(c->stream, 2, src, row_stride, c->cfg.c.rows, c->cfg.c.cols, c->cfg.TX, margin, c->dmask.user_mem, c->dmask.user);
  if (e == hipSuccess) e = mask_static_sync(c);
  if (e != hipSuccess) mask_static_free(c);
  return hip_status(c, "vslam_set_detection_mask", e);
}
VS_API int vslam_set_frame_masks(vslam_ctx* c, const uint8_t* left, const uint8_t* right, int32_t row_stride, size_t image_stride, int32_t margin, int on_device) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_frame_masks called inside a frame");
  vslam_ctx::DetMask& q = c->dmask;
  if (!left && !right) { q.pending = false; return VSLAM_OK; }
  std::string why;
  if (const int rc = frame_masks_check("vslam_set_frame_masks", c->B, c->cfg.c.rows, c->cfg.c.cols, row_stride, image_stride, margin, &why)) return fail(c, rc, why);
  if (c->sticky != VSLAM_OK) return c->sticky;
  q.pending = true; q.on_device = on_device != 0;
  q.src[0] = left; q.src[1] = right; q.row_stride = row_stride; q.image_stride = image_stride; q.margin = margin;
  return VSLAM_OK;
}
// Ahead of k_fast_box: what the frame's mask launch needs that can fail — the effective words, and the host masks' copy into the slab on
// the queue the launch goes to (the previous frame's launch, the slab's last reader, ran on the same queue or is ordered ahead of it by
// launch_image_pipeline's own waits).  Consumes the pending set.
static int mask_prepare(vslam_ctx* c, hipStream_t st) {
  vslam_ctx::DetMask& q = c->dmask;
  q.job_ready = false;
  if (!q.pending) return VSLAM_OK;
  q.pending = false;
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols, TX = c->cfg.TX, B = c->B;
  if (!q.eff) HIP_TRY(c, q.eff_mem.alloc(&q.eff, (size_t)B * 2 * rows * TX));
  const uint8_t* src[2] = {q.src[0], q.src[1]};
  if (!q.on_device) {
    const size_t one = (size_t)(rows - 1) * q.row_stride + cols, span = (size_t)(B - 1) * q.image_stride + one;
    if (q.slab_bytes < span) {
      sync_all(c);                 // the last frame's launch may still read the old slabs
      q.slab_mem.release(); q.slab[0] = q.slab[1] = nullptr; q.slab_bytes = 0;
      for (int k = 0; k < 2; ++k) HIP_TRY(c, q.slab_mem.alloc(&q.slab[k], span));
      q.slab_bytes = span;
    }
    bool all_active = true;
    for (int s = 0; s < B; ++s) all_active = all_active && ((c->buf.active[s >> 5] >> (s & 31)) & 1u);
    for (int k = 0; k < 2; ++k) {
      if (!src[k]) continue;
      if (all_active) HIP_TRY(c, hipMemcpyAsync(q.slab[k], src[k], span, hipMemcpyHostToDevice, st));
      else   // the mask of a switched-off stream is not read
        for (int s = 0; s < B; ++s)
          if ((c->buf.active[s >> 5] >> (s & 31)) & 1u)
            HIP_TRY(c, hipMemcpyAsync(q.slab[k] + (size_t)s * q.image_stride, src[k] + (size_t)s * q.image_stride, one, hipMemcpyHostToDevice, st));
      src[k] = q.slab[k];
    }
  }
  MaskPackArgs& a = q.job;
  a = MaskPackArgs{};
  a.src[0] = src[0]; a.src[1] = src[1]; a.src_stream_stride = q.image_stride; a.src_row_stride = q.row_stride;
  a.rows = rows; a.cols = cols; a.TX = TX; a.margin = q.margin; a.n = B; a.sides = 2;
  a.dst = q.eff; a.stat[0] = q.stat[0]; a.stat[1] = q.stat[1]; a.corner_sides = 2;
  q.job_ready = true;
  return VSLAM_OK;
}
// Between k_fast_box and k_emit, on their queue: the frame masks' fused pack / erode / apply, else the static words' apply, else nothing.
static void mask_enqueue(vslam_ctx* c, hipStream_t st, const DevBuf& bs) {
  vslam_ctx::DetMask& q = c->dmask;
  const bool stat = q.stat[0] || q.stat[1];
  if (q.job_ready) {
    q.job.corner = bs.mask;
    std::memcpy(q.job.active, bs.active, sizeof q.job.active);
    mask_pack_enqueue(st, q.job);
    q.job_ready = false;
    q.last = 2 | (stat ? 1 : 0);
    std::memcpy(q.last_active, bs.active, sizeof q.last_active);
  } else if (stat) {
    MaskApplyArgs a{};
    a.stat[0] = q.stat[0]; a.stat[1] = q.stat[1]; a.corner = bs.mask; a.nw = c->cfg.c.rows * c->cfg.TX; a.n = c->B; a.sides = 2;
    std::memcpy(a.active, bs.active, sizeof a.active);
    mask_apply_enqueue(st, a);
    q.last = 1;
    std::memcpy(q.last_active, bs.active, sizeof q.last_active);
  } else q.last = 0;
}
// k_emit over `streams` streams of `sides` images each (kernels_image.h): one workgroup per band of VS_EMIT_BAND mask words.
// run_controller: 0 none, 1 over a stream's two images, 2 over its one image.
static void launch_emit(hipStream_t st, const DevCfg& cfg, const DevBuf& buf, int streams, int sides, int border, int run_controller) {
  const int bands = (cfg.c.rows * cfg.TX + VS_EMIT_BAND - 1) / VS_EMIT_BAND;
  hipLaunchKernelGGL(k_emit, dim3(streams, sides, bands), dim3(VS_EMIT_THREADS), 0, st, cfg, buf, border, run_controller);
}
VS_API int vslam_get_detection_mask(vslam_ctx* c, int s, int side, uint64_t* words) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (side < 0 || side > 1 || !words) return fail(c, VSLAM_ERR_INVALID, "vslam_get_detection_mask: bad side or null output");
  const vslam_ctx::DetMask& q = c->dmask;
  if (!q.last) return fail(c, VSLAM_ERR_STATE, "vslam_get_detection_mask: the last frame used no mask");
  if (!((q.last_active[s >> 5] >> (s & 31)) & 1u)) return fail(c, VSLAM_ERR_STATE, "vslam_get_detection_mask: the stream was switched off during the last frame");
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols, TX = c->cfg.TX;
  const size_t nw = (size_t)rows * TX;
  const unsigned long long* from = (q.last & 2) ? q.eff + ((size_t)s * 2 + side) * nw : q.stat[side];
  if (from) { HIP_TRY(c, hipMemcpy(words, from, nw * sizeof(uint64_t), hipMemcpyDeviceToHost)); return VSLAM_OK; }
  for (int r = 0; r < rows; ++r)     // a static mask on the other side only: this one is all-keep
    for (int t = 0; t < TX; ++t) words[(size_t)r * TX + t] = mask_cols_word(t, cols);
  return VSLAM_OK;
}

VS_API int vslam_get_pose_guess(vslam_ctx* c, int s, double guess[12], double guess_previous[12]) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  StreamState* st = c->buf.st + s;
  if (guess) HIP_TRY(c, hipMemcpy(guess, st->guess, sizeof st->guess, hipMemcpyDeviceToHost));
  if (guess_previous) HIP_TRY(c, hipMemcpy(guess_previous, st->guess_prev, sizeof st->guess_prev, hipMemcpyDeviceToHost));
  return VSLAM_OK;
}
