// host_switches.h — the stereo context's input-stage switches and their getters: rectification (vslam_set_rectification), the equalisation
// slot (vslam_set_equalization, vslam_set_clahe), colour input (vslam_set_color_input), the downscale (vslam_set_downscale) and smoothing (vslam_set_smoothing), the stores behind them, and the stand-alone
// vslam_remap_u8; behind them the motion model and the pose guesses of CAMERA_ODOMETRY (vslam_set_motion_model, vslam_set_pose_guess*),
// with launch_motion_prior, the head of the frame's launch sequence.  What the switches share with the RGB-D tracker is host_prestage.h; a frame's routing through the stages is route_frame
// in host_frame.h.  Host code, included by vslam_hip.hip after host_ctx.h and ahead of host_frame.h.
#pragma once

// ---- the stores ------------------------------------------------------------------------------------
static void rect_free(vslam_ctx* c) {
  c->rect.mem.release();
  c->rect = vslam_ctx::Rect();
}
static void eq_free(vslam_ctx* c) {
  c->eq.release();
  c->eq.keep_mem.release();
  c->eq.keep[0] = c->eq.keep[1] = nullptr;
}
// the rectified pair's own slabs exist exactly while rectification and equalisation are both on and smoothing, which then takes the
// rectified pair into sm.in, is off (called by the three setters, queues idle)
static hipError_t eq_keep_sync(vslam_ctx* c) {
  vslam_ctx::Eq& q = c->eq;
  const bool want = q.on && c->rect.on && !c->sm.mode;
  if (want == (q.keep[0] != nullptr)) return hipSuccess;
  q.keep_mem.release();
  q.keep[0] = q.keep[1] = nullptr;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && want && e == hipSuccess; ++k) e = q.keep_mem.alloc(&q.keep[k], (size_t)c->B * c->up_stream_stride);
  if (e != hipSuccess) { q.keep_mem.release(); q.keep[0] = q.keep[1] = nullptr; }
  return e;
}
static void col_free(vslam_ctx* c) {
  c->col.mem.release();
  c->col = vslam_ctx::Col();
}
static void sm_free(vslam_ctx* c) {
  c->sm.mem.release();
  c->sm.out_mem.release();
  c->sm = vslam_ctx::Sm();
}
// the smoothed pair's own slabs exist exactly while smoothing and equalisation are both on (called by the setters of both, queues idle)
static hipError_t sm_out_sync(vslam_ctx* c) {
  vslam_ctx::Sm& q = c->sm;
  const bool want = q.mode && c->eq.on;
  if (want == (q.out[0] != nullptr)) return hipSuccess;
  q.out_mem.release();
  q.out[0] = q.out[1] = nullptr;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && want && e == hipSuccess; ++k) e = q.out_mem.alloc(&q.out[k], (size_t)c->B * c->up_stream_stride);
  if (e != hipSuccess) { q.out_mem.release(); q.out[0] = q.out[1] = nullptr; }
  return e;
}
static void ds_free(vslam_ctx* c) {
  c->ds.mem.release();
  c->ds = vslam_ctx::Ds();
}
// the size of the frames that come in: the full size while downscaling, else the raw size while rectification is set, else rows x cols
static void incoming_size(const vslam_ctx* c, int* rows, int* cols) {
  if (c->ds.factor > 1) { *rows = c->ds.full_rows; *cols = c->ds.full_cols; }
  else if (c->rect.on) { *rows = c->rect.maps.raw_rows; *cols = c->rect.maps.raw_cols; }
  else { *rows = c->cfg.c.rows; *cols = c->cfg.c.cols; }
}
// the colour slabs exist while the switch is on, at the size of the frames that come in (called by the three setters that change it,
// queues idle)
static hipError_t col_slab_sync(vslam_ctx* c) {
  vslam_ctx::Col& q = c->col;
  const int fmt = q.format;
  int rows, cols;
  incoming_size(c, &rows, &cols);
  const int wb = fmt == VSLAM_PIXEL_GRAY8 ? 0 : gray_channels(fmt) * cols;
  if (fmt != 0 && q.slab[0][0] && q.slab_rows == rows && q.slab_cols == wb) return hipSuccess;
  col_free(c);
  q.format = fmt;
  if (fmt == 0) return hipSuccess;
  q.slab_rows = rows; q.slab_cols = wb;
  q.stride = (wb + 63) & ~63;
  q.stream_stride = (size_t)rows * q.stride;
  hipError_t e = hipSuccess;
  for (int p = 0; p < 2; ++p) for (int k = 0; k < 2 && e == hipSuccess; ++k) e = q.mem.alloc(&q.slab[p][k], (size_t)c->B * q.stream_stride);
  if (e != hipSuccess) col_free(c);
  return e;
}
// the slabs of the context as image pairs: upload[set], and where k_rectify writes the pair of product set `set` (with equalisation on as
// well: in slabs of its own, the equalised pair goes to upload[set])
static ImgPlanes upload_planes(const vslam_ctx* c, int set) { return {{c->upload[set][0], c->upload[set][1]}, c->up_stride, c->up_stream_stride}; }
static ImgPlanes unsmoothed_planes(const vslam_ctx* c, int set) { return {{c->sm.in[set][0], c->sm.in[set][1]}, c->up_stride, c->up_stream_stride}; }
static ImgPlanes rectified_planes(const vslam_ctx* c, int set) {
  if (c->sm.mode) return unsmoothed_planes(c, set);
  return c->eq.keep[0] ? ImgPlanes{{c->eq.keep[0], c->eq.keep[1]}, c->up_stride, c->up_stream_stride} : upload_planes(c, set);
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
  // while downscaling, the maps address the reduced raw image: full / factor is what this stage is handed
  if (c->ds.factor > 1) {
    const int want_rows = off ? rows : raw_rows, want_cols = off ? cols : raw_cols;
    if (ds_out(c->ds.full_rows, c->ds.factor) != want_rows || ds_out(c->ds.full_cols, c->ds.factor) != want_cols)
      return fail(c, VSLAM_ERR_INVALID, off ? "vslam_set_rectification: the downscaled frames (vslam_set_downscale) do not have the context's size"
                                            : "vslam_set_rectification: the raw size is not the size of the downscaled frames (vslam_set_downscale)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old maps and raw slabs
  rect_free(c);
  const bool valid_on = c->dmask.valid_on;       // the maps' validity mask: recomputed from new maps, off with them
  const int valid_margin = c->dmask.valid_margin;
  if (valid_on) { mask_valid_free(c); c->dmask.last = 0; }
  if (off) { (void)eq_keep_sync(c); return col_slab_sync(c) == hipSuccess ? VSLAM_OK : fail(c, VSLAM_ERR_HIP, "vslam_set_rectification: colour slabs"); }
  vslam_ctx::Rect& q = c->rect;
  q.raw_stride = (raw_cols + 63) & ~63;
  q.raw_stream_stride = (size_t)raw_rows * q.raw_stride;
  hipError_t e = remap_maps_upload(q.mem, q.maps, 2, raw_rows, raw_cols, rows, cols, xy, a);
  for (int k = 0; k < 2; ++k)
    for (int p = 0; p < 2 && e == hipSuccess; ++p) e = q.mem.alloc(&q.raw[p][k], (size_t)c->B * q.raw_stream_stride);
  if (e != hipSuccess) { rect_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_rectification: ") + hipGetErrorString(e)); }
  q.on = true;
  e = eq_keep_sync(c);
  if (e == hipSuccess) e = col_slab_sync(c);
  if (e == hipSuccess && valid_on) e = mask_valid_build(c, valid_margin);
  if (e != hipSuccess) { mask_valid_free(c); rect_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_rectification: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
}
VS_API int vslam_get_rectified_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_rectified_images: null output");
  if (!c->rect.on || !c->rect.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_rectified_images: no frame has been rectified since vslam_set_rectification");
  return pair_to_host(c, rectified_planes(c, c->last_set), s, c->cfg.c.rows, c->cfg.c.cols, left, right);
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
  const int rc = c->eq.switch_to(on, geo, clip_limit, c->B, 2, names, &why,
                                 [&] { (void)hipSetDevice(c->device); sync_all(c); eq_free(c); },     // the frames in flight still read the tables and the slabs
                                 [&] { const hipError_t e = eq_keep_sync(c); return e == hipSuccess ? sm_out_sync(c) : e; });
  if (!c->eq.on) (void)sm_out_sync(c);      // switched off: the smoothed pair goes to upload[parity] again (this can only free)
  return rc ? fail(c, rc, why) : VSLAM_OK;
}
VS_API int vslam_set_equalization(vslam_ctx* c, int on) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_equalization called inside a frame");
  if ((size_t)c->cfg.c.rows * c->cfg.c.cols > (size_t)VS_EQ_MAX_PIXELS) return fail(c, VSLAM_ERR_INVALID, "vslam_set_equalization: more than 2^24 pixels per image");
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
  if (format < VSLAM_PIXEL_GRAY8 || format > VSLAM_PIXEL_RGBA8) return fail(c, VSLAM_ERR_INVALID, "vslam_set_color_input: unknown pixel format");
  if (format == c->col.format) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the slabs
  if (format == VSLAM_PIXEL_GRAY8) mapcol_free(c);     // no colour left to sample
  col_free(c);
  c->col.format = format;
  const hipError_t e = col_slab_sync(c);
  if (e != hipSuccess) { col_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_color_input: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
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
  if (factor != 1) {
    if (!ds_factor_ok(factor)) return fail(c, VSLAM_ERR_INVALID, "vslam_set_downscale: factor outside 1 .. 4");
    if (!ds_size_ok(full_rows, full_cols, factor)) return fail(c, VSLAM_ERR_INVALID, "vslam_set_downscale: full size outside 1 .. 32767 or below one block");
    const int want_rows = c->rect.on ? c->rect.maps.raw_rows : c->cfg.c.rows, want_cols = c->rect.on ? c->rect.maps.raw_cols : c->cfg.c.cols;
    if (ds_out(full_rows, factor) != want_rows || ds_out(full_cols, factor) != want_cols)
      return fail(c, VSLAM_ERR_INVALID, c->rect.on ? "vslam_set_downscale: full size / factor is not the raw size of the rectification maps"
                                                   : "vslam_set_downscale: full size / factor is not the context's image size");
  }
  if (c->sticky != VSLAM_OK) return c->sticky;
  const vslam_ctx::Ds& q = c->ds;
  if (factor == 1 ? q.factor == 1 : (q.factor == factor && q.full_rows == full_rows && q.full_cols == full_cols)) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the slabs
  ds_free(c);
  hipError_t e = hipSuccess;
  if (factor != 1) {
    vslam_ctx::Ds& d = c->ds;
    d.factor = factor; d.full_rows = full_rows; d.full_cols = full_cols;
    d.stride = (full_cols + 63) & ~63;
    d.stream_stride = (size_t)full_rows * d.stride;
    for (int p = 0; p < 2; ++p) for (int k = 0; k < 2 && e == hipSuccess; ++k) e = d.mem.alloc(&d.full[p][k], (size_t)c->B * d.stream_stride);
  }
  if (e == hipSuccess) e = col_slab_sync(c);     // colour frames come in at the new size
  if (e != hipSuccess) { ds_free(c); (void)col_slab_sync(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_downscale: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
}
VS_API int vslam_get_downscale(vslam_ctx* c, int32_t* factor, int32_t* full_rows, int32_t* full_cols) {
  if (!c) return VSLAM_ERR_INVALID;
  if (factor) *factor = c->ds.factor;
  if (full_rows) *full_rows = c->ds.factor > 1 ? c->ds.full_rows : 0;
  if (full_cols) *full_cols = c->ds.factor > 1 ? c->ds.full_cols : 0;
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
static_assert(VSLAM_SMOOTH_OFF == VS_SMOOTH_OFF && VSLAM_SMOOTH_GAUSSIAN == VS_SMOOTH_GAUSSIAN && VSLAM_SMOOTH_MEDIAN == VS_SMOOTH_MEDIAN, "smoothing modes");
// what both setters and the stand-alone entry refuse: 0, or VSLAM_ERR_INVALID with *why filled
static int smooth_check(const char* who, int mode, int32_t ksize, int rows, int cols, std::string* why) {
  const char* what = nullptr;
  if (mode != VSLAM_SMOOTH_GAUSSIAN && mode != VSLAM_SMOOTH_MEDIAN) what = ": unknown mode";
  else if (!smooth_mode_ok(mode, ksize)) what = mode == VSLAM_SMOOTH_GAUSSIAN ? ": a Gaussian has ksize 3, 5 or 7" : ": a median has ksize 3 or 5";
  else if (!smooth_size_ok(mode, ksize, rows, cols)) what = ": a Gaussian needs rows and cols above ksize / 2";
  if (!what) return VSLAM_OK;
  *why = std::string(who) + what;
  return VSLAM_ERR_INVALID;
}
VS_API int vslam_set_smoothing(vslam_ctx* c, int mode, int32_t ksize) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_smoothing called inside a frame");
  std::string why;
  if (mode != VSLAM_SMOOTH_OFF)
    if (const int rc = smooth_check("vslam_set_smoothing", mode, ksize, c->cfg.c.rows, c->cfg.c.cols, &why)) return fail(c, rc, why);
  if (c->sticky != VSLAM_OK) return c->sticky;
  vslam_ctx::Sm& q = c->sm;
  if (mode == VSLAM_SMOOTH_OFF ? q.mode == VSLAM_SMOOTH_OFF : (q.mode == mode && q.ksize == ksize)) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the slabs
  if (mode != VSLAM_SMOOTH_OFF && q.mode != VSLAM_SMOOTH_OFF) { q.mode = mode; q.ksize = ksize; q.have_frame = false; return VSLAM_OK; }     // the slabs stay
  sm_free(c);
  hipError_t e = hipSuccess;
  if (mode != VSLAM_SMOOTH_OFF) {
    for (int p = 0; p < 2; ++p) for (int k = 0; k < 2 && e == hipSuccess; ++k) e = q.mem.alloc(&q.in[p][k], (size_t)c->B * c->up_stream_stride);
    if (e == hipSuccess) { q.mode = mode; q.ksize = ksize; e = sm_out_sync(c); }
  }
  if (e == hipSuccess) e = eq_keep_sync(c);
  if (e != hipSuccess) { sm_free(c); (void)eq_keep_sync(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_smoothing: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
}
VS_API int vslam_get_smoothing(vslam_ctx* c, int* mode, int32_t* ksize) {
  if (!c) return VSLAM_ERR_INVALID;
  if (mode) *mode = c->sm.mode;
  if (ksize) *ksize = c->sm.mode ? c->sm.ksize : 0;
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
// k_mask_pack on `n` streams of `sides` masks; fused when a.corner is set
static void mask_pack_enqueue(hipStream_t st, const MaskPackArgs& a) {
  hipLaunchKernelGGL(k_mask_pack, dim3((a.TX + VS_MASK_CW - 1) / VS_MASK_CW, (a.rows + VS_MASK_BR - 1) / VS_MASK_BR, a.n * a.sides), dim3(256), 0, st, a);
}
// what both setters refuse about a mask's geometry
static int mask_args_check(vslam_ctx* c, const char* who, int32_t row_stride, int32_t margin) {
  if (margin < 0 || margin > VS_MASK_MAX_MARGIN) return fail(c, VSLAM_ERR_INVALID, std::string(who) + ": margin outside 0 .. 64");
  if (row_stride < c->cfg.c.cols) return fail(c, VSLAM_ERR_INVALID, std::string(who) + ": row stride smaller than image width");
  return VSLAM_OK;
}
// k_mask_apply: corner words [n][2][nw] &= stat (stat_stream_stride 0: shared by the streams, else the stream's own words [n][nw] of side 0)
static void mask_apply_enqueue(hipStream_t st, const MaskApplyArgs& a) {
  hipLaunchKernelGGL(k_mask_apply, dim3(((a.nw + 1) / 2 + 255) / 256, a.sides, (a.n + VS_MASK_SB - 1) / VS_MASK_SB), dim3(256), 0, st, a);
}
// k_map_valid on `sides` maps of m: the eroded validity words [sides][rows][TX] into dst
static void map_valid_enqueue(hipStream_t st, const RemapMaps& m, int sides, int margin, unsigned long long* dst) {
  MapValidArgs v{};
  for (int k = 0; k < sides; ++k) { v.map_xy[k] = m.xy[k]; v.map_a[k] = m.a[k]; }
  v.map_stride = m.stride; v.raw_rows = m.raw_rows; v.raw_cols = m.raw_cols;
  v.rows = m.rows; v.cols = m.cols; v.TX = (m.cols + 63) / 64; v.margin = margin; v.sides = sides; v.dst = dst;
  hipLaunchKernelGGL(k_map_valid, dim3((v.TX + VS_MASK_CW - 1) / VS_MASK_CW, (v.rows + VS_MASK_BR - 1) / VS_MASK_BR, sides), dim3(256), 0, st, v);
}
// The context-wide keep words of `sides` images out of the user's words and the maps' validity words: the one there is, or both ANDed in
// `comb` ([2][nw]: the validity words copied, the user's applied by k_mask_apply as to one stream's corner words).  Queues idle.
static hipError_t mask_static_combine(hipStream_t st, int sides, size_t nw, unsigned long long* const* user, unsigned long long* const* valid,
                                      DeviceStore& comb_mem, unsigned long long** comb, unsigned long long** stat) {
  comb_mem.release();
  comb[0] = comb[1] = nullptr;
  bool both = false;
  for (int k = 0; k < sides; ++k) { stat[k] = user[k] ? user[k] : valid[k]; both = both || (user[k] && valid[k]); }
  if (!both) return hipSuccess;
  unsigned long long* base = nullptr;
  hipError_t e = comb_mem.alloc(&base, 2 * nw);
  if (e != hipSuccess) return e;
  MaskApplyArgs a{};
  a.corner = base; a.nw = (int32_t)nw; a.n = 1; a.sides = sides;
  active_all(a.active, 1);
  for (int k = 0; k < sides && e == hipSuccess; ++k) {
    if (!(user[k] && valid[k])) continue;
    comb[k] = base + (size_t)k * nw;
    e = hipMemcpyAsync(comb[k], valid[k], nw * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st);
    a.stat[k] = user[k];
    stat[k] = comb[k];
  }
  if (e == hipSuccess) { mask_apply_enqueue(st, a); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e;
}
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
  const size_t nw = (size_t)c->cfg.c.rows * c->cfg.TX;
  q.valid_mem.release();
  q.valid[0] = q.valid[1] = nullptr;
  unsigned long long* base = nullptr;
  hipError_t e = q.valid_mem.alloc(&base, 2 * nw);
  if (e == hipSuccess) { map_valid_enqueue(c->stream, c->rect.maps, 2, margin, base); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) { q.valid[0] = base; q.valid[1] = base + nw; q.valid_on = true; q.valid_margin = margin; e = mask_static_sync(c); }
  return e;
}
VS_API int vslam_set_rectification_mask(vslam_ctx* c, int on, int32_t margin) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_rectification_mask called inside a frame");
  if (on && (margin < 0 || margin > VS_MASK_MAX_MARGIN)) return fail(c, VSLAM_ERR_INVALID, "vslam_set_rectification_mask: margin outside 0 .. 64");
  if (on && !c->rect.on) return fail(c, VSLAM_ERR_STATE, "vslam_set_rectification_mask: no rectification maps are set (vslam_set_rectification)");
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (!on && !c->dmask.valid_on) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old words
  c->dmask.last = 0;               // no frame has run under the new setting
  if (!on) { mask_valid_free(c); return VSLAM_OK; }
  const hipError_t e = mask_valid_build(c, margin);
  if (e != hipSuccess) { mask_valid_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_rectification_mask: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
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
  if (!off) if (int rc = mask_args_check(c, "vslam_set_detection_mask", row_stride, margin)) return rc;
  if (c->sticky != VSLAM_OK) return c->sticky;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old words
  mask_static_free(c);
  c->dmask.last = 0;               // no frame has run under the new setting
  if (off) return VSLAM_OK;
  vslam_ctx::DetMask& q = c->dmask;
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols, TX = c->cfg.TX;
  const size_t bytes = (size_t)(rows - 1) * row_stride + cols;
  const uint8_t* const src[2] = {left, right};
  uint8_t* tmp = nullptr;
  hipError_t e = hipMalloc((void**)&tmp, bytes);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    if (!src[k]) continue;
    e = q.user_mem.alloc(&q.user[k], (size_t)rows * TX);
    if (e == hipSuccess) e = hipMemcpy(tmp, src[k], bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) break;
    MaskPackArgs a{};
    a.src[0] = tmp; a.src_row_stride = row_stride; a.rows = rows; a.cols = cols; a.TX = TX; a.margin = margin; a.n = 1; a.sides = 1;
    a.dst = q.user[k];
    active_all(a.active, 1);
    mask_pack_enqueue(c->stream, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);     // tmp is refilled for the other side
  }
  if (tmp) (void)hipFree(tmp);
  if (e == hipSuccess) e = mask_static_sync(c);
  if (e != hipSuccess) { mask_static_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_detection_mask: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
}
VS_API int vslam_set_frame_masks(vslam_ctx* c, const uint8_t* left, const uint8_t* right, int32_t row_stride, size_t image_stride, int32_t margin, int on_device) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_frame_masks called inside a frame");
  vslam_ctx::DetMask& q = c->dmask;
  if (!left && !right) { q.pending = false; return VSLAM_OK; }
  if (int rc = mask_args_check(c, "vslam_set_frame_masks", row_stride, margin)) return rc;
  if (c->B > 1 && image_stride < (size_t)(c->cfg.c.rows - 1) * row_stride + c->cfg.c.cols)
    return fail(c, VSLAM_ERR_INVALID, "vslam_set_frame_masks: image stride smaller than one mask");
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
