// host_prestage.h — the input stages ahead of the detector, written once for the stereo context and the RGB-D tracker: colour to grey
// (kernels_gray.h), integer-factor reduction (kernels_downscale.h), remap (rectification / undistortion, kernels_rectify.h), smoothing
// (Gaussian / median, kernels_smooth.h) and the equalisation slot (global or CLAHE, kernels_equalize.h / kernels_clahe.h).  Where an image pair lies (ImgPlanes), the one filler of the kernels' argument blocks (place),
// the slot (EqSlot), the intake of remap maps, what the switches' setters refuse (one check each, worded by the owner's vocabulary), the
// per-frame plan (PrePlan) with its one enqueue, the plane read-out of the getters, the colour source of the map's colours and the
// detection masks' launches, static upload and validity words.  Owner-independent host code: no context, no tracker; errors come back as hipError_t or as text.
// Included by vslam_hip.hip ahead of host_ctx.h (the context holds these types); rgbd_device.h uses it too.
#pragma once

// ---- where an image pair lies --------------------------------------------------------------------
// stream s of side k at p[k] + s * stream_stride, rows row_stride bytes apart.  One image per stream (RGB-D): p[1] stays null.
struct ImgPlanes { const uint8_t* p[2] = {nullptr, nullptr}; int32_t row_stride = 0; size_t stream_stride = 0; };
// DevBuf::img*, which the kernels read, pointed at a pair (a one-sided one is mirrored into img[1])
static void buf_set_planes(DevBuf& b, const ImgPlanes& x) {
  b.img[0] = x.p[0]; b.img[1] = x.p[1] ? x.p[1] : x.p[0];
  b.img_row_stride = x.row_stride; b.img_stream_stride = x.stream_stride;
}
// streams 0 .. n - 1 switched on, in the form of DevBuf::active
static void active_all(uint32_t* active, int n) {
  std::memset(active, 0, sizeof(uint32_t) * (VS_MAX_STREAMS / 32));
  for (int s = 0; s < n; ++s) active[s >> 5] |= 1u << (s & 31);
}

// ---- the one argument filler -----------------------------------------------------------------------
// what GrayArgs, DownscaleArgs, SmoothArgs, EqArgs, ClaheArgs and RectArgs have in common
template <class A>
static void place(A& a, const ImgPlanes& src, const ImgPlanes& dst, int rows, int cols, int n, int sides, const uint32_t* active) {
  for (int k = 0; k < 2; ++k) { a.src[k] = src.p[k]; a.dst[k] = const_cast<uint8_t*>(dst.p[k]); }
  a.src_row_stride = src.row_stride; a.src_stream_stride = src.stream_stride;
  a.dst_row_stride = dst.row_stride; a.dst_stream_stride = dst.stream_stride;
  a.rows = rows; a.cols = cols; a.n = n; a.sides = sides;
  std::memcpy(a.active, active, sizeof a.active);
}
// one image (the stand-alone entries)
template <class A>
static void place(A& a, const uint8_t* src, int32_t src_row_stride, uint8_t* dst, int32_t dst_row_stride, int rows, int cols) {
  uint32_t active[VS_MAX_STREAMS / 32];
  active_all(active, 1);
  place(a, ImgPlanes{{src, nullptr}, src_row_stride, 0}, ImgPlanes{{dst, nullptr}, dst_row_stride, 0}, rows, cols, 1, 1, active);
}

// ---- remap maps ------------------------------------------------------------------------------------
// Host maps in the CV_16SC2 + CV_16UC1 layout -> device maps with rows padded to a multiple of 4 entries (the padding is zero: in range,
// never stored), so that every lane's 16-B / 8-B map loads are aligned and inside the allocation.
static int rect_maps_ok(const uint16_t* map_a, size_t n) {
  for (size_t i = 0; i < n; ++i) if (map_a[i] >= 1024) return 0;
  return 1;
}
static void rect_pad_maps(const int16_t* xy, const uint16_t* fa, int rows, int cols, int ms, std::vector<int16_t>& pxy, std::vector<uint16_t>& pa) {
  pxy.assign((size_t)rows * ms * 2, 0);
  pa.assign((size_t)rows * ms, 0);
  for (int r = 0; r < rows; ++r) {
    std::memcpy(&pxy[(size_t)r * ms * 2], xy + (size_t)r * cols * 2, (size_t)cols * 4);
    std::memcpy(&pa[(size_t)r * ms], fa + (size_t)r * cols, (size_t)cols * 2);
  }
}
// the device maps of a switch: `sides` pairs at rows x cols (stride entries per row) over raw images of raw_rows x raw_cols
struct RemapMaps {
  int16_t* xy[2] = {nullptr, nullptr}; uint16_t* a[2] = {nullptr, nullptr};
  int32_t stride = 0, rows = 0, cols = 0, raw_rows = 0, raw_cols = 0;
};
// What a map setter refuses before it touches anything: 0, or the status with *why filled (`who`: the entry's name).  *off: every map
// is null, the switch goes off.
static int remap_maps_check(const char* who, int sides, int raw_rows, int raw_cols, int rows, int cols, const int16_t* const* xy, const uint16_t* const* a,
                            bool* off, std::string* why) {
  int given = 0;
  for (int k = 0; k < sides; ++k) given += (xy[k] != nullptr) + (a[k] != nullptr);
  *off = given == 0;
  if (*off) return VSLAM_OK;
  const char* what = nullptr;
  if (given != 2 * sides) what = sides == 2 ? ": all four maps or none" : ": both maps or none";
  else if (raw_rows < 1 || raw_cols < 1 || raw_rows > 32767 || raw_cols > 32767) what = ": invalid raw image dimensions";
  else
    for (int k = 0; k < sides && !what; ++k)
      if (!rect_maps_ok(a[k], (size_t)rows * cols)) what = ": interpolation table index >= 1024";
  if (!what) return VSLAM_OK;
  *why = std::string(who) + what;
  return VSLAM_ERR_INVALID;
}
// checked maps -> m: padded, allocated from mem and uploaded.  On failure the caller releases mem (it holds the half-built maps).
static hipError_t remap_maps_upload(DeviceStore& mem, RemapMaps& m, int sides, int raw_rows, int raw_cols, int rows, int cols, const int16_t* const* xy,
                                    const uint16_t* const* a) {
  m = RemapMaps();
  m.rows = rows; m.cols = cols; m.raw_rows = raw_rows; m.raw_cols = raw_cols;
  m.stride = (cols + 3) & ~3;
  std::vector<int16_t> pxy;
  std::vector<uint16_t> pa;
  hipError_t e = hipSuccess;
  for (int k = 0; k < sides && e == hipSuccess; ++k) {
    rect_pad_maps(xy[k], a[k], rows, cols, m.stride, pxy, pa);
    e = mem.alloc(&m.xy[k], pxy.size());
    if (e == hipSuccess) e = mem.alloc(&m.a[k], pa.size());
    if (e == hipSuccess) e = hipMemcpy(m.xy[k], pxy.data(), pxy.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m.a[k], pa.data(), pa.size() * 2, hipMemcpyHostToDevice);
  }
  return e;
}
// k_rectify on n streams of `sides` images: src (raw size of m) -> dst (m's own size)
static void remap_enqueue(hipStream_t st, const RemapMaps& m, const ImgPlanes& src, const ImgPlanes& dst, int n, int sides, const uint32_t* active) {
  RectArgs ra{};
  place(ra, src, dst, m.rows, m.cols, n, sides, active);
  for (int k = 0; k < 2; ++k) { ra.map_xy[k] = m.xy[k]; ra.map_a[k] = m.a[k]; }
  ra.map_stride = m.stride; ra.src_rows = m.raw_rows; ra.src_cols = m.raw_cols; ra.s0 = 0;
  dim3 grid = undistort_grid(m.rows, m.cols, n);
  grid.z *= sides;
  hipLaunchKernelGGL(k_rectify, grid, dim3(256), 0, st, ra);
}

// ---- what the switches' setters refuse, written once --------------------------------------------------
// Each check returns 0, or the status with *why filled.  The owner's vocabulary keeps every message what it is for that owner.
struct OwnerWords { const char* prefix; const char* owner; const char* remap; };
static const OwnerWords VS_CONTEXT_WORDS = {"vslam_", "context", "rectification"};
static const OwnerWords VS_TRACKER_WORDS = {"vslam_rgbd_", "tracker", "undistortion"};
static int refuse(std::string* why, int status, const std::string& text) { *why = text; return status; }
// the downscale switch as both owners hold it: off while factor == 1
struct DownscaleSwitch {
  int factor = 1, full_rows = 0, full_cols = 0;
  bool is(int f, int rows, int cols) const { return f == 1 ? factor == 1 : (factor == f && full_rows == rows && full_cols == cols); }
  void get(int32_t* f, int32_t* rows, int32_t* cols) const {
    if (f) *f = factor;
    if (rows) *rows = factor > 1 ? full_rows : 0;
    if (cols) *cols = factor > 1 ? full_cols : 0;
  }
};
// the downscale setter: full / factor must be red_rows x red_cols, what the next stage takes (the raw size while remapping, else the processed size)
static int downscale_check(const OwnerWords& w, int factor, int full_rows, int full_cols, bool remap, int red_rows, int red_cols, std::string* why) {
  if (factor == 1) return VSLAM_OK;
  const std::string who = std::string(w.prefix) + "set_downscale: ";
  if (!ds_factor_ok(factor)) return refuse(why, VSLAM_ERR_INVALID, who + "factor outside 1 .. 4");
  if (!ds_size_ok(full_rows, full_cols, factor)) return refuse(why, VSLAM_ERR_INVALID, who + "full size outside 1 .. 32767 or below one block");
  if (ds_out(full_rows, factor) == red_rows && ds_out(full_cols, factor) == red_cols) return VSLAM_OK;
  return refuse(why, VSLAM_ERR_INVALID, who + "full size / factor is not the " + (remap ? std::string("raw size of the ") + w.remap + " maps" : std::string(w.owner) + "'s image size"));
}
// the remap setter while downscaling: the maps address the reduced raw image, full / factor is what this stage is handed (off: the detector)
static int remap_downscale_check(const OwnerWords& w, const DownscaleSwitch& ds, bool off, int raw_rows, int raw_cols, int rows, int cols, std::string* why) {
  if (ds.factor == 1 || (ds_out(ds.full_rows, ds.factor) == (off ? rows : raw_rows) && ds_out(ds.full_cols, ds.factor) == (off ? cols : raw_cols))) return VSLAM_OK;
  const std::string who = std::string(w.prefix) + "set_" + w.remap, ds_name = std::string(" (") + w.prefix + "set_downscale)";
  return refuse(why, VSLAM_ERR_INVALID, off ? who + ": the downscaled frames" + ds_name + " do not have the " + w.owner + "'s size"
                                            : who + ": the raw size is not the size of the downscaled frames" + ds_name);
}
static int color_format_check(const OwnerWords& w, int format, std::string* why) {
  return format < VSLAM_PIXEL_GRAY8 || format > VSLAM_PIXEL_RGBA8 ? refuse(why, VSLAM_ERR_INVALID, std::string(w.prefix) + "set_color_input: unknown pixel format") : VSLAM_OK;
}
static int equalization_size_check(const OwnerWords& w, int rows, int cols, std::string* why) {
  return (size_t)rows * cols > (size_t)VS_EQ_MAX_PIXELS ? refuse(why, VSLAM_ERR_INVALID, std::string(w.prefix) + "set_equalization: more than 2^24 pixels per image") : VSLAM_OK;
}
// the smoothing switch as both owners hold it: off while mode == VSLAM_SMOOTH_OFF
static_assert(VSLAM_SMOOTH_OFF == VS_SMOOTH_OFF && VSLAM_SMOOTH_GAUSSIAN == VS_SMOOTH_GAUSSIAN && VSLAM_SMOOTH_MEDIAN == VS_SMOOTH_MEDIAN, "smoothing modes");
struct SmoothSwitch {
  int mode = 0, ksize = 0;
  bool is(int m, int k) const { return m == VSLAM_SMOOTH_OFF ? mode == VSLAM_SMOOTH_OFF : (mode == m && ksize == k); }
  void get(int* m, int32_t* k) const {
    if (m) *m = mode;
    if (k) *k = mode ? ksize : 0;
  }
};
// what both setters and the stand-alone entry refuse about a mode that is not OFF
static int smooth_check(const char* who, int mode, int32_t ksize, int rows, int cols, std::string* why) {
  const char* what = nullptr;
  if (mode != VSLAM_SMOOTH_GAUSSIAN && mode != VSLAM_SMOOTH_MEDIAN) what = ": unknown mode";
  else if (!smooth_mode_ok(mode, ksize)) what = mode == VSLAM_SMOOTH_GAUSSIAN ? ": a Gaussian has ksize 3, 5 or 7" : ": a median has ksize 3 or 5";
  else if (!smooth_size_ok(mode, ksize, rows, cols)) what = ": a Gaussian needs rows and cols above ksize / 2";
  return what ? refuse(why, VSLAM_ERR_INVALID, std::string(who) + what) : VSLAM_OK;
}
// the mask setters (`who`: the entry's name): the margin; a static mask's rows; a set of frame masks, one per stream image_stride apart
static int mask_margin_check(const char* who, int32_t margin, std::string* why) {
  return margin < 0 || margin > VS_MASK_MAX_MARGIN ? refuse(why, VSLAM_ERR_INVALID, std::string(who) + ": margin outside 0 .. 64") : VSLAM_OK;
}
static int mask_args_check(const char* who, int cols, int32_t row_stride, int32_t margin, std::string* why) {
  if (const int rc = mask_margin_check(who, margin, why)) return rc;
  return row_stride < cols ? refuse(why, VSLAM_ERR_INVALID, std::string(who) + ": row stride smaller than image width") : VSLAM_OK;
}
static int frame_masks_check(const char* who, int n, int rows, int cols, int32_t row_stride, size_t image_stride, int32_t margin, std::string* why) {
  if (const int rc = mask_args_check(who, cols, row_stride, margin, why)) return rc;
  return n > 1 && image_stride < (size_t)(rows - 1) * row_stride + cols ? refuse(why, VSLAM_ERR_INVALID, std::string(who) + ": image stride smaller than one mask") : VSLAM_OK;
}

// ---- the equalisation slot -------------------------------------------------------------------------
// Global equalisation (k_hist_u8, k_equalize_apply: the count table [image][256], zeroed and refilled every frame) or CLAHE (k_clahe_lut,
// k_clahe_apply: the tables [image][tilesY][tilesX][256], geo holding what clahe_geometry made of the switch's arguments), image = stream *
// sides + side.  The two modes exclude each other; switching one off while the other is on changes nothing.  The owner says which
// queues drain before a switch and what else goes with it, and when have_frame holds; src / dst are this frame's routing.
struct EqSlot {
  bool on = false, clahe = false, have_frame = false;
  double clip_limit = 0;
  ClaheArgs geo{};
  uint32_t* hist = nullptr;
  uint8_t* luts = nullptr;
  int sides = 0;
  DeviceStore mem;
  ImgPlanes src, dst;
  size_t luts_per_image() const { return (size_t)geo.tiles_x * geo.tiles_y * 256; }

  void release() {
    mem.release();
    on = clahe = have_frame = false; clip_limit = 0; geo = ClaheArgs{}; hist = nullptr; luts = nullptr; sides = 0; src = dst = ImgPlanes();
  }
  // The switch.  new_geo null: global equalisation, else CLAHE; names: the two entries {global, CLAHE}, for the messages; tables for n *
  // sides_ images, zeroed.  clear(): the owner drains its queues and frees the slot (release()) with what goes with it; more(): it
  // allocates what it routes through.  0, or the status with *why filled.
  template <class Clear, class More>
  int switch_to(bool want, const ClaheArgs* new_geo, double new_clip, int n, int sides_, const char* const names[2], std::string* why, Clear&& clear, More&& more) {
    const bool want_clahe = new_geo != nullptr;
    if (on && clahe != want_clahe) {
      if (!want) return VSLAM_OK;
      *why = std::string(names[want_clahe]) + (want_clahe ? ": global equalisation is on (" : ": CLAHE is on (") + names[!want_clahe] + ")";
      return VSLAM_ERR_STATE;
    }
    const bool same = !want_clahe || (clip_limit == new_clip && geo.tiles_x == new_geo->tiles_x && geo.tiles_y == new_geo->tiles_y);
    if (want ? (on && same) : !on) return VSLAM_OK;
    clear();
    if (!want) return VSLAM_OK;
    const size_t images = (size_t)n * sides_;
    hipError_t e;
    if (!want_clahe) {
      e = mem.alloc(&hist, images * 256);
      if (e == hipSuccess) e = hipMemset(hist, 0, images * 256 * sizeof(uint32_t));
    } else {
      geo = *new_geo; clip_limit = new_clip;
      e = mem.alloc(&luts, images * luts_per_image());
      if (e == hipSuccess) e = hipMemset(luts, 0, images * luts_per_image());
    }
    on = e == hipSuccess;
    clahe = on && want_clahe;
    sides = sides_;
    if (e == hipSuccess) e = more();
    if (e == hipSuccess) return VSLAM_OK;
    clear();
    *why = std::string(names[want_clahe]) + ": " + hipGetErrorString(e);
    return VSLAM_ERR_HIP;
  }
  // src -> dst (may be src: in place) on streams 0 .. n - 1
  hipError_t enqueue(hipStream_t st, int rows, int cols, int n, int sides_, const uint32_t* active) const {
    if (clahe) { ClaheArgs ca = geo; place(ca, src, dst, rows, cols, n, sides_, active); ca.luts = luts; return clahe_enqueue(st, ca); }
    EqArgs ea{};
    place(ea, src, dst, rows, cols, n, sides_, active);
    ea.hist = hist;
    return equalize_enqueue(st, ea);
  }
  // the tables of stream s: uint32 [sides][256] / uint8 [sides][tilesY][tilesX][256]
  hipError_t hist_to_host(uint32_t* out, int s) const { return hipMemcpy(out, hist + (size_t)s * sides * 256, (size_t)sides * 256 * sizeof(uint32_t), hipMemcpyDeviceToHost); }
  hipError_t luts_to_host(uint8_t* out, int s) const { return hipMemcpy(out, luts + (size_t)s * sides * luts_per_image(), sides * luts_per_image(), hipMemcpyDeviceToHost); }
};

// ---- a frame's plan and its enqueue ----------------------------------------------------------------
// Which stage runs on this frame and where it reads and writes; the slot's part is EqSlot::on / src / dst.  Each owner fills it in ONE
// function (route_frame in host_frame.h, which reads the route from stage_plan.h, and in rgbd_device.h), from which switches are on and whether the
// frame is the caller's device memory.
//
// Stereo: stage_route of stage_plan.h is the table (the final pair is always in upload[parity], except an untouched caller device pair;
// smoothing never works in place, the slot does when the pair already lies in upload[parity]).  The getters read where a stage wrote.
// RGB-D (single buffers; caller memory is never written):
//   grey      d_img (host) or caller memory                                      col.gray
//   downscale previous                                                           ds.img (the depth image: on the space map's queue)
//   undistort previous                                                           und.img
//   smooth    previous                                                           sm.img
//   equalise  previous                                                           in place if the image is ours (host frame, grey,
//                                                                                undistorted, smoothed), else eq.img
// (so vslam_rgbd_get_smoothed, like vslam_rgbd_get_undistorted, returns the equalised image while the slot is on: it works in place)
struct PrePlan {
  int format = 0;               // VSLAM_PIXEL_*: the grey stage runs unless GRAY8
  bool remap = false;
  int factor = 1;               // the downscale stage runs unless 1
  int in_rows = 0, in_cols = 0; // the frames that come in (the full size while downscaling, else the raw size while remapping)
  int red_rows = 0, red_cols = 0; // downscale: the reduced size (the raw size while remapping, else rows x cols)
  int rows = 0, cols = 0;       // the size the detector works on
  ImgPlanes color, gray;        // grey stage: source, result (in_rows x in_cols)
  ImgPlanes full, reduced;      // downscale: source (in_rows x in_cols), result (red_rows x red_cols)
  ImgPlanes raw, mapped;        // remap: source (in_rows x in_cols), result (rows x cols)
  int smooth_mode = 0, smooth_ksize = 0;   // VSLAM_SMOOTH_*: the smoothing stage runs unless OFF
  ImgPlanes unsmoothed, smoothed;          // smoothing: source, result (rows x cols); never the same memory
};
// grey, then downscale, then remap, then smooth, then equalise, on one queue
static hipError_t prestage_enqueue(hipStream_t st, const PrePlan& pl, const RemapMaps& maps, const EqSlot& eq, int n, int sides, const uint32_t* active) {
  if (pl.format != VSLAM_PIXEL_GRAY8) {
    GrayArgs ga{};
    place(ga, pl.color, pl.gray, pl.in_rows, pl.in_cols, n, sides, active);
    ga.format = pl.format;
    const hipError_t e = gray_enqueue(st, ga);
    if (e != hipSuccess) return e;
  }
  if (pl.factor > 1) {
    DownscaleArgs da{};
    place(da, pl.full, pl.reduced, pl.red_rows, pl.red_cols, n, sides, active);
    da.factor = pl.factor;
    const hipError_t e = downscale_enqueue(st, da);
    if (e != hipSuccess) return e;
  }
  if (pl.remap) remap_enqueue(st, maps, pl.raw, pl.mapped, n, sides, active);
  if (pl.smooth_mode) {
    SmoothArgs sa{};
    place(sa, pl.unsmoothed, pl.smoothed, pl.rows, pl.cols, n, sides, active);
    sa.mode = pl.smooth_mode; sa.ksize = pl.smooth_ksize;
    const hipError_t e = smooth_enqueue(st, sa);
    if (e != hipSuccess) return e;
  }
  return eq.on ? eq.enqueue(st, pl.rows, pl.cols, n, sides, active) : hipSuccess;
}

// ---- read-out ----------------------------------------------------------------------------------------
// plane `side` of stream s, rows x cols, dense into out
static hipError_t planes_to_host(uint8_t* out, const ImgPlanes& x, int side, int s, int rows, int cols) {
  return hipMemcpy2D(out, (size_t)cols, x.p[side] + (size_t)s * x.stream_stride, (size_t)x.row_stride, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost);
}
// a frame's left colour image as the map-colour kernels read it: through the left map while remapping (maps non-null).  rows x cols: the
// grid the taps are addressed in — the image's own size, or, while downscaling (factor > 1), the reduced size: a tap is then the rounded
// average of its factor x factor block of the full-size colour image
static ColorSrc color_src(const ImgPlanes& colour, int rows, int cols, int format, const RemapMaps* maps, int factor = 1) {
  ColorSrc s{};
  s.img = colour.p[0]; s.stream_stride = colour.stream_stride; s.row_stride = colour.row_stride; s.rows = rows; s.cols = cols; s.format = format;
  s.factor = factor;
  if (maps) { s.map_xy = maps->xy[0]; s.map_a = maps->a[0]; s.map_stride = maps->stride; s.map_rows = maps->rows; s.map_cols = maps->cols; }
  return s;
}

// ---- detection masks (kernels_mask.h) ------------------------------------------------------------------
// k_mask_pack on `n` streams of `sides` masks; fused when a.corner is set
static void mask_pack_enqueue(hipStream_t st, const MaskPackArgs& a) {
  hipLaunchKernelGGL(k_mask_pack, dim3((a.TX + VS_MASK_CW - 1) / VS_MASK_CW, (a.rows + VS_MASK_BR - 1) / VS_MASK_BR, a.n * a.sides), dim3(256), 0, st, a);
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
// A static mask's host images src[side] (null: that side has none; rows x cols, row_stride bytes apart) -> their eroded packed words
// user[side] [rows][TX], allocated from mem; one after the other through one device copy, st synchronised behind each.  Queues idle.
static hipError_t mask_static_upload(hipStream_t st, int sides, const uint8_t* const* src, int32_t row_stride, int rows, int cols, int TX, int margin,
                                     DeviceStore& mem, unsigned long long** user) {
  const size_t bytes = (size_t)(rows - 1) * row_stride + cols;
  uint8_t* tmp = nullptr;
  hipError_t e = hipMalloc((void**)&tmp, bytes);
  for (int k = 0; k < sides && e == hipSuccess; ++k) {
    if (!src[k]) continue;
    e = mem.alloc(&user[k], (size_t)rows * TX);
    if (e == hipSuccess) e = hipMemcpy(tmp, src[k], bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) break;
    MaskPackArgs a{};
    a.src[0] = tmp; a.src_row_stride = row_stride; a.rows = rows; a.cols = cols; a.TX = TX; a.margin = margin; a.n = 1; a.sides = 1;
    a.dst = user[k];
    active_all(a.active, 1);
    mask_pack_enqueue(st, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);     // tmp is refilled for the other side
  }
  if (tmp) (void)hipFree(tmp);
  return e;
}
// the validity words of `sides` maps of m, nw words each, in one block of mem: valid[side] (what mem held before is released).  Queues idle.
static hipError_t mask_valid_words(hipStream_t st, const RemapMaps& m, int sides, int margin, size_t nw, DeviceStore& mem, unsigned long long** valid) {
  mem.release();
  valid[0] = valid[1] = nullptr;
  unsigned long long* base = nullptr;
  hipError_t e = mem.alloc(&base, sides * nw);
  if (e == hipSuccess) { map_valid_enqueue(st, m, sides, margin, base); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (int k = 0; k < sides && e == hipSuccess; ++k) valid[k] = base + (size_t)k * nw;
  return e;
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
