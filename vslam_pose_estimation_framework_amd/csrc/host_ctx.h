// host_ctx.h — the context behind the C ABI: vslam_ctx and what it owns (device buffers, the per-call scratch arena, event timers, the
// switchable stores), configuration, create / destroy / reset, the scratch-context pool of the stand-alone entries, pending setters, the
// stream index checks and the per-stream lifetime calls.  Host code, included by vslam_hip.hip behind host_prestage.h (whose types the
// context holds).
#pragma once

static thread_local std::string g_create_error;

#ifndef VS_SPLIT4_MAX_STREAMS
#define VS_SPLIT4_MAX_STREAMS 96  // up to this many streams the frame runs as launch sequence 4 (phase 0 | wide recovery kernel | phase 4 | phase 2 with the landmark
                                  // refinement in workgroups of its own in the same launch).  Measured, ms per step fused / sequence 4: 1 stream 0.255 (two launches) /
                                  // 0.223, 4: 0.296 / 0.258, 11: 0.343 / 0.292, 32: 0.400 / 0.353, 64: 0.491 / 0.452, 96: 0.584 / 0.561, 128: 0.664 / 0.667, 157: 0.73 / 0.81
#endif
struct vslam_ctx {
  DevCfg cfg;
  DevBuf buf;
  int device = 0;
  int B = 0;
  hipStream_t stream = nullptr;       // frame queue: tracker kernels (k_track_candidates, k_frame, stages) + read-back
  hipStream_t stream_img = nullptr;   // image queue: image pipeline (k_fast_box, k_emit, k_brief) + uploads; the frame queue itself under
                                      // VSLAM_IMG_STREAMS=0 and on a caller's stream (vslam_set_hip_stream)
  bool own_stream = false;
  hipEvent_t ev_img[2] = {nullptr, nullptr}, ev_frm[2] = {nullptr, nullptr};   // [product set]: image pipeline done / frame queue done with the set
  bool frm_pending[2] = {false, false};
  int q0_frm = 0, q0_img = 0;         // XCD that block 0 of a launch on the queue runs on (calibrate_queues)
  // image products are double-buffered: frame t+1 is detected/described while frame t is tracked
  struct ImgSet { uint16_t* box; uint8_t* score8; unsigned long long* mask; int16_t* kp_xy; uint8_t* kp_score; uint8_t* desc;
                  int32_t* n_kp; int32_t* rowcell; uint8_t* used; uint8_t* sdist; ImgInfo* iinfo; } sets[2];
  int parity = 0, last_set = 0;
  std::string err;
  std::vector<void*> allocs;
  DevCfg* d_cfg = nullptr;            // device-resident copies read by k_frame through the constant address space
  DevBuf* d_bufs = nullptr;           // [2 product sets]
  uint8_t* upload[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [step parity][left/right]
  int up_stride = 0;
  size_t up_stream_stride = 0;
  bool frame_begun = false;
  bool timers = false;
  struct EvRec { hipEvent_t a, b; int k; bool count; };
  std::vector<EvRec> evrec;
  struct EvShared { hipEvent_t a, b; int k; };      // interval whose start event belongs to an EvRec (only b returns to the pool)
  std::vector<EvShared> evshared;
  std::vector<hipEvent_t> evpool;
  double kern_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int kern_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // RGB-D components: the space map of the last vslam_depth_space_map call stays resident for vslam_depth_compute
  struct DepthMap { int rows = 0, cols = 0; uint16_t* depth = nullptr; unsigned long long* key = nullptr; int32_t* last = nullptr;
                    float* space = nullptr; int16_t* row_map = nullptr; int16_t* col_map = nullptr; bool valid = false; DeviceStore mem; } dm;
  // scratch contexts of the stand-alone entry points (one per distinct configuration), kept for reuse: creating one costs
  // ~45 device allocations plus streams and events — several milliseconds, which the host-driven RGB-D loop would pay
  // five times per frame
  struct Scratch { vslam_ctx* t; vslam_config cfg; bool busy; size_t base_allocs; };
  std::vector<Scratch> scratch;
  // per-call device scratch of the stand-alone entry points: blocks kept between calls and handed out by bumping an offset
  // (tmp_get / tmp_reset below) — hipMalloc and hipFree cost tens of microseconds each, hipFree synchronises the device, and the
  // host-driven RGB-D loop would pay ~60 of them per frame
  struct Tmp { std::vector<std::pair<char*, size_t>> blocks; size_t used = 0; } tmp;
  // stage reports (kernels_report.h): pinned, device-mapped host buffer the report kernel packs a stage's results into; pinned
  // staging of the stage path's host images (a pageable hipMemcpyAsync of 2 x 467 KB costs ~0.24 ms of host time)
  unsigned char* report = nullptr; unsigned char* report_dev = nullptr; ReportLayout rl;
  unsigned int* report_done = nullptr;                 // arrival counter of the multi-block report kernel (device)
  // stage path of a one-stream context: the image pipeline runs on the frame queue itself (the caller waits for every stage, so a
  // second queue buys no overlap and costs an event round trip per frame) and is timed by three events instead of two per kernel
  hipStream_t img_override = nullptr;
  bool img_on_frm_queue = false;
  int report_seq = 0;                                  // stamps every report launch; the header carries it back
  int report_xy_seq = -1;                              // the early coordinates-only keypoint report of the frame in flight (-1: none)
  int report_have = 0, report_have_ip = 0, report_have_stream = -1, report_have_seq = -1;   // what the LAST launch on the frame queue packed (0: nothing)
  // setters of a one-stream context wait here for the next stage launch (StageIo); flush_pending() launches them on their own
  struct Pending { int flags = 0; int status = 0, win = 0; double tau = 0; double prior[12], pose[12]; } pend;
  unsigned char* pin_img[2] = {nullptr, nullptr}; size_t pin_img_bytes = 0;     // [step parity]: left | right
  hipEvent_t pin_ev[2] = {nullptr, nullptr}; bool pin_used[2] = {false, false};
  int split = 0;   // launch sequence of the frame: 0 one fused k_frame launch; 4 phase launches around the wide recovery kernel, the landmark
                   // refinement in workgroups of its own inside the last one (fastest up to VS_SPLIT4_MAX_STREAMS streams)
  bool lm_published = false;                            // vslam_prune_recover has published the frame's history (one stream): vslam_compute runs the landmark refinement beside the stereo stage
  // The input stages ahead of the detector.  Every slab a stage reads or writes besides upload[parity] lives in `slabs`; which of them exist,
  // at which geometry, and how a frame is routed through them is decided by stage_plan.h alone, from the switches below (stage_switches,
  // host_switches.h).  All B x rows x stride bytes per image: COLOR / FULL / RAW [step parity][left/right] take the host frames that come in
  // (colour, full-size, raw) and the stage outputs at those sizes; SM_IN [step parity][left/right] takes what would have gone to
  // upload[parity] while smoothing, which cannot work in place; KEEP and SM_OUT (one pair: their only readers are the same frame's kernels on
  // the same queue and a getter) hold the rectified / smoothed pair while the equalisation slot writes upload[parity] behind them.
  StageSlabs<DeviceStore> slabs;
  // rectification of raw input pairs (vslam_set_rectification): maps at the rectified size, padded to map_stride entries per row
  struct Rect { bool on = false, have_frame = false; RemapMaps maps; DeviceStore mem; } rect;
  // the equalisation slot of the input pair (vslam_set_equalization / vslam_set_clahe: EqSlot, host_prestage.h), its tables [stream][side];
  // dst: where the pair the last frame was processed on lies (inside upload[last_set])
  EqSlot eq;
  // colour input (vslam_set_color_input, kernels_gray.h): off while format == VSLAM_PIXEL_GRAY8
  struct Col { int format = 0; bool have_frame = false; } col;
  // integer-factor reduction of the incoming frames (vslam_set_downscale, kernels_downscale.h): off while factor == 1
  struct Ds : DownscaleSwitch { bool have_frame = false; } ds;
  // smoothing of the grey pair ahead of the equalisation slot (vslam_set_smoothing, kernels_smooth.h): off while mode == VSLAM_SMOOTH_OFF
  struct Sm : SmoothSwitch { bool have_frame = false; } sm;
  // this frame's routing through the input stages (route_frame, host_frame.h): the colour pair (a slab or the caller's device memory) and
  // where k_gray_u8 writes the grey pair, so where vslam_get_gray_images reads it; the raw pair k_rectify reads and the pair it writes
  PrePlan pre;
  // the landmark map (vslam_enable_map, kernels_map.h): off while cap == 0; its own allocations, freed by vslam_enable_map(0) and destroy
  struct MapStore { int32_t cap = 0; DevMap d{}; DeviceStore mem; } map;
  // the observation log on top of it (vslam_enable_observations, kernels_obs.h): off while cap == 0; freed by vslam_enable_observations(0),
  // vslam_enable_map(0) and destroy
  struct ObsStore { int32_t cap = 0; DevObs d{}; DeviceStore mem; } obs;
  // the colour of every map entry (vslam_enable_map_colors, kernels_map_color.h): [B][map.cap] words (r, g, b, 0); off while rgb is null;
  // freed by vslam_enable_map_colors(0), any vslam_enable_map, vslam_set_color_input(GRAY8) and destroy
  struct MapColors { uint32_t* rgb = nullptr; DeviceStore mem; } mapcol;
  // pose guesses waiting for the head of the next frame (vslam_set_pose_guess*, kernels_motion.h): `dev` the caller's device array, `host` /
  // `mask` [B][12] / [B] what was set one stream at a time or as a host array (any: some mask entry is set), d_host / d_mask their device
  // copies, pin[turn] / pin_ev[turn] the two pinned staging buffers (guesses | mask) the copies leave from in turn, each reused once its
  // last copy has finished; the device side is allocated with the first frame that hands guesses over and freed by destroy.  The model itself lives in cfg (DevCfg::motion_model).
  struct Guess { const double* dev = nullptr; std::vector<double> host; std::vector<int32_t> mask; bool any = false;
                 double* d_host = nullptr; int32_t* d_mask = nullptr; DeviceStore mem;
                 unsigned char* pin[2] = {nullptr, nullptr}; hipEvent_t pin_ev[2] = {nullptr, nullptr}; bool pin_used[2] = {false, false}; int turn = 0; } guess;
  // detection masks (vslam_set_detection_mask / vslam_set_frame_masks, kernels_mask.h).  stat[side]: the static mask's eroded packed words
  // [rows][TX], null: that side is unmasked; freed when both go.  The frame masks wait here for the next frame's image pipeline: src the
  // caller's pointers (null: that side has none), read in place on the device, copied into `slab` at the caller's strides when they are
  // host memory; eff [B][2][rows][TX]: the effective words of the last frame that had frame masks.  last: what the last frame used (bit 0
  // static, bit 1 frame masks) and on which streams (last_active).  Nothing of this is allocated, launched or copied while no mask is set.
  // The context-wide keep words are the user's static mask AND the rectification maps' validity (vslam_set_rectification_mask): user[side]
  // and valid[side] hold either alone, stat[side] points at the one there is, or at comb[side] = both ANDed (mask_static_sync).
  struct DetMask { unsigned long long* stat[2] = {nullptr, nullptr};
                   unsigned long long* user[2] = {nullptr, nullptr}; DeviceStore user_mem;
                   bool valid_on = false; int valid_margin = 0; unsigned long long* valid[2] = {nullptr, nullptr}; DeviceStore valid_mem;
                   unsigned long long* comb[2] = {nullptr, nullptr}; DeviceStore comb_mem;
                   bool pending = false, on_device = false; const uint8_t* src[2] = {nullptr, nullptr}; int32_t row_stride = 0; size_t image_stride = 0; int margin = 0;
                   uint8_t* slab[2] = {nullptr, nullptr}; size_t slab_bytes = 0; DeviceStore slab_mem;
                   unsigned long long* eff = nullptr; DeviceStore eff_mem;
                   MaskPackArgs job{}; bool job_ready = false;
                   int last = 0; uint32_t last_active[VS_MAX_STREAMS / 32] = {}; } dmask;
  // the range cells of vslam_bilateral_depth_u16 (kernels_bilateral.h): four words, armed when allocated with the first call and re-armed
  // by every call's k_bilateral_lut
  uint32_t* bl_cells = nullptr;
  int sticky = VSLAM_OK;
};

static int fail(vslam_ctx* c, int code, const std::string& msg) {
  if (c) { c->err = msg; if (code == VSLAM_ERR_HIP) c->sticky = code; }
  else g_create_error = msg;
  return code;
}
#define HIP_TRY(ctx, expr)                                                                              \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail(ctx, VSLAM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <typename T>
static hipError_t dalloc(vslam_ctx* c, T** p, size_t count) {
  void* q = nullptr;
  hipError_t e = hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T));
  if (e == hipSuccess) { c->allocs.push_back(q); *p = (T*)q; }
  return e;
}

// ---- per-call device scratch ------------------------------------------------------------------------------
static hipError_t tmp_get(vslam_ctx* c, void** p, size_t bytes) {
  bytes = (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255;
  auto& T = c->tmp;
  if (T.blocks.empty() || T.used + bytes > T.blocks.back().second) {
    (void)hipSetDevice(c->device);     // the caller's thread may have another device current (torch switches it)
    const size_t want = std::max<size_t>(bytes, T.blocks.empty() ? ((size_t)1 << 20) : 2 * T.blocks.back().second);
    void* q = nullptr;
    const hipError_t e = hipMalloc(&q, want);
    if (e != hipSuccess) return e;
    T.blocks.push_back({(char*)q, want});
    T.used = 0;
  }
  *p = T.blocks.back().first + T.used;
  T.used += bytes;
  return hipSuccess;
}
// start of an entry point: everything handed out before is dead (every entry synchronises before it returns its results); blocks that
// had to be chained during a call are merged into one, so that a steady caller allocates nothing
static void tmp_reset(vslam_ctx* c) {
  if (!c) return;
  auto& T = c->tmp;
  if (T.blocks.size() > 1) {
    (void)hipSetDevice(c->device);     // entries call tmp_reset first: the merged block must live on the context's device
    size_t total = 0;
    for (auto& b : T.blocks) { total += b.second; (void)hipFree(b.first); }
    T.blocks.clear();
    void* q = nullptr;
    if (hipMalloc(&q, total) == hipSuccess) T.blocks.push_back({(char*)q, total});
  }
  T.used = 0;
}
static void tmp_free(vslam_ctx* c) {
  for (auto& b : c->tmp.blocks) (void)hipFree(b.first);
  c->tmp.blocks.clear(); c->tmp.used = 0;
}

static void sync_all(vslam_ctx* c) {
  (void)hipStreamSynchronize(c->stream_img);
  (void)hipStreamSynchronize(c->stream);
}
// ---- optional per-kernel timing (HIP events on the context stream) -----------------------------------
static hipEvent_t ev_get(vslam_ctx* c) {
  if (!c->evpool.empty()) { hipEvent_t e = c->evpool.back(); c->evpool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
struct KernelTimer {
  vslam_ctx* c; int k; hipStream_t st; bool count; hipEvent_t a = nullptr;
  KernelTimer(vslam_ctx* c_, int k_, hipStream_t st_, bool count_ = true, bool enabled_ = true) : c(c_), k(k_), st(st_), count(count_) { if (c->timers && enabled_) { a = ev_get(c); (void)hipEventRecord(a, st); } }
  ~KernelTimer() { if (a) { hipEvent_t b = ev_get(c); (void)hipEventRecord(b, st); c->evrec.push_back({a, b, k, count}); } }
};
static void harvest_events(vslam_ctx* c) {
  sync_all(c);
  for (auto& r : c->evshared) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->kern_ms[r.k] += ms; c->kern_n[r.k] += 1; }
    c->evpool.push_back(r.b);
  }
  c->evshared.clear();
  for (auto& r : c->evrec) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { c->kern_ms[r.k] += ms; if (r.count) c->kern_n[r.k] += 1; }
    c->evpool.push_back(r.a); c->evpool.push_back(r.b);
  }
  c->evrec.clear();
}

static DevBuf buf_set(const vslam_ctx* c, int set, int q0 = 0) {
  DevBuf b = c->buf;
  b.xcd_rot = q0 & 7;     // dev_types.h: stream s on physical XCD s % 8 whatever queue the launch goes to
  const vslam_ctx::ImgSet& q = c->sets[set];
  b.box = q.box; b.score8 = q.score8; b.mask = q.mask; b.kp_xy = q.kp_xy; b.kp_score = q.kp_score; b.desc = q.desc;
  b.n_kp = q.n_kp; b.rowcell = q.rowcell; b.used = q.used; b.sdist = q.sdist; b.iinfo = q.iinfo;
  return b;
}

// ---- defaults (configurations/configuration_{kitti,euroc}.yaml, src/types/parameters.h) -----------
static void common_defaults(vslam_config* c) {
  std::memset(c, 0, sizeof *c);
  c->det_rows = 1; c->det_cols = 1;
  c->detector_threshold_minimum = 20; c->detector_threshold_maximum = 100;
  c->detector_threshold_maximum_change = 0.1; c->target_number_of_keypoints_tolerance = 0.1;
  c->bin_size_pixels = 15; c->enable_keypoint_binning = 1;
  c->minimum_projection_tracking_distance_pixels = 15; c->maximum_projection_tracking_distance_pixels = 50;
  c->minimum_descriptor_distance_tracking = 25.6; c->maximum_descriptor_distance_tracking = 51.2;
  c->maximum_reliable_depth_meters = 15; c->maximum_depth_meters = 1000; c->minimum_depth_meters = 0.1;
  c->maximum_matching_distance_triangulation = 51.2; c->minimum_disparity_pixels = 1;
  c->maximum_epipolar_search_offset_pixels = 0;
  c->minimum_track_length_for_landmark_creation = 1; c->minimum_number_of_landmarks_to_track = 5;
  c->tunnel_vision_ratio = 0.5; c->good_tracking_ratio = 0.2; c->enable_landmark_recovery = 1;
  c->minimum_delta_angular_for_movement = 0.001; c->minimum_delta_translational_for_movement = 0.01;
  c->aligner_error_delta_for_convergence = 1e-3; c->aligner_maximum_error_kernel = 4; c->aligner_damping = 5;
  c->aligner_maximum_number_of_iterations = 1000; c->aligner_minimum_number_of_inliers = 100;
  c->landmark_maximum_error_squared_meters = 25; c->landmark_maximum_number_of_iterations = 100;
  c->max_keypoints = 16384; c->max_points = 8192; c->max_history_frames = 512;
}
VS_API void vslam_default_config_kitti(vslam_config* c) {
  common_defaults(c);
  c->rows = 376; c->cols = 1241;
  const double K[9] = {718.856, 0, 607.1928, 0, 718.856, 185.2157, 0, 0, 1};
  std::memcpy(c->K, K, sizeof K);
  c->baseline_h[0] = -386.1448;
}
VS_API void vslam_default_config_euroc(vslam_config* c) {
  common_defaults(c);
  c->rows = 480; c->cols = 752;
  const double K[9] = {458.654, 0, 367.215, 0, 457.296, 248.375, 0, 0, 1};
  std::memcpy(c->K, K, sizeof K);
  c->baseline_h[0] = -458.654 * 0.11;
  c->det_rows = 2; c->det_cols = 2;
  c->detector_threshold_minimum = 10; c->detector_threshold_maximum = 30; c->detector_threshold_maximum_change = 1.0;
  c->bin_size_pixels = 20;
  c->minimum_descriptor_distance_tracking = 25; c->maximum_descriptor_distance_tracking = 50;
  c->maximum_reliable_depth_meters = 5; c->maximum_depth_meters = 100;
  c->maximum_matching_distance_triangulation = 50;
  c->minimum_track_length_for_landmark_creation = 2; c->good_tracking_ratio = 0.25;
  c->aligner_damping = 0;
  c->descriptor_type = VSLAM_DESCRIPTOR_ORB;   // configuration_euroc.yaml:52 "ORB-256": unknown to the parser -> cv::ORB::create() (:219-224)
}

VS_API const char* vslam_last_error(const vslam_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

// ---- ORB extractor constants, computed on the host with OpenCV's own expressions [recalled: orb.cpp, smooth.cpp] --------------
static void orb_rotation_host(float angle_degrees, float* a, float* b) {
  float angle = angle_degrees;
  angle *= (float)(3.1415926535897932384626433832795 / 180.f);
  *a = (float)std::cos(angle); *b = (float)std::sin(angle);
}
static void gauss7_kernel_host(int32_t k4[4]) {   // getGaussianKernel(7, 2, CV_32F) -> cvRound(k * 256): centre .. outermost tap
  float cf[7];
  double sum = 0;
  for (int i = 0; i < 7; ++i) { const double x = i - 3.0; cf[i] = (float)std::exp(-0.5 / 4.0 * x * x); sum += cf[i]; }
  sum = 1. / sum;
  for (int i = 0; i < 4; ++i) k4[i] = (int32_t)std::lrint((double)(float)(cf[3 + i] * sum) * 256.0);
}
// ---- configure (BaseFramePointGenerator::configure, base_framepoint_generator.cpp:229-329) ----------
static void derive_cfg(const vslam_config& in, int n_streams, DevCfg* d) {
  std::memset(d, 0, sizeof *d);
  d->c = in;
  d->TX = (in.cols + VS_TILE_W - 1) / VS_TILE_W;
  d->CW = d->TX * 4;
  d->bstride = d->TX * VS_TILE_W;
  const int nv = in.det_rows, nh = in.det_cols;
  const double ph = (double)in.rows / nv, pw = (double)in.cols / nh;
  int k = 0;
  for (int r = 0; r < nv; ++r)
    for (int cc = 0; cc < nh; ++cc) {
      int off_w = nh > 1 ? 2 : 0, off_h = nv > 1 ? 2 : 0, off_r = 0, off_c = 0;
      if (r > 0) { off_r = -off_h; if (r < nv - 1) off_h *= 2; }
      if (cc > 0) { off_c = -off_w; if (cc < nh - 1) off_w *= 2; }
      d->regions[k].x = (int)(std::round(cc * pw) + off_c);
      d->regions[k].y = (int)(std::round(r * ph) + off_r);
      d->regions[k].w = (int)(pw + off_w);
      d->regions[k].h = (int)(ph + off_h);
      ++k;
    }
  d->n_regions = k;
  d->cols_bin = (int)(std::floor((double)in.cols / in.bin_size_pixels) + 1);
  d->rows_bin = (int)(std::floor((double)in.rows / in.bin_size_pixels) + 1);
  d->target_kp = d->cols_bin * d->rows_bin;
  d->target_per_detector = (int)((double)d->target_kp / (double)d->n_regions);
  d->n_offsets = 0;
  d->offsets[d->n_offsets++] = 0;
  for (int u = 1; u <= in.maximum_epipolar_search_offset_pixels; ++u) { d->offsets[d->n_offsets++] = u; d->offsets[d->n_offsets++] = -u; }
  orb_rotation_host(-1.f, &d->orb_cos, &d->orb_sin);   // FAST keypoints: KeyPoint::angle = -1, never recomputed by ORB::compute
  gauss7_kernel_host(d->gauss7);
  d->NMAX = in.max_keypoints;
  d->MAXP = in.max_points;
  d->HCAP = in.max_history_frames;
  d->trail = in.max_points <= 65535 ? 1 : 0;
  d->n_streams = n_streams;
}

// PoseTracker3D::configure (pose_tracker_3d.cpp:11-21) + a fresh generator / aligner / world map for one stream
static void fresh_stream_state(const vslam_ctx* c, StreamState& x) {
  std::memset(&x, 0, sizeof x);
  for (int r = 0; r < c->cfg.n_regions; ++r) x.thr[r] = c->cfg.c.detector_threshold_minimum;
  x.status = VSLAM_LOCALIZING;
  x.win = c->cfg.c.maximum_projection_tracking_distance_pixels;
  x.tau_track = c->cfg.c.minimum_descriptor_distance_tracking;
  x.tau_tri = 0.1 * 256;
  tf_identity(x.prior);
  tf_identity(x.pose);
  tf_identity(x.guess);
  tf_identity(x.guess_prev);
}
// guesses that were waiting for a frame belong to the sequence that ended
static void guess_drop_pending(vslam_ctx* c, int s = -1) {
  vslam_ctx::Guess& g = c->guess;
  if (s < 0) { g.dev = nullptr; std::fill(g.mask.begin(), g.mask.end(), 0); g.any = false; return; }
  if (!g.mask.empty()) { g.mask[s] = 0; g.any = std::any_of(g.mask.begin(), g.mask.end(), [](int32_t m) { return m != 0; }); }
}
static int upload_buffer_tables(vslam_ctx* c) {
  const DevBuf hb[2] = {buf_set(c, 0, c->q0_frm), buf_set(c, 1, c->q0_frm)};
  HIP_TRY(c, hipMemcpy(c->d_bufs, hb, sizeof hb, hipMemcpyHostToDevice));
  return VSLAM_OK;
}
static int init_state(vslam_ctx* c) {
  c->pend.flags = 0;          // a reset drops setters that were waiting for a stage launch: the fresh state is the state
  guess_drop_pending(c);
  c->dmask.pending = false;   // frame masks that were waiting for a frame belong to the sequence that ended (the static mask stays)
  c->dmask.last = 0;
  c->report_have = 0;
  std::vector<StreamState> st(c->B);
  for (int s = 0; s < c->B; ++s) fresh_stream_state(c, st[s]);
  bool all_active = true;
  for (int s = 0; s < c->B; ++s) all_active = all_active && ((c->buf.active[s >> 5] >> (s & 31)) & 1u);
  if (!all_active) {   // a reset of the whole context re-activates every stream
    sync_all(c);
    std::memset(c->buf.active, 0xff, sizeof c->buf.active);
    int rc = upload_buffer_tables(c);
    if (rc != VSLAM_OK) return rc;
  }
  HIP_TRY(c, hipMemcpyAsync(c->buf.st, st.data(), sizeof(StreamState) * c->B, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->buf.info, 0, sizeof(vslam_frame_info) * c->B, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->buf.n_points, 0, sizeof(int32_t) * c->B * 2, c->stream));
  if (c->map.cap) HIP_TRY(c, hipMemsetAsync(c->map.d.count, 0, sizeof(int32_t) * c->B, c->stream));
  if (c->obs.cap) HIP_TRY(c, hipMemsetAsync(c->obs.d.count, 0, sizeof(int32_t) * c->B, c->stream));
  sync_all(c);
  for (int q = 0; q < 2; ++q) {
    HIP_TRY(c, hipMemsetAsync(c->sets[q].n_kp, 0, sizeof(int32_t) * c->B * 2, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->sets[q].iinfo, 0, sizeof(ImgInfo) * c->B, c->stream));
    c->frm_pending[q] = false;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->parity = 0; c->last_set = 0;
  c->frame_begun = false;
  return VSLAM_OK;
}

// the queues' events, and the queues themselves unless they are the caller's
static void destroy_streams(vslam_ctx* c) {
  for (int q = 0; q < 2; ++q) {
    if (c->ev_img[q]) (void)hipEventDestroy(c->ev_img[q]);
    if (c->ev_frm[q]) (void)hipEventDestroy(c->ev_frm[q]);
    c->ev_img[q] = c->ev_frm[q] = nullptr;
  }
  if (c->own_stream) {
    if (c->stream_img && c->stream_img != c->stream) (void)hipStreamDestroy(c->stream_img);
    if (c->stream) (void)hipStreamDestroy(c->stream);
  }
  c->stream = c->stream_img = nullptr;
}
// Workgroup b of a launch runs on XCD (q0 + b) % 8 with q0 a property of the hardware queue behind the HIP stream (constant from launch
// to launch, idle or loaded: tools/probe/xcd_map.hip).  One one-block launch per queue reads it.
__global__ void k_xcc_probe(int* out) {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  if (threadIdx.x == 0) *out = (int)(v & 7u);
}
static int calibrate_queues(vslam_ctx* c) {
  int* d = nullptr;
  if (hipMalloc(&d, 2 * sizeof(int)) != hipSuccess) return VSLAM_OK;     // affinity is an optimisation: without it rot stays 0
  int h[2] = {0, 0};
  hipStream_t q[2] = {c->stream, c->stream_img};
  bool ok = true;
  for (int k = 0; k < 2 && ok; ++k) { hipLaunchKernelGGL(k_xcc_probe, dim3(1), dim3(64), 0, q[k], d + k); ok = hipStreamSynchronize(q[k]) == hipSuccess; }
  if (ok && hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) { c->q0_frm = h[0]; c->q0_img = h[1]; }
  (void)hipFree(d);
  return VSLAM_OK;
}

static int create_internal(const vslam_config* cfg, int device, int n_streams, vslam_ctx** out) {
  if (!cfg || !out || n_streams < 1) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: null argument or n_streams < 1");
  if (n_streams > VS_MAX_STREAMS) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: more than 4096 streams in one context");
  if (cfg->rows < 1 || cfg->cols < 1 || cfg->cols > 32767 || cfg->rows > 32767) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: invalid image dimensions");
  if (cfg->det_rows < 1 || cfg->det_cols < 1 || cfg->det_rows * cfg->det_cols > VSLAM_MAX_REGIONS) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: invalid detector grid");
  if (!(-cfg->baseline_h[0] / cfg->K[0] > 0)) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: invalid baseline (m), verify intrinsic camera parameters");
  if (cfg->maximum_epipolar_search_offset_pixels < 0 || cfg->maximum_epipolar_search_offset_pixels > VSLAM_MAX_EPI) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: epipolar offset out of range");
  if (cfg->descriptor_type != VSLAM_DESCRIPTOR_BRIEF && cfg->descriptor_type != VSLAM_DESCRIPTOR_ORB) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: unknown descriptor_type");
  if (cfg->max_keypoints < 64 || cfg->max_keypoints > 65535 || cfg->max_points < 64 || cfg->max_history_frames < 2 || cfg->bin_size_pixels < 1) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: invalid capacities");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(nullptr, VSLAM_ERR_NO_DEVICE, "vslam_create: no HIP device available (the HIP path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(nullptr, VSLAM_ERR_NO_DEVICE, "vslam_create: device ordinal out of range");
  if (hipSetDevice(device) != hipSuccess) return fail(nullptr, VSLAM_ERR_NO_DEVICE, "vslam_create: hipSetDevice failed");
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_frame)) != hipSuccess)
    return fail(nullptr, VSLAM_ERR_NO_DEVICE, "vslam_create: no gfx950 kernel image for this device");
  vslam_ctx* c = new vslam_ctx;
  c->device = device;
  c->B = n_streams;
  derive_cfg(*cfg, n_streams, &c->cfg);
  {
    // one frame queue and one image queue for all streams (stream groups on queues of their own, a second image queue
    // and queue priorities were measured and removed)
    bool ok = hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, 0) == hipSuccess &&
              hipStreamCreateWithPriority(&c->stream_img, hipStreamNonBlocking, 0) == hipSuccess;
    // VSLAM_IMG_STREAMS=0: everything on one HIP stream (no overlap) — measurement aid for stand-alone kernel times
    if (ok && getenv("VSLAM_IMG_STREAMS") && atoi(getenv("VSLAM_IMG_STREAMS")) == 0) { (void)hipStreamDestroy(c->stream_img); c->stream_img = c->stream; }
    for (int k = 0; k < 2 && ok; ++k)
      ok = hipEventCreateWithFlags(&c->ev_img[k], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&c->ev_frm[k], hipEventDisableTiming) == hipSuccess;
    c->own_stream = true;
    if (!ok) { destroy_streams(c); delete c; return fail(nullptr, VSLAM_ERR_HIP, "hipStreamCreate failed"); }
    c->split = n_streams <= VS_SPLIT4_MAX_STREAMS ? 4 : 0;
    // test hook: VSLAM_SPLIT=0 / 4 forces that launch sequence, any other value leaves the choice to the library
    if (const char* e = getenv("VSLAM_SPLIT")) { const int v = atoi(e); if (v == 0 || v == 4) c->split = v; }
  }
  const DevCfg& d = c->cfg;
  DevBuf& b = c->buf;
  std::memset(&b, 0, sizeof b);
  std::memset(b.active, 0xff, sizeof b.active);
  const size_t B = n_streams, S2 = B * 2, rows = cfg->rows, N = d.NMAX, P = d.MAXP, Hc = d.HCAP;
  hipError_t e = hipSuccess;
#define A(field, count) if (e == hipSuccess) e = dalloc(c, &b.field, (count))
  A(box, S2 * rows * d.bstride); A(score8, S2 * rows * d.bstride); A(mask, S2 * rows * d.TX);
  A(kp_xy, S2 * N * 2); A(kp_score, S2 * N); A(desc, S2 * N * 32); A(n_kp, S2);
  A(rowcell, S2 * rows * (d.CW + 1)); A(used, S2 * N); A(kill, S2 * N);
  A(st, B); A(info, B); A(pose_log, B * VS_POSE_LOG * 12);
  A(p_kp, S2 * P * 4); A(p_desc, S2 * P * 64); A(p_meta, S2 * P * META); A(p_cam, S2 * P * 3); A(p_camlm, S2 * P * 3);
  A(p_lm, S2 * P * 3); A(n_points, S2); A(p_trail, d.trail ? S2 * P * VS_TRAIL : (size_t)64);
  A(proj, B * P * 8); A(proj_q, B * P * 2); A(cand_key, B * P * VS_MAXCAND); A(cand_rkey, B * P * VS_MAXRCAND);
  A(res, B * P * 8); A(trk, B * P * 4); A(lost, B * P);
  A(al_moving, B * P * 3); A(al_fixed, B * P * 4); A(al_omega, B * P); A(al_weight, B * P); A(al_chi, B * P); A(al_inl, B * P);
  A(rec, B * P * 6); A(rec_desc, B * P * 64);
  A(st_match, B * N * 3); A(sc, B * N * 4); A(bin_occ, B * (size_t)d.rows_bin * d.cols_bin); A(sdist, B * N * 16); A(bin_aux, B * (2 * ((size_t)d.rows_bin * d.cols_bin + 1) + N));
  A(h_pose, B * Hc * 24); A(h_cam, B * Hc * P * 4); A(h_prev, B * Hc * P);
#undef A
  for (int q = 0; q < 2 && e == hipSuccess; ++q) {
    vslam_ctx::ImgSet& t = c->sets[q];
    if (q == 0) { t = {b.box, b.score8, b.mask, b.kp_xy, b.kp_score, b.desc, b.n_kp, b.rowcell, b.used, b.sdist, nullptr}; }
    else {
      e = dalloc(c, &t.box, S2 * rows * d.bstride);
      if (e == hipSuccess) e = dalloc(c, &t.score8, S2 * rows * d.bstride);
      if (e == hipSuccess) e = dalloc(c, &t.mask, S2 * rows * d.TX);
      if (e == hipSuccess) e = dalloc(c, &t.kp_xy, S2 * N * 2);
      if (e == hipSuccess) e = dalloc(c, &t.kp_score, S2 * N);
      if (e == hipSuccess) e = dalloc(c, &t.desc, S2 * N * 32);
      if (e == hipSuccess) e = dalloc(c, &t.n_kp, S2);
      if (e == hipSuccess) e = dalloc(c, &t.rowcell, S2 * rows * (d.CW + 1));
      if (e == hipSuccess) e = dalloc(c, &t.used, S2 * N);
      if (e == hipSuccess) e = dalloc(c, &t.sdist, B * N * 16);
    }
    if (e == hipSuccess) e = dalloc(c, &t.iinfo, B);
  }
  if (e == hipSuccess) b.iinfo = c->sets[0].iinfo;
  c->up_stride = d.bstride;
  c->up_stream_stride = (size_t)rows * d.bstride;       // rows * up_stride: stage_plan.h sizes SM_IN, KEEP and SM_OUT by that product (stage_switches asserts it)
  for (int q = 0; q < 2; ++q)
    for (int d2 = 0; d2 < 2; ++d2)
      if (e == hipSuccess) e = dalloc(c, &c->upload[q][d2], B * c->up_stream_stride);
  // a half-built context: nothing beyond its allocations and queues exists yet
  auto abandon = [&](int code, const std::string& msg) {
    for (void* p : c->allocs) (void)hipFree(p);
    destroy_streams(c);
    delete c;
    return fail(nullptr, code, msg);
  };
  if (e != hipSuccess) return abandon(VSLAM_ERR_HIP, std::string("vslam_create: hipMalloc failed: ") + hipGetErrorString(e));
  // score8 must read 0 where no corner was ever written only through the mask, box/mask are fully
  // rewritten every frame; nothing else needs initialisation besides the stream state.
  {
    // the frame kernel's view of the configuration and of the buffer table (image pointers excluded: it never reads them)
    calibrate_queues(c);
    e = dalloc(c, &c->d_cfg, 1);
    if (e == hipSuccess) e = dalloc(c, &c->d_bufs, 2);
    if (e == hipSuccess) e = hipMemcpy(c->d_cfg, &c->cfg, sizeof(DevCfg), hipMemcpyHostToDevice);
    if (e == hipSuccess && upload_buffer_tables(c) != VSLAM_OK) e = hipErrorUnknown;
    if (e != hipSuccess) return abandon(VSLAM_ERR_HIP, std::string("vslam_create: device tables: ") + hipGetErrorString(e));
  }
  int rc = init_state(c);
  if (rc != VSLAM_OK) return abandon(rc, std::string(c->err));
  *out = c;
  return VSLAM_OK;
}

static void depth_map_free(vslam_ctx* c) {
  vslam_ctx::DepthMap& m = c->dm;
  m.mem.release();
  m = vslam_ctx::DepthMap();
}
// the resident space map at rows x cols: its own allocations (it outlives the call that fills it), kept while the size stays
static hipError_t depth_map_resize(vslam_ctx* c, int rows, int cols) {
  vslam_ctx::DepthMap& m = c->dm;
  if (m.rows == rows && m.cols == cols) return hipSuccess;
  depth_map_free(c);
  const size_t n = (size_t)rows * cols;
  hipError_t e = m.mem.alloc(&m.depth, n);
  if (e == hipSuccess) e = m.mem.alloc(&m.key, n);
  if (e == hipSuccess) e = m.mem.alloc(&m.last, n);
  if (e == hipSuccess) e = m.mem.alloc(&m.space, n * 3);
  if (e == hipSuccess) e = m.mem.alloc(&m.row_map, n);
  if (e == hipSuccess) e = m.mem.alloc(&m.col_map, n);
  if (e != hipSuccess) { depth_map_free(c); return e; }
  m.rows = rows; m.cols = cols;
  return hipSuccess;
}
// the switchable stores: what vslam_enable_observations(0), vslam_enable_map(0) and vslam_destroy call (those of the input stages:
// host_switches.h)
static void obs_free(vslam_ctx* c) {
  c->obs.mem.release();
  c->obs.d = DevObs{};
  c->obs.cap = 0;
}
static void mapcol_free(vslam_ctx* c) {
  c->mapcol.mem.release();
  c->mapcol.rgb = nullptr;
}
static void map_free(vslam_ctx* c) {
  mapcol_free(c);                    // the colours are indexed by the map's ids
  c->map.mem.release();
  c->map.d = DevMap{};
  c->map.cap = 0;
}
VS_API int vslam_create(const vslam_config* cfg, int device, int n_streams, vslam_ctx** out) {
  // a tracker needs room for a keypoint (descriptor border 28 / 31 px); the scratch contexts of the stand-alone entries accept
  // any image, a tiny one simply has no valid pixel
  if (cfg && (cfg->rows < 16 || cfg->cols < 16)) return fail(nullptr, VSLAM_ERR_INVALID, "vslam_create: invalid image dimensions");
  return create_internal(cfg, device, n_streams, out);
}
VS_API void vslam_destroy(vslam_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  sync_all(c);
  for (auto& e : c->scratch) vslam_destroy(e.t);
  c->scratch.clear();
  for (void* p : c->allocs) (void)hipFree(p);
  c->slabs.release(); c->rect.mem.release(); c->eq.mem.release();     // the input stages' stores
  for (DeviceStore* m : {&c->dmask.user_mem, &c->dmask.valid_mem, &c->dmask.comb_mem, &c->dmask.slab_mem, &c->dmask.eff_mem}) m->release();    // detection masks
  c->guess.mem.release();
  for (int q = 0; q < 2; ++q) { if (c->guess.pin[q]) (void)hipHostFree(c->guess.pin[q]); if (c->guess.pin_ev[q]) (void)hipEventDestroy(c->guess.pin_ev[q]); }
  map_free(c);
  obs_free(c);
  tmp_free(c);
  depth_map_free(c);
  if (c->report) (void)hipHostFree(c->report);
  for (int q = 0; q < 2; ++q) { if (c->pin_img[q]) (void)hipHostFree(c->pin_img[q]); if (c->pin_ev[q]) (void)hipEventDestroy(c->pin_ev[q]); }
  harvest_events(c);
  for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
  destroy_streams(c);
  delete c;
}
VS_API int vslam_reset(vslam_ctx* c) {
  if (!c) return VSLAM_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  c->sm.have_frame = false;        // the smoothing switch stays; what its getter would read belongs to the sequence that ended
  return init_state(c);
}
// check a scratch context of configuration `cfg` out of the parent's pool (fresh stream state, pristine DevCfg) / back in
static int scratch_get(vslam_ctx* parent, const vslam_config& cfg, vslam_ctx** out) {
  for (auto& e : parent->scratch)
    if (!e.busy && std::memcmp(&e.cfg, &cfg, sizeof cfg) == 0) {
      derive_cfg(cfg, 1, &e.t->cfg);            // stand-alone entries edit the detector regions of their scratch DevCfg
      e.t->err.clear(); e.t->sticky = VSLAM_OK; e.t->timers = false;
      const int rc = init_state(e.t);
      if (rc != VSLAM_OK) { parent->err = e.t->err; return rc; }
      e.busy = true;
      *out = e.t;
      return VSLAM_OK;
    }
  vslam_ctx* t = nullptr;
  const int rc = create_internal(&cfg, parent->device, 1, &t);
  if (rc != VSLAM_OK) { parent->err = g_create_error; return rc; }
  if (parent->scratch.size() >= 12) {           // bound the pool: drop an idle entry
    for (size_t i = 0; i < parent->scratch.size(); ++i)
      if (!parent->scratch[i].busy) { vslam_destroy(parent->scratch[i].t); parent->scratch.erase(parent->scratch.begin() + i); break; }
  }
  parent->scratch.push_back({t, cfg, true, t->allocs.size()});
  *out = t;
  return VSLAM_OK;
}
static void scratch_put(vslam_ctx* parent, vslam_ctx* t) {
  if (!t) return;
  for (auto& e : parent->scratch)
    if (e.t == t) {
      sync_all(t);
      for (size_t i = e.base_allocs; i < t->allocs.size(); ++i) (void)hipFree(t->allocs[i]);   // per-call extras (dalloc on the scratch)
      t->allocs.resize(e.base_allocs);
      e.busy = false;
      return;
    }
  vslam_destroy(t);
}
// setters that were not folded into a stage launch (the next launch is not a stage kernel, or a getter reads the state)
static int flush_pending(vslam_ctx* c) {
  if (!c->pend.flags) return VSLAM_OK;
  const int fl = c->pend.flags;
  c->pend.flags = 0;
  hipStream_t q = c->stream;
  if (fl & 1) { D12 p; std::memcpy(p.v, c->pend.prior, sizeof p.v); hipLaunchKernelGGL(k_set_tracker_state, dim3(1), dim3(1), 0, q, c->buf, 0, c->pend.status, c->pend.win, c->pend.tau, p); }
  if (fl & 2) { D12 p; std::memcpy(p.v, c->pend.pose, sizeof p.v); hipLaunchKernelGGL(k_set_pose, dim3(1), dim3(1), 0, q, c->buf, 0, p); }
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
// the one range test of a stream index; nothing is launched or waited for (the setters are queued on the stream's frame queue, in
// order with the stage launches around them)
static int check_stream_index(vslam_ctx* c, int s) {
  if (!c) return VSLAM_ERR_INVALID;
  if (s < 0 || s >= c->B) return fail(c, VSLAM_ERR_INVALID, "stream index out of range");
  return VSLAM_OK;
}
// start of a read-back of stream s
static int check_stream(vslam_ctx* c, int s) {
  int rc = check_stream_index(c, s);
  if (rc == VSLAM_OK) rc = flush_pending(c);
  if (rc) return rc;
  sync_all(c);   // read-back: every group's queued work must have finished
  return VSLAM_OK;
}
// ---- per-stream lifetime: whole sequences of different lengths on the streams of one context (exact mode) --------------
VS_API int vslam_set_stream_active(vslam_ctx* c, int s, int active) {
  if (int rc = check_stream_index(c, s)) return rc;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_stream_active called inside a frame (between vslam_frame_begin and vslam_stereo_new)");
  const uint32_t bit = 1u << (s & 31);
  const bool was = (c->buf.active[s >> 5] & bit) != 0;
  if (was == (active != 0)) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                       // the buffer tables in flight still carry the old mask
  if (active) c->buf.active[s >> 5] |= bit; else c->buf.active[s >> 5] &= ~bit;
  return upload_buffer_tables(c);
}
VS_API int vslam_reset_streams(vslam_ctx* c, int32_t n, const int32_t* streams) {
  if (!c || n < 0 || (n && !streams)) return VSLAM_ERR_INVALID;
  for (int i = 0; i < n; ++i) if (int rc = check_stream_index(c, streams[i])) return rc;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_reset_stream called inside a frame");
  if (n == 0) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->B == 1) { c->pend.flags = 0; c->report_have = 0; }     // the one stream starts over: pending setters belong to the old sequence
  // no host synchronisation: each half of the state is reset in order on the HIP stream that owns it, one launch per
  // half for up to 63 streams
  ResetList l;
  l.n = 0;
  auto flush = [&]() -> int {
    if (!l.n) return VSLAM_OK;
    hipLaunchKernelGGL(k_reset_stream_img, dim3(1), dim3(64), 0, c->stream_img, c->cfg, c->buf, l);
    hipLaunchKernelGGL(k_reset_stream_trk, dim3(1), dim3(64), 0, c->stream, c->cfg, c->buf, l);
    if (c->map.cap)     // the stream's map starts over with its sequence (frame 0 never reads the previous frame's ids)
      for (int i = 0; i < l.n; ++i) HIP_TRY(c, hipMemsetAsync(c->map.d.count + l.ids[i], 0, sizeof(int32_t), c->stream));
    if (c->obs.cap)     // and its observation log with it
      for (int i = 0; i < l.n; ++i) HIP_TRY(c, hipMemsetAsync(c->obs.d.count + l.ids[i], 0, sizeof(int32_t), c->stream));
    l.n = 0;
    return VSLAM_OK;
  };
  for (int i = 0; i < n; ++i) {
    guess_drop_pending(c, streams[i]);
    l.ids[l.n++] = streams[i];
    if (l.n == 63) { int rc = flush(); if (rc) return rc; }
  }
  int rc = flush();
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
VS_API int vslam_reset_stream(vslam_ctx* c, int s) { const int32_t id = s; return vslam_reset_streams(c, 1, &id); }
VS_API int vslam_set_hip_stream(vslam_ctx* c, void* s) {
  if (!c) return VSLAM_ERR_INVALID;
  sync_all(c);
  destroy_streams(c);
  // one caller stream: image pipeline and tracker run back to back on it
  c->stream = c->stream_img = (hipStream_t)s;
  for (int k = 0; k < 2; ++k) { (void)hipEventCreateWithFlags(&c->ev_img[k], hipEventDisableTiming); (void)hipEventCreateWithFlags(&c->ev_frm[k], hipEventDisableTiming); }
  c->frm_pending[0] = c->frm_pending[1] = false;
  c->own_stream = false;
  calibrate_queues(c);      // the caller's queue has its own first XCD
  return upload_buffer_tables(c);
}
VS_API int vslam_synchronize(vslam_ctx* c) {
  if (!c) return VSLAM_ERR_INVALID;
  HIP_TRY(c, hipStreamSynchronize(c->stream_img));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return c->sticky;
}
