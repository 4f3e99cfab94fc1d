// vslam_hip.hip — host side of libvslam_hip.so: context / device-buffer management, kernel launches
// and read-back behind the C ABI of include/vslam_hip.h.  gfx950 only; there is no CPU fallback:
// every entry point fails with VSLAM_ERR_NO_DEVICE / VSLAM_ERR_HIP when the GPU path is unusable.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kernels_frame2.h"
#include "kernels_depth.h"
#include "kernels_orb.h"
#include "kernels_landmark.h"
#include "kernels_report.h"
#include "kernels_rectify.h"
#include "kernels_map.h"
#include "kernels_obs.h"

#define VS_API extern "C" __attribute__((visibility("default")))

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
  double timer_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EvRec { hipEvent_t a, b; int k; bool count; };
  std::vector<EvRec> evrec;
  struct EvShared { hipEvent_t a, b; int k; };      // interval whose start event belongs to an EvRec (only b returns to the pool)
  std::vector<EvShared> evshared;
  std::vector<hipEvent_t> evpool;
  double kern_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int kern_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // RGB-D components: the space map of the last vslam_depth_space_map call stays resident for vslam_depth_compute
  struct DepthMap { int rows = 0, cols = 0; uint16_t* depth = nullptr; unsigned long long* key = nullptr; int32_t* last = nullptr;
                    float* space = nullptr; int16_t* row_map = nullptr; int16_t* col_map = nullptr; bool valid = false; } dm;
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
  // rectification of raw input pairs (vslam_set_rectification): maps at the rectified size, padded to map_stride entries per row, and
  // the raw slabs [step parity][left/right] host images are copied into (B x raw_rows x raw_stride each).  k_rectify writes the rectified
  // pair into upload[parity], so everything downstream, and the two-parity lifetime of the image slabs, is unchanged.
  struct Rect { bool on = false, have_frame = false; int raw_rows = 0, raw_cols = 0, raw_stride = 0, map_stride = 0; size_t raw_stream_stride = 0;
                int16_t* map_xy[2] = {nullptr, nullptr}; uint16_t* map_a[2] = {nullptr, nullptr};
                uint8_t* raw[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
                const uint8_t* src[2] = {nullptr, nullptr}; int32_t src_row_stride = 0; size_t src_stream_stride = 0;   // this step's raw input
                std::vector<void*> mem; } rect;
  // the landmark map (vslam_enable_map, kernels_map.h): off while cap == 0; its own allocations, freed by vslam_enable_map(0) and destroy
  struct MapStore { int32_t cap = 0; DevMap d{}; std::vector<void*> mem; } map;
  // the observation log on top of it (vslam_enable_observations, kernels_obs.h): off while cap == 0; freed by vslam_enable_observations(0),
  // vslam_enable_map(0) and destroy
  struct ObsStore { int32_t cap = 0; DevObs d{}; } obs;
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
static void sync_all(vslam_ctx* c);
static int flush_pending(vslam_ctx* c);
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


static void sync_all(vslam_ctx* c) {
  (void)hipStreamSynchronize(c->stream_img);
  (void)hipStreamSynchronize(c->stream);
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
}
static int upload_buffer_tables(vslam_ctx* c) {
  const DevBuf hb[2] = {buf_set(c, 0, c->q0_frm), buf_set(c, 1, c->q0_frm)};
  HIP_TRY(c, hipMemcpy(c->d_bufs, hb, sizeof hb, hipMemcpyHostToDevice));
  return VSLAM_OK;
}
static int init_state(vslam_ctx* c) {
  c->pend.flags = 0;          // a reset drops setters that were waiting for a stage launch: the fresh state is the state
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
static int create_internal(const vslam_config* cfg, int device, int n_streams, vslam_ctx** out);
static int init_state(vslam_ctx* c);
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
  c->up_stream_stride = (size_t)rows * d.bstride;
  for (int q = 0; q < 2; ++q)
    for (int d2 = 0; d2 < 2; ++d2)
      if (e == hipSuccess) e = dalloc(c, &c->upload[q][d2], B * c->up_stream_stride);
  if (e != hipSuccess) {
    std::string msg = std::string("vslam_create: hipMalloc failed: ") + hipGetErrorString(e);
    for (void* p : c->allocs) (void)hipFree(p);
    destroy_streams(c);
    delete c;
    return fail(nullptr, VSLAM_ERR_HIP, msg);
  }
  // score8 must read 0 where no corner was ever written only through the mask, box/mask are fully
  // rewritten every frame; nothing else needs initialisation besides the stream state.
  for (int i = 0; i < 6; ++i) (void)hipEventCreate(&c->ev[i]);
  {
    // the frame kernel's view of the configuration and of the buffer table (image pointers excluded: it never reads them)
    calibrate_queues(c);
    e = dalloc(c, &c->d_cfg, 1);
    if (e == hipSuccess) e = dalloc(c, &c->d_bufs, 2);
    if (e == hipSuccess) e = hipMemcpy(c->d_cfg, &c->cfg, sizeof(DevCfg), hipMemcpyHostToDevice);
    if (e == hipSuccess && upload_buffer_tables(c) != VSLAM_OK) e = hipErrorUnknown;
    if (e != hipSuccess) {
      std::string msg = std::string("vslam_create: device tables: ") + hipGetErrorString(e);
      for (void* p : c->allocs) (void)hipFree(p);
      for (int i = 0; i < 6; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
      destroy_streams(c);
      delete c;
      return fail(nullptr, VSLAM_ERR_HIP, msg);
    }
  }
  int rc = init_state(c);
  if (rc != VSLAM_OK) {
    g_create_error = c->err;
    for (void* p : c->allocs) (void)hipFree(p);
    for (int i = 0; i < 6; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    destroy_streams(c);
    delete c;
    return rc;
  }
  *out = c;
  return VSLAM_OK;
}

static void depth_map_free(vslam_ctx* c) {
  vslam_ctx::DepthMap& m = c->dm;
  (void)hipFree(m.depth); (void)hipFree(m.key); (void)hipFree(m.last); (void)hipFree(m.space);
  (void)hipFree(m.row_map); (void)hipFree(m.col_map);
  m = vslam_ctx::DepthMap();
}
// the resident space map at rows x cols: its own allocations (it outlives the call that fills it), kept while the size stays
static hipError_t depth_map_resize(vslam_ctx* c, int rows, int cols) {
  vslam_ctx::DepthMap& m = c->dm;
  if (m.rows == rows && m.cols == cols) return hipSuccess;
  depth_map_free(c);
  const size_t n = (size_t)rows * cols;
  hipError_t e = hipMalloc((void**)&m.depth, n * sizeof(uint16_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m.key, n * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMalloc((void**)&m.last, n * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m.space, n * 3 * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&m.row_map, n * sizeof(int16_t));
  if (e == hipSuccess) e = hipMalloc((void**)&m.col_map, n * sizeof(int16_t));
  if (e != hipSuccess) { depth_map_free(c); return e; }
  m.rows = rows; m.cols = cols;
  return hipSuccess;
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
  for (void* p : c->rect.mem) (void)hipFree(p);
  for (void* p : c->map.mem) (void)hipFree(p);
  if (c->obs.d.log) (void)hipFree(c->obs.d.log);
  if (c->obs.d.count) (void)hipFree(c->obs.d.count);
  tmp_free(c);
  depth_map_free(c);
  if (c->report) (void)hipHostFree(c->report);
  for (int q = 0; q < 2; ++q) { if (c->pin_img[q]) (void)hipHostFree(c->pin_img[q]); if (c->pin_ev[q]) (void)hipEventDestroy(c->pin_ev[q]); }
  for (int i = 0; i < 6; ++i) if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  harvest_events(c);
  for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
  destroy_streams(c);
  delete c;
}
VS_API int vslam_reset(vslam_ctx* c) {
  if (!c) return VSLAM_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  return init_state(c);
}
// ---- per-stream lifetime: whole sequences of different lengths on the streams of one context (exact mode) --------------
VS_API int vslam_set_stream_active(vslam_ctx* c, int s, int active) {
  if (!c) return VSLAM_ERR_INVALID;
  if (s < 0 || s >= c->B) return fail(c, VSLAM_ERR_INVALID, "stream index out of range");
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
  for (int i = 0; i < n; ++i) if (streams[i] < 0 || streams[i] >= c->B) return fail(c, VSLAM_ERR_INVALID, "stream index out of range");
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
    l.ids[l.n++] = streams[i];
    if (l.n == 63) { int rc = flush(); if (rc) return rc; }
  }
  int rc = flush();
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
VS_API int vslam_reset_stream(vslam_ctx* c, int s) { const int32_t id = s; return vslam_reset_streams(c, 1, &id); }
VS_API int vslam_copy_current_poses_device(vslam_ctx* c, double* dst) {
  if (!c || !dst) return VSLAM_ERR_INVALID;
  { int rc = flush_pending(c); if (rc) return rc; }
  hipLaunchKernelGGL(k_gather_poses, dim3((c->B * 12 + 255) / 256), dim3(256), 0, c->stream, buf_set(c, c->last_set), c->B, dst);
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
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


// ---- launches ------------------------------------------------------------------------------------
static int launch_image_pipeline(vslam_ctx* c) {
  const DevCfg& d = c->cfg;
  const int set = c->parity;
  const int n = c->B;
  hipStream_t st = c->img_override ? c->img_override : c->stream_img;
  const DevBuf bs = buf_set(c, set, c->img_override ? c->q0_frm : c->q0_img);
  if (!c->img_override && c->img_on_frm_queue) {
    // the last frame's image pipeline ran on the frame queue (stage path) and left no event behind: a caller that switches to
    // the fused path mid-sequence pays one synchronisation here, once
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->img_on_frm_queue = false;
  }
  if (c->img_override) c->img_on_frm_queue = true;
  const bool coarse = c->img_override != nullptr;     // stage path: detection = [k_fast_box .. k_emit], extraction = k_brief: three events
  // the image products of this set were last read by the frame kernel two steps ago; the detector thresholds come
  // from the controller in k_emit of the previous step (same queue)
  if (c->frm_pending[set] && st != c->stream) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_frm[set], 0));
  if (c->rect.on) {
    // raw pair -> rectified pair in upload[set] (the slab the wait above has freed), ahead of the detector
    const vslam_ctx::Rect& q = c->rect;
    RectArgs ra;
    for (int k = 0; k < 2; ++k) { ra.src[k] = q.src[k]; ra.map_xy[k] = q.map_xy[k]; ra.map_a[k] = q.map_a[k]; ra.dst[k] = c->upload[set][k]; }
    ra.src_stream_stride = q.src_stream_stride; ra.src_row_stride = q.src_row_stride; ra.src_rows = q.raw_rows; ra.src_cols = q.raw_cols;
    ra.map_stride = q.map_stride; ra.dst_stream_stride = c->up_stream_stride; ra.dst_row_stride = c->up_stride;
    ra.rows = d.c.rows; ra.cols = d.c.cols; ra.s0 = 0; ra.n = n; ra.sides = 2;
    std::memcpy(ra.active, c->buf.active, sizeof ra.active);
    hipLaunchKernelGGL(k_rectify, dim3((d.c.cols + 255) / 256, (d.c.rows + 3) / 4, 2 * ((n + VS_RECT_SB - 1) / VS_RECT_SB)), dim3(256), 0, st, ra);
  }
  dim3 g1(d.TX, (d.c.rows + VS_TILE_H - 1) / VS_TILE_H, 2 * n);
  const bool orb = d.c.descriptor_type == VSLAM_DESCRIPTOR_ORB;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (coarse && c->timers) { e0 = ev_get(c); (void)hipEventRecord(e0, st); }
  { KernelTimer t(c, 0, st, true, !coarse); hipLaunchKernelGGL(k_fast_box, g1, dim3(256), VS_FB_DYN_LDS, st, c->cfg, bs); }
  { KernelTimer t(c, 1, st, true, !coarse); hipLaunchKernelGGL(k_emit, dim3(n, 2), dim3(512), 0, st, c->cfg, bs, orb ? (int)VSLAM_ORB_BORDER : (int)VSLAM_BRIEF_BORDER, 1); }
  if (e0) { e1 = ev_get(c); (void)hipEventRecord(e1, st); c->evrec.push_back({e0, e1, 0, true}); c->kern_n[1] += 1; }
  if (c->img_override && c->report && c->B == 1) {
    // stage path with a view reader: coordinates and scores leave for the host as soon as k_emit has written them, so that the caller
    // builds its cv::KeyPoint lists while k_brief / k_stereo_dist / k_begin still run (vslam_view_keypoints_xy)
    c->report_xy_seq = ++c->report_seq;
    hipLaunchKernelGGL(k_report, dim3(8), dim3(256), 0, st, c->cfg, bs, 0, (int)VS_REPORT_KEYPOINTS_XY, 0, c->report_xy_seq, c->rl, c->report_dev, c->report_done);
  }
  if (orb) {   // cv::ORB::create() as extractor: Gaussian image (in the box image's memory), steered tests per keypoint
    KernelTimer t(c, 2, st, true, !coarse);
    Gauss7 gk; for (int i = 0; i < 4; ++i) gk.k[i] = d.gauss7[i];
    hipLaunchKernelGGL(k_gauss7, g1, dim3(256), 0, st, c->cfg, bs, gk);
    hipLaunchKernelGGL(k_orb_describe, dim3((d.c.cols + VS_BT_W - 1) / VS_BT_W, (d.c.rows + VS_BT_H - 1) / VS_BT_H, 2 * n), dim3(256), 0, st, c->cfg, bs, d.orb_cos, d.orb_sin);
  } else {
    dim3 g3((d.c.cols + VS_BT_W - 1) / VS_BT_W, (d.c.rows + VS_BT_H - 1) / VS_BT_H, 2 * n);
    KernelTimer t(c, 2, st, true, !coarse); hipLaunchKernelGGL(k_brief, g3, dim3(256), 0, st, c->cfg, bs);
  }
  if (e1) { hipEvent_t e2 = ev_get(c); (void)hipEventRecord(e2, st); hipEvent_t e1b = e1; c->evshared.push_back({e1b, e2, 2}); }
  // left-right descriptor distances of the first epipolar pass: a product of the images alone, so it is computed
  // here, wide, instead of inside the per-stream frame workgroup
  { KernelTimer t(c, 7, st, true, !coarse); hipLaunchKernelGGL(k_stereo_dist, dim3((d.NMAX + 255) / 256, n), dim3(256), 0, st, c->cfg, bs); }
  HIP_TRY(c, hipGetLastError());
  if (st != c->stream) { HIP_TRY(c, hipEventRecord(c->ev_img[set], st)); HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_img[set], 0)); }
  c->last_set = set;
  if (c->rect.on) c->rect.have_frame = true;
  return VSLAM_OK;
}
static int frame_done(vslam_ctx* c) {
  const int set = c->last_set;
  if (c->stream_img != c->stream) { HIP_TRY(c, hipEventRecord(c->ev_frm[set], c->stream)); c->frm_pending[set] = true; }
  c->parity = set ^ 1;
  return VSLAM_OK;
}
// blocks per stream of the candidate kernel (16 point groups each).  Streams differ in cost by an order of magnitude (a
// Localizing stream searches 101 x 101 windows by appearance, a Tracking stream ~31 x 31), so the points are spread over
// many small blocks — about one previous point per 16-lane group at ~700 points — and the hardware scheduler balances
// them: 0.154 -> 0.086 ms back to back at 160 streams of mixed phase against 12 blocks per stream (profiles/r02_*).
static int cand_blocks(int n_streams) { return std::max(4, std::min(128, 7040 / std::max(n_streams, 1))); }
// blocks per stream of k_recover_brief (four wavefronts each, one lost point per wavefront)
static int recover_blocks(int n_streams) { return std::max(4, std::min(64, 1024 / std::max(n_streams, 1))); }
static int launch_frame(vslam_ctx* c) {
  const int n = c->B;
  hipStream_t st = c->stream;
  const DevBuf bs = buf_set(c, c->last_set, c->q0_frm);
  ConstDevCfg* kc = (ConstDevCfg*)c->d_cfg;
  ConstDevBuf* kb = (ConstDevBuf*)(c->d_bufs + c->last_set);
  { KernelTimer t(c, 3, st); hipLaunchKernelGGL(k_track_candidates, dim3(cand_blocks(n), n), dim3(256), 0, st, c->cfg, bs, -1); }
  if (c->split == 0) {
    KernelTimer t(c, 4, st);
    hipLaunchKernelGGL(k_frame, dim3(n), dim3(VS_WG), 0, st, kc, kb, -1);
  } else {
    // few streams on an otherwise idle chip: the landmark refinement (a serial chain per track) leaves the frame's critical path — it runs in
    // workgroups of its own beside the stereo sweep, inside the frame's last launch
    { KernelTimer t(c, 4, st, false); hipLaunchKernelGGL(k_frame, dim3(n), dim3(VS_WG), 0, st, kc, kb, 0); }
    if (c->cfg.c.enable_landmark_recovery) { KernelTimer t(c, 5, st); hipLaunchKernelGGL(k_recover_brief, dim3(recover_blocks(n), n), dim3(256), 0, st, c->cfg, bs); }
    { KernelTimer t(c, 4, st, false); hipLaunchKernelGGL(k_frame, dim3(n), dim3(VS_WG), 0, st, kc, kb, 4); }
    // phase 2 and the landmark refinement in ONE launch: n frame workgroups + G refinement workgroups per stream (k_tail_lm)
    { KernelTimer t(c, 4, st); const int G = std::max(1, std::min(16, 64 / std::max(n, 1)));
      hipLaunchKernelGGL(k_tail_lm, dim3(n * (1 + G)), dim3(VS_WG), 0, st, kc, kb, n, G); }
  }
  // the landmark map, behind the frame's last launch (sequence 4: behind the refinement workgroups of k_tail_lm as well)
  if (c->map.cap) hipLaunchKernelGGL(k_map_commit, dim3(n), dim3(VS_MAP_WG), 0, st, c->cfg, bs, c->map.d);
  // the observation log, behind the ids k_map_commit has just left for this frame
  if (c->obs.cap) hipLaunchKernelGGL(k_obs_append, dim3(n), dim3(VS_OBS_WG), 0, st, c->cfg, bs, c->map.d, c->obs.d);
  HIP_TRY(c, hipGetLastError());
  return frame_done(c);
}
static int set_images_device(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride) {
  if (!L || !R) return fail(c, VSLAM_ERR_INVALID, "called with empty frame");  // stereo_framepoint_generator.cpp:75-78
  if (row_stride < c->cfg.c.cols) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than image width");
  c->buf.img[0] = L; c->buf.img[1] = R;
  c->buf.img_row_stride = row_stride;
  c->buf.img_stream_stride = image_stride;
  return VSLAM_OK;
}
// where a step's input images live on the device
struct ImgLoc { const uint8_t* p[2]; int32_t row_stride; size_t stream_stride; };
// Host images of all streams (rows x cols each) into the device slabs dst[left/right] (dst_stride bytes per row, dst_stream_stride per
// stream); *out receives where they landed: one copy per side keeps the caller's strides.
static int upload_to(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, int rows, int cols,
                     uint8_t* const dst[2], int32_t dst_stride, size_t dst_stream_stride, ImgLoc* out) {
  if (!L || !R) return fail(c, VSLAM_ERR_INVALID, "called with empty frame");
  if (row_stride < cols) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than image width");
  // Host images of all streams in one (nearly) dense block: one copy per side, the caller's strides kept on the device
  // (2 B strided 2-D copies per step cost more in submission than in transfer).
  const size_t span = (size_t)(c->B - 1) * image_stride + (size_t)(rows - 1) * row_stride + cols;   // last byte the caller owns
  const size_t dense = (size_t)c->B * rows * cols;
  const bool ordered = c->B == 1 || image_stride >= (size_t)rows * row_stride;
  if (ordered && span <= (size_t)c->B * dst_stream_stride && span <= dense + dense / 8) {
    hipStream_t st = c->img_override ? c->img_override : c->stream_img;
    // A small pageable source (the literal drop-in: one cv::Mat pair per call) goes through pinned memory of the context: the
    // runtime's own staging of a pageable hipMemcpyAsync costs ~0.12 ms of host time per 467 KB image here, a memcpy into a pinned
    // buffer + a true asynchronous copy ~0.03 ms; the left image's DMA runs while the right one is being staged.
    if (span <= ((size_t)4 << 20)) {
      hipPointerAttribute_t at;
      const bool pinned = hipPointerGetAttributes(&at, L) == hipSuccess && at.type == hipMemoryTypeHost;
      if (!pinned) {
        (void)hipGetLastError();   // "invalid value" for a plain malloc'ed pointer is the expected answer, not an error of this call
        const size_t half = (span + 255) & ~(size_t)255;
        if (c->pin_img_bytes < 2 * half) {
          for (int q = 0; q < 2; ++q) {
            if (c->pin_ev[q]) HIP_TRY(c, hipEventSynchronize(c->pin_ev[q]));
            if (c->pin_img[q]) { (void)hipHostFree(c->pin_img[q]); c->pin_img[q] = nullptr; }
            void* h = nullptr;
            HIP_TRY(c, hipHostMalloc(&h, 2 * half, hipHostMallocDefault));
            c->pin_img[q] = (unsigned char*)h;
            if (!c->pin_ev[q]) HIP_TRY(c, hipEventCreateWithFlags(&c->pin_ev[q], hipEventDisableTiming));
          }
          c->pin_img_bytes = 2 * half;
        } else if (c->pin_used[c->parity]) {
          HIP_TRY(c, hipEventSynchronize(c->pin_ev[c->parity]));     // the copy that last read this staging buffer (two frames ago)
        }
        unsigned char* stage = c->pin_img[c->parity];
        std::memcpy(stage, L, span);
        HIP_TRY(c, hipMemcpyAsync(dst[0], stage, span, hipMemcpyHostToDevice, st));
        std::memcpy(stage + half, R, span);
        HIP_TRY(c, hipMemcpyAsync(dst[1], stage + half, span, hipMemcpyHostToDevice, st));
        HIP_TRY(c, hipEventRecord(c->pin_ev[c->parity], st));
        c->pin_used[c->parity] = true;
        *out = {{dst[0], dst[1]}, row_stride, image_stride};
        return VSLAM_OK;
      }
    }
    HIP_TRY(c, hipMemcpyAsync(dst[0], L, span, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(dst[1], R, span, hipMemcpyHostToDevice, st));
    *out = {{dst[0], dst[1]}, row_stride, image_stride};
    return VSLAM_OK;
  }
  if (row_stride <= dst_stride) {
    // one contiguous copy per image, rows keep the caller's stride (a pitched host-to-device copy is issued row by row
    // by the runtime: measured 0.13 GB/s against 43 GB/s for the plain copy)
    for (int s = 0; s < c->B; ++s) {
      const size_t bytes = (size_t)(rows - 1) * row_stride + cols;
      HIP_TRY(c, hipMemcpyAsync(dst[0] + s * dst_stream_stride, L + s * image_stride, bytes, hipMemcpyHostToDevice, c->stream_img));
      HIP_TRY(c, hipMemcpyAsync(dst[1] + s * dst_stream_stride, R + s * image_stride, bytes, hipMemcpyHostToDevice, c->stream_img));
    }
    *out = {{dst[0], dst[1]}, row_stride, dst_stream_stride};
    return VSLAM_OK;
  }
  for (int s = 0; s < c->B; ++s) {
    HIP_TRY(c, hipMemcpy2DAsync(dst[0] + s * dst_stream_stride, dst_stride, L + s * image_stride, row_stride,
                                cols, rows, hipMemcpyHostToDevice, c->stream_img));
    HIP_TRY(c, hipMemcpy2DAsync(dst[1] + s * dst_stream_stride, dst_stride, R + s * image_stride, row_stride,
                                cols, rows, hipMemcpyHostToDevice, c->stream_img));
  }
  *out = {{dst[0], dst[1]}, dst_stride, dst_stream_stride};
  return VSLAM_OK;
}
static int upload_images(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride) {
  ImgLoc o;
  const int rc = upload_to(c, L, R, row_stride, image_stride, c->cfg.c.rows, c->cfg.c.cols, c->upload[c->parity], c->up_stride, c->up_stream_stride, &o);
  return rc != VSLAM_OK ? rc : set_images_device(c, o.p[0], o.p[1], o.row_stride, o.stream_stride);
}
// Raw input of a rectifying context: host images go to the raw slabs of this step's parity, device images are read in place (by k_rectify
// only); the image pipeline reads the rectified pair k_rectify leaves in upload[parity].
static int set_raw_inputs(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, bool on_device) {
  vslam_ctx::Rect& q = c->rect;
  if (!L || !R) return fail(c, VSLAM_ERR_INVALID, "called with empty frame");
  if (row_stride < q.raw_cols) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than the raw image width");
  ImgLoc o = {{L, R}, row_stride, image_stride};
  if (!on_device) {
    const int rc = upload_to(c, L, R, row_stride, image_stride, q.raw_rows, q.raw_cols, q.raw[c->parity], q.raw_stride, q.raw_stream_stride, &o);
    if (rc != VSLAM_OK) return rc;
  }
  q.src[0] = o.p[0]; q.src[1] = o.p[1]; q.src_row_stride = o.row_stride; q.src_stream_stride = o.stream_stride;
  return set_images_device(c, c->upload[c->parity][0], c->upload[c->parity][1], c->up_stride, c->up_stream_stride);
}
static int set_inputs(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, bool on_device) {
  if (c->rect.on) return set_raw_inputs(c, L, R, row_stride, image_stride, on_device);
  return on_device ? set_images_device(c, L, R, row_stride, image_stride) : upload_images(c, L, R, row_stride, image_stride);
}

VS_API int vslam_process_device(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->sticky != VSLAM_OK) return c->sticky;
  int rc = set_inputs(c, L, R, row_stride, image_stride, true);
  if (rc != VSLAM_OK) return rc;
  rc = flush_pending(c);
  if (rc != VSLAM_OK) return rc;
  rc = launch_image_pipeline(c);
  if (rc != VSLAM_OK) return rc;
  return launch_frame(c);
}
VS_API int vslam_process_host(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->sticky != VSLAM_OK) return c->sticky;
  HIP_TRY(c, hipSetDevice(c->device));
  int rc = set_inputs(c, L, R, row_stride, image_stride, false);
  if (rc != VSLAM_OK) return rc;
  rc = flush_pending(c);
  if (rc != VSLAM_OK) return rc;
  rc = launch_image_pipeline(c);
  if (rc != VSLAM_OK) return rc;
  return launch_frame(c);
}

// ---- rectification of raw input pairs ------------------------------------------------------------
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
static void rect_free(vslam_ctx* c) {
  for (void* p : c->rect.mem) (void)hipFree(p);
  c->rect = vslam_ctx::Rect();
}
VS_API int vslam_set_rectification(vslam_ctx* c, int32_t raw_rows, int32_t raw_cols, const int16_t* xyL, const uint16_t* aL, const int16_t* xyR,
                                   const uint16_t* aR) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_rectification called inside a frame");
  const bool off = !xyL && !aL && !xyR && !aR;
  if (!off && (!xyL || !aL || !xyR || !aR)) return fail(c, VSLAM_ERR_INVALID, "vslam_set_rectification: all four maps or none");
  if (!off && (raw_rows < 1 || raw_cols < 1 || raw_rows > 32767 || raw_cols > 32767))
    return fail(c, VSLAM_ERR_INVALID, "vslam_set_rectification: invalid raw image dimensions");
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols;
  if (!off && (!rect_maps_ok(aL, (size_t)rows * cols) || !rect_maps_ok(aR, (size_t)rows * cols)))
    return fail(c, VSLAM_ERR_INVALID, "vslam_set_rectification: interpolation table index >= 1024");
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the old maps and raw slabs
  rect_free(c);
  if (off) return VSLAM_OK;
  vslam_ctx::Rect& q = c->rect;
  q.raw_rows = raw_rows; q.raw_cols = raw_cols;
  q.raw_stride = (raw_cols + 63) & ~63;
  q.raw_stream_stride = (size_t)raw_rows * q.raw_stride;
  q.map_stride = (cols + 3) & ~3;
  auto get = [&](void** p, size_t bytes) -> hipError_t {
    const hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 1));
    if (e == hipSuccess) q.mem.push_back(*p);
    return e;
  };
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = get((void**)&q.map_xy[k], (size_t)rows * q.map_stride * 4);
    if (e == hipSuccess) e = get((void**)&q.map_a[k], (size_t)rows * q.map_stride * 2);
    for (int p = 0; p < 2 && e == hipSuccess; ++p) e = get((void**)&q.raw[p][k], (size_t)c->B * q.raw_stream_stride);
  }
  std::vector<int16_t> pxy;
  std::vector<uint16_t> pa;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    rect_pad_maps(k ? xyR : xyL, k ? aR : aL, rows, cols, q.map_stride, pxy, pa);
    e = hipMemcpy(q.map_xy[k], pxy.data(), pxy.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(q.map_a[k], pa.data(), pa.size() * 2, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) { rect_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_rectification: ") + hipGetErrorString(e)); }
  q.on = true;
  return VSLAM_OK;
}
VS_API int vslam_remap_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, const int16_t* map_xy,
                          const uint16_t* map_a, int32_t drows, int32_t dcols, uint8_t* dst) {
  tmp_reset(c);
  if (!c) return VSLAM_ERR_INVALID;
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (!src || !dst || !map_xy || !map_a || rows < 1 || cols < 1 || row_stride < cols || drows < 1 || dcols < 1)
    return fail(c, VSLAM_ERR_INVALID, "remap: bad argument");
  if (!rect_maps_ok(map_a, (size_t)drows * dcols)) return fail(c, VSLAM_ERR_INVALID, "remap: interpolation table index >= 1024");
  HIP_TRY(c, hipSetDevice(c->device));
  const int ms = (dcols + 3) & ~3;
  std::vector<int16_t> pxy;
  std::vector<uint16_t> pa;
  rect_pad_maps(map_xy, map_a, drows, dcols, ms, pxy, pa);
  uint8_t *ds = nullptr, *dd = nullptr;
  int16_t* dxy = nullptr;
  uint16_t* da = nullptr;
  hipError_t e = tmp_get(c, (void**)&ds, (size_t)rows * row_stride);
  if (e == hipSuccess) e = tmp_get(c, (void**)&dxy, pxy.size() * 2);
  if (e == hipSuccess) e = tmp_get(c, (void**)&da, pa.size() * 2);
  if (e == hipSuccess) e = tmp_get(c, (void**)&dd, (size_t)drows * ms);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, src, (size_t)(rows - 1) * row_stride + cols, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dxy, pxy.data(), pxy.size() * 2, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(da, pa.data(), pa.size() * 2, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    RectArgs ra;
    std::memset(&ra, 0, sizeof ra);
    ra.src[0] = ds; ra.src_row_stride = row_stride; ra.src_rows = rows; ra.src_cols = cols;
    ra.map_xy[0] = dxy; ra.map_a[0] = da; ra.map_stride = ms;
    ra.dst[0] = dd; ra.dst_row_stride = ms; ra.dst_stream_stride = (size_t)drows * ms;
    ra.rows = drows; ra.cols = dcols; ra.s0 = 0; ra.n = 1; ra.sides = 1; ra.active[0] = 1u;
    hipLaunchKernelGGL(k_rectify, dim3((dcols + 255) / 256, (drows + 3) / 4, 1), dim3(256), 0, c->stream, ra);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy2DAsync(dst, dcols, dd, ms, dcols, drows, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, VSLAM_ERR_HIP, hipGetErrorString(e));
  return VSLAM_OK;
}

// ---- read-back -----------------------------------------------------------------------------------
static int check_stream(vslam_ctx* c, int s) {
  if (!c) return VSLAM_ERR_INVALID;
  if (s < 0 || s >= c->B) return fail(c, VSLAM_ERR_INVALID, "stream index out of range");
  { int rc = flush_pending(c); if (rc) return rc; }
  sync_all(c);   // read-back: every group's queued work must have finished
  return VSLAM_OK;
}
VS_API int vslam_get_rectified_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_rectified_images: null output");
  if (!c->rect.on || !c->rect.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_rectified_images: no frame has been rectified since vslam_set_rectification");
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols;
  for (int k = 0; k < 2; ++k)
    HIP_TRY(c, hipMemcpy2D(k ? right : left, cols, c->upload[c->last_set][k] + (size_t)s * c->up_stream_stride, c->up_stride, cols, rows,
                           hipMemcpyDeviceToHost));
  return VSLAM_OK;
}
template <typename T>
static hipError_t d2h(vslam_ctx* c, T* dst, const T* src, size_t count) {
  if (!dst || !count) return hipSuccess;
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream);
}
VS_API int vslam_get_frame_info(vslam_ctx* c, int s, vslam_frame_info* out) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!out) return fail(c, VSLAM_ERR_INVALID, "null output");
  HIP_TRY(c, d2h(c, out, c->buf.info + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out->error_flags) { c->err = "device buffer capacity exceeded (error_flags != 0)"; }
  return VSLAM_OK;
}
VS_API int vslam_get_keypoints(vslam_ctx* c, int s, int side, int32_t cap, int32_t* n, int16_t* xy, int32_t* score, uint8_t* desc) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!n || side < 0 || side > 1) return fail(c, VSLAM_ERR_INVALID, "bad argument");
  int32_t cnt = 0;
  const vslam_ctx::ImgSet& iset = c->sets[c->last_set];
  HIP_TRY(c, hipStreamSynchronize(c->stream_img));
  HIP_TRY(c, d2h(c, &cnt, iset.n_kp + s * 2 + side, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n = cnt;
  if (cnt > cap) return fail(c, VSLAM_ERR_CAPACITY, "keypoint output capacity too small");
  const size_t o = ((size_t)s * 2 + side) * c->cfg.NMAX;
  std::vector<uint8_t> sc(cnt);
  HIP_TRY(c, d2h(c, xy, iset.kp_xy + o * 2, (size_t)cnt * 2));
  HIP_TRY(c, d2h(c, sc.data(), iset.kp_score + o, (size_t)cnt));
  HIP_TRY(c, d2h(c, desc, iset.desc + o * 32, (size_t)cnt * 32));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (score) for (int i = 0; i < cnt; ++i) score[i] = sc[i];
  return VSLAM_OK;
}
static int get_points_impl(vslam_ctx* c, int s, int in_progress, int32_t cap, int32_t* n, int16_t* kp, int32_t* meta, double* cam, double* lm,
                           uint8_t* desc) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!n) return fail(c, VSLAM_ERR_INVALID, "bad argument");
  StreamState st;
  HIP_TRY(c, d2h(c, &st, c->buf.st + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int32_t cnt = 0;
  const int pb = in_progress ? (st.cur ^ 1) : st.cur;
  if (in_progress) cnt = st.n_cur;
  else {
    HIP_TRY(c, d2h(c, &cnt, c->buf.n_points + s * 2 + st.cur, 1));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!st.has_prev) cnt = 0;
  }
  *n = cnt;
  if (cnt > cap) return fail(c, VSLAM_ERR_CAPACITY, "point output capacity too small");
  const size_t o = ((size_t)s * 2 + pb) * c->cfg.MAXP;
  std::vector<int32_t> m((size_t)cnt * META);
  std::vector<int16_t> k((size_t)cnt * 4);
  HIP_TRY(c, d2h(c, k.data(), c->buf.p_kp + o * 4, (size_t)cnt * 4));
  HIP_TRY(c, d2h(c, m.data(), c->buf.p_meta + o * META, (size_t)cnt * META));
  HIP_TRY(c, d2h(c, cam, c->buf.p_cam + o * 3, (size_t)cnt * 3));
  HIP_TRY(c, d2h(c, lm, c->buf.p_lm + o * 3, (size_t)cnt * 3));
  HIP_TRY(c, d2h(c, desc, c->buf.p_desc + o * 64, (size_t)cnt * 64));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < cnt; ++i) {
    if (kp) for (int q = 0; q < 4; ++q) kp[4 * i + q] = k[4 * i + q];
    if (meta) {
      meta[6 * i + 0] = m[META * i + M_DIST]; meta[6 * i + 1] = m[META * i + M_EPI]; meta[6 * i + 2] = m[META * i + M_PREV];
      meta[6 * i + 3] = m[META * i + M_TLEN]; meta[6 * i + 4] = m[META * i + M_LMUP]; meta[6 * i + 5] = k[4 * i] - k[4 * i + 2];
    }
    if (lm && m[META * i + M_LMUP] == 0) { lm[3 * i] = lm[3 * i + 1] = lm[3 * i + 2] = 0; }
  }
  return VSLAM_OK;
}
VS_API int vslam_get_points(vslam_ctx* c, int s, int32_t cap, int32_t* n, int16_t* kp, int32_t* meta, double* cam, double* lm) {
  return get_points_impl(c, s, 0, cap, n, kp, meta, cam, lm, nullptr);
}
VS_API int vslam_get_frame_points(vslam_ctx* c, int s, int in_progress, int32_t cap, int32_t* n, int16_t* kp, int32_t* meta, double* cam,
                                  double* lm, uint8_t* desc) {
  return get_points_impl(c, s, in_progress, cap, n, kp, meta, cam, lm, desc);
}
// ---- the landmark map (kernels_map.h) -------------------------------------------------------------
static void obs_free(vslam_ctx* c) {
  if (c->obs.d.log) (void)hipFree(c->obs.d.log);
  if (c->obs.d.count) (void)hipFree(c->obs.d.count);
  c->obs.d = DevObs{};
  c->obs.cap = 0;
}
static void map_free(vslam_ctx* c) {
  for (void* p : c->map.mem) (void)hipFree(p);
  c->map.mem.clear();
  c->map.d = DevMap{};
  c->map.cap = 0;
}
template <typename T>
static hipError_t map_alloc(vslam_ctx* c, T** p, size_t count) {
  const hipError_t e = hipMalloc((void**)p, count * sizeof(T));
  if (e == hipSuccess) c->map.mem.push_back(*p);
  return e;
}
VS_API int vslam_enable_map(vslam_ctx* c, int32_t cap) {
  if (!c) return VSLAM_ERR_INVALID;
  if (cap < 0) return fail(c, VSLAM_ERR_INVALID, "vslam_enable_map: negative capacity");
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_enable_map called inside a frame");
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                        // no commit of the old store may still be in flight
  map_free(c);
  if (cap == 0) { obs_free(c); return VSLAM_OK; }     // no ids, no log
  // a new store hands out ids from 0 again: the observation log starts over with it
  if (c->obs.cap) HIP_TRY(c, hipMemsetAsync(c->obs.d.count, 0, sizeof(int32_t) * c->B, c->stream));
  const size_t B = (size_t)c->B, n = B * (size_t)cap;
  DevMap d{};
  d.cap = cap; d.B = c->B;
  hipError_t e = map_alloc(c, &d.xyz, n * 3);
  if (e == hipSuccess) e = map_alloc(c, &d.info, n * 3);
  if (e == hipSuccess) e = map_alloc(c, &d.desc, n * 32);
  if (e == hipSuccess) e = map_alloc(c, &d.count, B);
  if (e == hipSuccess) e = map_alloc(c, &d.ids, 2 * B * (size_t)c->cfg.MAXP);
  if (e == hipSuccess) e = hipMemsetAsync(d.xyz, 0, n * 3 * sizeof(double), c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d.info, 0, n * 3 * sizeof(int32_t), c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d.desc, 0, n * 32, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d.count, 0, B * sizeof(int32_t), c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d.ids, 0xff, 2 * B * (size_t)c->cfg.MAXP * sizeof(int32_t), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { map_free(c); obs_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_enable_map: ") + hipGetErrorString(e)); }
  c->map.d = d;
  c->map.cap = cap;
  return VSLAM_OK;
}
static int map_size(vslam_ctx* c, int s, int32_t* n) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!c->map.cap) return fail(c, VSLAM_ERR_STATE, "the landmark map is not enabled (vslam_enable_map)");
  HIP_TRY(c, d2h(c, n, c->map.d.count + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_get_map_size(vslam_ctx* c, int s, int32_t* n) {
  if (c && !n) return fail(c, VSLAM_ERR_INVALID, "vslam_get_map_size: null output");
  return map_size(c, s, n);
}
VS_API int vslam_get_map(vslam_ctx* c, int s, int32_t first_id, int32_t cap, int32_t* n, double* xyz, int32_t* info, uint8_t* desc) {
  if (c && (!n || first_id < 0 || cap < 0)) return fail(c, VSLAM_ERR_INVALID, "vslam_get_map: null count, negative first id or capacity");
  int32_t size = 0;
  int rc = map_size(c, s, &size);
  if (rc) return rc;
  const int32_t cnt = std::max(0, std::min(cap, size - first_id));
  *n = cnt;
  const size_t o = (size_t)s * c->map.cap + (size_t)first_id;
  HIP_TRY(c, d2h(c, xyz, c->map.d.xyz + o * 3, (size_t)cnt * 3));
  HIP_TRY(c, d2h(c, info, c->map.d.info + o * 3, (size_t)cnt * 3));
  HIP_TRY(c, d2h(c, desc, c->map.d.desc + o * 32, (size_t)cnt * 32));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
// ---- the observation log (kernels_obs.h) ------------------------------------------------------------
VS_API int vslam_enable_observations(vslam_ctx* c, int32_t cap) {
  if (!c) return VSLAM_ERR_INVALID;
  if (cap < 0) return fail(c, VSLAM_ERR_INVALID, "vslam_enable_observations: negative capacity");
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_enable_observations called inside a frame");
  if (!c->map.cap) return fail(c, VSLAM_ERR_STATE, "vslam_enable_observations needs the landmark map (vslam_enable_map): ids come from it");
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                        // no append to the old store may still be in flight
  obs_free(c);
  if (cap == 0) return VSLAM_OK;
  const size_t B = (size_t)c->B;
  DevObs d{};
  d.cap = cap;
  hipError_t e = hipMalloc((void**)&d.log, B * (size_t)cap * sizeof(uint4));
  if (e == hipSuccess) e = hipMalloc((void**)&d.count, B * sizeof(int32_t));
  if (e == hipSuccess) e = hipMemsetAsync(d.log, 0, B * (size_t)cap * sizeof(uint4), c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d.count, 0, B * sizeof(int32_t), c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    if (d.log) (void)hipFree(d.log);
    if (d.count) (void)hipFree(d.count);
    return fail(c, VSLAM_ERR_HIP, std::string("vslam_enable_observations: ") + hipGetErrorString(e));
  }
  c->obs.d = d;
  c->obs.cap = cap;
  return VSLAM_OK;
}
static int obs_count(vslam_ctx* c, int s, int32_t* n) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!c->obs.cap) return fail(c, VSLAM_ERR_STATE, "the observation log is not enabled (vslam_enable_observations)");
  HIP_TRY(c, d2h(c, n, c->obs.d.count + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_get_observation_count(vslam_ctx* c, int s, int32_t* n) {
  if (c && !n) return fail(c, VSLAM_ERR_INVALID, "vslam_get_observation_count: null output");
  return obs_count(c, s, n);
}
VS_API int vslam_get_observations(vslam_ctx* c, int s, int32_t first, int32_t cap, int32_t* n, int32_t* id_frame, int16_t* kp) {
  if (c && (!n || first < 0 || cap < 0)) return fail(c, VSLAM_ERR_INVALID, "vslam_get_observations: null count, negative first entry or capacity");
  int32_t size = 0;
  int rc = obs_count(c, s, &size);
  if (rc) return rc;
  const int32_t cnt = std::max(0, std::min(cap, size - first));
  *n = cnt;
  if (!cnt || (!id_frame && !kp)) return VSLAM_OK;
  std::vector<uint4> e((size_t)cnt);
  HIP_TRY(c, d2h(c, e.data(), c->obs.d.log + (size_t)s * c->obs.cap + (size_t)first, (size_t)cnt));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int32_t i = 0; i < cnt; ++i) {
    if (id_frame) { id_frame[2 * i] = (int32_t)e[i].x; id_frame[2 * i + 1] = (int32_t)e[i].y; }
    if (kp) std::memcpy(kp + 4 * (size_t)i, &e[i].z, 8);
  }
  return VSLAM_OK;
}
VS_API int vslam_get_point_ids(vslam_ctx* c, int s, int32_t cap, int32_t* n, int32_t* ids) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!n || cap < 0) return fail(c, VSLAM_ERR_INVALID, "vslam_get_point_ids: null count or negative capacity");
  if (!c->map.cap) return fail(c, VSLAM_ERR_STATE, "the landmark map is not enabled (vslam_enable_map)");
  StreamState st;
  HIP_TRY(c, d2h(c, &st, c->buf.st + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int32_t cnt = 0;
  HIP_TRY(c, d2h(c, &cnt, c->buf.n_points + s * 2 + st.cur, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!st.has_prev) cnt = 0;           // the point list vslam_get_points reports
  *n = cnt;
  if (cnt > cap) return fail(c, VSLAM_ERR_CAPACITY, "point id output capacity too small");
  HIP_TRY(c, d2h(c, ids, c->map.d.ids + ((size_t)st.cur * c->B + s) * c->cfg.MAXP, (size_t)cnt));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_get_track_result(vslam_ctx* c, int s, int32_t cap, int32_t* n_tracked, int32_t* out4, int32_t* n_lost, int32_t* lost) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!n_tracked || !n_lost) return fail(c, VSLAM_ERR_INVALID, "bad argument");
  StreamState st;
  HIP_TRY(c, d2h(c, &st, c->buf.st + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_tracked = st.n_trk; *n_lost = st.n_lost;
  if (st.n_trk > cap || st.n_lost > cap) return fail(c, VSLAM_ERR_CAPACITY, "track output capacity too small");
  HIP_TRY(c, d2h(c, out4, c->buf.trk + (size_t)s * c->cfg.MAXP * 4, (size_t)st.n_trk * 4));
  HIP_TRY(c, d2h(c, lost, c->buf.lost + (size_t)s * c->cfg.MAXP, (size_t)st.n_lost));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_get_aligner_result(vslam_ctx* c, int s, int32_t cap, int32_t* n, double* chi, uint8_t* inlier, double T[12], double H[36]) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!n) return fail(c, VSLAM_ERR_INVALID, "bad argument");
  StreamState st;
  HIP_TRY(c, d2h(c, &st, c->buf.st + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n = st.al_n;
  if (st.al_n > cap) return fail(c, VSLAM_ERR_CAPACITY, "aligner output capacity too small");
  HIP_TRY(c, d2h(c, chi, c->buf.al_chi + (size_t)s * c->cfg.MAXP, (size_t)st.al_n));
  HIP_TRY(c, d2h(c, inlier, c->buf.al_inl + (size_t)s * c->cfg.MAXP, (size_t)st.al_n));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (T) std::memcpy(T, st.al_T, sizeof(double) * 12);
  if (H) std::memcpy(H, st.al_H, sizeof(double) * 36);
  return VSLAM_OK;
}
VS_API int vslam_get_aligner_weights(vslam_ctx* c, int s, int32_t cap, int32_t* n, double* weight) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!n) return fail(c, VSLAM_ERR_INVALID, "bad argument");
  StreamState st;
  HIP_TRY(c, d2h(c, &st, c->buf.st + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n = st.al_wsize;
  if (st.al_wsize > cap) return fail(c, VSLAM_ERR_CAPACITY, "aligner weight output capacity too small");
  HIP_TRY(c, d2h(c, weight, c->buf.al_weight + (size_t)s * c->cfg.MAXP, (size_t)st.al_wsize));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_get_poses(vslam_ctx* c, int s, int32_t first, int32_t nf, double* out) {
  int rc = check_stream(c, s);
  if (rc) return rc;
  if (!out || first < 0 || nf < 0 || first + nf > VS_POSE_LOG) return fail(c, VSLAM_ERR_INVALID, "bad pose range");
  HIP_TRY(c, d2h(c, out, c->buf.pose_log + ((size_t)s * VS_POSE_LOG + first) * 12, (size_t)nf * 12));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_copy_poses_device(vslam_ctx* c, int32_t first, int32_t nf, double* dst) {
  if (!c || !dst || first < 0 || nf < 0 || first + nf > VS_POSE_LOG) return VSLAM_ERR_INVALID;
  sync_all(c);
  HIP_TRY(c, hipMemcpy2DAsync(dst, (size_t)nf * 12 * sizeof(double), c->buf.pose_log + (size_t)first * 12,
                              (size_t)VS_POSE_LOG * 12 * sizeof(double), (size_t)nf * 12 * sizeof(double), c->B,
                              hipMemcpyDeviceToDevice, c->stream));
  return VSLAM_OK;
}
VS_API int vslam_get_timers(vslam_ctx* c, double seconds[8]) {
  if (!c || !seconds) return VSLAM_ERR_INVALID;
  harvest_events(c);
  std::vector<StreamState> st(c->B);
  HIP_TRY(c, hipMemcpy(st.data(), c->buf.st, sizeof(StreamState) * c->B, hipMemcpyDeviceToHost));
  double ph[5] = {0, 0, 0, 0, 0};
  for (int s = 0; s < c->B; ++s) for (int k = 0; k < 5; ++k) ph[k] += (double)st[s].ticks[k] * 1e-8 / c->B;  // 100 MHz ticks
  seconds[0] = (c->kern_ms[0] + c->kern_ms[1]) * 1e-3;  // keypoint_detection: FAST/NMS + emission/controller
  seconds[1] = c->kern_ms[2] * 1e-3;                    // descriptor_extraction
  seconds[2] = ph[4];                                   // point_triangulation (compute())
  seconds[3] = c->kern_ms[3] * 1e-3 + ph[0];            // tracking: candidate search + resolution
  seconds[4] = ph[4];                                   // track_creation (tracker's timer around compute())
  seconds[5] = ph[1];                                   // pose_optimization
  seconds[6] = ph[3] + c->kern_ms[6] * 1e-3;            // landmark_optimization (in-kernel part + wide kernel)
  seconds[7] = ph[2] + c->kern_ms[5] * 1e-3;            // point_recovery
  return VSLAM_OK;
}
VS_API int vslam_get_kernel_times(vslam_ctx* c, double ms[8], int32_t launches[8]) {
  if (!c || !ms || !launches) return VSLAM_ERR_INVALID;
  harvest_events(c);
  for (int k = 0; k < 8; ++k) { ms[k] = c->kern_ms[k]; launches[k] = c->kern_n[k]; }
  return VSLAM_OK;
}
VS_API int vslam_enable_timers(vslam_ctx* c, int on) {
  if (!c) return VSLAM_ERR_INVALID;
  harvest_events(c);
  if (on && !c->timers) { for (int k = 0; k < 8; ++k) { c->kern_ms[k] = 0; c->kern_n[k] = 0; } }
  c->timers = on != 0;
  return VSLAM_OK;
}

// ---- stand-alone component entries (one piece of the pipeline on caller data) and their helpers ----
#include "host_entries.h"

// ---- stage entry points (the reference's plug-in virtuals; control flow stays with the caller) ----------
static StageIo stage_io(vslam_ctx* c, int report, int in_progress) {
  StageIo io;
  std::memset(&io, 0, sizeof io);
  if (c->B == 1 && c->pend.flags) {
    io.set_flags = c->pend.flags; io.status = c->pend.status; io.win = c->pend.win; io.tau = c->pend.tau;
    std::memcpy(io.prior, c->pend.prior, sizeof io.prior); std::memcpy(io.pose, c->pend.pose, sizeof io.pose);
    c->pend.flags = 0;
  }
  c->report_have = 0;
  if (report && c->report) {
    io.report = report; io.report_in_progress = in_progress; io.report_stream = 0; io.seq = ++c->report_seq; io.L = c->rl; io.out = c->report_dev;
    c->report_have = report; c->report_have_ip = in_progress; c->report_have_stream = 0; c->report_have_seq = io.seq;
  }
  return io;
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
static int launch_begin(vslam_ctx* c) {
  const StageIo io = stage_io(c, 0, 0);
  hipLaunchKernelGGL(k_begin, dim3(c->B), dim3(256), 0, c->stream, c->cfg, buf_set(c, c->last_set, c->q0_frm), io);
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
static int launch_stage(vslam_ctx* c, int stage, int arg, int report = 0, int in_progress = 0) {
  const StageIo io = stage_io(c, report, in_progress);
  hipLaunchKernelGGL(k_stage, dim3(c->B), dim3(VS_WG), 0, c->stream, c->cfg, buf_set(c, c->last_set, c->q0_frm), stage, arg, io);
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
VS_API int vslam_frame_begin(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, int on_device) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->sticky != VSLAM_OK) return c->sticky;
  HIP_TRY(c, hipSetDevice(c->device));
  c->img_override = c->B == 1 ? c->stream : nullptr;
  c->report_xy_seq = -1;
  c->lm_published = false;
  int rc = set_inputs(c, L, R, row_stride, image_stride, on_device != 0);
  if (rc == VSLAM_OK) rc = launch_image_pipeline(c);
  c->img_override = nullptr;
  if (rc != VSLAM_OK) return rc;
  rc = launch_begin(c);
  c->frame_begun = rc == VSLAM_OK;
  if (rc == VSLAM_OK && c->report) {
    // a caller that reads stage views wants the keypoints next (initialize() fills Frame::keypoints / descriptors): packed right
    // behind k_begin, no host round trip in between
    const int seq = ++c->report_seq;
    hipLaunchKernelGGL(k_report, dim3(32), dim3(256), 0, c->stream, c->cfg, buf_set(c, c->last_set), 0, (int)VS_REPORT_KEYPOINTS, 0, seq, c->rl, c->report_dev, c->report_done);
    HIP_TRY(c, hipGetLastError());
    c->report_have = VS_REPORT_KEYPOINTS; c->report_have_ip = 0; c->report_have_stream = 0; c->report_have_seq = seq;
  }
  return rc;
}
VS_API int vslam_frame_finish(vslam_ctx* c) {
  if (!c) return VSLAM_ERR_INVALID;
  if (!c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_frame_finish called before vslam_frame_begin");
  c->frame_begun = false;
  int rc = flush_pending(c);
  return rc == VSLAM_OK ? launch_frame(c) : rc;
}
#define NEED_FRAME(name) if (!c) return VSLAM_ERR_INVALID; if (!c->frame_begun) return fail(c, VSLAM_ERR_STATE, name " called before vslam_frame_begin")
VS_API int vslam_frame_restore(vslam_ctx* c) {
  // initialize(frame, false) only rebuilds the two feature stores; the device stores are rebuilt from the
  // keypoint arrays by every vslam_track call (kill / used flags are recomputed), so nothing to launch.
  NEED_FRAME("vslam_frame_restore");
  return VSLAM_OK;
}
VS_API int vslam_track(vslam_ctx* c, int by_appearance) {
  NEED_FRAME("vslam_track");
  { int rc = flush_pending(c); if (rc) return rc; }     // the candidate kernel reads prior / window / distance before the stage kernel runs
  hipLaunchKernelGGL(k_track_candidates, dim3(cand_blocks(c->B), c->B), dim3(256), 0, c->stream, c->cfg, buf_set(c, c->last_set, c->q0_frm), by_appearance ? 1 : 0);
  return launch_stage(c, VS_STAGE_TRACK, by_appearance ? 1 : 0, VS_REPORT_TRACK);
}
VS_API int vslam_align(vslam_ctx* c, int inverse_depth) { NEED_FRAME("vslam_align"); return launch_stage(c, VS_STAGE_ALIGN, inverse_depth, VS_REPORT_ALIGNER); }
VS_API int vslam_prune_recover(vslam_ctx* c) {
  NEED_FRAME("vslam_prune_recover");
  if (!c->cfg.c.enable_landmark_recovery) return launch_stage(c, VS_STAGE_PRUNE_RECOVER, 0, VS_REPORT_POINTS, 1);
  // with recovery: prune + projection | descriptors of the projected points, wide | append + report — the per-point patch reads of the
  // descriptors go through every CU's memory pipe instead of one (59 -> ~25 us for one stream)
  int rc = launch_stage(c, VS_STAGE_PRUNE_PROJECT, 1);
  if (rc != VSLAM_OK) return rc;
  hipLaunchKernelGGL(k_recover_brief, dim3(recover_blocks(c->B), c->B), dim3(256), 0, c->stream, c->cfg, buf_set(c, c->last_set, c->q0_frm));
  HIP_TRY(c, hipGetLastError());
  // one stream: the stage also publishes the frame's history, so that vslam_compute can run the landmark refinement beside the stereo stage
  // instead of in front of it
  const bool side = c->B == 1;
  rc = launch_stage(c, VS_STAGE_RECOVER_APPEND, side ? 3 : 1, VS_REPORT_POINTS, 1);
  c->lm_published = rc == VSLAM_OK && side;
  return rc;
}
VS_API int vslam_update_points(vslam_ctx* c) { NEED_FRAME("vslam_update_points"); c->lm_published = false; return launch_stage(c, VS_STAGE_UPDATE, 0); }
VS_API int vslam_stereo_new(vslam_ctx* c) {
  NEED_FRAME("vslam_stereo_new");
  c->frame_begun = false;  // compute() is the last call PoseTracker3D::compute makes on a frame
  int rc = launch_stage(c, VS_STAGE_STEREO, 0, VS_REPORT_POINTS, 0);
  return rc == VSLAM_OK ? frame_done(c) : rc;
}
VS_API int vslam_compute(vslam_ctx* c) {     // vslam_update_points + vslam_stereo_new in one launch
  NEED_FRAME("vslam_compute");
  c->frame_begun = false;
  if (c->lm_published) {
    // one stream, its history already published by vslam_prune_recover: the landmark refinement (lm_teams_body, the frame workgroup's refinement
    // spread over several workgroups) runs BESIDE the stereo stage in the same launch (k_stage_lm); the stage only counts the active landmarks.
    // The report — it carries the landmark update counts — is packed by the next launch on the queue.
    c->lm_published = false;
    const StageIo io = stage_io(c, 0, 0);
    hipLaunchKernelGGL(k_stage_lm, dim3(c->B * (1 + 16)), dim3(VS_WG), 0, c->stream, c->cfg, buf_set(c, c->last_set, c->q0_frm), (int)VS_STAGE_STEREO_COUNT, 0, io, c->B, 16);
    HIP_TRY(c, hipGetLastError());
    if (c->report) {
      const int seq = ++c->report_seq;
      hipLaunchKernelGGL(k_report, dim3(16), dim3(256), 0, c->stream, c->cfg, buf_set(c, c->last_set), 0, (int)VS_REPORT_POINTS, 0, seq, c->rl, c->report_dev, c->report_done);
      HIP_TRY(c, hipGetLastError());
      c->report_have = VS_REPORT_POINTS; c->report_have_ip = 0; c->report_have_stream = 0; c->report_have_seq = seq;
    }
    return frame_done(c);
  }
  int rc = launch_stage(c, VS_STAGE_COMPUTE, 0, VS_REPORT_POINTS, 0);
  return rc == VSLAM_OK ? frame_done(c) : rc;
}
// the setters are queued on the stream's frame queue, in order with the stage launches around them: no synchronisation
static int check_stream_index(vslam_ctx* c, int s) {
  if (!c) return VSLAM_ERR_INVALID;
  if (s < 0 || s >= c->B) return fail(c, VSLAM_ERR_INVALID, "stream index out of range");
  return VSLAM_OK;
}
VS_API int vslam_set_tracker_state(vslam_ctx* c, int s, int status, const double prior[12], int win, double tau) {
  int rc = check_stream_index(c, s);
  if (rc) return rc;
  if (!prior) return fail(c, VSLAM_ERR_INVALID, "null prior");
  if (c->B == 1) {      // rides with the next stage launch (StageIo)
    c->pend.flags |= 1; c->pend.status = status; c->pend.win = win; c->pend.tau = tau; std::memcpy(c->pend.prior, prior, sizeof c->pend.prior);
    return VSLAM_OK;
  }
  D12 p;
  std::memcpy(p.v, prior, sizeof p.v);
  hipLaunchKernelGGL(k_set_tracker_state, dim3(1), dim3(1), 0, c->stream, c->buf, s, status, win, tau, p);
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}
VS_API int vslam_set_pose(vslam_ctx* c, int s, const double pose[12]) {
  int rc = check_stream_index(c, s);
  if (rc) return rc;
  if (!pose) return fail(c, VSLAM_ERR_INVALID, "null pose");
  if (c->B == 1) { c->pend.flags |= 2; std::memcpy(c->pend.pose, pose, sizeof c->pend.pose); return VSLAM_OK; }
  D12 p;
  std::memcpy(p.v, pose, sizeof p.v);
  hipLaunchKernelGGL(k_set_pose, dim3(1), dim3(1), 0, c->stream, c->buf, s, p);
  HIP_TRY(c, hipGetLastError());
  return VSLAM_OK;
}


// ---- pinned host memory for the caller's images -------------------------------------------------------------------------------------
VS_API int vslam_host_alloc(void** out, size_t bytes) {
  if (!out || !bytes) return VSLAM_ERR_INVALID;
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, VSLAM_ERR_HIP, "vslam_host_alloc: hipHostMalloc failed"); }
  *out = p;
  return VSLAM_OK;
}
VS_API void vslam_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- stage views: one report kernel + one synchronisation of the stream's frame queue per stage (kernels_report.h) -------------
static uint32_t rl_take(uint32_t* off, size_t bytes) { const uint32_t o = *off; *off = (uint32_t)((o + bytes + 63) & ~(size_t)63); return o; }
static int report_ready(vslam_ctx* c) {
  if (c->report) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  ReportLayout& L = c->rl;
  uint32_t off = (uint32_t)((sizeof(ReportHeader) + 255) & ~(size_t)255);
  const size_t N = c->cfg.NMAX, P = c->cfg.MAXP;
  for (int d = 0; d < 2; ++d) { L.kp_xy[d] = rl_take(&off, N * 4); L.kp_score[d] = rl_take(&off, N); L.desc[d] = rl_take(&off, N * 32); }
  L.trk = rl_take(&off, P * 16); L.lost = rl_take(&off, P * 4);
  L.chi = rl_take(&off, P * 8); L.inl = rl_take(&off, P);
  L.p_kp = rl_take(&off, P * 8); L.p_meta = rl_take(&off, P * 24); L.p_cam = rl_take(&off, P * 24); L.p_desc = rl_take(&off, P * 64);
  L.total = off;
  void* h = nullptr;
  // coherent (fine-grained) on purpose: the GPU's stores go out over PCIe as they are issued and the completion flag's system-scope
  // release orders them for a host that polls it mid-kernel; with any other flag set and no coherence flag, HIP's default is a
  // NON-coherent mapping whose lines may sit in the GPU's L2 until the kernel ends
  HIP_TRY(c, hipHostMalloc(&h, L.total, hipHostMallocMapped | hipHostMallocCoherent));
  void* d = nullptr;
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipHostFree(h); return fail(c, VSLAM_ERR_HIP, "hipHostGetDevicePointer(report buffer)"); }
  std::memset(h, 0, L.total);
  if (dalloc(c, &c->report_done, 1) != hipSuccess || hipMemset(c->report_done, 0, sizeof(unsigned int)) != hipSuccess) { (void)hipHostFree(h); return fail(c, VSLAM_ERR_HIP, "report counter"); }
  c->report = (unsigned char*)h; c->report_dev = (unsigned char*)d;
  return VSLAM_OK;
}
// packs `what` of stream s and waits for it: everything queued on the stream's frame queue before (the image pipeline is ordered
// before it by the frame's event) has finished when this returns
static int report_run(vslam_ctx* c, int s, int what, int in_progress, const ReportHeader** hdr) {
  int rc = check_stream_index(c, s);
  if (rc) return rc;
  if (c->sticky != VSLAM_OK) return c->sticky;
  rc = report_ready(c);
  if (rc) return rc;
  int seq = c->report_have_seq;
  const bool folded = c->report_have == what && c->report_have_ip == in_progress && c->report_have_stream == s && !c->pend.flags;
  if (!folded) {      // the stage was launched before the report buffer existed, or something else ran since: pack it now
    rc = flush_pending(c);
    if (rc) return rc;
    seq = ++c->report_seq;
    const int blocks = what == VS_REPORT_KEYPOINTS ? 32 : (what == VS_REPORT_POINTS ? 16 : 4);
    hipLaunchKernelGGL(k_report, dim3(blocks), dim3(256), 0, c->stream, c->cfg, buf_set(c, c->last_set), s, what, in_progress, seq, c->rl, c->report_dev, c->report_done);
    HIP_TRY(c, hipGetLastError());
    c->report_have = what; c->report_have_ip = in_progress; c->report_have_stream = s; c->report_have_seq = seq;
  }
  // the report's completion flag (its seq, stored last with system-scope release) is polled in the pinned buffer: the caller's
  // thread sees the stage end a few microseconds after the kernel's last store instead of waiting for the runtime's own
  // completion path (~10-15 us per synchronisation, five per frame).  Bounded: after ~0.1 s without the flag the queue is
  // synchronised the ordinary way (an inactive stream never writes a report: that is the STATE error below)
  const ReportHeader* h = reinterpret_cast<const ReportHeader*>(c->report);
  bool seen = false;
  for (long spin = 0; spin < 4000000L; ++spin) {
    if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) == seq) { seen = true; break; }
    __builtin_ia32_pause();
  }
  if (!seen) HIP_TRY(c, hipStreamSynchronize(c->stream));
  *hdr = h;
  if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) != seq || h->what != what) return fail(c, VSLAM_ERR_STATE, "stage report is stale (the stream is inactive?)");
  if ((*hdr)->info.error_flags) c->err = "device buffer capacity exceeded (error_flags != 0)";
  return VSLAM_OK;
}
VS_API int vslam_view_keypoints(vslam_ctx* c, int s, vslam_keypoints_view* out);
// polls a report flag (bounded), falling back to an ordinary synchronisation of the queue
static int report_wait(vslam_ctx* c, const int32_t* flag, int seq) {
  for (long spin = 0; spin < 4000000L; ++spin) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return VSLAM_OK;
    __builtin_ia32_pause();
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
}
VS_API int vslam_view_keypoints_xy(vslam_ctx* c, int s, vslam_keypoints_view* out) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  int rc = check_stream_index(c, s);
  if (rc) return rc;
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (!c->report || s != 0 || c->report_xy_seq < 0 || !c->frame_begun) return vslam_view_keypoints(c, s, out);   // no early report in flight: the full one
  const ReportHeader* h = reinterpret_cast<const ReportHeader*>(c->report);
  rc = report_wait(c, &h->seq_xy, c->report_xy_seq);
  if (rc) return rc;
  if (__atomic_load_n(&h->seq_xy, __ATOMIC_ACQUIRE) != c->report_xy_seq) return fail(c, VSLAM_ERR_STATE, "early keypoint report is stale (the stream is inactive?)");
  for (int d = 0; d < 2; ++d) {
    out->n[d] = std::min(h->n_kp[d], c->cfg.NMAX);
    out->xy[d] = reinterpret_cast<const int16_t*>(c->report + c->rl.kp_xy[d]);
    out->score[d] = c->report + c->rl.kp_score[d];
    out->desc[d] = nullptr;                       // not there yet: vslam_view_keypoints
  }
  return VSLAM_OK;
}
VS_API int vslam_view_keypoints(vslam_ctx* c, int s, vslam_keypoints_view* out) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  const ReportHeader* h = nullptr;
  int rc = report_run(c, s, VS_REPORT_KEYPOINTS, 0, &h);
  if (rc) return rc;
  for (int d = 0; d < 2; ++d) {
    out->n[d] = std::min(h->n_kp[d], c->cfg.NMAX);
    out->xy[d] = reinterpret_cast<const int16_t*>(c->report + c->rl.kp_xy[d]);
    out->score[d] = c->report + c->rl.kp_score[d];
    out->desc[d] = c->report + c->rl.desc[d];
  }
  return VSLAM_OK;
}
VS_API int vslam_view_track(vslam_ctx* c, int s, vslam_track_view* out) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  const ReportHeader* h = nullptr;
  int rc = report_run(c, s, VS_REPORT_TRACK, 0, &h);
  if (rc) return rc;
  out->n_tracked = h->n_trk; out->n_lost = h->n_lost; out->n_tracked_landmarks = h->n_tracked_landmarks;
  out->tracked4 = reinterpret_cast<const int32_t*>(c->report + c->rl.trk);
  out->lost = reinterpret_cast<const int32_t*>(c->report + c->rl.lost);
  return VSLAM_OK;
}
VS_API int vslam_view_aligner(vslam_ctx* c, int s, vslam_aligner_view* out) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  const ReportHeader* h = nullptr;
  int rc = report_run(c, s, VS_REPORT_ALIGNER, 0, &h);
  if (rc) return rc;
  out->n = h->al_n; out->n_inliers = h->al_inliers; out->n_outliers = h->al_outliers; out->iterations = h->al_iterations;
  out->converged = h->al_converged; out->total_error = h->al_total_error;
  out->chi = reinterpret_cast<const double*>(c->report + c->rl.chi);
  out->inlier = c->report + c->rl.inl;
  std::memcpy(out->T, h->al_T, sizeof out->T);
  std::memcpy(out->H, h->al_H, sizeof out->H);
  return VSLAM_OK;
}
VS_API int vslam_view_points(vslam_ctx* c, int s, int in_progress, vslam_points_view* out) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  const ReportHeader* h = nullptr;
  int rc = report_run(c, s, VS_REPORT_POINTS, in_progress ? 1 : 0, &h);
  if (rc) return rc;
  out->n = h->n_points;
  out->kp = reinterpret_cast<const int16_t*>(c->report + c->rl.p_kp);
  out->meta = reinterpret_cast<const int32_t*>(c->report + c->rl.p_meta);
  out->cam = reinterpret_cast<const double*>(c->report + c->rl.p_cam);
  out->desc = in_progress ? c->report + c->rl.p_desc : nullptr;
  out->first_full = in_progress ? std::min(h->n_after_prune, h->n_points) : 0;
  out->info = h->info;
  // the generator's chronometers from the same report (no further copy): accumulated seconds like vslam_get_timers
  const double inv = 1e-8;
  out->seconds_tracking = (double)h->ticks[0] * inv; out->seconds_pose_optimization = (double)h->ticks[1] * inv;
  out->seconds_point_recovery = (double)h->ticks[2] * inv; out->seconds_landmark_optimization = (double)h->ticks[3] * inv;
  out->seconds_point_triangulation = (double)h->ticks[4] * inv;
  return VSLAM_OK;
}

// ---- RGB-D mode -----------------------------------------------------------------------------------------------------------------
// Two implementations behind the same entry points: the device-resident loop (csrc/rgbd_device.h + kernels_rgbd.h; the default) and the
// host-driven loop over the library's own stand-alone entry points (csrc/rgbd_tracker.h; VSLAM_RGBD_HOST=1), kept as the cross-check.
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
static int rgbd_create(const vslam_config* cfg, const vslam_depth_params* p, int device, int n_streams, vslam_rgbd** out);
VS_API int vslam_rgbd_wait(vslam_rgbd* r);
VS_API int vslam_rgbd_get_frame_info(vslam_rgbd* r, vslam_frame_info* out, int32_t* n_temporary);
VS_API int vslam_rgbd_get_points(vslam_rgbd* r, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc);
VS_API int vslam_rgbd_create(const vslam_config* cfg, const vslam_depth_params* p, int device, vslam_rgbd** out) { return rgbd_create(cfg, p, device, 1, out); }
VS_API int vslam_rgbd_create_batch(const vslam_config* cfg, const vslam_depth_params* p, int device, int32_t n_streams, vslam_rgbd** out) {
  return rgbd_create(cfg, p, device, n_streams, out);
}
static int rgbd_create(const vslam_config* cfg, const vslam_depth_params* p, int device, int n_streams, vslam_rgbd** out) {
  if (!cfg || !p || !out) { g_rgbd_error = "vslam_rgbd_create: null argument"; return VSLAM_ERR_INVALID; }
  vslam_rgbd* r = new vslam_rgbd;
  if (const char* e = std::getenv("VSLAM_RGBD_HOST")) r->on_host = std::atoi(e) != 0;
  // detector_type ORB (no shipped configuration): the OrbDetector is a host-driven sequence of per-level kernels (vslam_orb_detect) and several
  // features can share a pixel — the device-resident loop's image pipeline is FAST's; the host-driven loop serves this mode
  if (p->detector_type == VSLAM_DETECTOR_ORB) r->on_host = true;
  else if (p->detector_type != VSLAM_DETECTOR_FAST) { g_rgbd_error = "vslam_rgbd_create: unknown detector_type"; delete r; return VSLAM_ERR_INVALID; }
  if (r->on_host && n_streams != 1) { g_rgbd_error = "vslam_rgbd_create_batch: the host-driven loop (VSLAM_RGBD_HOST=1, detector_type ORB) tracks one sequence per object"; delete r; return VSLAM_ERR_INVALID; }
  const int rc = r->on_host ? r->t.create(*cfg, *p, device) : r->d.create(*cfg, *p, device, n_streams);
  if (rc != VSLAM_OK) { g_rgbd_error = r->err(); delete r; return rc; }
  *out = r;
  return VSLAM_OK;
}
VS_API void vslam_rgbd_destroy(vslam_rgbd* r) { delete r; }
VS_API int vslam_rgbd_reset(vslam_rgbd* r) {
  if (!r) return VSLAM_ERR_INVALID;
  if (r->on_host) { r->t.reset(); return VSLAM_OK; }
  return r->d.reset();
}
VS_API int vslam_rgbd_process_host(vslam_rgbd* r, const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride) {
  if (!r) return VSLAM_ERR_INVALID;
  if (!left || !depth) { r->err() = "called with empty frame"; return VSLAM_ERR_INVALID; }   // depth_framepoint_generator.cpp:48-50
  const int cols = r->on_host ? r->t.cfg.cols : r->d.cfg.cols;
  if (lstride < cols || dstride < cols) { r->err() = "row stride smaller than image width"; return VSLAM_ERR_INVALID; }
  return r->on_host ? r->t.process(left, lstride, depth, dstride) : r->d.process(left, lstride, depth, dstride);
}
VS_API int vslam_rgbd_submit_host(vslam_rgbd* r, const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride) {
  if (!r) return VSLAM_ERR_INVALID;
  if (!left || !depth) { r->err() = "called with empty frame"; return VSLAM_ERR_INVALID; }
  const int cols = r->on_host ? r->t.cfg.cols : r->d.cfg.cols;
  if (lstride < cols || dstride < cols) { r->err() = "row stride smaller than image width"; return VSLAM_ERR_INVALID; }
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
  if (!left || !depth) { r->d.err = "called with empty frame"; return VSLAM_ERR_INVALID; }
  if (lstride < r->d.cfg.cols || dstride < r->d.cfg.cols) { r->d.err = "row stride smaller than image width"; return VSLAM_ERR_INVALID; }
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
  if (!left || !depth) { r->d.err = "called with empty frame"; return VSLAM_ERR_INVALID; }
  if (lstride < r->d.cfg.cols || dstride < r->d.cfg.cols) { r->d.err = "row stride smaller than image width"; return VSLAM_ERR_INVALID; }
  return r->d.submit(left, lstride, depth, dstride, left_stream_stride, depth_stream_stride, true);
}
VS_API int vslam_rgbd_get_frame_info_stream(vslam_rgbd* r, int32_t stream, vslam_frame_info* out, int32_t* n_temporary) {
  if (!r || !out) return VSLAM_ERR_INVALID;
  if (r->on_host) return stream == 0 ? vslam_rgbd_get_frame_info(r, out, n_temporary) : VSLAM_ERR_INVALID;
  if (stream < 0 || stream >= r->d.B) { r->d.err = "stream index out of range"; return VSLAM_ERR_INVALID; }
  if (r->d.frame_in_flight()) { r->d.err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
  *out = r->d.hosts[stream].info;
  if (n_temporary) *n_temporary = r->d.hosts[stream].n_temporary;
  return VSLAM_OK;
}
VS_API int vslam_rgbd_get_points_stream(vslam_rgbd* r, int32_t stream, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc) {
  if (!r || !n) return VSLAM_ERR_INVALID;
  if (r->on_host) return stream == 0 ? vslam_rgbd_get_points(r, cap, n, xy, cam, meta4, desc) : VSLAM_ERR_INVALID;
  return r->d.get_points(stream, cap, n, xy, cam, meta4, desc);
}
VS_API int vslam_rgbd_get_frame_info(vslam_rgbd* r, vslam_frame_info* out, int32_t* n_temporary) {
  if (!r || !out) return VSLAM_ERR_INVALID;
  if (r->on_host) { *out = r->t.info; if (n_temporary) *n_temporary = r->t.n_temporary; return VSLAM_OK; }
  if (r->d.frame_in_flight()) { r->d.err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
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
// ---- the RGB-D landmark map and observation log (kernels_rgbd_map.h): the device-resident loop only ----
static int rgbd_map_host_refusal(vslam_rgbd* r, const char* what) {
  r->t.err = std::string(what) + ": the host-driven loop (VSLAM_RGBD_HOST=1, detector_type ORB) keeps no landmark map or observation log; use the device-resident loop";
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

// ---- pose all-gather on RCCL (loaded lazily: the single-GPU path has no dependency on librccl.so) ----------------------------
#include <dlfcn.h>
namespace {
struct RcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, struct Id128, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
struct Id128 { char internal[VSLAM_COMM_ID_BYTES]; };   // ncclUniqueId: passed BY VALUE to ncclCommInitRank
RcclApi g_rccl;
thread_local std::string g_comm_error;
int comm_fail(int code, const std::string& msg) { g_comm_error = msg; return code; }
int rccl_load() {
  if (g_rccl.lib) return VSLAM_OK;
  void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return comm_fail(VSLAM_ERR_NO_DEVICE, std::string("librccl.so not found: ") + dlerror());
  RcclApi a;
  a.lib = h;
  a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
  a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
  a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(h, "ncclAllGather"));
  a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
  a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
  if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) return comm_fail(VSLAM_ERR_NO_DEVICE, "librccl.so lacks an expected symbol");
  g_rccl = a;
  return VSLAM_OK;
}
}  // namespace
struct vslam_comm { void* comm = nullptr; int rank = 0, nranks = 1, device = 0; };
VS_API const char* vslam_comm_last_error(void) { return g_comm_error.c_str(); }
VS_API int vslam_comm_available(int device) {
  int rc = rccl_load();
  if (rc != VSLAM_OK) return rc;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return comm_fail(VSLAM_ERR_NO_DEVICE, "vslam_comm_available: no such HIP device");
  return VSLAM_OK;
}
VS_API int vslam_comm_unique_id(uint8_t id[VSLAM_COMM_ID_BYTES]) {
  if (!id) return comm_fail(VSLAM_ERR_INVALID, "null id");
  int rc = rccl_load();
  if (rc != VSLAM_OK) return rc;
  Id128 u;
  const int r = g_rccl.GetUniqueId(&u);
  if (r != 0) return comm_fail(VSLAM_ERR_HIP, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
  std::memcpy(id, u.internal, VSLAM_COMM_ID_BYTES);
  return VSLAM_OK;
}
VS_API int vslam_comm_init(int rank, int nranks, const uint8_t id[VSLAM_COMM_ID_BYTES], int device, vslam_comm** out) {
  if (!out || !id || nranks < 1 || rank < 0 || rank >= nranks) return comm_fail(VSLAM_ERR_INVALID, "vslam_comm_init: bad argument");
  int rc = rccl_load();
  if (rc != VSLAM_OK) return rc;
  if (hipSetDevice(device) != hipSuccess) return comm_fail(VSLAM_ERR_NO_DEVICE, "vslam_comm_init: hipSetDevice failed");
  Id128 u;
  std::memcpy(u.internal, id, VSLAM_COMM_ID_BYTES);
  vslam_comm* c = new vslam_comm;
  c->rank = rank; c->nranks = nranks; c->device = device;
  const int r = g_rccl.CommInitRank(&c->comm, nranks, u, rank);
  if (r != 0) { delete c; return comm_fail(VSLAM_ERR_HIP, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r)); }
  *out = c;
  return VSLAM_OK;
}
VS_API int vslam_allgather_poses(vslam_comm* c, const double* send, double* recv, size_t count, void* stream) {
  if (!c || !send || !recv) return comm_fail(VSLAM_ERR_INVALID, "vslam_allgather_poses: bad argument");
  if (count == 0) return VSLAM_OK;
  if (hipSetDevice(c->device) != hipSuccess) return comm_fail(VSLAM_ERR_NO_DEVICE, "hipSetDevice failed");
  const int r = g_rccl.AllGather(send, recv, count, /*ncclDouble*/ 8, c->comm, (hipStream_t)stream);
  if (r != 0) return comm_fail(VSLAM_ERR_HIP, std::string("ncclAllGather: ") + g_rccl.GetErrorString(r));
  return VSLAM_OK;
}
VS_API void vslam_comm_destroy(vslam_comm* c) {
  if (!c) return;
  if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
  delete c;
}

// profiling aid (not part of the ABI): mean per-stream ticks of the fine-grained phase stamps, in microseconds
VS_API int vslam_debug_ticks(vslam_ctx* c, double us[12]) {
  if (!c || !us) return VSLAM_ERR_INVALID;
  harvest_events(c);
  std::vector<StreamState> st(c->B);
  HIP_TRY(c, hipMemcpy(st.data(), c->buf.st, sizeof(StreamState) * c->B, hipMemcpyDeviceToHost));
  for (int k = 0; k < 12; ++k) { double a = 0; for (int s = 0; s < c->B; ++s) a += (double)st[s].dbg[k]; us[k] = a * 1e-2 / c->B; }
  return VSLAM_OK;
}
// profiling aid (not part of the ABI): per stream, the 5 chronometer tick counters followed by the 12 phase stamps
// (cumulative, 100 MHz ticks)
VS_API int vslam_debug_stream_ticks(vslam_ctx* c, unsigned long long* out /* [B][17] */) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  std::vector<StreamState> st(c->B);
  HIP_TRY(c, hipMemcpy(st.data(), c->buf.st, sizeof(StreamState) * c->B, hipMemcpyDeviceToHost));
  for (int s = 0; s < c->B; ++s) {
    for (int k = 0; k < 5; ++k) out[17 * s + k] = st[s].ticks[k];
    for (int k = 0; k < 12; ++k) out[17 * s + 5 + k] = st[s].dbg[k];
  }
  return VSLAM_OK;
}
