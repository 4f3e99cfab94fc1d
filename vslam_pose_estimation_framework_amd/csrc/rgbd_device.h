// rgbd_device.h — host side of the device-resident RGB-D loop (kernels_rgbd.h): buffers, the per-frame launch sequence on one HIP stream,
// one small read-back per frame.  Included by host_rgbd.h after the context code (it uses create_internal / buf_set / fail of host_ctx.h
// and the input stages of host_prestage.h).
//
// A frame is: two host-to-device copies (image, depth), ~17 kernel launches on two streams (the space map runs beside the image pipeline), one 1.2 KB device-to-host copy, one stream synchronisation.
// A context tracks n_streams independent sequences side by side (vslam_rgbd_create_batch): the same ~17 launches serve all of them — one
// workgroup per sequence in the single-workgroup kernels, a grid dimension in the wide ones —, a step takes the time of its slowest sequence.  When
// the registration asks for another attempt (RgbdState::done still 0 after the tail skipped itself: pose_tracker_3d.cpp:333-418, a lost
// track), the block image pipeline .. aligner .. tail is enqueued again, at most twice.
// detector_type ORB (kernels_rgbd_orb.h): the image pipeline of an attempt is enqueue_orb_detect instead — the OrbDetector of every region on
// pyramids of the region's view, the extractor on the whole image, k_orbd_install — and the rest of the frame is the same launches.
#pragma once
#include "kernels_rgbd.h"
#include "kernels_rgbd_map.h"
#include "kernels_undistort.h"
#include "kernels_bilateral.h"
#include "kernels_rgbd_orb.h"

namespace vs_rgbd {

class DeviceTracker {
public:
  vslam_ctx* ic = nullptr;       // inner context: image pipeline buffers, aligner SoA, detector thresholds (one stream per sequence)
  vslam_config cfg;
  vslam_depth_params p;
  std::string err;
  int B = 1;                     // sequences tracked side by side
  std::vector<RgbdState> hosts;  // last state block of every sequence
  RgbdState host;                // == hosts[0] (the one-sequence entry points)
  bool failed = false;
  std::string failed_why;

  ~DeviceTracker() { release(); }
  // detector_type ORB on this loop: every region of the grid has the size of the first (grids of up to two rows and two columns: all shipped
  // RGB-D configurations)
  static bool orb_grid_supported(const vslam_config& cfg) { return cfg.det_rows <= 2 && cfg.det_cols <= 2; }

  int create(const vslam_config& c, const vslam_depth_params& dp, int device, int n_streams = 1) {
    cfg = c; p = dp; B = n_streams;
    if (B < 1 || B > 1024) { err = "RGB-D mode: 1 .. 1024 sequences per context"; return VSLAM_ERR_INVALID; }
    if (cfg.det_rows < 1 || cfg.det_cols < 1 || cfg.det_rows * cfg.det_cols > VSLAM_MAX_REGIONS) { err = "RGB-D mode: bad detector grid"; return VSLAM_ERR_INVALID; }
    if (p.rows != cfg.rows || p.cols != cfg.cols) { err = "RGB-D mode: depth parameters and configuration disagree on the image size"; return VSLAM_ERR_INVALID; }
    if (cfg.max_points > 65535) { err = "RGB-D mode: max_points above 65535 (16-bit trail indices)"; return VSLAM_ERR_INVALID; }
    vslam_config in = cfg;
    in.descriptor_type = p.descriptor_type;      // the extractor initialize() uses (depth_framepoint_generator.cpp:24-44 -> computeDescriptors)
    in.max_history_frames = 2;                    // the stereo tracker's history ring is not used in this mode
    int rc = create_internal(&in, device, B, &ic);
    if (rc != VSLAM_OK) { err = vslam_last_error(nullptr); return rc; }
    q = ic->stream_img;
    ic->cfg.mono = 1;                             // the tile kernels run ONE image per sequence (grid z = sequences); k_emit's one-image controller
    const size_t MAXP = ic->cfg.MAXP, NMAX = ic->cfg.NMAX, npx = (size_t)p.rows * p.cols, nB = (size_t)B;
    if (const char* e = std::getenv("VSLAM_RGBD_WG")) { const int v = std::atoi(e); if (v == 256 || v == 512 || v == 1024) wg1 = v; }
    H = std::max(4, std::min(cfg.max_history_frames, 512));   // measurements of a track the landmark refinement can address
    TR = H - 2;
    const int rows_bin = p.enable_keypoint_binning ? p.rows / std::max(p.bin_size_pixels, 1) + 1 : 0, cols_bin = p.enable_keypoint_binning ? p.cols / std::max(p.bin_size_pixels, 1) + 1 : 0;
    const size_t nbins = (size_t)(rows_bin + 1) * (cols_bin + 1);
    std::memset(&rb, 0, sizeof rb);
    rb.p = p; rb.TR = TR; rb.H = H;
    rb.MAXP = (int32_t)MAXP; rb.NMAX = (int32_t)NMAX; rb.npx = (int32_t)npx; rb.nbins = (int32_t)nbins; rb.n_streams = B;
    hipError_t e = hipSuccess;
    auto A = [&](auto** ptr, size_t count) { if (e == hipSuccess) e = dalloc(ic, ptr, count * nB); };      // n_streams slices of the per-sequence size
    A(&rb.st, 1);
    for (RgbdList* l : {&rb.fl[0], &rb.fl[1], &rb.tmp}) {
      A(&l->xy, MAXP * 2); A(&l->desc, MAXP * 32); A(&l->cam, MAXP * 3); A(&l->prev, MAXP); A(&l->tlen, MAXP); A(&l->flags, MAXP);
      A(&l->lmw, MAXP * 3); A(&l->lmu, MAXP); A(&l->lmm, MAXP);
      if (l != &rb.tmp) A(&l->trail, MAXP * (size_t)TR);
    }
    A(&rb.order, NMAX); A(&rb.matched, NMAX);
    rb.ncsr = (int32_t)((size_t)ic->cfg.c.rows * (ic->cfg.CW + 1));
    A(&rb.a_kxy, NMAX * 2); A(&rb.a_desc, NMAX * 32); A(&rb.a_score, NMAX); A(&rb.a_rowcell, (size_t)rb.ncsr); A(&rb.a_order, NMAX); A(&rb.a_vis, NMAX);
    A(&rb.t_kxy, NMAX * 2); A(&rb.t_desc, NMAX * 32); A(&rb.t_score, NMAX); A(&rb.t_order, NMAX); A(&rb.m_rank, NMAX * 2); A(&rb.fvis, NMAX);
    A(&d_depth, npx); A(&rb.dkey, npx); A(&rb.dlast, npx); A(&rb.space, npx * 3); A(&rb.row_map, npx); A(&rb.col_map, npx);
    A(&rb.hold, NMAX * 2); A(&rb.pick, MAXP); A(&rb.cand, MAXP * (VS_DT_K + 1)); A(&rb.out2, MAXP * 2); A(&rb.xyz, MAXP * 3); A(&rb.temp2, MAXP * 2); A(&rb.lost_raw, MAXP);
    A(&rb.lost, MAXP); A(&rb.lost_has, MAXP); A(&rb.lost_lm, MAXP * 3); A(&rb.lost_desc, MAXP * 32);
    A(&rb.rbxy, MAXP * 2); A(&rb.rkxy, MAXP * 2); A(&rb.rcell, MAXP); A(&rb.rkeep, MAXP); A(&rb.rdesc, MAXP * 32); A(&rb.ridx, MAXP); A(&rb.rxy, MAXP * 2);
    A(&rb.rrdesc, MAXP * 32); A(&rb.rxyz, MAXP * 3);
    A(&rb.rcF, NMAX * 2); A(&rb.remf, NMAX); A(&rb.rcT, MAXP * 2); A(&rb.bins, nbins); A(&rb.cls, NMAX);
    A(&rb.new_feat, NMAX); A(&rb.new_xyz, NMAX * 3); A(&rb.temp_feat, NMAX); A(&rb.temp_xyz, NMAX * 3);
    A(&rb.weights, MAXP); A(&rb.cross, 1); A(&rb.guess_in, 12);
    A(&rb.h_cam, (size_t)H * MAXP * 4); A(&rb.h_pose, (size_t)H * 24); A(&rb.pose_log, (size_t)VS_POSE_LOG * 12);
    if (e == hipSuccess) e = hipHostMalloc((void**)&pinned, sizeof(RgbdState) * nB, hipHostMallocDefault);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&q2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_depth, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming);
    if (const char* g = std::getenv("VSLAM_RGBD_GRAPH")) use_graph = std::atoi(g) != 0;
    if (e != hipSuccess) { err = std::string("RGB-D mode: ") + hipGetErrorString(e); release(); return VSLAM_ERR_HIP; }
    rb.depth = d_depth;
    if (p.detector_type == VSLAM_DETECTOR_ORB) { rc = orb_create(); if (rc != VSLAM_OK) { release(); return rc; } }
    {   // the premise of k_depth_direct, as kernels_depth.h depth_source tests it
      const double* Ki = p.K_right_inverse; const double* K = p.K_left; const double* T = p.right_to_left;
      depth_plain = Ki[1] == 0 && Ki[3] == 0 && Ki[6] == 0 && Ki[7] == 0 && Ki[8] == 1 && K[1] == 0 && K[3] == 0 && K[6] == 0 && K[7] == 0 && K[8] == 1 &&
                    T[0] == 1 && T[1] == 0 && T[2] == 0 && T[3] == 0 && T[4] == 0 && T[5] == 1 && T[6] == 0 && T[7] == 0 && T[8] == 0 && T[9] == 0 && T[10] == 1 && T[11] == 0;
      if (const char* e2 = std::getenv("VSLAM_RGBD_DEPTH_DIRECT")) depth_plain = depth_plain && std::atoi(e2) != 0;
      if (const char* e3 = std::getenv("VSLAM_RGBD_DEPTH_FORCE_CROSS")) force_cross = std::atoi(e3) != 0;
    }
    hosts.resize(B);
    return reset();
  }

  int reset() {
    if (!ic) return VSLAM_ERR_STATE;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    if (q2) (void)hipStreamSynchronize(q2);
    int rc = init_state(ic);                                                 // detector thresholds back to the minimum (FastDetector of a fresh generator)
    if (rc != VSLAM_OK) { err = ic->err; return rc; }
    RgbdState s;
    std::memset(&s, 0, sizeof s);
    s.status = VSLAM_LOCALIZING;
    s.win = cfg.maximum_projection_tracking_distance_pixels;
    s.tau_track = cfg.minimum_descriptor_distance_tracking;
    tf_identity(s.prior); tf_identity(s.world); tf_identity(s.guess_prev);
    s.motion_model = motion_model; s.dead_reckoning_limit = dead_reckoning_limit;      // the model survives a reset, the guesses do not
    for (int i = 0; i < B; ++i) hosts[i] = s;
    host = s;
    hipError_t e = hipMemcpy(rb.st, hosts.data(), sizeof(RgbdState) * (size_t)B, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      std::vector<double> id((size_t)B * 12);
      for (int i = 0; i < B; ++i) tf_identity(&id[(size_t)i * 12]);
      e = hipMemcpy(rb.guess_in, id.data(), id.size() * sizeof(double), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    {   // the space maps' z-buffers: initialised here, every frame's k_depth_write puts them back
      const size_t npx = (size_t)p.rows * p.cols;
      const float f0 = (float)p.maximum_depth_meters;
      uint32_t f0_bits;
      std::memcpy(&f0_bits, &f0, 4);
      hipLaunchKernelGGL(k_depth_init, dim3((unsigned)((npx + 255) / 256), B), dim3(256), 0, q, (int)npx, f0_bits, rb.dkey, rb.dlast);
      (void)hipMemsetAsync(rb.cross, 0, sizeof(int32_t) * (size_t)B, q);
      if (hipStreamSynchronize(q) != hipSuccess) { err = "RGB-D reset: space-map buffers"; return VSLAM_ERR_HIP; }
    }
    failed = false; failed_why.clear(); pending = false;
    und.have_frame = false;                                                  // the maps stay (like the rig of a rectifying context)
    eq.have_frame = false;                                                   // and so does the equalisation switch
    col.have_frame = false;                                                  // and the colour format
    ds.have_frame = false;                                                   // and the downscale
    sm.have_frame = false;                                                   // and the smoothing
    bl.have_frame = false;                                                   // and the depth image's bilateral filter
    dmask.have_frame = false;                                                // and the detection mask, with the maps' validity mask
    dmask.fm_pending = false; dmask.fm_frame = false; dmask.fm_have = false;  // frame masks that waited for a frame belong to the sequence that ended
    if (mp.cap && map_clear() != hipSuccess) { err = "RGB-D reset: landmark map"; return VSLAM_ERR_HIP; }     // map and log start over, still enabled
    return VSLAM_OK;
  }

  // ---- motion models (kernels_motion.h): the model lives in every sequence's state block, the guesses in rb.guess_in, both read
  // by k_rgbd_begin inside the frame's (possibly captured) launch sequence ----
  int motion_model = VSLAM_MOTION_CONSTANT_VELOCITY, dead_reckoning_limit = 0;
  int set_motion_model(int model, int32_t limit) {
    if (model < VSLAM_MOTION_CONSTANT_VELOCITY || model > VSLAM_MOTION_CAMERA_ODOMETRY) { err = "vslam_rgbd_set_motion_model: unknown motion model"; return VSLAM_ERR_INVALID; }
    if (limit < 0) { err = "vslam_rgbd_set_motion_model: negative dead_reckoning_limit"; return VSLAM_ERR_INVALID; }
    if (limit > 0 && model != VSLAM_MOTION_CAMERA_ODOMETRY) { err = "vslam_rgbd_set_motion_model: dead_reckoning_limit needs VSLAM_MOTION_CAMERA_ODOMETRY"; return VSLAM_ERR_INVALID; }
    if (pending) { err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    motion_model = model; dead_reckoning_limit = limit;
    hipLaunchKernelGGL(k_rgbd_set_motion_model, dim3((B + 63) / 64), dim3(64), 0, q, rb, model, (int)limit);
    if (hipGetLastError() != hipSuccess) { err = "vslam_rgbd_set_motion_model: launch failed"; return VSLAM_ERR_HIP; }
    return VSLAM_OK;
  }
  // T: one sequence's guess (stream >= 0) or all of them (stream < 0, [B][12]); on_device: read on the frame's queue, no host synchronisation
  int set_pose_guess(int stream, const double* T, bool on_device) {
    if (!T) { err = "vslam_rgbd_set_pose_guess: null pose"; return VSLAM_ERR_INVALID; }
    if (stream >= B) { err = "stream index out of range"; return VSLAM_ERR_INVALID; }
    if (pending) { err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    double* dst = rb.guess_in + (stream < 0 ? 0 : (size_t)stream * 12);
    const size_t bytes = (stream < 0 ? (size_t)B : 1) * 12 * sizeof(double);
    // no frame is in flight: the queue holds at most the copy of a device array set before; the host form waits for it, so that whichever
    // was set last holds, and its blocking copy is then in order with the next frame's kernels
    hipError_t e = on_device ? hipMemcpyAsync(dst, T, bytes, hipMemcpyDeviceToDevice, q) : hipStreamSynchronize(q);
    if (e == hipSuccess && !on_device) e = hipMemcpy(dst, T, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { err = std::string("vslam_rgbd_set_pose_guess: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    return VSLAM_OK;
  }

  // ---- the landmark map and the observation log (kernels_rgbd_map.h): opt-in, their own allocations, nothing launched while cap == 0 ----
  int enable_map(int32_t cap) {
    if (cap < 0) { err = "vslam_rgbd_enable_map: negative capacity"; return VSLAM_ERR_INVALID; }
    if (pending) { err = "vslam_rgbd_enable_map: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    map_free();                                     // also the log: its ids are the map's
    drop_graph();                                   // a captured launch sequence holds the old store (or none)
    if (cap == 0) return VSLAM_OK;
    const size_t nB = (size_t)B, n = nB * (size_t)cap;
    RgbdMap d{};
    d.cap = cap; d.B = B;
    hipError_t e = map_mem.alloc(&d.rows, n * 4);
    if (e == hipSuccess) e = map_mem.alloc(&d.first, n);
    if (e == hipSuccess) e = map_mem.alloc(&d.count, nB);
    if (e == hipSuccess) e = map_mem.alloc(&d.committed, nB);
    if (e == hipSuccess) e = map_mem.alloc(&d.ids, 2 * nB * (size_t)rb.MAXP);
    if (e == hipSuccess) { mp = d; e = map_clear(); }
    if (e != hipSuccess) { map_free(); err = std::string("vslam_rgbd_enable_map: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    return VSLAM_OK;
  }
  int enable_observations(int32_t cap) {
    if (cap < 0) { err = "vslam_rgbd_enable_observations: negative capacity"; return VSLAM_ERR_INVALID; }
    if (pending) { err = "vslam_rgbd_enable_observations: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (!mp.cap) { err = "vslam_rgbd_enable_observations needs the landmark map (vslam_rgbd_enable_map): ids come from it"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    obs_free();
    drop_graph();
    if (cap == 0) return VSLAM_OK;
    const size_t nB = (size_t)B;
    hipError_t e = obs_mem.alloc_fill(&mp.log, nB * (size_t)cap * 3, 0, q);
    if (e == hipSuccess) e = obs_mem.alloc_fill(&mp.ocount, nB, 0, q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e != hipSuccess) { obs_free(); err = std::string("vslam_rgbd_enable_observations: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    mp.ocap = cap;
    return VSLAM_OK;
  }
  // the map's colours (kernels_map_color.h): [B][cap] words (r, g, b, 0) and the kernel's per-sequence mark; they need the map and a colour
  // format, and leave with either
  int enable_map_colors(int on) {
    if (pending) { err = "vslam_rgbd_enable_map_colors: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (on && !mp.cap) { err = "vslam_rgbd_enable_map_colors needs the landmark map (vslam_rgbd_enable_map): colours are indexed by its ids"; return VSLAM_ERR_STATE; }
    if (on && !col.format) { err = "vslam_rgbd_enable_map_colors needs colour input (vslam_rgbd_set_color_input)"; return VSLAM_ERR_STATE; }
    if ((on != 0) == (mc.rgb != nullptr)) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    mapcol_free();
    drop_graph();                                   // a captured launch sequence holds the kernel (or lacks it)
    if (!on) return VSLAM_OK;
    RgbdMapColor d{};
    hipError_t e = mapcol_mem.alloc_fill(&d.rgb, (size_t)B * (size_t)mp.cap, 0, q);      // (0, 0, 0) until an entry's next update
    if (e == hipSuccess) e = mapcol_mem.alloc(&d.colored, (size_t)B);
    // the frames so far are not coloured: the mark starts at every sequence's frame count, as the commit's does after its frame
    std::vector<int32_t> fc((size_t)B);
    for (int s = 0; s < B; ++s) fc[s] = hosts[s].frame_count;
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    if (e == hipSuccess) e = hipMemcpy(d.colored, fc.data(), fc.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { mapcol_free(); err = std::string("vslam_rgbd_enable_map_colors: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    mc = d;
    return VSLAM_OK;
  }
  int get_map_colors(int stream, int32_t first_id, int32_t cap, int32_t* n, uint8_t* rgb) {
    if (!n || first_id < 0 || cap < 0) { err = "vslam_rgbd_get_map_colors: null count, negative first id or capacity"; return VSLAM_ERR_INVALID; }
    int32_t size = 0;
    const int rc = map_ready(stream, false, &size);
    if (rc) return rc;
    if (!mc.rgb) { err = "the map's colours are not enabled (vslam_rgbd_enable_map_colors)"; return VSLAM_ERR_STATE; }
    const int32_t cnt = std::max(0, std::min(cap, size - first_id));
    *n = cnt;
    if (!cnt || !rgb) return VSLAM_OK;
    std::vector<uint32_t> w((size_t)cnt);
    const hipError_t e = hipMemcpy(w.data(), mc.rgb + (size_t)stream * mp.cap + (size_t)first_id, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    for (int32_t i = 0; i < cnt; ++i) { rgb[3 * i] = (uint8_t)w[i]; rgb[3 * i + 1] = (uint8_t)(w[i] >> 8); rgb[3 * i + 2] = (uint8_t)(w[i] >> 16); }
    return VSLAM_OK;
  }
  // what every getter below checks first; *size: entries of the store the call reads
  int map_ready(int stream, bool log, int32_t* size) {
    if (int rc = readable(stream)) return rc;
    if (!mp.cap) { err = "the landmark map is not enabled (vslam_rgbd_enable_map)"; return VSLAM_ERR_STATE; }
    if (log && !mp.ocap) { err = "the observation log is not enabled (vslam_rgbd_enable_observations)"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    if (size) {
      const hipError_t e = hipMemcpy(size, (log ? mp.ocount : mp.count) + stream, sizeof(int32_t), hipMemcpyDeviceToHost);
      if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    }
    return VSLAM_OK;
  }
  int get_map(int stream, int32_t first_id, int32_t cap, int32_t* n, double* xyz, int32_t* info3, uint8_t* desc) {
    if (!n || first_id < 0 || cap < 0) { err = "vslam_rgbd_get_map: null count, negative first id or capacity"; return VSLAM_ERR_INVALID; }
    int32_t size = 0;
    const int rc = map_ready(stream, false, &size);
    if (rc) return rc;
    const int32_t cnt = std::max(0, std::min(cap, size - first_id));
    *n = cnt;
    if (!cnt || (!xyz && !info3 && !desc)) return VSLAM_OK;
    const size_t o = (size_t)stream * mp.cap + (size_t)first_id;
    std::vector<uint4> rows((size_t)cnt * 4);
    std::vector<int32_t> first((size_t)cnt);
    hipError_t e = hipMemcpy(rows.data(), mp.rows + o * 4, rows.size() * sizeof(uint4), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(first.data(), mp.first + o, first.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    for (int32_t i = 0; i < cnt; ++i) {
      const uint4* r4 = rows.data() + 4 * (size_t)i;
      if (xyz) { std::memcpy(xyz + 3 * (size_t)i, &r4[0], 16); std::memcpy(xyz + 3 * (size_t)i + 2, &r4[1], 8); }
      if (info3) { info3[3 * i] = first[i]; info3[3 * i + 1] = (int32_t)r4[1].z; info3[3 * i + 2] = (int32_t)r4[1].w; }
      if (desc) std::memcpy(desc + 32 * (size_t)i, &r4[2], 32);
    }
    return VSLAM_OK;
  }
  int get_observations(int stream, int32_t first, int32_t cap, int32_t* n, int32_t* id_frame2, float* xy, double* cam) {
    if (!n || first < 0 || cap < 0) { err = "vslam_rgbd_get_observations: null count, negative first entry or capacity"; return VSLAM_ERR_INVALID; }
    int32_t size = 0;
    const int rc = map_ready(stream, true, &size);
    if (rc) return rc;
    const int32_t cnt = std::max(0, std::min(cap, size - first));
    *n = cnt;
    if (!cnt || (!id_frame2 && !xy && !cam)) return VSLAM_OK;
    std::vector<uint4> e3((size_t)cnt * 3);
    const hipError_t e = hipMemcpy(e3.data(), mp.log + ((size_t)stream * mp.ocap + (size_t)first) * 3, e3.size() * sizeof(uint4), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    for (int32_t i = 0; i < cnt; ++i) {
      const uint4* r3 = e3.data() + 3 * (size_t)i;
      if (id_frame2) { id_frame2[2 * i] = (int32_t)r3[0].x; id_frame2[2 * i + 1] = (int32_t)r3[0].y; }
      if (xy) std::memcpy(xy + 2 * (size_t)i, &r3[0].z, 8);
      if (cam) { std::memcpy(cam + 3 * (size_t)i, &r3[1], 16); std::memcpy(cam + 3 * (size_t)i + 2, &r3[2], 8); }
    }
    return VSLAM_OK;
  }
  int get_point_ids(int stream, int32_t cap, int32_t* n, int32_t* ids) {
    if (!n || cap < 0) { err = "vslam_rgbd_get_point_ids: null count or negative capacity"; return VSLAM_ERR_INVALID; }
    const int rc = map_ready(stream, false, nullptr);
    if (rc) return rc;
    const RgbdState& hs = hosts[stream];
    const int np = hs.frame_count == 0 ? 0 : hs.last_points;     // the point list vslam_rgbd_get_points reports
    *n = np;
    if (np > cap) { err = "point id output capacity too small"; return VSLAM_ERR_CAPACITY; }
    if (!np || !ids) return VSLAM_OK;
    const hipError_t e = hipMemcpy(ids, mp.ids + ((size_t)((hs.frame_count - 1) & 1) * B + stream) * rb.MAXP, (size_t)np * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    return VSLAM_OK;
  }

  // ---- undistortion of raw frames (kernels_undistort.h): opt-in, its own allocations, nothing launched while und.on is false ----
  // size of the frames the submit entries take: the full size while downscaling (set_downscale), else the raw camera's while the maps are
  // set; red_*: what the undistortion, else the detector and the space map work on (the downscale's result)
  int red_rows() const { return und.on ? und.maps.raw_rows : p.rows; }
  int red_cols() const { return und.on ? und.maps.raw_cols : p.cols; }
  int in_rows() const { return ds.factor > 1 ? ds.full_rows : red_rows(); }
  int in_cols() const { return ds.factor > 1 ? ds.full_cols : red_cols(); }
  int set_undistortion(int32_t raw_rows, int32_t raw_cols, const int16_t* map_xy, const uint16_t* map_a) {
    bool off = false;
    if (const int rc = remap_maps_check("vslam_rgbd_set_undistortion", 1, raw_rows, raw_cols, p.rows, p.cols, &map_xy, &map_a, &off, &err)) return rc;
    if (pending) { err = "vslam_rgbd_set_undistortion: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (const int rc = remap_downscale_check(VS_TRACKER_WORDS, ds, off, raw_rows, raw_cols, p.rows, p.cols, &err)) return rc;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    (void)hipStreamSynchronize(q2);
    und_free();
    drop_graph();                                   // a captured launch sequence holds the old maps and buffers (or none)
    const bool valid_on = dmask.valid_on;           // the maps' validity mask: recomputed from new maps, off with them
    const int valid_margin = dmask.valid_margin;
    if (valid_on) dmask_valid_free();
    if (off) return VSLAM_OK;
    hipError_t e = remap_maps_upload(und_mem, und.maps, 1, raw_rows, raw_cols, p.rows, p.cols, &map_xy, &map_a);
    und.img.row_stride = und.maps.stride;           // k_rectify stores words: rows 4-byte aligned
    und.img.stream_stride = ((size_t)p.rows * und.img.row_stride + 255) & ~(size_t)255;
    uint8_t* img = nullptr;
    if (e == hipSuccess) e = und_mem.alloc(&img, und.img.stream_stride * (size_t)B + 64);
    if (e == hipSuccess) e = und_mem.alloc(&und.raw_depth, (size_t)B * raw_rows * raw_cols);
    if (e != hipSuccess) { und_free(); err = std::string("vslam_rgbd_set_undistortion: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    und.img.p[0] = img;
    und.on = true;
    if (valid_on && (e = dmask_valid_build(valid_margin)) != hipSuccess) { dmask_valid_free(); und_free(); return hip_fail(e, "vslam_rgbd_set_undistortion"); }
    return VSLAM_OK;
  }
  // the undistorted image and depth image the last finished frame of `stream` was processed on (dense; either may be null)
  int get_undistorted(int stream, uint8_t* image, uint16_t* depth) {
    if (int rc = readable(stream)) return rc;
    if (!und.on || !und.have_frame) { err = "vslam_rgbd_get_undistorted: no frame has been undistorted since vslam_rgbd_set_undistortion / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    hipError_t e = image ? planes_to_host(image, und.img, 0, stream, p.rows, p.cols) : hipSuccess;
    if (e == hipSuccess && depth) e = hipMemcpy(depth, d_depth + (size_t)stream * p.rows * p.cols, (size_t)p.rows * p.cols * 2, hipMemcpyDeviceToHost);
    return fetched(e);
  }

  // ---- histogram equalisation of the intensity image (kernels_equalize.h): opt-in, its own allocations, nothing launched while eq.on is
  // false.  The depth image is untouched.  In place in the image the detector reads (the staged copy of a host frame, the undistorted
  // image); a caller's device image without undistortion is equalised into eq.img, so that caller memory is never written.
  // CLAHE (kernels_clahe.h) is the slot's second mode: the same routing and the same place in the launch sequence, the tables [B][tilesY]
  // [tilesX][256] instead of the count table.  The two modes exclude each other; switching one off while the other is on changes nothing.
  int set_equalization(int on) {
    if (pending) { err = "vslam_rgbd_set_equalization: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (const int rc = equalization_size_check(VS_TRACKER_WORDS, p.rows, p.cols, &err)) return rc;
    return eq_switch(on != 0, nullptr, 0);
  }
  int set_clahe(int on, double clip_limit, int tiles_x, int tiles_y) {
    if (pending) { err = "vslam_rgbd_set_clahe: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    ClaheArgs geo{};
    const char* why = "";
    if (on && !clahe_geometry(p.rows, p.cols, clip_limit, tiles_x, tiles_y, geo, &why)) { err = std::string("vslam_rgbd_set_clahe: ") + why; return VSLAM_ERR_INVALID; }
    return eq_switch(on != 0, &geo, clip_limit);
  }
  int eq_switch(bool on, const ClaheArgs* geo, double clip_limit) {
    static const char* const names[2] = {"vslam_rgbd_set_equalization", "vslam_rgbd_set_clahe"};
    return eq.switch_to(on, geo, clip_limit, B, 1, names, &err,
                        // (a captured launch sequence holds the two kernels, or lacks them)
                        [&] { (void)hipSetDevice(ic->device); (void)hipStreamSynchronize(q); (void)hipStreamSynchronize(q2); eq_free(); drop_graph(); },
                        [&] {                             // the image a caller's device frame is equalised into
                          uint8_t* img = nullptr;
                          const int32_t stride = (p.cols + 15) & ~15;
                          const hipError_t e = eq.mem.alloc(&img, (size_t)p.rows * stride * (size_t)B);
                          eq.img = {{img, nullptr}, stride, (size_t)p.rows * stride};
                          return e;
                        });
  }
  // uint8 [tilesY][tilesX][256]: the tables of the image the last finished frame of `stream` was processed on
  int get_clahe_luts(int stream, uint8_t* luts) {
    if (int rc = readable(stream)) return rc;
    if (!eq.on || !eq.clahe || !eq.have_frame) { err = "vslam_rgbd_get_clahe_luts: no frame has run under CLAHE since vslam_rgbd_set_clahe / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    if (!luts) { err = "vslam_rgbd_get_clahe_luts: null output"; return VSLAM_ERR_INVALID; }
    (void)hipSetDevice(ic->device);
    return fetched(eq.luts_to_host(luts, stream));
  }
  // the equalised image the last finished frame of `stream` was processed on (dense)
  int get_equalized(int stream, uint8_t* image) {
    if (int rc = readable(stream)) return rc;
    if (!eq.on || !eq.have_frame) { err = "vslam_rgbd_get_equalized: no frame has been equalised since vslam_rgbd_set_equalization / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    if (!image) { err = "vslam_rgbd_get_equalized: null output"; return VSLAM_ERR_INVALID; }
    (void)hipSetDevice(ic->device);
    return fetched(planes_to_host(image, eq.dst, 0, stream, p.rows, p.cols));
  }

  // ---- detection masks (kernels_mask.h): opt-in, their own allocations, nothing launched while none is set.  The context-wide keep words
  // dmask.stat[0] are the static mask (one image, shared by every sequence of a batch) AND the undistortion maps' validity
  // (set_undistortion_mask); a frame mask per sequence (set_frame_masks) is packed, eroded and ANDed with them once per frame into
  // dmask.eff [B][rows][TX], ahead of the first detection.  k_mask_apply ANDs the frame's words into the corner words between k_fast_box
  // and k_emit of every attempt (enqueue_attempt), inside the captured launch sequence as well.
  // detector_type ORB: cv::ORB::detect resizes its mask for every pyramid level, and nothing here restates that: masks are refused, the context
  // stays as it was
  int orb_mask_refusal(const char* what) {
    err = std::string(what) + ": detection masks are not built for detector_type ORB (cv::ORB::detect resizes its mask per pyramid level; the library has no restatement of that)";
    return VSLAM_ERR_STATE;
  }
  int set_detection_mask(const uint8_t* mask, int32_t row_stride, int32_t margin) {
    if (orbdet && mask) return orb_mask_refusal("vslam_rgbd_set_detection_mask");
    if (pending) { err = "vslam_rgbd_set_detection_mask: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (mask) if (const int rc = mask_args_check("vslam_rgbd_set_detection_mask", p.cols, row_stride, margin, &err)) return rc;
    if (!mask && !dmask.user[0]) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q); (void)hipStreamSynchronize(q2);
    dmask_user_free();
    drop_graph();                  // a captured launch sequence holds the launch, or lacks it
    if (!mask) return VSLAM_OK;
    hipError_t e = mask_static_upload(q, 1, &mask, row_stride, p.rows, p.cols, ic->cfg.TX, margin, dmask.mem, dmask.user);
    if (e == hipSuccess) e = dmask_sync();
    if (e != hipSuccess) { dmask_user_free(); return hip_fail(e, "vslam_rgbd_set_detection_mask"); }
    return VSLAM_OK;
  }
  // the context-wide eroded packed keep-mask (static AND validity) the last finished frame used: rows * TX words
  int get_detection_mask(uint64_t* words) {
    if (int rc = readable(0)) return rc;
    if (!dmask.stat[0] || !dmask.have_frame) { err = "vslam_rgbd_get_detection_mask: no frame has run under a mask since vslam_rgbd_set_detection_mask / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    if (!words) { err = "vslam_rgbd_get_detection_mask: null output"; return VSLAM_ERR_INVALID; }
    (void)hipSetDevice(ic->device);
    return fetched(hipMemcpy(words, dmask.stat[0], (size_t)p.rows * ic->cfg.TX * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  // the undistortion maps' validity as part of the context-wide keep-mask (k_map_valid, once per call and per new maps)
  int set_undistortion_mask(int on, int32_t margin) {
    if (orbdet && on) return orb_mask_refusal("vslam_rgbd_set_undistortion_mask");
    if (pending) { err = "vslam_rgbd_set_undistortion_mask: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (on) if (const int rc = mask_margin_check("vslam_rgbd_set_undistortion_mask", margin, &err)) return rc;
    if (on && !und.on) { err = "vslam_rgbd_set_undistortion_mask: no undistortion maps are set (vslam_rgbd_set_undistortion)"; return VSLAM_ERR_STATE; }
    if (!on && !dmask.valid_on) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q); (void)hipStreamSynchronize(q2);
    drop_graph();                  // a captured launch sequence holds the launch on the old words, or lacks it
    dmask.have_frame = false;
    if (!on) { dmask_valid_free(); return VSLAM_OK; }
    const hipError_t e = dmask_valid_build(margin);
    if (e != hipSuccess) { dmask_valid_free(); return hip_fail(e, "vslam_rgbd_set_undistortion_mask"); }
    return VSLAM_OK;
  }
  int get_undistortion_mask(int* on, int32_t* margin) const {
    if (on) *on = dmask.valid_on ? 1 : 0;
    if (margin) *margin = dmask.valid_on ? dmask.valid_margin : 0;
    return VSLAM_OK;
  }
  // One mask per sequence for the next submit only: sequence s at masks + s * image_stride; null cancels a pending set.  Host masks are
  // copied by that submit; device masks are read by its one pack launch and never written.
  int set_frame_masks(const uint8_t* masks, int32_t row_stride, size_t image_stride, int32_t margin, bool on_device) {
    if (orbdet && masks) return orb_mask_refusal("vslam_rgbd_set_frame_masks");
    if (pending) { err = "vslam_rgbd_set_frame_masks: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (!masks) { dmask.fm_pending = false; return VSLAM_OK; }
    if (const int rc = frame_masks_check("vslam_rgbd_set_frame_masks", B, p.rows, p.cols, row_stride, image_stride, margin, &err)) return rc;
    dmask.fm_pending = true; dmask.fm_on_device = on_device;
    dmask.fm_src = masks; dmask.fm_row_stride = row_stride; dmask.fm_image_stride = image_stride; dmask.fm_margin = margin;
    return VSLAM_OK;
  }
  // the effective words (static AND validity AND frame mask) the last finished frame of `stream` used: rows * TX words
  int get_frame_detection_mask(int stream, uint64_t* words) {
    if (int rc = readable(stream)) return rc;
    const bool stat = dmask.stat[0] && dmask.have_frame;
    if (!dmask.fm_have && !stat) { err = "vslam_rgbd_get_frame_detection_mask: the last frame used no mask"; return VSLAM_ERR_STATE; }
    if (!words) { err = "vslam_rgbd_get_frame_detection_mask: null output"; return VSLAM_ERR_INVALID; }
    (void)hipSetDevice(ic->device);
    const size_t nw = (size_t)p.rows * ic->cfg.TX;
    return fetched(hipMemcpy(words, dmask.fm_have ? dmask.eff + (size_t)stream * nw : dmask.stat[0], nw * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }

  // ---- bilateral filtering of the depth image (kernels_bilateral.h): opt-in, its own allocations, nothing launched while bl.on is false.
  // The three kernels read this frame's depth image (d_depth: the upload or the undistorted image; else the caller's device images) and
  // write bl.depth, which the space map's kernels read instead: caller memory and d_depth (vslam_rgbd_get_undistorted) are never written.
  int set_bilateral(int on, double sigma_color, double sigma_space) {
    if (pending) { err = "vslam_rgbd_set_bilateral: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    BilateralArgs ba;
    std::memset(&ba, 0, sizeof ba);
    if (on) {
      if (!(sigma_color >= 0) || !(sigma_space >= 0)) { err = "vslam_rgbd_set_bilateral: negative or non-finite sigma"; return VSLAM_ERR_INVALID; }
      if (sigma_color == 0) sigma_color = 2.0;      // depth_framepoint_generator.cpp:419: cv::bilateralFilter(.., -1, 2, 2)
      if (sigma_space == 0) sigma_space = 2.0;
      const char* why = "";
      if (!bilateral_args(p.rows, p.cols, p.depth_scale_factor_intensity_to_meters, sigma_color, sigma_space, ba, &why)) { err = std::string("vslam_rgbd_set_bilateral: ") + why; return VSLAM_ERR_INVALID; }
    }
    if (!on && !bl.on) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    (void)hipStreamSynchronize(q2);
    bl_free();
    drop_graph();                                   // a captured launch sequence holds the three kernels (or lacks them)
    if (!on) return VSLAM_OK;
    const size_t npx = (size_t)p.rows * p.cols;
    hipError_t e = bl.mem.alloc(&bl.depth, npx * (size_t)B + 2);
    if (e == hipSuccess) e = bl.mem.alloc(&ba.cells, (size_t)B * 4);
    if (e == hipSuccess) e = bl.mem.alloc(&ba.lut, (size_t)B * VS_BL_LUT);
    if (e == hipSuccess) e = bilateral_arm(ba.cells, B, q);
    if (e != hipSuccess) { bl_free(); err = std::string("vslam_rgbd_set_bilateral: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    ba.dst = bl.depth; ba.dst_stream_stride = npx; ba.dst_row_stride = p.cols; ba.n = B;
    bl.args = ba; bl.sigma_color = sigma_color; bl.sigma_space = sigma_space;
    bl.on = true;
    return VSLAM_OK;
  }
  int get_bilateral(int* on, double* sigma_color, double* sigma_space) const {
    if (on) *on = bl.on ? 1 : 0;
    if (sigma_color) *sigma_color = bl.on ? bl.sigma_color : 0.0;
    if (sigma_space) *sigma_space = bl.on ? bl.sigma_space : 0.0;
    return VSLAM_OK;
  }
  // the filtered depth image the last finished frame of `stream` was mapped from (dense) and its colour table; either may be null
  int get_filtered_depth(int stream, uint16_t* depth, float* lut4098) {
    if (int rc = readable(stream)) return rc;
    if (!bl.on || !bl.have_frame) { err = "vslam_rgbd_get_filtered_depth: no frame has been filtered since vslam_rgbd_set_bilateral / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    const size_t npx = (size_t)p.rows * p.cols;
    hipError_t e = depth ? hipMemcpy(depth, bl.depth + (size_t)stream * npx, npx * 2, hipMemcpyDeviceToHost) : hipSuccess;
    if (e == hipSuccess && lut4098) e = hipMemcpy(lut4098, bl.args.lut + (size_t)stream * VS_BL_LUT, VS_BL_LUT * sizeof(float), hipMemcpyDeviceToHost);
    return fetched(e);
  }

  // ---- downscale of the incoming frames (kernels_downscale.h): opt-in, its own allocations, nothing launched while ds.factor is 1.  The
  // image: behind the grey stage and ahead of the undistortion, on the image queue, into ds.img.  The depth image: on the space map's
  // queue behind the upload and ahead of the depth undistortion and the bilateral filter, from the full-size staging (host frames) or the
  // caller's device images into what the next stage reads — und.raw_depth while undistorting, else d_depth.  Caller memory is only read.
  int set_downscale(int32_t factor, int32_t full_rows, int32_t full_cols) {
    if (pending) { err = "vslam_rgbd_set_downscale: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (const int rc = downscale_check(VS_TRACKER_WORDS, factor, full_rows, full_cols, und.on, red_rows(), red_cols(), &err)) return rc;
    if (ds.is(factor, full_rows, full_cols)) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    (void)hipStreamSynchronize(q2);
    ds_free();
    drop_graph();                                   // a captured launch sequence holds the kernels and buffers (or lacks them)
    if (factor == 1) return VSLAM_OK;
    const int rr = red_rows(), rc = red_cols();
    ds.img.row_stride = (rc + 15) & ~15;
    ds.img.stream_stride = (size_t)rr * ds.img.row_stride;
    uint8_t* img = nullptr;
    hipError_t e = ds.mem.alloc(&img, ds.img.stream_stride * (size_t)B + 64);
    if (e == hipSuccess) e = ds.mem.alloc(&ds.full_depth, (size_t)B * full_rows * full_cols);
    if (e != hipSuccess) { ds_free(); return hip_fail(e, "vslam_rgbd_set_downscale"); }
    ds.img.p[0] = img;
    ds.factor = factor; ds.full_rows = full_rows; ds.full_cols = full_cols;
    return VSLAM_OK;
  }
  void get_downscale(int32_t* factor, int32_t* full_rows, int32_t* full_cols) const { ds.get(factor, full_rows, full_cols); }
  // the reduced image and depth image of the last finished frame of `stream` (dense, full / factor; either may be null)
  int get_downscaled(int stream, uint8_t* image, uint16_t* depth) {
    if (int rc = readable(stream)) return rc;
    if (ds.factor == 1 || !ds.have_frame) { err = "vslam_rgbd_get_downscaled: no frame has been downscaled since vslam_rgbd_set_downscale / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    (void)hipSetDevice(ic->device);
    const int rr = red_rows(), rc = red_cols();
    hipError_t e = image ? planes_to_host(image, ds.img, 0, stream, rr, rc) : hipSuccess;
    const uint16_t* reduced = und.on ? und.raw_depth : d_depth;
    if (e == hipSuccess && depth) e = hipMemcpy(depth, reduced + (size_t)stream * rr * rc, (size_t)rr * rc * 2, hipMemcpyDeviceToHost);
    return fetched(e);
  }

  // ---- smoothing of the intensity image (kernels_smooth.h): opt-in, its own allocation, nothing launched while sm.mode is OFF.  Behind
  // the undistortion and ahead of the equalisation slot, on the image queue, once per frame, from wherever the image lies (the staged copy,
  // the grey / reduced / undistorted image, the caller's device memory: only read) into sm.img, which the slot then equalises in place
  // and the detector reads.  The depth image is untouched.
  int set_smoothing(int mode, int32_t ksize) {
    if (pending) { err = "vslam_rgbd_set_smoothing: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (mode != VSLAM_SMOOTH_OFF)
      if (const int rc = smooth_check("vslam_rgbd_set_smoothing", mode, ksize, p.rows, p.cols, &err)) return rc;
    if (sm.is(mode, ksize)) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    (void)hipStreamSynchronize(q2);
    drop_graph();                                   // a captured launch sequence holds the kernel and its buffer (or lacks them)
    if (mode != VSLAM_SMOOTH_OFF && sm.mode != VSLAM_SMOOTH_OFF) { sm.mode = mode; sm.ksize = ksize; sm.have_frame = false; return VSLAM_OK; }   // the image stays
    sm_free();
    if (mode == VSLAM_SMOOTH_OFF) return VSLAM_OK;
    const int32_t stride = (p.cols + 15) & ~15;
    uint8_t* img = nullptr;
    const hipError_t e = sm.mem.alloc(&img, (size_t)p.rows * stride * (size_t)B);
    if (e != hipSuccess) { sm_free(); return hip_fail(e, "vslam_rgbd_set_smoothing"); }
    sm.img = {{img, nullptr}, stride, (size_t)p.rows * stride};
    sm.mode = mode; sm.ksize = ksize;
    return VSLAM_OK;
  }
  void get_smoothing(int* mode, int32_t* ksize) const { sm.get(mode, ksize); }
  // the smoothed image of the last finished frame of `stream` (dense); equalised in place afterwards while the slot is on
  int get_smoothed(int stream, uint8_t* image) {
    if (int rc = readable(stream)) return rc;
    if (!sm.mode || !sm.have_frame) { err = "vslam_rgbd_get_smoothed: no frame has been smoothed since vslam_rgbd_set_smoothing / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    if (!image) { err = "vslam_rgbd_get_smoothed: null output"; return VSLAM_ERR_INVALID; }
    (void)hipSetDevice(ic->device);
    return fetched(planes_to_host(image, sm.img, 0, stream, p.rows, p.cols));
  }

  // ---- colour input (kernels_gray.h): opt-in, its own allocation, nothing launched while col.format is VSLAM_PIXEL_GRAY8.  The intensity
  // image of every entry is interleaved colour then (strides in bytes); k_gray_u8 converts it into col.gray, an image of the tracker's own at
  // the input size, which everything behind it reads — the undistortion, else the equalisation (in place) and the detector.  The caller's
  // image, host copy or device memory, is only read.  The depth image is untouched.
  int in_bytes() const { return (col.format ? gray_channels(col.format) : 1) * in_cols(); }      // of one row of the intensity image that comes in
  int set_color_input(int format) {
    if (pending) { err = "vslam_rgbd_set_color_input: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    if (const int rc = color_format_check(VS_TRACKER_WORDS, format, &err)) return rc;
    if (format == col.format) return VSLAM_OK;
    (void)hipSetDevice(ic->device);
    (void)hipStreamSynchronize(q);
    (void)hipStreamSynchronize(q2);
    if (format == VSLAM_PIXEL_GRAY8) mapcol_free();  // no colour left to sample
    col_free();
    drop_graph();                                   // a captured launch sequence holds the kernel (or lacks it)
    col.format = format;
    return VSLAM_OK;
  }
  // the grey image the last finished frame of `stream` was converted to (dense, at the input size)
  int get_gray(int stream, uint8_t* image) {
    if (int rc = readable(stream)) return rc;
    if (!col.format || !col.have_frame) { err = "vslam_rgbd_get_gray: no frame has been converted since vslam_rgbd_set_color_input / vslam_rgbd_reset"; return VSLAM_ERR_STATE; }
    if (!image) { err = "vslam_rgbd_get_gray: null output"; return VSLAM_ERR_INVALID; }
    (void)hipSetDevice(ic->device);
    return fetched(planes_to_host(image, col.gray, 0, stream, col.rows, col.cols));
  }

  int process(const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride, size_t left_stream_stride = 0, size_t depth_stream_stride = 0) {
    const int rc = submit(left, lstride, depth, dstride, left_stream_stride, depth_stream_stride);
    return rc != VSLAM_OK ? rc : wait();
  }
  // submit(): copies the frame(s) in and enqueues the kernels; returns without waiting.  wait(): the result (and, for the rare frame whose
  // registration asks for another attempt, the further attempts).  left / depth: n_streams images, `*_stream_stride` bytes / elements apart.
  // on_device: left / depth are DEVICE pointers (images already in HBM, e.g. written by a capture pipeline): nothing is copied, the kernels
  // read them where they are; the depth images must then be dense per sequence (depth_stream_stride == rows * depth_row_stride)
  int submit(const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride, size_t left_stream_stride = 0, size_t depth_stream_stride = 0, bool on_device = false) {
    if (!left || !depth) { err = "called with empty frame"; return VSLAM_ERR_INVALID; }
    if (on_device && !und.on && ds.factor == 1 && B > 1 && depth_stream_stride != (size_t)p.rows * dstride) { err = "RGB-D batch on device images: depth images must be dense per sequence"; return VSLAM_ERR_INVALID; }
    if (failed) { err = "RGB-D tracker: an earlier frame failed (" + failed_why + "); reset() before the next frame"; return VSLAM_ERR_STATE; }
    if (pending) { err = "RGB-D tracker: the previous frame has not been waited for"; return VSLAM_ERR_STATE; }
    if (und.on && ds.factor == 1 && (size_t)und.maps.raw_rows * (size_t)dstride > 0x7fffffffu) { err = "RGB-D frame: raw depth row stride too large"; return VSLAM_ERR_INVALID; }   // k_undistort_depth's 32-bit tap offsets
    if (B > 1 && (left_stream_stride < (size_t)(in_rows() - 1) * lstride + in_bytes() || depth_stream_stride < (size_t)(in_rows() - 1) * dstride + in_cols())) {
      err = "RGB-D batch: stream strides smaller than an image"; return VSLAM_ERR_INVALID;
    }
    // a submit refused above has changed nothing: frame masks that wait for a frame go on waiting.  From here on the set is this frame's: an
    // accepted submit consumes it (frame_masks_prepare), and one that fails afterwards drops it with the frame
    const int rc = submit_frame(left, lstride, depth, dstride, left_stream_stride, depth_stream_stride, on_device);
    if (rc != VSLAM_OK) { failed = true; failed_why = err; dmask.fm_pending = false; dmask.fm_frame = false; }
    else pending = true;
    return rc;
  }
  int wait() {
    if (!pending) { err = "RGB-D tracker: no frame in flight"; return VSLAM_ERR_STATE; }
    pending = false;
    const int rc = finish_frame();
    if (rc != VSLAM_OK) { failed = true; failed_why = err; }
    else { und.have_frame = und.on; eq.have_frame = eq.on; col.have_frame = col.format != VSLAM_PIXEL_GRAY8; ds.have_frame = ds.factor > 1; sm.have_frame = sm.mode != 0; bl.have_frame = bl.on; dmask.have_frame = dmask.stat[0] != nullptr; dmask.fm_have = dmask.fm_frame; }
    return rc;
  }

  // what every getter of sequence `stream` checks first; a frame between submit() and wait() is rewriting the lists the getters read (and
  // flags of the previous list): not readable
  int readable(int stream) {
    if (stream < 0 || stream >= B) { err = "stream index out of range"; return VSLAM_ERR_INVALID; }
    if (pending) { err = "RGB-D tracker: a frame is in flight (call vslam_rgbd_wait first)"; return VSLAM_ERR_STATE; }
    return VSLAM_OK;
  }
  int get_points(int stream, int32_t cap, int32_t* n, float* xy, double* cam, int32_t* meta4, uint8_t* desc) {
    if (int rc = readable(stream)) return rc;
    const RgbdState& hs = hosts[stream];
    if (hs.frame_count == 0) { *n = 0; return VSLAM_OK; }
    const int np = hs.last_points;
    *n = np;
    if (np > cap) { err = "point output capacity too small"; return VSLAM_ERR_CAPACITY; }
    if (np == 0) return VSLAM_OK;
    const RgbdList& l = rb.fl[(hs.frame_count - 1) & 1];
    const size_t P = (size_t)rb.MAXP, o = (size_t)stream * P;
    hipError_t e = hipSuccess;
    if (xy) e = hipMemcpy(xy, l.xy + o * 2, (size_t)np * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cam) e = hipMemcpy(cam, l.cam + o * 3, (size_t)np * 24, hipMemcpyDeviceToHost);
    if (e == hipSuccess && desc) e = hipMemcpy(desc, l.desc + o * 32, (size_t)np * 32, hipMemcpyDeviceToHost);
    if (e == hipSuccess && meta4) {
      std::vector<int32_t> prev(np), tlen(np), lmu(np); std::vector<uint8_t> fl(np);
      e = hipMemcpy(prev.data(), l.prev + o, (size_t)np * 4, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(tlen.data(), l.tlen + o, (size_t)np * 4, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(lmu.data(), l.lmu + o, (size_t)np * 4, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(fl.data(), l.flags + o, (size_t)np, hipMemcpyDeviceToHost);
      for (int i = 0; i < np && e == hipSuccess; ++i) {
        meta4[4 * i] = prev[i]; meta4[4 * i + 1] = tlen[i]; meta4[4 * i + 2] = (fl[i] & RGBD_F_LM) ? lmu[i] : 0; meta4[4 * i + 3] = (fl[i] & RGBD_F_UNREL) ? 1 : 0;
      }
    }
    if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; }
    return VSLAM_OK;
  }

private:
  RgbdBuf rb;
  hipStream_t q = nullptr, q2 = nullptr;      // q: everything of a frame; q2: the depth image's copy and the space map, beside the image pipeline
  hipEvent_t ev_depth = nullptr;
  int H = 0, TR = 0;
  int wg1 = 1024;                // threads of the single-workgroup kernels (VSLAM_RGBD_WG = 256 | 512 | 1024; measured at 620 x 188, ~700 features: 0.256 / 0.258 / 0.265 ms per frame for 1024 / 512 / 256: their barriers are not what a frame waits for)
  uint16_t* d_depth = nullptr;   // [B][rows * cols], rows re-packed
  const uint16_t* depth_src = nullptr; int32_t depth_src_stride = 0;   // what the space-map kernels read this frame: d_depth, or the caller's device images
  uint8_t* d_img = nullptr; size_t img_stream = 0;     // [B][img_stream] bytes, the caller's row stride kept
  RgbdState* pinned = nullptr;   // [B]
  bool depth_pending = false, pending = false, depth_plain = false, force_cross = false;
  DevBuf bs;                      // the inner context's buffer table with this frame's image pointers
  // VSLAM_RGBD_GRAPH=1 (opt-in): the frame's launch sequence (depth map on q2 beside the image pipeline on q, registration, tail, the state
  // block's copy out) captured once into a hipGraph and replayed — two copies and ONE launch per frame instead of ~22.  Measured on MI355X /
  // ROCm 7.2 (tests/validation/rgbd_submit_time.py): submit() takes 80 us of host time either way (the two pageable copies; the runtime replays a
  // graph node by node) and the frame 0.31 against 0.30 ms: the frame is bound by its dependent kernels, not by their launches.  Kept as a
  // tested switch, captured again when the image stride or buffer changes, or when a frame with frame masks follows one without (or the
  // reverse): the pack launch stays outside, the sequence holds the apply launches on eff or on the context-wide words.
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  bool use_graph = false;
  int32_t graph_stride = -1;
  const uint8_t* graph_img = nullptr;
  bool graph_fm = false;         // the captured sequence applies the frame masks' effective words (else the context-wide ones, or none)
  hipEvent_t ev_fork = nullptr;
  // the landmark map and the observation log (kernels_rgbd_map.h): off while cap / ocap == 0.  Allocations of their own, freed when the
  // store is turned off or replaced (the inner context's allocation list only grows until destroy)
  RgbdMap mp{};
  DeviceStore map_mem, obs_mem;
  RgbdMapColor mc{};             // the map's colours: off while mc.rgb is null
  DeviceStore mapcol_mem;
  // undistortion of raw frames: off while und.on is false.  The maps at the tracker's size (rows padded to map_stride entries), the
  // undistorted images the image pipeline reads, and the raw depth images of a host frame (raw images go through d_img; the
  // undistorted depth images are d_depth).  raw_*: where this frame's raw images are — the staging buffers or the caller's device memory
  struct Undist {
    bool on = false, have_frame = false;
    RemapMaps maps;
    ImgPlanes img;
    uint16_t* raw_depth = nullptr;
  } und;
  DeviceStore und_mem;
  // equalisation of the intensity image: the slot (EqSlot, host_prestage.h: tables [B], this frame's src and dst, dst being what the image
  // pipeline reads) and the image a caller's device frame is equalised into, allocated from the slot's store
  struct Equal : EqSlot { ImgPlanes img; } eq;
  // colour input: off while col.format is VSLAM_PIXEL_GRAY8.  The grey image [B] at the input size rows x cols (allocated with the first frame
  // at that size)
  struct Colour { int format = 0; bool have_frame = false; ImgPlanes gray; int32_t rows = 0, cols = 0; } col;
  DeviceStore col_mem;
  // downscale of the incoming frames: off while factor is 1.  img: the reduced images [B]; full_depth: the full-size depth images of a host
  // frame [B][full_rows * full_cols], re-packed.  full_dep*: where this frame's full-size depth images are (the staging or caller memory)
  struct Down : DownscaleSwitch { bool have_frame = false; ImgPlanes img; uint16_t* full_depth = nullptr; DeviceStore mem; } ds;
  const uint16_t* full_dep = nullptr; int32_t full_dep_stride = 0; size_t full_dep_stream = 0;
  // smoothing of the intensity image: off while mode is VSLAM_SMOOTH_OFF.  img: the smoothed images [B]
  struct Smooth : SmoothSwitch { bool have_frame = false; ImgPlanes img; DeviceStore mem; } sm;
  // bilateral filtering of the depth image: off while bl.on is false.  depth: the filtered images [B][rows * cols] the space map reads;
  // args: what the three kernels get but for this frame's source (sizes, scales, taps, the range cells [B][4] and the tables [B][4098])
  struct Bilateral { bool on = false, have_frame = false; double sigma_color = 0, sigma_space = 0; uint16_t* depth = nullptr; BilateralArgs args; DeviceStore mem; } bl;
  // detection masks.  user / valid: the static mask's and the maps' validity's eroded packed words [rows][TX] (index 0; the pairs are
  // what mask_static_combine takes), stat[0]: the context-wide words, the one there is or comb[0] = both ANDed; off while null.  The
  // frame masks wait in fm_* for the next submit; slab: the device copy of host masks at the caller's strides; eff [B][rows][TX]: the
  // effective words of the frame under way (fm_frame) / of the last finished frame (fm_have).
  struct DetMask { unsigned long long* stat[2] = {nullptr, nullptr}; bool have_frame = false;
                   unsigned long long* user[2] = {nullptr, nullptr}; DeviceStore mem;
                   bool valid_on = false; int valid_margin = 0; unsigned long long* valid[2] = {nullptr, nullptr}; DeviceStore valid_mem;
                   unsigned long long* comb[2] = {nullptr, nullptr}; DeviceStore comb_mem;
                   bool fm_pending = false, fm_on_device = false; const uint8_t* fm_src = nullptr; int32_t fm_row_stride = 0; size_t fm_image_stride = 0; int fm_margin = 0;
                   uint8_t* slab = nullptr; size_t slab_bytes = 0; DeviceStore slab_mem;
                   unsigned long long* eff = nullptr; DeviceStore eff_mem;
                   bool fm_frame = false, fm_have = false; } dmask;
  hipError_t dmask_sync() { return mask_static_combine(q, 1, (size_t)p.rows * ic->cfg.TX, dmask.user, dmask.valid, dmask.comb_mem, dmask.comb, dmask.stat); }
  void dmask_user_free() { dmask.mem.release(); dmask.user[0] = nullptr; dmask.have_frame = false; (void)dmask_sync(); }
  void dmask_valid_free() { dmask.valid_mem.release(); dmask.valid[0] = nullptr; dmask.valid_on = false; dmask.valid_margin = 0; dmask.have_frame = false; (void)dmask_sync(); }
  hipError_t dmask_valid_build(int margin) {
    hipError_t e = mask_valid_words(q, und.maps, 1, margin, (size_t)p.rows * ic->cfg.TX, dmask.valid_mem, dmask.valid);
    if (e == hipSuccess) { dmask.valid_on = true; dmask.valid_margin = margin; e = dmask_sync(); }
    return e;
  }
  void dmask_free() {
    for (DeviceStore* m : {&dmask.mem, &dmask.valid_mem, &dmask.comb_mem, &dmask.slab_mem, &dmask.eff_mem}) m->release();
    dmask = DetMask{};
  }
  // Ahead of the frame's first launch (and outside a captured sequence, whose launches read eff at its fixed address): a pending set of
  // frame masks is consumed — host masks copied into the slab on the frame's queue, then ONE k_mask_pack over all sequences packs, erodes
  // and ANDs the context-wide words into eff.  The previous frame has been waited for: nothing reads slab or eff any more.
  int frame_masks_prepare() {
    dmask.fm_frame = false;
    if (!dmask.fm_pending) return VSLAM_OK;
    dmask.fm_pending = false;
    const int TX = ic->cfg.TX;
    hipError_t e = hipSuccess;
    if (!dmask.eff) e = dmask.eff_mem.alloc(&dmask.eff, (size_t)B * p.rows * TX);
    if (e != hipSuccess) return hip_fail(e, "frame masks");
    const uint8_t* src = dmask.fm_src;
    if (!dmask.fm_on_device) {
      const size_t span = (size_t)(B - 1) * dmask.fm_image_stride + (size_t)(p.rows - 1) * dmask.fm_row_stride + p.cols;
      if (dmask.slab_bytes < span) {
        dmask.slab_mem.release(); dmask.slab = nullptr; dmask.slab_bytes = 0;
        if ((e = dmask.slab_mem.alloc(&dmask.slab, span)) != hipSuccess) return hip_fail(e, "frame masks");
        dmask.slab_bytes = span;
      }
      if ((e = hipMemcpyAsync(dmask.slab, src, span, hipMemcpyHostToDevice, q)) != hipSuccess) return hip_fail(e, "frame masks");
      src = dmask.slab;
    }
    MaskPackArgs a{};
    a.src[0] = src; a.src_stream_stride = dmask.fm_image_stride; a.src_row_stride = dmask.fm_row_stride;
    a.rows = p.rows; a.cols = p.cols; a.TX = TX; a.margin = dmask.fm_margin; a.n = B; a.sides = 1;
    a.dst = dmask.eff; a.stat[0] = dmask.stat[0];
    active_all(a.active, B);
    mask_pack_enqueue(q, a);
    dmask.fm_frame = true;
    return VSLAM_OK;
  }
  PrePlan pre;                   // this frame's routing through the input stages (route_frame): pre.color is its colour source
  const uint16_t* raw_dep = nullptr; int32_t raw_dep_stride = 0; size_t raw_dep_stream = 0;
  bool src_on_device = false;    // this frame's images are the caller's device memory: q2 is ordered behind q before it reads them

  void obs_free() {
    obs_mem.release();
    mp.log = nullptr; mp.ocount = nullptr; mp.ocap = 0;
  }
  void eq_free() {
    eq.release();
    eq.img = ImgPlanes();
  }
  void bl_free() {
    bl.mem.release();
    bl.on = false; bl.have_frame = false; bl.depth = nullptr;
    std::memset(&bl.args, 0, sizeof bl.args);
  }
  void col_free() {
    col_mem.release();
    col = Colour{};
  }
  void ds_free() {
    ds.mem.release();
    ds = Down{};
  }
  void sm_free() {
    sm.mem.release();
    sm = Smooth{};
  }
  // This frame's routing through the input stages (the table: host_prestage.h, PrePlan), from which switches are on: `in` is
  // the intensity image that came in (the staged copy or the caller's device memory), own: it is ours to overwrite.  Fills pre and the
  // slot's src / dst and points bs at what the detector reads.  The grey image is allocated here, with the first frame at its size.
  hipError_t route_frame(ImgPlanes in, bool own) {
    pre.format = col.format; pre.remap = und.on; pre.factor = ds.factor;
    pre.in_rows = in_rows(); pre.in_cols = in_cols(); pre.red_rows = red_rows(); pre.red_cols = red_cols(); pre.rows = p.rows; pre.cols = p.cols;
    if (col.format) {
      if (!col.gray.p[0] || col.rows != pre.in_rows || col.cols != pre.in_cols) {
        (void)hipStreamSynchronize(q);
        col_mem.release();
        col.gray = ImgPlanes();
        drop_graph();                              // it holds the old image
        col.rows = pre.in_rows; col.cols = pre.in_cols;
        uint8_t* g = nullptr;
        const int32_t stride = (col.cols + 15) & ~15;
        const hipError_t e = col_mem.alloc(&g, (size_t)col.rows * stride * (size_t)B);
        if (e != hipSuccess) return e;
        col.gray = {{g, nullptr}, stride, (size_t)col.rows * stride};
      }
      pre.color = in; pre.gray = col.gray; in = col.gray; own = true;
    }
    if (ds.factor > 1) { pre.full = in; pre.reduced = ds.img; in = ds.img; own = true; }
    if (und.on) { pre.raw = in; pre.mapped = und.img; in = und.img; own = true; }
    pre.smooth_mode = sm.mode; pre.smooth_ksize = sm.ksize;
    if (sm.mode) { pre.unsmoothed = in; pre.smoothed = sm.img; in = sm.img; own = true; }
    if (eq.on) { eq.src = in; eq.dst = own ? in : eq.img; in = eq.dst; }
    buf_set_planes(bs, in);
    return hipSuccess;
  }
  void und_free() {
    und_mem.release();
    und = Undist{};
  }
  void mapcol_free() {
    mapcol_mem.release();
    mc = RgbdMapColor{};
  }
  // this frame's colour image as k_rgbd_map_color reads it (pre.color: the staged copy of a host frame, which the next submit overwrites, or the
  // caller's device memory, which must stay as it is until wait() has returned: further attempts colour the frame from there); the raw
  // image behind the undistortion map while undistorting
  // while downscaling: the full-size image, tapped by block averages at the reduced size
  ColorSrc map_color_src() const {
    const bool down = ds.factor > 1;
    return color_src(pre.color, down ? red_rows() : col.rows, down ? red_cols() : col.cols, col.format, und.on ? &und.maps : nullptr, ds.factor);
  }
  void map_free() {
    obs_free();
    mapcol_free();                                  // the colours are indexed by the map's ids
    map_mem.release();
    mp = RgbdMap{};
  }
  // ids from 0 again, no point labelled, nothing logged; the rows are cleared too so that a read never returns another run's data
  hipError_t map_clear() {
    const size_t nB = (size_t)B, n = nB * (size_t)mp.cap;
    hipError_t e = hipMemsetAsync(mp.rows, 0, n * 4 * sizeof(uint4), q);
    if (e == hipSuccess) e = hipMemsetAsync(mp.first, 0, n * sizeof(int32_t), q);
    if (e == hipSuccess) e = hipMemsetAsync(mp.count, 0, nB * sizeof(int32_t), q);
    if (e == hipSuccess) e = hipMemsetAsync(mp.committed, 0, nB * sizeof(int32_t), q);
    if (e == hipSuccess) e = hipMemsetAsync(mp.ids, 0xff, 2 * nB * (size_t)rb.MAXP * sizeof(int32_t), q);
    if (e == hipSuccess && mp.ocap) e = hipMemsetAsync(mp.ocount, 0, nB * sizeof(int32_t), q);
    if (e == hipSuccess && mc.rgb) e = hipMemsetAsync(mc.rgb, 0, n * sizeof(uint32_t), q);
    if (e == hipSuccess && mc.rgb) e = hipMemsetAsync(mc.colored, 0, nB * sizeof(int32_t), q);
    if (e == hipSuccess) e = hipStreamSynchronize(q);
    return e;
  }

  void release() {
    // an un-waited frame may still be copying into `pinned` and running on q / q2: both queues drain before anything is freed
    if (q) (void)hipStreamSynchronize(q);
    if (q2) (void)hipStreamSynchronize(q2);
    pending = false;
    if (pinned) { (void)hipHostFree(pinned); pinned = nullptr; }
    drop_graph();
    map_free();
    und_free();
    eq_free();
    col_free();
    ds_free();
    sm_free();
    bl_free();
    dmask_free();
    if (ev_fork) { (void)hipEventDestroy(ev_fork); ev_fork = nullptr; }
    if (q2) { (void)hipStreamDestroy(q2); q2 = nullptr; }
    if (ev_depth) { (void)hipEventDestroy(ev_depth); ev_depth = nullptr; }
    if (d_img) { (void)hipFree(d_img); d_img = nullptr; }
    if (ic) { vslam_destroy(ic); ic = nullptr; }      // frees everything dalloc() registered
  }
  int fetched(hipError_t e) { if (e != hipSuccess) { err = hipGetErrorString(e); return VSLAM_ERR_HIP; } return VSLAM_OK; }     // the end of an image getter
  int hip_fail(hipError_t e, const char* where) { err = std::string(where) + ": " + hipGetErrorString(e); return VSLAM_ERR_HIP; }

  // initialize() .. registration of one attempt: the image pipeline on ONE image per sequence (DevCfg::mono: grid z = sequences; k_emit with
  // its one-image controller), track, aligner.  Sequences whose bit in b.active is cleared are skipped by every kernel.
  // again: attempt 2 / 3 of a frame — its keypoint vector keeps the earlier attempts' keypoints (frame_->keypointsLeft() is appended to and never
  // cleared between the initialize() calls of one frame: base_framepoint_generator.cpp:422, pose_tracker_3d.cpp:320,402): the list so far is
  // saved before the detection overwrites it and merged with the new one before anything reads the features.
  void enqueue_attempt(const DevBuf& b, bool again = false) {
    const DevCfg& d = ic->cfg;
    const dim3 g1(d.TX, (d.c.rows + VS_TILE_H - 1) / VS_TILE_H, B);
    if (orbdet) { enqueue_orb_detect(b, again); enqueue_registration(b); return; }
    if (again) hipLaunchKernelGGL(k_rgbd_save_features, dim3(B), dim3(1024), 0, q, d, b, rb);
    hipLaunchKernelGGL(k_fast_box, g1, dim3(256), VS_FB_DYN_LDS, q, d, b);
    const bool orb = d.c.descriptor_type == VSLAM_DESCRIPTOR_ORB;
    if (dmask.fm_frame || dmask.stat[0]) {     // the detection mask: the keep words into every sequence's corner words, ahead of the count
      MaskApplyArgs ma{};                       // (under frame masks: the sequence's own effective words, which hold the context-wide ones)
      ma.corner = b.mask; ma.nw = d.c.rows * d.TX; ma.n = B; ma.sides = 1;
      if (dmask.fm_frame) { ma.stat[0] = dmask.eff; ma.stat_stream_stride = (size_t)ma.nw; }
      else ma.stat[0] = dmask.stat[0];
      std::memcpy(ma.active, b.active, sizeof ma.active);
      mask_apply_enqueue(q, ma);
    }
    launch_emit(q, d, b, B, 1, orb ? (int)VSLAM_ORB_BORDER : (int)VSLAM_BRIEF_BORDER, 2);
    const dim3 g3((d.c.cols + VS_BT_W - 1) / VS_BT_W, (d.c.rows + VS_BT_H - 1) / VS_BT_H, B);
    if (orb) {
      Gauss7 gk; for (int i = 0; i < 4; ++i) gk.k[i] = d.gauss7[i];
      hipLaunchKernelGGL(k_gauss7, g1, dim3(256), 0, q, d, b, gk);
      hipLaunchKernelGGL(k_orb_describe, g3, dim3(256), 0, q, d, b, d.orb_cos, d.orb_sin);
    } else {
      hipLaunchKernelGGL(k_brief, g3, dim3(256), 0, q, d, b);
    }
    if (again) hipLaunchKernelGGL(k_rgbd_merge_features, dim3(B), dim3(1024), 0, q, d, b, rb);
    enqueue_registration(b);
  }
  void enqueue_registration(const DevBuf& b) {
    const DevCfg& d = ic->cfg;
    if (depth_pending) { (void)hipStreamWaitEvent(q, ev_depth, 0); depth_pending = false; }     // the space map is first read here
    hipLaunchKernelGGL(k_rgbd_track_candidates, dim3(std::max(8, std::min(256, 4096 / B)), B), dim3(256), 0, q, d, b, rb);
    hipLaunchKernelGGL(k_rgbd_track, dim3(B), dim3(wg1), 0, q, d, b, rb);
    hipLaunchKernelGGL(k_rgbd_align, dim3(B), dim3(VS_WG), 0, q, d, b, rb);
  }

  // ---- detector_type ORB (kernels_rgbd_orb.h) ------------------------------------------------------------------------------------------------
  // Launches of one attempt, whatever the batch size and the detector grid (L <= 8: the levels a region holds): 1 (level 0, thresholds)
  // + (L - 1) resizes + 2 L (k_fast_box, k_emit per level) + 5 (two selects, Harris, control, angle) + the extractor's + 1 (install).
  // The ORB extractor adds k_gauss7, (L - 1) resizes of the whole image, (L - 1) Gaussians and the describe kernel = 2 L (one region that
  // is the whole image: the pyramid is the detector's, L + 1); BRIEF adds k_fast_box for the box image and its describe kernel = 2.
  // Together 5 L + 6 (ORB extractor on a grid), 4 L + 7 (ORB extractor, one region), 3 L + 8 (BRIEF), then the three registration launches.
  bool orbdet = false;
  OrbDet od{};
  OrbDet* d_od = nullptr;
  std::vector<DevCfg> lcfg;      // the level contexts: what k_fast_box / k_emit take, level-sized, their streams the (sequence, region) pairs
  std::vector<DevBuf> lbuf;
  bool walias = false;           // one region that is the whole image: the extractor's pyramid is the detector's
  std::vector<uint8_t*> wraw;    // else the whole image's levels 1 .. L - 1, [B][wrows * wstride]
  int orb_create() {
    const DevCfg& d = ic->cfg;
    const int R = d.n_regions, BR = B * R;
    for (int r = 1; r < R; ++r)
      if (d.regions[r].w != d.regions[0].w || d.regions[r].h != d.regions[0].h) { err = "RGB-D mode, detector_type ORB: detector regions of different sizes"; return VSLAM_ERR_INVALID; }
    if (BR > VS_MAX_STREAMS) { err = "RGB-D mode, detector_type ORB: more than 4096 (sequence, region) pairs"; return VSLAM_ERR_INVALID; }
    const int rr = d.regions[0].h, rc = d.regions[0].w;
    if (rr < 2 * VS_ORBD_EDGE + 8 || rc < 2 * VS_ORBD_EDGE + 8) { err = "RGB-D mode, detector_type ORB: a detector region smaller than 70 pixels"; return VSLAM_ERR_INVALID; }
    const OrbPlan plan = orb_plan(rr, rc, VS_ORBD_FEATURES, 1.2f, VS_ORBD_LEVELS, VS_ORBD_EDGE);
    const OrbPlan whole = orb_plan(p.rows, p.cols, VS_ORBD_FEATURES, 1.2f, VS_ORBD_LEVELS, VS_ORBD_EDGE);
    const int L = plan.n_levels;
    const bool orb_ext = p.descriptor_type == VSLAM_DESCRIPTOR_ORB;
    walias = R == 1 && rr == p.rows && rc == p.cols;
    std::memset(&od, 0, sizeof od);
    od.L = L; od.R = R; od.B = B; od.NMAX = d.NMAX;
    for (int r = 0; r < R; ++r) { od.rx[r] = d.regions[r].x; od.ry[r] = d.regions[r].y; }
    od.um = orb_umax_table(VS_ORBD_PATCH / 2);
    hipError_t e = hipSuccess;
    auto A = [&](auto** ptr, size_t count) {          // zeroed: counts, tickets and level states start from nothing
      if (e == hipSuccess) e = dalloc(ic, ptr, count);
      if (e == hipSuccess) e = hipMemset(*ptr, 0, std::max<size_t>(count, 1) * sizeof(**ptr));
    };
    lcfg.assign(L, DevCfg{}); lbuf.assign(L, DevBuf{}); wraw.assign(L, nullptr);
    const size_t nBR = (size_t)BR, S2 = 2 * nBR, nB = (size_t)B, N = (size_t)d.NMAX;
    for (int l = 0; l < L; ++l) {
      OrbdLevel& v = od.lv[l];
      v.rows = plan.rows[l]; v.cols = plan.cols[l]; v.stride = (v.cols + 63) & ~63; v.quota = plan.quota[l]; v.sc = plan.scale[l];
      // corners that survive the strict 3 x 3 maximum never touch: one per 2 x 2 block at most; 65535 is the detector's own bound
      v.nmax = (int32_t)std::max<size_t>(64, std::min<size_t>(65535, (size_t)((v.rows + 1) / 2) * ((v.cols + 1) / 2)));
      vslam_config lc = d.c;
      lc.rows = v.rows; lc.cols = v.cols; lc.det_rows = 1; lc.det_cols = 1; lc.max_keypoints = v.nmax;
      lc.descriptor_type = VSLAM_DESCRIPTOR_ORB;      // no box image at the levels
      derive_cfg(lc, BR, &lcfg[l]);
      lcfg[l].mono = 1;
      DevBuf& lb = lbuf[l];
      std::memset(&lb, 0, sizeof lb);
      const DevCfg& c = lcfg[l];
      const size_t n = (size_t)v.nmax;
      A(&v.pyr, nBR * v.rows * v.stride);
      A(&lb.score8, S2 * v.rows * c.bstride); A(&lb.mask, S2 * v.rows * c.TX); A(&lb.kp_xy, S2 * n * 2); A(&lb.kp_score, S2 * n); A(&lb.n_kp, S2);
      A(&lb.rowcell, S2 * v.rows * (c.CW + 1)); A(&lb.used, S2 * n); A(&lb.iinfo, nBR); A(&lb.st, nBR);
      lb.img[0] = lb.img[1] = v.pyr; lb.img_row_stride = v.stride; lb.img_stream_stride = (size_t)v.rows * v.stride;
      v.kp_xy = lb.kp_xy; v.kp_score = lb.kp_score; v.n_kp = lb.n_kp; v.st = lb.st;
      A(&v.xy1, nBR * n * 2); A(&v.xy2, nBR * n * 2); A(&v.r1, nBR * n); A(&v.rh, nBR * n); A(&v.r2, nBR * n); A(&v.n1, nBR); A(&v.n2, nBR);
      v.wrows = l ? whole.rows[l] : p.rows; v.wcols = l ? whole.cols[l] : p.cols; v.wstride = (v.wcols + 63) & ~63;
      if (orb_ext && l > 0) {
        if (walias) wraw[l] = v.pyr;
        else A(&wraw[l], nB * v.wrows * v.wstride);
        uint8_t* blur = nullptr;
        A(&blur, nB * v.wrows * v.wstride);
        v.wblur = blur;
      }
    }
    A(&od.base, nB * (size_t)(R * L + 1)); A(&od.n_new, nB); A(&od.kp, nB * N * 4); A(&od.keep, nB * N); A(&od.kdesc, nB * N * 32);
    A(&od.v_key, nB * N); A(&od.v_vp, nB * N); A(&od.v_lvl, nB * N); A(&od.v_fxy, nB * N * 2); A(&od.v_desc, nB * N * 32); A(&od.s_key, nB * N);
    A(&od.bucket, nB * N); A(&od.row_start, nB * (size_t)(p.rows + 1)); A(&od.row_fill, nB * (size_t)(p.rows + 1));
    A(&rb.fkxy, nB * N * 2); A(&rb.flvl, nB * N);
    A(&d_od, 1);
    if (e == hipSuccess) e = hipMemcpy(d_od, &od, sizeof od, hipMemcpyHostToDevice);
    if (e != hipSuccess) { err = std::string("RGB-D mode, detector_type ORB: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
    orbdet = true;
    return VSLAM_OK;
  }
  void enqueue_orb_detect(const DevBuf& b, bool again) {
    const DevCfg& d = ic->cfg;
    const int R = od.R, L = od.L, BR = B * R;
    uint32_t act[VS_MAX_STREAMS / 32];
    std::memset(act, 0, sizeof act);
    for (int s = 0; s < B; ++s)
      if ((b.active[s >> 5] >> (s & 31)) & 1u) for (int r = 0; r < R; ++r) { const int z = s * R + r; act[z >> 5] |= 1u << (z & 31); }
    const OrbdLevel& l0 = od.lv[0];
    hipLaunchKernelGGL(k_orbd_begin, dim3((l0.cols + 255) / 256, l0.rows, BR), dim3(256), 0, q, d, b, d_od);
    for (int l = 1; l < L; ++l) {
      const OrbdLevel& u = od.lv[l - 1]; const OrbdLevel& v = od.lv[l];
      hipLaunchKernelGGL(k_orbd_resize, dim3((v.cols + 255) / 256, v.rows, BR), dim3(256), 0, q, b, R, u.pyr, u.rows, u.cols, u.stride, (size_t)u.rows * u.stride,
                         v.pyr, v.rows, v.cols, v.stride, (size_t)v.rows * v.stride);
    }
    for (int l = 0; l < L; ++l) {
      std::memcpy(lbuf[l].active, act, sizeof act);
      hipLaunchKernelGGL(k_fast_box, dim3(lcfg[l].TX, (lcfg[l].c.rows + VS_TILE_H - 1) / VS_TILE_H, BR), dim3(256), VS_FB_DYN_LDS, q, lcfg[l], lbuf[l]);
      launch_emit(q, lcfg[l], lbuf[l], BR, 1, (int)VS_ORBD_EDGE, 0);        // runByImageBorder(edgeThreshold)
    }
    hipLaunchKernelGGL(k_orbd_select_fast, dim3(BR, L), dim3(1024), 0, q, b, d_od);
    const int gk = std::max(4, std::min(64, 8192 / (BR * L)));       // blocks of four wavefronts per (sequence, region, level) list
    hipLaunchKernelGGL(k_orbd_harris, dim3(gk, BR, L), dim3(256), 0, q, b, d_od);
    hipLaunchKernelGGL(k_orbd_select_harris, dim3(BR, L), dim3(1024), 0, q, b, d_od);
    hipLaunchKernelGGL(k_orbd_control, dim3(B), dim3(64), 0, q, d, b, d_od);
    hipLaunchKernelGGL(k_orbd_angle, dim3(gk, BR, L), dim3(256), 0, q, b, d_od);
    const dim3 g1(d.TX, (d.c.rows + VS_TILE_H - 1) / VS_TILE_H, B);
    const dim3 gd(std::max(4, std::min(64, 1024 / B)), B);
    if (p.descriptor_type == VSLAM_DESCRIPTOR_ORB) {
      Gauss7 g7; for (int i = 0; i < 4; ++i) g7.k[i] = d.gauss7[i];
      hipLaunchKernelGGL(k_gauss7, g1, dim3(256), 0, q, d, b, g7);          // level 0's Gaussian: the image the recovery samples as well
      const uint8_t* src = b.img[0]; int srows = d.c.rows, scols = d.c.cols, sstride = b.img_row_stride; size_t sstream = b.img_stream_stride;
      for (int l = 1; l < L; ++l) {
        const OrbdLevel& v = od.lv[l];
        const size_t ws = (size_t)v.wrows * v.wstride;
        if (!walias) hipLaunchKernelGGL(k_orbd_resize, dim3((v.wcols + 255) / 256, v.wrows, B), dim3(256), 0, q, b, 1, src, srows, scols, sstride, sstream, wraw[l], v.wrows, v.wcols, v.wstride, ws);
        hipLaunchKernelGGL(k_orbd_gauss7, dim3((v.wcols + VS_TILE_W - 1) / VS_TILE_W, (v.wrows + VS_TILE_H - 1) / VS_TILE_H, B), dim3(256), 0, q, b, (const uint8_t*)wraw[l], v.wstride,
                           v.wrows, v.wcols, ws, g7, const_cast<uint8_t*>(v.wblur), v.wstride, ws);
        src = wraw[l]; srows = v.wrows; scols = v.wcols; sstride = v.wstride; sstream = ws;
      }
      hipLaunchKernelGGL(k_orbd_describe, gd, dim3(256), 0, q, d, b, d_od);
    } else {
      hipLaunchKernelGGL(k_fast_box, g1, dim3(256), VS_FB_DYN_LDS, q, d, b);       // the whole frame's box image (BRIEF here, and at the recovery)
      hipLaunchKernelGGL(k_orbd_brief, gd, dim3(256), 0, q, d, b, d_od);
    }
    hipLaunchKernelGGL(k_orbd_install, dim3(B), dim3(1024), 0, q, d, b, rb, d_od, again ? 1 : 0);
  }
  void enqueue_tail(const DevBuf& b) {
    const DevCfg& d = ic->cfg;
    hipLaunchKernelGGL(k_rgbd_prune, dim3(B), dim3(wg1), 0, q, d, b, rb);
    hipLaunchKernelGGL(k_rgbd_describe_at, dim3(std::max(4, std::min(64, 1024 / B)), B), dim3(256), 0, q, d, b, rb);
    hipLaunchKernelGGL(k_rgbd_recover_finish, dim3(B), dim3(wg1), 0, q, d, rb);
    // 99 KB of LDS per workgroup: one per CU.  One sequence: a workgroup per 32 framepoints; many: a few workgroups per sequence that loop
    const int lm_gx = std::max(2, std::min((d.MAXP + RGBD_LM_PTS - 1) / RGBD_LM_PTS, 256 / B));
    hipLaunchKernelGGL(k_rgbd_landmarks, dim3(lm_gx, B), dim3(256), 0, q, d, rb);
    hipLaunchKernelGGL(k_rgbd_finish, dim3(B), dim3(wg1), 0, q, d, b, rb);
    // opt-in: ids, map rows and log entries of the frame k_rgbd_finish has just closed, ahead of the state block's copy out (it raises the
    // capacity bits in the frame's report); skips itself like the rest of the tail, and serves a frame once however many attempts it took
    if (mp.cap) hipLaunchKernelGGL(k_rgbd_map_commit, dim3(B), dim3(VS_RGBD_MAP_WG), 0, q, rb, mp);
    // opt-in: the colour of every entry the commit has just written, on the same queue directly behind it, once per frame like it
    if (mc.rgb) hipLaunchKernelGGL(k_rgbd_map_color, dim3(B), dim3(VS_MAP_COLOR_WG), 0, q, rb, mp, map_color_src(), mc);
  }

  int submit_frame(const uint8_t* left, int32_t lstride, const uint16_t* depth, int32_t dstride, size_t lss, size_t dss, bool on_device) {
    (void)hipSetDevice(ic->device);
    const int rows = in_rows(), cols = in_cols();      // of the frames that come in: raw ones while the undistortion maps are set
    src_on_device = on_device;
    if (on_device) {
      use_graph = false;                       // the captured graph holds the staging buffers' addresses
      if (const int mrc = frame_masks_prepare()) return mrc;
      bs = buf_set(ic, 0, 0);
      // the first stage that is on (k_gray_u8, else the undistortion, else the equalisation) alone reads the caller's image
      if (const hipError_t ce = route_frame({{left, nullptr}, lstride, lss}, false)) return hip_fail(ce, "grey image");
      if (ds.factor > 1) {                     // k_downscale_depth_u16 is the only reader of the caller's depth images
        full_dep = depth; full_dep_stride = dstride; full_dep_stream = dss;
        raw_dep = und.raw_depth; raw_dep_stride = red_cols(); raw_dep_stream = (size_t)red_rows() * red_cols();
        depth_src = d_depth; depth_src_stride = p.cols;
      } else if (und.on) {                     // k_undistort_depth is the only reader of the caller's depth images
        raw_dep = depth; raw_dep_stride = dstride; raw_dep_stream = dss;
        depth_src = d_depth; depth_src_stride = p.cols;
      } else {
        depth_src = depth; depth_src_stride = dstride;
      }
      active_all(bs.active, B);
      enqueue_first_attempt(false);
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipMemcpyAsync(pinned, rb.st, sizeof(RgbdState) * (size_t)B, hipMemcpyDeviceToHost, q);
      if (e != hipSuccess) { ic->sticky = VSLAM_ERR_HIP; return hip_fail(e, "RGB-D frame"); }
      return VSLAM_OK;
    }
    depth_src = d_depth; depth_src_stride = p.cols;
    uint16_t* const depth_up = ds.factor > 1 ? ds.full_depth : und.on ? und.raw_depth : d_depth;     // where the depth images are copied to, re-packed
    // inputs: the caller's row stride kept on the device for the image, the depth image re-packed
    const size_t ib = (size_t)(rows - 1) * lstride + in_bytes();           // bytes of one image the caller owns
    // device bytes per sequence: the caller's own stream stride when the images lie in one (nearly) dense block — then ONE copy brings all of
    // them in (a pageable copy costs ~40 us of host time whatever its size: 128 sequences are 10 ms of copies one by one, 0.6 ms as a block)
    const bool dense = B > 1 && lss >= (size_t)rows * lstride && lss <= (size_t)rows * lstride + 4096;
    const size_t need = dense ? lss : (((size_t)rows * lstride + 255) & ~(size_t)255);
    if (need != img_stream || !d_img) {
      (void)hipStreamSynchronize(q);
      if (d_img) (void)hipFree(d_img);
      d_img = nullptr; img_stream = 0;
      drop_graph();                            // it holds the old buffer and its stream stride
      const hipError_t e = hipMalloc((void**)&d_img, need * (size_t)B + 64);
      if (e != hipSuccess) return hip_fail(e, "image buffer");
      img_stream = need;
    }
    hipError_t e = hipSuccess;
    // the depth images go in on the second stream, beside the images' copy (replaying a captured graph: on the first, the graph forks itself)
    hipStream_t qd = use_graph ? q : q2;
    if (dense) e = hipMemcpyAsync(d_img, left, (size_t)(B - 1) * lss + ib, hipMemcpyHostToDevice, q);
    else for (int s = 0; s < B && e == hipSuccess; ++s) e = hipMemcpyAsync(d_img + (size_t)s * img_stream, left + (size_t)s * lss, ib, hipMemcpyHostToDevice, q);
    if (e == hipSuccess) {
      if (dstride == cols && (B == 1 || dss == (size_t)rows * cols)) e = hipMemcpyAsync(depth_up, depth, (size_t)B * rows * cols * 2, hipMemcpyHostToDevice, qd);
      else for (int s = 0; s < B && e == hipSuccess; ++s) {
        const uint16_t* dsrc = depth + (size_t)s * dss;
        uint16_t* ddst = depth_up + (size_t)s * rows * cols;
        if (dstride == cols) e = hipMemcpyAsync(ddst, dsrc, (size_t)rows * cols * 2, hipMemcpyHostToDevice, qd);
        else e = hipMemcpy2DAsync(ddst, (size_t)cols * 2, dsrc, (size_t)dstride * 2, (size_t)cols * 2, rows, hipMemcpyHostToDevice, qd);
      }
    }
    if (e != hipSuccess) return hip_fail(e, "image / depth upload");
    if (const int mrc = frame_masks_prepare()) return mrc;
    bs = buf_set(ic, 0, 0);
    if (const hipError_t ce = route_frame({{d_img, nullptr}, lstride, img_stream}, true)) return hip_fail(ce, "grey image");
    if (ds.factor > 1) { full_dep = ds.full_depth; full_dep_stride = cols; full_dep_stream = (size_t)rows * cols; }
    if (und.on) { raw_dep = und.raw_depth; raw_dep_stride = red_cols(); raw_dep_stream = (size_t)red_rows() * red_cols(); }
    active_all(bs.active, B);
    if (use_graph && (!graph_exec || graph_stride != lstride || graph_img != d_img || graph_fm != dmask.fm_frame)) capture_graph(lstride);
    if (use_graph && graph_exec) {
      e = hipGraphLaunch(graph_exec, q);
      if (e != hipSuccess) { ic->sticky = VSLAM_ERR_HIP; return hip_fail(e, "RGB-D frame (graph launch)"); }
      return VSLAM_OK;
    }
    enqueue_first_attempt(false);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(pinned, rb.st, sizeof(RgbdState) * (size_t)B, hipMemcpyDeviceToHost, q);
    if (e != hipSuccess) { ic->sticky = VSLAM_ERR_HIP; return hip_fail(e, "RGB-D frame"); }
    return VSLAM_OK;
  }

  // everything of a frame's first attempt after the uploads: frame scalars, the space maps on q2 beside the image pipeline, registration, tail
  void enqueue_first_attempt(bool fork) {
    const int rows = p.rows, cols = p.cols;
    hipLaunchKernelGGL(k_rgbd_begin, dim3(B), dim3(64), 0, q, rb);
    // _computeDepthMap (once per frame: every initialize() of the frame sees the same depth image) on the second stream, joined before the
    // first reader of the map (the candidate kernel)
    if (fork) { (void)hipEventRecord(ev_fork, q); (void)hipStreamWaitEvent(q2, ev_fork, 0); }     // inside a capture: q2 joins the graph here
    const float f0 = (float)p.maximum_depth_meters;
    uint32_t f0_bits;
    std::memcpy(&f0_bits, &f0, 4);
    const dim3 grid((cols + 255) / 256, rows, B);
    if (src_on_device) { (void)hipEventRecord(ev_fork, q); (void)hipStreamWaitEvent(q2, ev_fork, 0); }   // device images: whatever wrote them was ordered before q
    // full-size depth -> reduced depth on the space map's queue, behind the depth upload and ahead of the undistortion: into the raw depth
    // images while undistorting, else into d_depth
    if (ds.factor > 1) {
      DownscaleDepthArgs da{};
      da.src = full_dep; da.src_stream_stride = full_dep_stream; da.src_row_stride = full_dep_stride;
      da.rows = red_rows(); da.cols = red_cols(); da.n = B; da.factor = ds.factor;
      da.dst = und.on ? und.raw_depth : d_depth; da.dst_row_stride = da.cols; da.dst_stream_stride = (size_t)da.rows * da.cols;
      (void)downscale_depth_enqueue(q2, da);
    }
    // raw depth -> undistorted depth on the space map's queue, behind the depth upload and ahead of the map's first kernel
    if (und.on) {
      UndistortDepthArgs ua{};
      ua.src = raw_dep; ua.src_stream_stride = raw_dep_stream; ua.src_row_stride = raw_dep_stride; ua.src_rows = und.maps.raw_rows; ua.src_cols = und.maps.raw_cols;
      ua.map_xy = und.maps.xy[0]; ua.map_a = und.maps.a[0]; ua.map_stride = und.maps.stride;
      ua.dst = d_depth; ua.dst_stream_stride = (size_t)rows * cols; ua.dst_row_stride = cols; ua.rows = rows; ua.cols = cols; ua.n = B;
      hipLaunchKernelGGL(k_undistort_depth, undistort_grid(rows, cols, B), dim3(256), 0, q2, ua);
    }
    // the depth image's bilateral filter behind it: range, table and filter into bl.depth, which the map's kernels read from here on
    // (dense images: a batch's stream stride is rows * row stride on either source)
    if (bl.on) {
      BilateralArgs ba = bl.args;
      ba.src = depth_src; ba.src_row_stride = depth_src_stride; ba.src_stream_stride = (size_t)rows * depth_src_stride;
      bilateral_enqueue(q2, ba);
      depth_src = bl.depth; depth_src_stride = cols;
    }
    // pinhole matrices, identity offset: one direct pass; the general three passes stay enqueued behind it and skip every image whose depth
    // pixels all landed on themselves (k_depth_direct checks that and raises rb.cross[image] otherwise)
    const int32_t* gate = nullptr;
    if (depth_plain) {
      if (force_cross) (void)hipMemsetAsync(rb.cross, 1, sizeof(int32_t) * (size_t)B, q2);     // test switch: the general passes run behind the direct one
      const dim3 dgrid((cols + 255) / 256, std::min(rows, std::max(8, 4096 / B)), B);      // one sequence: a workgroup per row segment; many: workgroups walk down their strip
      hipLaunchKernelGGL(k_depth_direct, dgrid, dim3(256), 0, q2, p, depth_src, depth_src_stride, f0_bits, rb.space, rb.row_map, rb.col_map, rb.cross);
      gate = rb.cross;
    }
    const dim3 ggrid((cols + 255) / 256, gate ? std::min(rows, 4) : rows, B);     // gated: a token grid (the kernels loop over the rows); it almost never has work
    hipLaunchKernelGGL(k_depth_min, ggrid, dim3(256), 0, q2, p, depth_src, depth_src_stride, rb.dkey, gate);
    hipLaunchKernelGGL(k_depth_pick, ggrid, dim3(256), 0, q2, p, depth_src, depth_src_stride, f0_bits, rb.dkey, rb.dlast, gate);
    hipLaunchKernelGGL(k_depth_write, ggrid, dim3(256), 0, q2, p, depth_src, depth_src_stride, f0_bits, rb.dkey, rb.dlast, rb.space, rb.row_map, rb.col_map, 1, gate);   // leaves the z-buffer initialised for the next frame
    (void)hipEventRecord(ev_depth, q2);
    depth_pending = true;
    // raw image -> undistorted image on the image pipeline's queue, ahead of the detector and behind the fork, so that the space map's
    // queue does not wait for it (once per frame: further attempts read the undistorted image again)
    // colour -> grey at the head of the image queue's work, once per frame, behind the fork like the undistortion; the image equalised
    // behind the undistortion and ahead of the detector, once per frame like it
    (void)prestage_enqueue(q, pre, und.maps, eq, B, 1, bs.active);
    enqueue_attempt(bs);
    enqueue_tail(bs);
  }

  void drop_graph() {
    if (graph_exec) { (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
    if (graph) { (void)hipGraphDestroy(graph); graph = nullptr; }
  }
  // stream capture of enqueue_first_attempt + the state block's copy out; any failure leaves the direct launches in charge
  void capture_graph(int32_t lstride) {
    drop_graph();
    (void)hipStreamSynchronize(q);
    hipError_t e = hipStreamBeginCapture(q, hipStreamCaptureModeRelaxed);
    if (e != hipSuccess) { (void)hipGetLastError(); use_graph = false; return; }
    enqueue_first_attempt(true);
    (void)hipMemcpyAsync(pinned, rb.st, sizeof(RgbdState) * (size_t)B, hipMemcpyDeviceToHost, q);
    e = hipStreamEndCapture(q, &graph);
    depth_pending = false;
    if (e == hipSuccess) e = hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess || !graph_exec) { (void)hipGetLastError(); drop_graph(); use_graph = false; return; }
    graph_stride = lstride; graph_img = d_img; graph_fm = dmask.fm_frame;
  }

  int finish_frame() {
    (void)hipSetDevice(ic->device);
    hipError_t e = hipSuccess;
    bool all_done = false;
    for (int attempt = 0; attempt < 3 && !all_done; ++attempt) {
      if (attempt) {
        // some sequence's registration asked for another attempt: initialize() .. aligner .. tail once more, for those sequences only (the
        // others' detector thresholds and features must not move: their bits in the activity mask are cleared)
        DevBuf b2 = bs;
        std::memset(b2.active, 0, sizeof b2.active);
        for (int s = 0; s < B; ++s) if (!hosts[s].tail_done) b2.active[s >> 5] |= 1u << (s & 31);
        enqueue_attempt(b2, true);
        enqueue_tail(b2);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(pinned, rb.st, sizeof(RgbdState) * (size_t)B, hipMemcpyDeviceToHost, q);
      }
      if (e == hipSuccess) e = hipStreamSynchronize(q);
      if (e != hipSuccess) { ic->sticky = VSLAM_ERR_HIP; return hip_fail(e, "RGB-D frame"); }
      all_done = true;
      for (int s = 0; s < B; ++s) { hosts[s] = pinned[s]; all_done = all_done && hosts[s].tail_done; }
    }
    host = hosts[0];
    if (!all_done) { err = "RGB-D frame: registration did not finish in three attempts"; return VSLAM_ERR_STATE; }
    // bit 0: more corners than max_keypoints (k_emit), bit 1: more points than max_points — results would be truncated: the frame fails.
    // bit 2 (a track longer than the history ring: its oldest measurements are left out of the landmark refinement) is reported in
    // vslam_frame_info::error_flags only, like the stereo tracker does.
    for (int s = 0; s < B; ++s)
      if (hosts[s].error_flags & 3) {
        err = std::string("RGB-D frame: capacity exceeded (") + ((hosts[s].error_flags & 1) ? "max_keypoints " : "") + ((hosts[s].error_flags & 2) ? "max_points" : "") + ")" +
              (B > 1 ? " in sequence " + std::to_string(s) : std::string());
        return VSLAM_ERR_CAPACITY;
      }
    return VSLAM_OK;
  }
};

}  // namespace vs_rgbd
