// host_readback.h — what a caller reads back from a context: frame results, the landmark map and the observation log (with their
// switches), tracker and aligner results, poses, timers.  Every getter of a stream starts with check_stream (host_ctx.h): the pending
// setters are flushed and both queues have drained.  Host code, included by vslam_hip.hip after host_frame.h.
#pragma once

template <typename T>
static hipError_t d2h(vslam_ctx* c, T* dst, const T* src, size_t count) {
  if (!dst || !count) return hipSuccess;
  return hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, c->stream);
}
// stream s's StreamState as the frame queue left it
static int fetch_state(vslam_ctx* c, int s, StreamState* st) {
  HIP_TRY(c, d2h(c, st, c->buf.st + s, 1));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return VSLAM_OK;
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
  rc = fetch_state(c, s, &st);
  if (rc) return rc;
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
  DeviceStore& m = c->map.mem;
  hipError_t e = m.alloc_fill(&d.xyz, n * 3, 0, c->stream);
  if (e == hipSuccess) e = m.alloc_fill(&d.info, n * 3, 0, c->stream);
  if (e == hipSuccess) e = m.alloc_fill(&d.desc, n * 32, 0, c->stream);
  if (e == hipSuccess) e = m.alloc_fill(&d.count, B, 0, c->stream);
  if (e == hipSuccess) e = m.alloc_fill(&d.ids, 2 * B * (size_t)c->cfg.MAXP, 0xff, c->stream);
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
// ---- the map's colours (kernels_map_color.h) --------------------------------------------------------
VS_API int vslam_enable_map_colors(vslam_ctx* c, int on) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_enable_map_colors called inside a frame");
  if (on && !c->map.cap) return fail(c, VSLAM_ERR_STATE, "vslam_enable_map_colors needs the landmark map (vslam_enable_map): colours are indexed by its ids");
  if (on && c->col.format == VSLAM_PIXEL_GRAY8) return fail(c, VSLAM_ERR_STATE, "vslam_enable_map_colors needs colour input (vslam_set_color_input)");
  if ((on != 0) == (c->mapcol.rgb != nullptr)) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                        // no frame may still be writing the old store
  mapcol_free(c);
  if (!on) return VSLAM_OK;
  uint32_t* rgb = nullptr;
  hipError_t e = c->mapcol.mem.alloc_fill(&rgb, (size_t)c->B * (size_t)c->map.cap, 0, c->stream);     // (0, 0, 0) until an entry's next update
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { mapcol_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_enable_map_colors: ") + hipGetErrorString(e)); }
  c->mapcol.rgb = rgb;
  return VSLAM_OK;
}
VS_API int vslam_get_map_colors(vslam_ctx* c, int s, int32_t first_id, int32_t cap, int32_t* n, uint8_t* rgb) {
  if (c && (!n || first_id < 0 || cap < 0)) return fail(c, VSLAM_ERR_INVALID, "vslam_get_map_colors: null count, negative first id or capacity");
  int32_t size = 0;
  int rc = map_size(c, s, &size);
  if (rc) return rc;
  if (!c->mapcol.rgb) return fail(c, VSLAM_ERR_STATE, "the map's colours are not enabled (vslam_enable_map_colors)");
  const int32_t cnt = std::max(0, std::min(cap, size - first_id));
  *n = cnt;
  if (!cnt || !rgb) return VSLAM_OK;
  std::vector<uint32_t> w((size_t)cnt);
  HIP_TRY(c, d2h(c, w.data(), c->mapcol.rgb + (size_t)s * c->map.cap + (size_t)first_id, (size_t)cnt));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int32_t i = 0; i < cnt; ++i) { rgb[3 * i] = (uint8_t)w[i]; rgb[3 * i + 1] = (uint8_t)(w[i] >> 8); rgb[3 * i + 2] = (uint8_t)(w[i] >> 16); }
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
  hipError_t e = c->obs.mem.alloc_fill(&d.log, B * (size_t)cap, 0, c->stream);
  if (e == hipSuccess) e = c->obs.mem.alloc_fill(&d.count, B, 0, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { obs_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_enable_observations: ") + hipGetErrorString(e)); }
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
  rc = fetch_state(c, s, &st);
  if (rc) return rc;
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
  rc = fetch_state(c, s, &st);
  if (rc) return rc;
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
  rc = fetch_state(c, s, &st);
  if (rc) return rc;
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
  rc = fetch_state(c, s, &st);
  if (rc) return rc;
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
VS_API int vslam_copy_current_poses_device(vslam_ctx* c, double* dst) {
  if (!c || !dst) return VSLAM_ERR_INVALID;
  { int rc = flush_pending(c); if (rc) return rc; }
  hipLaunchKernelGGL(k_gather_poses, dim3((c->B * 12 + 255) / 256), dim3(256), 0, c->stream, buf_set(c, c->last_set), c->B, dst);
  HIP_TRY(c, hipGetLastError());
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
