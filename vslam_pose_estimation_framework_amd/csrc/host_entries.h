// host_entries.h — the stand-alone component entries of the C ABI: one piece of the pipeline on caller data (known-answer and random-size
// tests, the host-driven RGB-D loop of rgbd_tracker.h).  Host code only, included by vslam_hip.hip once the context, the per-call arena
// (tmp_get / tmp_reset), the scratch-context pool and the frame path's upload helpers are defined.  Every entry is the same five steps:
// entry_begin + argument checks, device scratch and uploads through a Call, launches, read-back, Call::finish.
#pragma once

// ---- per-call staging -----------------------------------------------------------------------------------------------
// Device scratch from the arena of context c, copies on ONE stream (often a scratch context's, hence a parameter), and the first
// hipError_t of the call: after a failure every later operation does nothing, so an entry is written without error plumbing and asks
// once, in finish().  Launches stay with the entry, behind `if (k.ok())`.
struct Call {
  vslam_ctx* c; hipStream_t st; hipError_t e = hipSuccess;
  Call(vslam_ctx* c_, hipStream_t st_) : c(c_), st(st_) {}
  bool ok() const { return e == hipSuccess; }
  void note(hipError_t x) { if (ok()) e = x; }
  template <typename T> T* dev(size_t count) {                          // arena memory; a zero count still yields a valid pointer
    void* p = nullptr;
    if (ok()) e = tmp_get(c, &p, count * sizeof(T));
    return (T*)p;
  }
  template <typename T> void up_to(T* dst, const T* host, size_t count) { if (ok() && count) e = hipMemcpyAsync(dst, host, count * sizeof(T), hipMemcpyHostToDevice, st); }
  template <typename T> T* up(const T* host, size_t count) { T* p = dev<T>(count); up_to(p, host, count); return p; }
  template <typename T> void down(T* host, const T* dev, size_t count) { if (ok() && count) e = hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, st); }
  // blocking copy of results whose count is known only after finish()
  template <typename T> void fetch(T* host, const T* dev, size_t count) { if (ok() && count) e = hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost); }
  void launched() { if (ok()) e = hipGetLastError(); }
  int status() { return ok() ? VSLAM_OK : fail(c, VSLAM_ERR_HIP, hipGetErrorString(e)); }
  int finish() {                                                        // host staging buffers may go out of scope after this
    launched();
    if (ok()) e = hipStreamSynchronize(st);
    return status();
  }
};
// start of every stand-alone entry; argument checks follow it, per entry
static int entry_begin(vslam_ctx* c) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->sticky != VSLAM_OK) return c->sticky;
  HIP_TRY(c, hipSetDevice(c->device));
  tmp_reset(c);
  return VSLAM_OK;
}

// ---- shared host pieces ---------------------------------------------------------------------------------------------
static int make_scratch_ctx(vslam_ctx* parent, int rows, int cols, int nmax, int maxp, vslam_ctx** out) {
  vslam_config cfg = parent->cfg.c;
  cfg.rows = rows; cfg.cols = cols; cfg.det_rows = 1; cfg.det_cols = 1;
  cfg.descriptor_type = VSLAM_DESCRIPTOR_BRIEF;   // the stand-alone FAST / BRIEF entries need the box image whatever the parent uses
  cfg.max_keypoints = std::max(64, nmax); cfg.max_points = std::max(64, maxp); cfg.max_history_frames = 2;
  return scratch_get(parent, cfg, out);
}
// k_fast_box of scratch context t on its current images (`sides` of them)
static void launch_fast_box(vslam_ctx* t, hipStream_t stream, int sides) {
  hipLaunchKernelGGL(k_fast_box, dim3(t->cfg.TX, (t->cfg.c.rows + VS_TILE_H - 1) / VS_TILE_H, sides), dim3(256), VS_FB_DYN_LDS, stream, t->cfg, t->buf);
}
static Gauss7 gauss7_of(const DevCfg& cfg) {
  Gauss7 gk;
  for (int i = 0; i < 4; ++i) gk.k[i] = cfg.gauss7[i];
  return gk;
}
// read-modify-write of scratch context t's StreamState: copies queued on stream q with one synchronisation between them, or blocking copies
// when q is null.  `st` is the caller's: the write-back on q may still be reading it when this returns.
template <typename F>
static void edit_stream_state(Call& k, vslam_ctx* t, hipStream_t q, StreamState& st, F&& edit) {
  if (!q) k.fetch(&st, t->buf.st, 1);
  else {
    if (k.ok()) k.note(hipMemcpyAsync(&st, t->buf.st, sizeof st, hipMemcpyDeviceToHost, q));
    if (k.ok()) k.note(hipStreamSynchronize(q));
  }
  if (!k.ok()) return;
  edit(st);
  k.note(q ? hipMemcpyAsync(t->buf.st, &st, sizeof st, hipMemcpyHostToDevice, q) : hipMemcpy(t->buf.st, &st, sizeof st, hipMemcpyHostToDevice));
}
// features as the image pipeline leaves them (k_emit): row-major order — (row, column, caller index), so features that share a pixel keep
// their list order —, coordinates (x, y), descriptors, and the (row, 16-px cell) CSR with CW1 entries per row.  ord[k] = caller index of
// sorted feature k.  False: a feature lies outside the image.
struct SortedFeatures { std::vector<int> ord; std::vector<int16_t> xy; std::vector<uint8_t> desc; std::vector<int32_t> rowcell; };
static bool sort_features(const int32_t* rc, const uint8_t* desc, int n, int rows, int cols, int CW1, SortedFeatures& f) {
  f.ord.resize(n);
  for (int i = 0; i < n; ++i) {
    f.ord[i] = i;
    if (rc[2 * i] < 0 || rc[2 * i] >= rows || rc[2 * i + 1] < 0 || rc[2 * i + 1] >= cols) return false;
  }
  std::sort(f.ord.begin(), f.ord.end(), [&](int a, int b) { return rc[2 * a] != rc[2 * b] ? rc[2 * a] < rc[2 * b] : (rc[2 * a + 1] != rc[2 * b + 1] ? rc[2 * a + 1] < rc[2 * b + 1] : a < b); });
  f.xy.resize((size_t)n * 2); f.desc.resize((size_t)n * 32); f.rowcell.resize((size_t)rows * CW1);
  for (int k = 0; k < n; ++k) {
    f.xy[2 * k] = (int16_t)rc[2 * f.ord[k] + 1]; f.xy[2 * k + 1] = (int16_t)rc[2 * f.ord[k]];
    std::memcpy(&f.desc[(size_t)32 * k], desc + (size_t)32 * f.ord[k], 32);
  }
  for (int r = 0, k = 0; r < rows; ++r)
    for (int cc = 0; cc < CW1; ++cc) {
      while (k < n && (f.xy[2 * k + 1] < r || (f.xy[2 * k + 1] == r && f.xy[2 * k] < 16 * cc))) ++k;
      f.rowcell[(size_t)r * CW1 + cc] = k;
    }
  return true;
}

VS_API int vslam_aligner_weights(vslam_ctx* c, int32_t n_calls, const int32_t* n, const int32_t* inverse_depth, const double* depth, double* out) {
  if (int rc = entry_begin(c)) return rc;
  if (n_calls < 0 || (n_calls && (!n || !inverse_depth))) return fail(c, VSLAM_ERR_INVALID, "aligner_weights: bad argument");
  size_t total = 0; int nmax = 0;
  for (int k = 0; k < n_calls; ++k) { if (n[k] < 0) return fail(c, VSLAM_ERR_INVALID, "aligner_weights: negative size"); total += (size_t)n[k]; nmax = std::max(nmax, n[k]); }
  if (total && (!depth || !out)) return fail(c, VSLAM_ERR_INVALID, "aligner_weights: bad argument");
  if (!n_calls || !total) return VSLAM_OK;
  Call k(c, c->stream);
  int32_t* dn = k.up(n, n_calls); int32_t* di = k.up(inverse_depth, n_calls); double* dd = k.up(depth, total);
  double* dw = k.dev<double>(nmax); double* dout = k.dev<double>(total);
  if (k.ok()) hipLaunchKernelGGL(k_aligner_weights, dim3(1), dim3(256), 0, c->stream, n_calls, dn, di, dd, c->cfg.c.maximum_reliable_depth_meters, dw, dout);
  k.down(out, dout, total);
  return k.finish();
}
// ---- RGB-D components (DepthFramePointGenerator pieces, stand-alone) ------------------------------------------------
static int depth_params_ok(vslam_ctx* c, const vslam_depth_params* p) {
  if (!p || p->rows <= 0 || p->cols <= 0 || p->rows > 32767 || p->cols > 32767) return fail(c, VSLAM_ERR_INVALID, "depth: image size out of range");
  if (!(p->maximum_depth_meters > 0) || (p->enable_keypoint_binning && p->bin_size_pixels <= 0)) return fail(c, VSLAM_ERR_INVALID, "depth: bad parameters");
  return VSLAM_OK;
}
static bool depth_map_resident(const vslam_ctx* c, const vslam_depth_params* p) { return c->dm.valid && c->dm.rows == p->rows && c->dm.cols == p->cols; }
VS_API int vslam_depth_space_map(vslam_ctx* c, const vslam_depth_params* p, const uint16_t* depth, int32_t row_stride, float* space,
                                 int16_t* row_map, int16_t* col_map) {
  int rc = entry_begin(c);
  if (rc == VSLAM_OK) rc = depth_params_ok(c, p);
  if (rc != VSLAM_OK) return rc;
  if (!depth) return fail(c, VSLAM_ERR_INVALID, "depth tracker requires a 16bit mono image to encode depth");   // :411-413
  if (row_stride < p->cols) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than image width");
  vslam_ctx::DepthMap& m = c->dm;
  const size_t n = (size_t)p->rows * p->cols;
  const hipError_t em = depth_map_resize(c, p->rows, p->cols);
  if (em != hipSuccess) return fail(c, VSLAM_ERR_HIP, hipGetErrorString(em));
  m.valid = false;
  Call k(c, c->stream);
  // rows re-packed on the device side of the copy (dense device image, stride = cols)
  if (row_stride == p->cols) k.up_to(m.depth, depth, n);
  else k.note(hipMemcpy2DAsync(m.depth, (size_t)p->cols * 2, depth, (size_t)row_stride * 2, (size_t)p->cols * 2, p->rows, hipMemcpyHostToDevice, c->stream));
  const float f0 = (float)p->maximum_depth_meters;
  uint32_t f0_bits;
  std::memcpy(&f0_bits, &f0, 4);
  const dim3 grid((p->cols + 255) / 256, p->rows);
  if (k.ok()) {
    hipLaunchKernelGGL(k_depth_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (int)n, f0_bits, m.key, m.last);
    hipLaunchKernelGGL(k_depth_min, grid, dim3(256), 0, c->stream, *p, m.depth, p->cols, m.key, (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_depth_pick, grid, dim3(256), 0, c->stream, *p, m.depth, p->cols, f0_bits, m.key, m.last, (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_depth_write, grid, dim3(256), 0, c->stream, *p, m.depth, p->cols, f0_bits, m.key, m.last, m.space, m.row_map, m.col_map, 0, (const int32_t*)nullptr);
  }
  if (space) k.down(space, m.space, n * 3);
  if (row_map) k.down(row_map, m.row_map, n);
  if (col_map) k.down(col_map, m.col_map, n);
  rc = k.finish();
  m.valid = rc == VSLAM_OK;
  return rc;
}
VS_API int vslam_depth_compute(vslam_ctx* c, const vslam_depth_params* p, const float* space, int32_t nF, const int32_t* rcF, int32_t nT,
                               const int32_t* rcT, int32_t cap, int32_t* n_new, int32_t* new_feat, double* new_xyz, int32_t* n_temp,
                               int32_t* temp_feat, double* temp_xyz) {
  int rc = entry_begin(c);
  if (rc == VSLAM_OK) rc = depth_params_ok(c, p);
  if (rc != VSLAM_OK) return rc;
  if (nF < 0 || nT < 0 || cap < 0 || !n_new || !n_temp || (nF && !rcF) || (nT && !rcT) || (cap && (!new_feat || !new_xyz || !temp_feat || !temp_xyz)))
    return fail(c, VSLAM_ERR_INVALID, "depth_compute: bad argument");
  for (int i = 0; i < nF; ++i) if (rcF[2 * i] < 0 || rcF[2 * i] >= p->rows || rcF[2 * i + 1] < 0 || rcF[2 * i + 1] >= p->cols) return fail(c, VSLAM_ERR_INVALID, "depth_compute: feature outside the image");
  for (int i = 0; i < nT; ++i) if (rcT[2 * i] < 0 || rcT[2 * i] >= p->rows || rcT[2 * i + 1] < 0 || rcT[2 * i + 1] >= p->cols) return fail(c, VSLAM_ERR_INVALID, "depth_compute: point outside the image");
  if (!space && !depth_map_resident(c, p)) return fail(c, VSLAM_ERR_STATE, "depth_compute: no resident space map of this size");
  const size_t n = (size_t)p->rows * p->cols;
  const int rows_bin = p->enable_keypoint_binning ? p->rows / p->bin_size_pixels + 1 : 0;   // base_framepoint_generator.cpp:304-305
  const int cols_bin = p->enable_keypoint_binning ? p->cols / p->bin_size_pixels + 1 : 0;
  const int n_bins = (rows_bin + 1) * (cols_bin + 1);
  const size_t capa = std::max(cap, 1);
  Call k(c, c->stream);
  const float* dspace = space ? k.up(space, n * 3) : c->dm.space;
  int32_t* dF = k.up(rcF, (size_t)nF * 2); int32_t* dT = k.up(rcT, (size_t)nT * 2);
  int32_t* dcnt = k.dev<int32_t>(2); int32_t* dnf = k.dev<int32_t>(capa); int32_t* dtf = k.dev<int32_t>(capa);
  double* dnx = k.dev<double>(capa * 3); double* dtx = k.dev<double>(capa * 3);
  unsigned long long* dbins = k.dev<unsigned long long>(n_bins); uint8_t* dcls = k.dev<uint8_t>(nF);
  if (k.ok()) hipLaunchKernelGGL(k_depth_compute, dim3(1), dim3(1024), 0, c->stream, *p, dspace, nF, dF, nT, dT, dbins, n_bins, rows_bin, cols_bin, cap, dcnt, dnf, dnx, dtf, dtx, dcls);
  int32_t cnt[2] = {0, 0};
  k.down(cnt, dcnt, 2);
  if (k.finish() == VSLAM_OK) {
    *n_new = cnt[0]; *n_temp = cnt[1];
    const size_t a = std::min(cnt[0], cap), b = std::min(cnt[1], cap);
    k.fetch(new_feat, dnf, a); k.fetch(new_xyz, dnx, a * 3);
    k.fetch(temp_feat, dtf, b); k.fetch(temp_xyz, dtx, b * 3);
  }
  if (!k.ok()) return k.status();
  if (cnt[0] > cap || cnt[1] > cap) return fail(c, VSLAM_ERR_CAPACITY, "depth_compute: output capacity too small");
  return VSLAM_OK;
}
VS_API int vslam_depth_track(vslam_ctx* c, const vslam_depth_params* p, const float* space, const double T[12], int32_t d, double tau,
                             int32_t by_appearance, int32_t nP, const double* cam, const uint8_t* pdesc, const uint8_t* pflags, int32_t nL,
                             const int32_t* rcL, const uint8_t* dL, int32_t* n_tracked, int32_t* out2, double* xyz, int32_t* n_temp,
                             int32_t* temp2, int32_t* n_lost, int32_t* lost, int32_t* n_tracked_landmarks) {
  int rc = entry_begin(c);
  if (rc == VSLAM_OK) rc = depth_params_ok(c, p);
  if (rc != VSLAM_OK) return rc;
  if (!T || d < 0 || nP < 0 || nL < 0 || !n_tracked || !n_temp || !n_lost || !n_tracked_landmarks || (nP && (!cam || !pdesc || !pflags || !out2 || !xyz || !temp2 || !lost)) ||
      (nL && (!rcL || !dL)))
    return fail(c, VSLAM_ERR_INVALID, "depth_track: bad argument");
  if (!space && !depth_map_resident(c, p)) return fail(c, VSLAM_ERR_STATE, "depth_track: no resident space map of this size");
  const int rows = p->rows, cols = p->cols, CW = (cols + 15) / 16;
  // Several features on ONE pixel (an OrbDetector finds a corner on more than one pyramid level): setFeatures
  // (intensity_feature_matcher.cpp:48-70) writes them into the lattice in list order, so only the LAST one can ever be found through the
  // lattice — the others stay in the feature vector (compute() still sees them) but are invisible to track(), also after the last one has
  // been taken.
  SortedFeatures f;
  if (!sort_features(rcL, dL, nL, rows, cols, CW + 1, f)) return fail(c, VSLAM_ERR_INVALID, "feature outside the image");
  std::vector<uint8_t> vis(nL, 1);
  bool duplicates = false;
  for (int k = 0; k + 1 < nL; ++k)
    if (f.xy[2 * k] == f.xy[2 * k + 2] && f.xy[2 * k + 1] == f.xy[2 * k + 3]) { vis[k] = 0; duplicates = true; }
  const size_t n = (size_t)rows * cols, P1 = std::max(nP, 1), L1 = std::max(nL, 1);
  DepthTrack a;
  std::memset(&a, 0, sizeof a);
  a.p = *p; std::memcpy(a.T, T, sizeof a.T); a.d = d; a.by_app = by_appearance ? 1 : 0; a.tau = tau; a.nP = nP; a.nL = nL; a.CW = CW;
  Call k(c, c->stream);
  a.space = space ? k.up(space, n * 3) : c->dm.space;
  a.fvis = duplicates ? k.up(vis.data(), (size_t)nL) : nullptr;
  a.cam = k.up(cam, (size_t)nP * 3); a.pdesc = k.up(pdesc, (size_t)nP * 32); a.pflags = k.up(pflags, (size_t)nP);
  a.desc = k.up(f.desc.data(), (size_t)nL * 32); a.kxy = k.up(f.xy.data(), (size_t)nL * 2); a.rowcell = k.up(f.rowcell.data(), f.rowcell.size());
  a.cand = k.dev<unsigned long long>(P1 * (VS_DT_K + 1)); a.hold = k.dev<int32_t>(L1 * 2); a.pick = k.dev<int32_t>(P1); a.counts = k.dev<int32_t>(4);
  a.out2 = k.dev<int32_t>(P1 * 2); a.xyz = k.dev<double>(P1 * 3); a.temp2 = k.dev<int32_t>(P1 * 2); a.lost = k.dev<int32_t>(P1);
  if (k.ok()) {
    if (nP) hipLaunchKernelGGL(k_depth_track_candidates, dim3(std::min(1024, (nP + 15) / 16)), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_depth_track, dim3(1), dim3(1024), 0, c->stream, a);
  }
  int32_t cnt[4] = {0, 0, 0, 0};
  k.down(cnt, a.counts, 4);
  if (k.finish() == VSLAM_OK) {        // also: the host staging vectors may go out of scope now
    *n_tracked = cnt[0]; *n_temp = cnt[1]; *n_lost = cnt[2]; *n_tracked_landmarks = cnt[3];
    k.fetch(out2, a.out2, (size_t)cnt[0] * 2); k.fetch(xyz, a.xyz, (size_t)cnt[0] * 3);
    k.fetch(temp2, a.temp2, (size_t)cnt[1] * 2);
    k.fetch(lost, a.lost, (size_t)cnt[2]);
    for (int u = 0; u < cnt[0] && k.ok(); ++u) out2[2 * u + 1] = f.ord[out2[2 * u + 1]];     // back to the caller's feature numbering
    for (int u = 0; u < cnt[1] && k.ok(); ++u) temp2[2 * u + 1] = f.ord[temp2[2 * u + 1]];
  }
  return k.status();
}
VS_API int vslam_depth_recover(vslam_ctx* c, const vslam_depth_params* p, const float* space, const uint8_t* img, int32_t row_stride,
                               const double w2c[12], int32_t n, const uint8_t* has_lm, const double* lm, const uint8_t* pdesc, float kp_size,
                               double tau, int32_t* n_rec, int32_t* rec_index, float* rec_xy, uint8_t* rec_desc, double* rec_xyz) {
  int rc = entry_begin(c);
  if (rc == VSLAM_OK) rc = depth_params_ok(c, p);
  if (rc != VSLAM_OK) return rc;
  if (!img || !w2c || n < 0 || !n_rec || (n && (!has_lm || !lm || !pdesc || !rec_index || !rec_xy || !rec_desc || !rec_xyz)))
    return fail(c, VSLAM_ERR_INVALID, "depth_recover: bad argument");
  if (row_stride < p->cols) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than image width");
  if (!space && !depth_map_resident(c, p)) return fail(c, VSLAM_ERR_STATE, "depth_recover: no resident space map of this size");
  *n_rec = 0;
  if (n == 0) return VSLAM_OK;
  // box image of the left image through the image pipeline's own kernel (scratch context of the image size)
  vslam_ctx* t = nullptr;
  rc = make_scratch_ctx(c, p->rows, p->cols, 64, 64, &t);
  if (rc != VSLAM_OK) return rc;
  const size_t npx = (size_t)p->rows * p->cols, N = n;
  DepthRecover a;
  std::memset(&a, 0, sizeof a);
  a.p = *p; std::memcpy(a.w2c, w2c, sizeof a.w2c); a.kp_size = kp_size; a.tau = tau; a.n = n;
  hipStream_t q = t->stream_img;
  Call k(c, q);
  a.space = space ? k.up(space, npx * 3) : c->dm.space;
  a.has_lm = k.up(has_lm, N); a.lm = k.up(lm, N * 3); a.pdesc = k.up(pdesc, N * 32);
  a.kxy = k.dev<float>(N * 2); a.bxy = k.dev<int16_t>(N * 2); a.cell = k.dev<int32_t>(N); a.count = k.dev<int32_t>(1);
  uint8_t* dkeep = k.dev<uint8_t>(N); uint8_t* ddesc = k.dev<uint8_t>(N * 32);
  a.keep = dkeep; a.desc = ddesc;
  a.rec_index = k.dev<int32_t>(N); a.rec_xy = k.dev<float>(N * 2); a.rec_desc = k.dev<uint8_t>(N * 32); a.rec_xyz = k.dev<double>(N * 3);
  rc = k.ok() ? set_inputs(t, img, img, row_stride, 0, false) : k.status();
  if (rc == VSLAM_OK) {
    if (!space) (void)hipStreamSynchronize(c->stream);   // the resident map was written on the parent's stream
    hipLaunchKernelGGL(k_depth_recover_project, dim3((n + 255) / 256), dim3(256), 0, q, a);
    if (p->descriptor_type == VSLAM_DESCRIPTOR_ORB) {
      // cv::ORB::create() as extractor: Gaussian image (in the scratch context's box memory), steered tests at the rounded pixels
      uint8_t* dblur = reinterpret_cast<uint8_t*>(t->buf.box);
      hipLaunchKernelGGL(k_gauss7_plain, dim3((p->cols + VS_TILE_W - 1) / VS_TILE_W, (p->rows + VS_TILE_H - 1) / VS_TILE_H), dim3(256), 0, q,
                         t->buf.img[0], t->buf.img_row_stride, p->rows, p->cols, gauss7_of(t->cfg), dblur, t->cfg.bstride);
      hipLaunchKernelGGL(k_orb_at, dim3(std::min(64, (n + 3) / 4)), dim3(256), 0, q, dblur, t->cfg.bstride, p->rows, p->cols, n, a.bxy, t->cfg.orb_cos, t->cfg.orb_sin, dkeep, ddesc);
    } else {
      launch_fast_box(t, q, 2);
      hipLaunchKernelGGL(k_brief_at, dim3(std::min(64, (n + 3) / 4)), dim3(256), 0, q, t->buf.box, t->cfg.bstride, p->rows, p->cols, n, a.bxy, dkeep, ddesc);
    }
    hipLaunchKernelGGL(k_depth_recover_finish, dim3(1), dim3(1024), 0, q, a);
    int32_t cnt = 0;
    k.down(&cnt, a.count, 1);
    k.finish();
    k.fetch(rec_index, a.rec_index, (size_t)cnt); k.fetch(rec_xy, a.rec_xy, (size_t)cnt * 2);
    k.fetch(rec_desc, a.rec_desc, (size_t)cnt * 32); k.fetch(rec_xyz, a.rec_xyz, (size_t)cnt * 3);
    if (k.ok()) *n_rec = cnt;
    rc = k.status();
  }
  scratch_put(c, t);
  return rc;
}
VS_API int vslam_point_in_camera(vslam_ctx* c, int32_t n, const float* xp, const float* xc, const double T[12], const double K[9], double* out) {
  if (int rc = entry_begin(c)) return rc;
  if (n < 0 || !T || !K || (n && (!xp || !xc || !out))) return fail(c, VSLAM_ERR_INVALID, "point_in_camera: bad argument");
  if (n == 0) return VSLAM_OK;
  Call k(c, c->stream);
  float* dp = k.up(xp, (size_t)n * 2); float* dc = k.up(xc, (size_t)n * 2);
  double* dT = k.up(T, 12); double* dK = k.up(K, 9); double* dout = k.dev<double>((size_t)n * 3);
  if (k.ok()) hipLaunchKernelGGL(k_point_in_camera, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dp, dc, dT, dK, dout);
  k.down(out, dout, (size_t)n * 3);
  return k.finish();
}

// the CAMERA_ODOMETRY prior of the frame start (kernels_motion.h) on caller data
VS_API int vslam_motion_prior(vslam_ctx* c, int32_t n, const double* guess, const double* guess_previous, double* out) {
  if (int rc = entry_begin(c)) return rc;
  if (n < 0 || (n && (!guess || !guess_previous || !out))) return fail(c, VSLAM_ERR_INVALID, "motion_prior: bad argument");
  if (n == 0) return VSLAM_OK;
  Call k(c, c->stream);
  double* dg = k.up(guess, (size_t)n * 12); double* dp = k.up(guess_previous, (size_t)n * 12); double* dout = k.dev<double>((size_t)n * 12);
  if (k.ok()) hipLaunchKernelGGL(k_motion_prior_entry, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dg, dp, dout);
  k.down(out, dout, (size_t)n * 12);
  return k.finish();
}

VS_API int vslam_landmark_update(vslam_ctx* c, int32_t n, const int32_t* offsets, const int32_t* frame_of, int32_t n_frames, const double* w2c,
                                 const double* c2w, const double* cam, double* world, int32_t* updates) {
  if (int rc = entry_begin(c)) return rc;
  if (n < 0 || n_frames < 0 || (n && (!offsets || !world || !updates))) return fail(c, VSLAM_ERR_INVALID, "landmark_update: bad argument");
  if (n == 0) return VSLAM_OK;
  const int M = offsets[n];
  if (M < 0 || (M && (!frame_of || !w2c || !c2w || !cam))) return fail(c, VSLAM_ERR_INVALID, "landmark_update: bad argument");
  for (int i = 0; i < n; ++i) if (offsets[i] > offsets[i + 1] || offsets[i] < 0) return fail(c, VSLAM_ERR_INVALID, "landmark_update: offsets not ascending");
  for (int m = 0; m < M; ++m) if (frame_of[m] < 0 || frame_of[m] >= n_frames) return fail(c, VSLAM_ERR_INVALID, "landmark_update: frame index out of range");
  Call k(c, c->stream);
  int32_t* doff = k.up(offsets, (size_t)n + 1); int32_t* dfo = k.up(frame_of, (size_t)M); int32_t* dupd = k.up((const int32_t*)updates, (size_t)n);
  double* dw2c = k.up(w2c, (size_t)n_frames * 12); double* dc2w = k.up(c2w, (size_t)n_frames * 12);
  double* dcam = k.up(cam, (size_t)M * 3); double* dworld = k.up((const double*)world, (size_t)n * 3);
  if (k.ok())
    hipLaunchKernelGGL(k_landmark_update, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, doff, dfo, dw2c, dc2w, dcam, dworld, dupd,
                       c->cfg.c.landmark_maximum_number_of_iterations, c->cfg.c.landmark_maximum_error_squared_meters);
  k.down(world, dworld, (size_t)n * 3);
  k.down(updates, dupd, (size_t)n);
  return k.finish();
}

// ---- OrbDetector components ---------------------------------------------------------------------------------------
VS_API int vslam_resize_linear_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, uint8_t* dst, int32_t drows,
                                  int32_t dcols) {
  if (int rc = entry_begin(c)) return rc;
  if (!src || !dst || rows < 2 || cols < 2 || drows < 1 || dcols < 1 || row_stride < cols) return fail(c, VSLAM_ERR_INVALID, "resize: bad argument");
  Call k(c, c->stream);
  uint8_t* ds = k.dev<uint8_t>((size_t)rows * row_stride); uint8_t* dd = k.dev<uint8_t>((size_t)drows * dcols);
  k.up_to(ds, src, (size_t)(rows - 1) * row_stride + cols);
  if (k.ok()) hipLaunchKernelGGL(k_resize_linear_u8, dim3((dcols + 255) / 256, drows), dim3(256), 0, c->stream, ds, rows, cols, row_stride, dd, drows, dcols, dcols);
  k.down(dst, dd, (size_t)drows * dcols);
  return k.finish();
}
// k_undistort_depth stand-alone on a host image (beside vslam_remap_u8, the image's remap): nearest neighbour on the fixed-point maps
VS_API int vslam_remap_nearest_u16(vslam_ctx* c, const uint16_t* src, int32_t rows, int32_t cols, int32_t row_stride, const int16_t* map_xy,
                                   const uint16_t* map_a, int32_t drows, int32_t dcols, uint16_t* dst) {
  if (int rc = entry_begin(c)) return rc;
  if (!src || !dst || !map_xy || !map_a || rows < 1 || cols < 1 || rows > 32767 || cols > 32767 || row_stride < cols || drows < 1 || dcols < 1 ||
      (size_t)rows * (size_t)row_stride > 0x7fffffffu)
    return fail(c, VSLAM_ERR_INVALID, "remap: bad argument");
  if (!rect_maps_ok(map_a, (size_t)drows * dcols)) return fail(c, VSLAM_ERR_INVALID, "remap: interpolation table index >= 1024");
  const int ms = (dcols + 3) & ~3;
  std::vector<int16_t> pxy;
  std::vector<uint16_t> pa;
  rect_pad_maps(map_xy, map_a, drows, dcols, ms, pxy, pa);
  Call k(c, c->stream);
  uint16_t* ds = k.dev<uint16_t>((size_t)rows * row_stride); uint16_t* dd = k.dev<uint16_t>((size_t)drows * dcols);
  k.up_to(ds, src, (size_t)(rows - 1) * row_stride + cols);
  UndistortDepthArgs ua{};
  ua.src = ds; ua.src_row_stride = row_stride; ua.src_rows = rows; ua.src_cols = cols;
  ua.map_xy = k.up(pxy.data(), pxy.size()); ua.map_a = k.up(pa.data(), pa.size()); ua.map_stride = ms;
  ua.dst = dd; ua.dst_row_stride = dcols; ua.rows = drows; ua.cols = dcols; ua.n = 1;
  if (k.ok()) hipLaunchKernelGGL(k_undistort_depth, undistort_grid(drows, dcols, 1), dim3(256), 0, c->stream, ua);
  k.down(dst, dd, (size_t)drows * dcols);
  return k.finish();
}
static OrbUmax orb_umax_table(int half) {   // orb.cpp computeKeyPoints: row half-widths of the circular patch
  OrbUmax t;
  std::memset(&t, 0, sizeof t);
  const int vmax = (int)std::floor(half * std::sqrt(2.f) / 2 + 1), vmin = (int)std::ceil(half * std::sqrt(2.f) / 2);
  for (int v = 0; v <= vmax; ++v) t.v[v] = (int)std::lrint(std::sqrt((double)half * half - v * v));
  for (int v = half, v0 = 0; v >= vmin; --v) { while (t.v[v0] == t.v[v0 + 1]) ++v0; t.v[v] = v0; ++v0; }
  return t;
}
VS_API int vslam_harris_angle(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t row_stride, int32_t n, const int16_t* xy,
                              float* response, float* angle) {
  if (int rc = entry_begin(c)) return rc;
  if (!img || n < 0 || rows < 33 || cols < 33 || row_stride < cols || (n && (!xy || !response || !angle))) return fail(c, VSLAM_ERR_INVALID, "harris_angle: bad argument");
  for (int i = 0; i < n; ++i)
    if (xy[2 * i] < 16 || xy[2 * i + 1] < 16 || xy[2 * i] >= cols - 16 || xy[2 * i + 1] >= rows - 16) return fail(c, VSLAM_ERR_INVALID, "harris_angle: keypoint closer than 16 px to the border");
  if (n == 0) return VSLAM_OK;
  Call k(c, c->stream);
  uint8_t* di = k.dev<uint8_t>((size_t)rows * row_stride);
  k.up_to(di, img, (size_t)(rows - 1) * row_stride + cols);
  int16_t* dxy = k.up(xy, (size_t)n * 2); int32_t* dn = k.up(&n, 1);
  float* dr = k.dev<float>(n); float* da = k.dev<float>(n);
  if (k.ok()) {
    const int blocks = std::min(256, (n + 3) / 4);
    hipLaunchKernelGGL(k_orb_harris, dim3(blocks), dim3(256), 0, c->stream, di, row_stride, dn, dxy, dr);
    hipLaunchKernelGGL(k_orb_angle, dim3(blocks), dim3(256), 0, c->stream, di, row_stride, dn, dxy, dr, 15, orb_umax_table(15), da, (float*)nullptr,
                       (const int32_t*)nullptr, 0, 1.f, 0, 31);
  }
  k.down(response, dr, (size_t)n);
  k.down(angle, da, (size_t)n);
  return k.finish();
}
VS_API int vslam_orb_detect(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t row_stride, int32_t nfeatures, float scale_factor,
                            int32_t nlevels, int32_t edge, int32_t patch, int32_t fast_threshold, int32_t cap, int32_t* n, float* keypoints) {
  int rc = entry_begin(c);
  if (rc != VSLAM_OK) return rc;
  if (!img || !n || nlevels < 1 || nlevels > 16 || nfeatures < 0 || patch < 3 || patch > 63 || cap < 0 || (cap && !keypoints) || row_stride < cols ||
      !(scale_factor > 1.f) || edge < patch / 2 + 1 || edge < 4 || rows < 2 * edge + 8 || cols < 2 * edge + 8 || rows > 32767 || cols > 32767)
    return fail(c, VSLAM_ERR_INVALID, "orb_detect: bad argument");
  // level sizes, scales and features per level (orb.cpp computeKeyPoints): orb_plan.h, shared with the device-resident RGB-D loop
  const OrbPlan plan = orb_plan(rows, cols, nfeatures, scale_factor, nlevels, edge);
  const int half = patch / 2;
  const OrbUmax um = orb_umax_table(half);
  hipStream_t st = c->stream;
  // everything below lives in the parent's arena until the call returns; the scratch contexts of the levels have arenas of their own
  Call k(c, st);
  float* dout = k.dev<float>((size_t)std::max(cap, 1) * 6);
  int32_t* dtotal = k.dev<int32_t>(1);
  if (k.ok()) k.note(hipMemsetAsync(dtotal, 0, 4, st));
  int lrows = rows, lcols = cols, lstride = (cols + 63) & ~63;
  const uint8_t* lev = nullptr;
  {
    uint8_t* d0 = k.dev<uint8_t>((size_t)rows * lstride);
    if (k.ok()) k.note(hipMemcpy2DAsync(d0, lstride, img, row_stride, cols, rows, hipMemcpyHostToDevice, st));
    lev = d0;
  }
  std::vector<vslam_ctx*> scratch;
  StreamState sst;
  for (int l = 0; l < plan.n_levels && k.ok() && rc == VSLAM_OK; ++l) {
    const float sc = plan.scale[l];
    if (l > 0) {
      const int nr = plan.rows[l], nc = plan.cols[l];
      const int ns = (nc + 63) & ~63;
      uint8_t* dl = k.dev<uint8_t>((size_t)nr * ns);
      if (!k.ok()) break;
      hipLaunchKernelGGL(k_resize_linear_u8, dim3((nc + 255) / 256, nr), dim3(256), 0, st, lev, lrows, lcols, lstride, dl, nr, nc, ns);
      lev = dl; lrows = nr; lcols = nc; lstride = ns;
    }
    // FAST-9/16 + NMS + border filter through the image pipeline's own kernels on a scratch context of the level's size
    vslam_ctx* t = nullptr;
    rc = make_scratch_ctx(c, lrows, lcols, 65535, 64, &t);
    if (rc != VSLAM_OK) break;
    scratch.push_back(t);
    t->cfg.n_regions = 1;
    t->cfg.regions[0].x = 0; t->cfg.regions[0].y = 0; t->cfg.regions[0].w = lcols; t->cfg.regions[0].h = lrows;
    edit_stream_state(k, t, nullptr, sst, [&](StreamState& s) { s.thr[0] = fast_threshold; });
    if (!k.ok()) break;
    rc = set_inputs(t, lev, lev, lstride, 0, true);
    if (rc != VSLAM_OK) break;
    const size_t N = t->cfg.NMAX;
    int16_t* xy1 = k.dev<int16_t>(N * 2); int16_t* xy2 = k.dev<int16_t>(N * 2);
    float* r1 = k.dev<float>(N); float* r2 = k.dev<float>(N); float* rh = k.dev<float>(N);
    int32_t* n1 = k.dev<int32_t>(1); int32_t* n2 = k.dev<int32_t>(1);
    if (!k.ok()) break;
    launch_fast_box(t, st, 1);
    launch_emit(st, t->cfg, t->buf, 1, 1, edge, 0);                                  // runByImageBorder(edgeThreshold)
    hipLaunchKernelGGL(k_orb_select<uint8_t>, dim3(1), dim3(1024), 0, st, t->buf.n_kp, t->buf.kp_xy, t->buf.kp_score, 2 * plan.quota[l], n1, xy1, r1, (int)N);   // retainBest(2 n) on the FAST score
    hipLaunchKernelGGL(k_orb_harris, dim3(256), dim3(256), 0, st, lev, lstride, n1, xy1, rh);
    hipLaunchKernelGGL(k_orb_select<float>, dim3(1), dim3(1024), 0, st, n1, xy1, rh, plan.quota[l], n2, xy2, r2, (int)N);            // retainBest(n) on the Harris response
    hipLaunchKernelGGL(k_orb_angle, dim3(256), dim3(256), 0, st, lev, lstride, n2, xy2, r2, half, um, (float*)nullptr, dout, dtotal, cap, sc, l, patch);
    hipLaunchKernelGGL(k_orb_advance, dim3(1), dim3(1), 0, st, dtotal, n2);
    k.launched();
  }
  int32_t total = 0;
  if (rc == VSLAM_OK) k.down(&total, dtotal, 1);
  if (k.finish() == VSLAM_OK && rc == VSLAM_OK) {
    *n = total;
    k.fetch(keypoints, dout, (size_t)std::min(total, cap) * 6);
    for (vslam_ctx* t : scratch) { int32_t cnt = 0; if (hipMemcpy(&cnt, t->buf.n_kp, 4, hipMemcpyDeviceToHost) == hipSuccess && cnt >= t->cfg.NMAX) rc = fail(c, VSLAM_ERR_CAPACITY, "orb_detect: more than 65535 FAST corners on a level"); }
    if (rc == VSLAM_OK && total > cap) rc = fail(c, VSLAM_ERR_CAPACITY, "orb_detect: output capacity too small");
  }
  for (vslam_ctx* t : scratch) scratch_put(c, t);
  return k.ok() ? rc : k.status();
}

// ---- stand-alone kernels ---------------------------------------------------------------------------
VS_API int vslam_fast_detect(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t rx, int32_t ry,
                             int32_t rw, int32_t rh, int32_t threshold, int32_t cap, int32_t* n, int16_t* xy, int32_t* score) {
  int rc = entry_begin(c);
  if (rc != VSLAM_OK) return rc;
  if (!img || !n) return fail(c, VSLAM_ERR_INVALID, "fast_detect: bad argument");
  if (rx < 0 || ry < 0 || rw < 1 || rh < 1 || rx + rw > cols || ry + rh > rows || cap < 0 || (cap && (!xy))) return fail(c, VSLAM_ERR_INVALID, "ROI outside the image");
  vslam_ctx* t = nullptr;
  rc = make_scratch_ctx(c, rows, cols, std::min(rows * cols, 65535), 64, &t);   // 16-bit feature indices; independent of `cap`: one pooled scratch context serves every call
  if (rc != VSLAM_OK) return rc;
  t->cfg.n_regions = 1;
  t->cfg.regions[0].x = rx; t->cfg.regions[0].y = ry; t->cfg.regions[0].w = rw; t->cfg.regions[0].h = rh;
  Call k(c, t->stream_img);
  StreamState st;
  edit_stream_state(k, t, nullptr, st, [&](StreamState& s) { s.thr[0] = threshold; });
  rc = k.ok() ? set_inputs(t, img, img, stride, 0, false) : k.status();
  if (rc == VSLAM_OK) {
    launch_fast_box(t, t->stream_img, 2);
    launch_emit(t->stream_img, t->cfg, t->buf, 1, 2, 0, 0);
    int32_t cnt = 0;
    rc = vslam_get_keypoints(t, 0, 0, cap, &cnt, xy, score, nullptr);
    *n = cnt;
    if (rc == VSLAM_OK) {
      // more corners in the ROI than the scratch buffers hold (k_emit clamps and raises error bit 0): not a silent truncation
      ImgInfo ii;
      if (hipMemcpy(&ii, t->sets[t->last_set].iinfo, sizeof ii, hipMemcpyDeviceToHost) == hipSuccess && ii.raw_count[0][0] > cnt) {
        *n = ii.raw_count[0][0];
        rc = fail(c, VSLAM_ERR_CAPACITY, "fast_detect: more corners than the output capacity (65535 at most)");
      }
    }
    if (rc == VSLAM_OK) for (int i = 0; i < cnt; ++i) { xy[2 * i] = (int16_t)(xy[2 * i] - rx); xy[2 * i + 1] = (int16_t)(xy[2 * i + 1] - ry); }
    else if (rc != VSLAM_ERR_CAPACITY || c->err.empty()) c->err = t->err;
  }
  scratch_put(c, t);
  return rc;
}
VS_API int vslam_brief_describe(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t n,
                                const int16_t* xy, uint8_t* keep, uint8_t* desc) {
  int rc = entry_begin(c);
  if (rc != VSLAM_OK) return rc;
  if (!img || !xy || !keep || !desc || n < 0) return fail(c, VSLAM_ERR_INVALID, "brief_describe: bad argument");
  vslam_ctx* t = nullptr;
  rc = make_scratch_ctx(c, rows, cols, 64, 64, &t);
  if (rc != VSLAM_OK) return rc;
  Call k(c, t->stream_img);
  int16_t* dxy = k.up(xy, (size_t)n * 2); uint8_t* dkeep = k.dev<uint8_t>(n); uint8_t* ddesc = k.dev<uint8_t>((size_t)n * 32);
  rc = k.ok() ? set_inputs(t, img, img, stride, 0, false) : k.status();
  if (rc == VSLAM_OK && n) {
    launch_fast_box(t, t->stream_img, 2);
    hipLaunchKernelGGL(k_brief_at, dim3(std::min(64, (n + 3) / 4)), dim3(256), 0, t->stream_img, t->buf.box, t->cfg.bstride, rows, cols,
                       n, dxy, dkeep, ddesc);
    k.down(keep, dkeep, (size_t)n);
    k.down(desc, ddesc, (size_t)n * 32);
    rc = k.finish();
  }
  scratch_put(c, t);
  return rc;
}
// cv::ORB::create()->compute() pieces, stand-alone (known-answer tests): the image and its 7x7 Gaussian (dense, stride = cols) in the arena
static uint8_t* orb_blur_device(Call& k, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride) {
  uint8_t* dimg = k.dev<uint8_t>((size_t)rows * stride); uint8_t* dblur = k.dev<uint8_t>((size_t)rows * cols);
  k.up_to(dimg, img, (size_t)(rows - 1) * stride + cols);
  if (k.ok())
    hipLaunchKernelGGL(k_gauss7_plain, dim3((cols + VS_TILE_W - 1) / VS_TILE_W, (rows + VS_TILE_H - 1) / VS_TILE_H), dim3(256), 0, k.st, dimg, stride, rows, cols,
                       gauss7_of(k.c->cfg), dblur, cols);
  return dblur;
}
VS_API int vslam_gaussian_blur7_u8(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, uint8_t* out) {
  if (int rc = entry_begin(c)) return rc;
  if (!img || !out || rows < 4 || cols < 4 || stride < cols) return fail(c, VSLAM_ERR_INVALID, "gaussian_blur7: bad argument");   // one reflection per border
  Call k(c, c->stream);
  const uint8_t* dblur = orb_blur_device(k, img, rows, cols, stride);
  k.down(out, dblur, (size_t)rows * cols);
  return k.finish();
}
VS_API int vslam_orb_describe(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t n, const int16_t* xy,
                              float angle_degrees, uint8_t* keep, uint8_t* desc) {
  if (int rc = entry_begin(c)) return rc;
  if (!img || n < 0 || rows < 4 || cols < 4 || stride < cols || (n && (!xy || !keep || !desc))) return fail(c, VSLAM_ERR_INVALID, "orb_describe: bad argument");
  if (n == 0) return VSLAM_OK;
  if (rows < 2 * VSLAM_ORB_BORDER + 1 || cols < 2 * VSLAM_ORB_BORDER + 1) {   // no pixel is 31 px away from every border: all keypoints removed
    std::memset(keep, 0, (size_t)n);
    std::memset(desc, 0, (size_t)n * 32);
    return VSLAM_OK;
  }
  Call k(c, c->stream);
  const uint8_t* dblur = orb_blur_device(k, img, rows, cols, stride);
  int16_t* dxy = k.up(xy, (size_t)n * 2); uint8_t* dkeep = k.dev<uint8_t>(n); uint8_t* ddesc = k.dev<uint8_t>((size_t)n * 32);
  if (k.ok()) {
    float a, b;
    orb_rotation_host(angle_degrees, &a, &b);
    hipLaunchKernelGGL(k_orb_at, dim3(std::min(64, (n + 3) / 4)), dim3(256), 0, c->stream, dblur, cols, rows, cols, n, dxy, a, b, dkeep, ddesc);
  }
  k.down(keep, dkeep, (size_t)n);
  k.down(desc, ddesc, (size_t)n * 32);
  return k.finish();
}
// cv::ORB::create()->compute() on an OrbDetector's keypoints: a pyramid up to the highest octave present (level l from level l-1, as the detector
// builds it), the 7x7 Gaussian per level, the steered tests per keypoint at its level.  Positions, border filter and rotations are host arithmetic
// (float products rounded half-to-even, cos / sin through the host libm as OpenCV evaluates them).
VS_API int vslam_orb_describe_keypoints(vslam_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t n, const float* kp6,
                                        float scale_factor, uint8_t* keep, uint8_t* desc) {
  if (int rc = entry_begin(c)) return rc;
  if (!img || n < 0 || rows < 4 || cols < 4 || stride < cols || !(scale_factor > 1.f) || (n && (!kp6 || !keep || !desc))) return fail(c, VSLAM_ERR_INVALID, "orb_describe_keypoints: bad argument");
  if (n == 0) return VSLAM_OK;
  int top = 0;
  for (int i = 0; i < n; ++i) { const int o = (int)kp6[6 * (size_t)i + 5]; if (o < 0 || o > 15) return fail(c, VSLAM_ERR_INVALID, "orb_describe_keypoints: octave out of range"); top = std::max(top, o); }
  OrbLevels L;
  std::memset(&L, 0, sizeof L);
  float scale[16];
  uint8_t* raw[16];
  for (int l = 0; l <= top; ++l) {      // every level is validated BEFORE the first launch: an error return must not leave kernels running on the arena
    scale[l] = (float)std::pow((double)scale_factor, (double)l);
    L.rows[l] = l ? (int)std::lrint(rows / scale[l]) : rows; L.cols[l] = l ? (int)std::lrint(cols / scale[l]) : cols;
    if (L.rows[l] < 8 || L.cols[l] < 8) return fail(c, VSLAM_ERR_INVALID, "orb_describe_keypoints: pyramid level smaller than 8 pixels");
  }
  Call k(c, c->stream);
  for (int l = 0; l <= top && k.ok(); ++l) {
    L.stride[l] = L.cols[l];
    raw[l] = k.dev<uint8_t>(l ? (size_t)L.rows[l] * L.cols[l] : (size_t)rows * stride);
    uint8_t* blur = k.dev<uint8_t>((size_t)L.rows[l] * L.cols[l]);
    L.blur[l] = blur;
    const int lstride = l ? L.cols[l] : stride;
    if (l == 0) k.up_to(raw[0], img, (size_t)(rows - 1) * stride + cols);
    else if (k.ok())
      hipLaunchKernelGGL(k_resize_linear_u8, dim3((L.cols[l] + 255) / 256, L.rows[l]), dim3(256), 0, c->stream, raw[l - 1], L.rows[l - 1], L.cols[l - 1],
                         l == 1 ? stride : L.cols[l - 1], raw[l], L.rows[l], L.cols[l], L.cols[l]);
    if (k.ok())
      hipLaunchKernelGGL(k_gauss7_plain, dim3((L.cols[l] + VS_TILE_W - 1) / VS_TILE_W, (L.rows[l] + VS_TILE_H - 1) / VS_TILE_H), dim3(256), 0, c->stream, raw[l], lstride,
                         L.rows[l], L.cols[l], gauss7_of(c->cfg), blur, L.cols[l]);
  }
  std::vector<int32_t> pos((size_t)n * 3);
  std::vector<float> ab((size_t)n * 2);
  const int reach = 23;   // the rotated 31 x 31 pattern reaches cvRound(15 sqrt 2) = 21 pixels
  for (int i = 0; i < n; ++i) {
    const float* kp = kp6 + 6 * (size_t)i;
    const int lv = (int)kp[5];
    const float inv = 1.f / scale[lv];
    const int cx = (int)std::lrint(kp[0] * inv), cy = (int)std::lrint(kp[1] * inv);
    const int x0 = (int)std::lrint(kp[0]), y0 = (int)std::lrint(kp[1]);
    const bool in = x0 >= VSLAM_ORB_BORDER && x0 < cols - VSLAM_ORB_BORDER && y0 >= VSLAM_ORB_BORDER && y0 < rows - VSLAM_ORB_BORDER &&   // runByImageBorder(31) at level 0
                    cx >= reach && cy >= reach && cx < L.cols[lv] - reach && cy < L.rows[lv] - reach;
    pos[3 * (size_t)i] = cx; pos[3 * (size_t)i + 1] = cy; pos[3 * (size_t)i + 2] = in ? lv : -1;
    orb_rotation_host(kp[3], &ab[2 * (size_t)i], &ab[2 * (size_t)i + 1]);
  }
  int32_t* dpos = k.up(pos.data(), pos.size()); float* dab = k.up(ab.data(), ab.size());
  uint8_t* dkeep = k.dev<uint8_t>(n); uint8_t* ddesc = k.dev<uint8_t>((size_t)n * 32);
  if (k.ok()) hipLaunchKernelGGL(k_orb_at_levels, dim3(std::min(64, (n + 3) / 4)), dim3(256), 0, c->stream, L, n, dpos, dab, dkeep, ddesc);
  k.down(keep, dkeep, (size_t)n);
  k.down(desc, ddesc, (size_t)n * 32);
  return k.finish();    // also: the host staging vectors may go out of scope now
}
// ---- descriptor test pairs as run-time data (the tables are __constant__ arrays of this module: one copy per device) ------
static int pattern_io(int device, int which, const int8_t* in, int8_t* out) {
  if ((!in && !out) || device < 0) { g_create_error = "pattern: bad argument"; return VSLAM_ERR_INVALID; }
  if (in) {
    for (int i = 0; i < 256; ++i) {
      const int8_t* q = in + 4 * i;
      if (which == 0) {
        for (int k = 0; k < 4; ++k) if (q[k] < -VSLAM_BRIEF_PATCH_HALF || q[k] > VSLAM_BRIEF_PATCH_HALF) { g_create_error = "brief pattern: offset beyond the 48 px patch"; return VSLAM_ERR_INVALID; }
      } else {
        // a 31 x 31 patch: |x|, |y| <= 15 (OpenCV's bit_pattern_31_ reaches (12, -13), radius 17.7).  Where the reach matters: the
        // tiled extractor (k_orb_describe) stages a 16 px margin and rotates by the FAST keypoints' fixed -1 degree, so a rotated,
        // rounded offset is at most rint(15 cos 1 + 15 sin 1) = 15; the kernels that rotate by arbitrary angles gather from the
        // whole image behind the 31 px border, and 15 sqrt 2 < 22.
        for (int k = 0; k < 4; ++k) if (q[k] < -15 || q[k] > 15) { g_create_error = "orb pattern: offset beyond the 31 px patch (|x|, |y| <= 15)"; return VSLAM_ERR_INVALID; }
      }
    }
  }
  if (hipSetDevice(device) != hipSuccess) { g_create_error = "pattern: no such HIP device"; return VSLAM_ERR_NO_DEVICE; }
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess && in) e = which == 0 ? hipMemcpyToSymbol(HIP_SYMBOL(c_brief), in, 1024) : hipMemcpyToSymbol(HIP_SYMBOL(c_orb), in, 1024);
  if (e == hipSuccess && in && which == 0) {   // the footprint follows its pattern, inside the same pair of device synchronisations
    const BriefFootprint fp = brief_footprint(reinterpret_cast<const int8_t (*)[4]>(in));
    e = hipMemcpyToSymbol(HIP_SYMBOL(c_brief_fp), &fp, sizeof(fp));
  }
  if (e == hipSuccess && out) e = which == 0 ? hipMemcpyFromSymbol(out, HIP_SYMBOL(c_brief), 1024) : hipMemcpyFromSymbol(out, HIP_SYMBOL(c_orb), 1024);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) { g_create_error = std::string("pattern: ") + hipGetErrorString(e); return VSLAM_ERR_HIP; }
  return VSLAM_OK;
}
VS_API int vslam_set_brief_pattern(int device, const int8_t* pairs) { return pattern_io(device, 0, pairs, nullptr); }
VS_API int vslam_set_orb_pattern(int device, const int8_t* pairs) { return pattern_io(device, 1, pairs, nullptr); }
VS_API int vslam_get_brief_pattern(int device, int8_t* out) { return pattern_io(device, 0, nullptr, out); }
VS_API int vslam_get_orb_pattern(int device, int8_t* out) { return pattern_io(device, 1, nullptr, out); }

VS_API int vslam_knn2(vslam_ctx* c, int norm, int32_t nq, const uint8_t* q, int32_t nt, const uint8_t* t, int32_t* idx, float* dist) {
  if (int rc = entry_begin(c)) return rc;
  if (!q || !t || !idx || !dist || nq < 0 || nt < 0 || norm < 0 || norm > 3) return fail(c, VSLAM_ERR_INVALID, "knn2: bad argument");
  if (nq == 0) return VSLAM_OK;
  Call k(c, c->stream);
  uint8_t* dq = k.up(q, (size_t)nq * 32); uint8_t* dt = k.up(t, (size_t)nt * 32);
  int32_t* di = k.dev<int32_t>((size_t)nq * 2); float* dd = k.dev<float>((size_t)nq * 2);
  if (k.ok()) hipLaunchKernelGGL(k_knn2, dim3((nq + 15) / 16), dim3(256), 0, c->stream, norm, nq, dq, nt, dt, di, dd);
  k.down(idx, di, (size_t)nq * 2);
  k.down(dist, dd, (size_t)nq * 2);
  return k.finish();
}
static int align_points_impl(vslam_ctx* c, bool uvd, int32_t n, const double* moving, const double* fixed4, const double* omega,
                             const double* weight, const double T_init[12], double T_out[12], double* chi, uint8_t* inlier,
                             int32_t* n_inliers, double* total_error, int32_t* iterations, double H_out[36]) {
  vslam_ctx* t = nullptr;
  vslam_config cfg = c->cfg.c;
  cfg.max_points = (std::max(64, n) + 1023) / 1024 * 1024; cfg.max_keypoints = 64; cfg.max_history_frames = 2;   // rounded: one pooled scratch context serves every call
  int rc = scratch_get(c, cfg, &t);
  if (rc != VSLAM_OK) return rc;
  const size_t N = n;
  Call k(c, t->stream);
  double* dT = k.up(T_init, 12);
  k.up_to(t->buf.al_moving, moving, N * 3); k.up_to(t->buf.al_fixed, fixed4, N * 4);
  k.up_to(t->buf.al_omega, omega, N); k.up_to(t->buf.al_weight, weight, N);
  if (k.ok()) {
    if (uvd) hipLaunchKernelGGL(k_align_points<true>, dim3(1), dim3(VS_WG), 0, t->stream, t->cfg, t->buf, n, dT);
    else hipLaunchKernelGGL(k_align_points<false>, dim3(1), dim3(VS_WG), 0, t->stream, t->cfg, t->buf, n, dT);
  }
  StreamState st;
  k.down(&st, t->buf.st, 1);
  if (chi) k.down(chi, t->buf.al_chi, N);
  if (inlier) k.down(inlier, t->buf.al_inl, N);
  rc = k.finish();
  if (rc == VSLAM_OK) {
    if (T_out) std::memcpy(T_out, st.al_T, sizeof(double) * 12);
    if (H_out) std::memcpy(H_out, st.al_H, sizeof(double) * 36);
    if (n_inliers) *n_inliers = st.al_inliers;
    if (total_error) *total_error = st.al_total_error;
    if (iterations) *iterations = st.al_iterations;
  }
  scratch_put(c, t);
  return rc;
}
VS_API int vslam_align_points(vslam_ctx* c, int32_t n, const double* moving, const double* fixed, const double* omega,
                              const double* weight, const double T_init[12], double T_out[12], double* chi, uint8_t* inlier,
                              int32_t* n_inliers, double* total_error, int32_t* iterations, double H_out[36]) {
  if (int rc = entry_begin(c)) return rc;
  if (n < 0 || !moving || !fixed || !omega || !weight || !T_init) return fail(c, VSLAM_ERR_INVALID, "align_points: bad argument");
  return align_points_impl(c, false, n, moving, fixed, omega, weight, T_init, T_out, chi, inlier, n_inliers, total_error, iterations, H_out);
}
VS_API int vslam_align_points_uvd(vslam_ctx* c, int32_t n, const double* moving, const double* fixed_uvd, const double* omega_uv,
                                  const double* omega_depth, const double* weight, const double T_init[12], double T_out[12],
                                  double* chi, uint8_t* inlier, int32_t* n_inliers, double* total_error, int32_t* iterations,
                                  double H_out[36]) {
  if (int rc = entry_begin(c)) return rc;
  if (n < 0 || !moving || !fixed_uvd || !omega_uv || !omega_depth || !weight || !T_init) return fail(c, VSLAM_ERR_INVALID, "align_points_uvd: bad argument");
  std::vector<double> f4((size_t)std::max(n, 1) * 4);   // (u, v, depth, depth information) per measurement
  for (int i = 0; i < n; ++i) { f4[4 * (size_t)i] = fixed_uvd[3 * (size_t)i]; f4[4 * (size_t)i + 1] = fixed_uvd[3 * (size_t)i + 1]; f4[4 * (size_t)i + 2] = fixed_uvd[3 * (size_t)i + 2]; f4[4 * (size_t)i + 3] = omega_depth[i]; }
  return align_points_impl(c, true, n, moving, f4.data(), omega_uv, weight, T_init, T_out, chi, inlier, n_inliers, total_error, iterations, H_out);
}

// features of one image of scratch context t as the image pipeline would leave them (sort_features) plus cleared used flags and the
// count.  order[k] = caller index of sorted feature k.
static int upload_features(vslam_ctx* c, vslam_ctx* t, int side, int n, const int32_t* rcx, const uint8_t* dx, std::vector<int>& ord) {
  const DevCfg& dc = t->cfg;
  const int rows = dc.c.rows, cols = dc.c.cols, CW1 = dc.CW + 1;
  SortedFeatures f;
  if (!sort_features(rcx, dx, n, rows, cols, CW1, f)) return fail(c, VSLAM_ERR_INVALID, "feature outside the image");
  const std::vector<uint8_t> used(n, 0);
  const size_t N = dc.NMAX;
  Call k(c, t->stream);
  k.up_to(t->buf.kp_xy + side * N * 2, f.xy.data(), (size_t)n * 2);
  k.up_to(t->buf.desc + side * N * 32, f.desc.data(), (size_t)n * 32);
  k.up_to(t->buf.used + side * N, used.data(), (size_t)n);
  k.up_to(t->buf.rowcell + (size_t)side * rows * CW1, f.rowcell.data(), f.rowcell.size());
  k.up_to(t->buf.n_kp + side, &n, 1);
  ord.swap(f.ord);
  return k.finish();   // the host vectors go out of scope
}

VS_API int vslam_track_match(vslam_ctx* c, const double T[12], int32_t d, double tau_track, double tau_tri, int32_t by_appearance,
                             int32_t nP, const double* cam, const uint8_t* pdL, const uint8_t* pdR, const int32_t* epi,
                             int32_t nL, const int32_t* rcL, const uint8_t* dL, int32_t nR, const int32_t* rcR, const uint8_t* dR,
                             int32_t* n_tracked, int32_t* out4, int32_t* n_lost, int32_t* lost) {
  int rc = entry_begin(c);
  if (rc != VSLAM_OK) return rc;
  if (!T || nP < 0 || nL < 0 || nR < 0 || !n_tracked || !out4 || !n_lost || !lost || (nP && (!cam || !pdL || !pdR || !epi)) || (nL && (!rcL || !dL)) ||
      (nR && (!rcR || !dR)))
    return fail(c, VSLAM_ERR_INVALID, "track_match: bad argument");
  vslam_ctx* t = nullptr;
  vslam_config cfg = c->cfg.c;
  cfg.max_points = std::max(64, nP); cfg.max_keypoints = std::max(64, std::max(nL, nR)); cfg.max_history_frames = 2;
  rc = scratch_get(c, cfg, &t);
  if (rc != VSLAM_OK) return rc;
  std::vector<int> order[2];
  rc = upload_features(c, t, 0, nL, rcL, dL, order[0]);
  if (rc == VSLAM_OK) rc = upload_features(c, t, 1, nR, rcR, dR, order[1]);
  if (rc == VSLAM_OK) {
    // previous points in point buffer 0
    std::vector<uint8_t> pdesc((size_t)nP * 64);
    std::vector<int32_t> meta((size_t)nP * META, 0);
    for (int i = 0; i < nP; ++i) {
      std::memcpy(&pdesc[(size_t)64 * i], pdL + (size_t)32 * i, 32); std::memcpy(&pdesc[(size_t)64 * i + 32], pdR + (size_t)32 * i, 32);
      meta[(size_t)i * META + M_EPI] = epi[i]; meta[(size_t)i * META + M_PREV] = -1;
    }
    Call k(c, t->stream);
    k.up_to(t->buf.p_cam, cam, (size_t)nP * 3); k.up_to(t->buf.p_desc, pdesc.data(), pdesc.size()); k.up_to(t->buf.p_meta, meta.data(), meta.size());
    k.up_to(t->buf.n_points, &nP, 1);
    StreamState st;
    edit_stream_state(k, t, t->stream, st, [&](StreamState& s) {
      s.has_prev = 1; s.cur = 0; s.win = d; s.tau_track = tau_track; s.tau_tri = tau_tri;
      s.status = by_appearance ? VSLAM_LOCALIZING : VSLAM_TRACKING;
      std::memcpy(s.prior, T, sizeof(double) * 12);
    });
    if (k.ok()) {
      hipLaunchKernelGGL(k_track_candidates, dim3(16, 1), dim3(256), 0, t->stream, t->cfg, t->buf, by_appearance ? 1 : 0);
      hipLaunchKernelGGL(k_stage, dim3(1), dim3(VS_WG), 0, t->stream, t->cfg, t->buf, (int)VS_STAGE_TRACK, by_appearance ? 1 : 0, StageIo{});
    }
    k.down(&st, t->buf.st, 1);
    if (k.finish() == VSLAM_OK) {
      std::vector<int32_t> trk((size_t)st.n_trk * 4);
      k.fetch(trk.data(), t->buf.trk, trk.size());
      k.fetch(lost, t->buf.lost, (size_t)st.n_lost);
      if (k.ok()) {
        *n_tracked = st.n_trk; *n_lost = st.n_lost;
        for (int u = 0; u < st.n_trk; ++u) {
          out4[4 * u] = trk[4 * u]; out4[4 * u + 1] = order[0][trk[4 * u + 1]]; out4[4 * u + 2] = order[1][trk[4 * u + 2]]; out4[4 * u + 3] = trk[4 * u + 3];
        }
      }
    }
    rc = k.status();
  }
  scratch_put(c, t);
  return rc;
}

VS_API int vslam_stereo_match(vslam_ctx* c, double tau_tri, int32_t nL, const int32_t* rcL, const uint8_t* dL, int32_t nR,
                              const int32_t* rcR, const uint8_t* dR, int32_t cap, int32_t* n_out, int32_t* out4) {
  int rc = entry_begin(c);
  if (rc != VSLAM_OK) return rc;
  if (nL < 0 || nR < 0 || cap < 0 || !n_out || (cap && !out4) || (nL && (!rcL || !dL)) || (nR && (!rcR || !dR))) return fail(c, VSLAM_ERR_INVALID, "stereo_match: bad argument");
  vslam_ctx* t = nullptr;
  vslam_config cfg = c->cfg.c;
  cfg.max_keypoints = std::max(64, std::max(nL, nR)); cfg.max_points = std::max(64, nL); cfg.max_history_frames = 2;
  rc = scratch_get(c, cfg, &t);
  if (rc != VSLAM_OK) return rc;
  std::vector<int> order[2];
  rc = upload_features(c, t, 0, nL, rcL, dL, order[0]);
  if (rc == VSLAM_OK) rc = upload_features(c, t, 1, nR, rcR, dR, order[1]);
  if (rc == VSLAM_OK) {
    Call k(c, t->stream);
    StreamState st;
    edit_stream_state(k, t, t->stream, st, [&](StreamState& s) { s.tau_tri = tau_tri; s.n_cur = 0; s.cur = 0; });
    if (k.ok()) {
      hipLaunchKernelGGL(k_stereo_dist, dim3((t->cfg.NMAX + 255) / 256, 1), dim3(256), 0, t->stream, t->cfg, t->buf);
      hipLaunchKernelGGL(k_stage, dim3(1), dim3(VS_WG), 0, t->stream, t->cfg, t->buf, (int)VS_STAGE_STEREO, 0, StageIo{});
    }
    k.down(&st, t->buf.st, 1);
    rc = k.finish();
    if (rc == VSLAM_OK) {
      const int n = st.n_new;
      *n_out = n;
      if (n > cap) rc = fail(c, VSLAM_ERR_CAPACITY, "stereo_match: output capacity too small");
      else if (n) {
        // the new points were written to point buffer 1 (current = previous ^ 1)
        const size_t P = t->cfg.MAXP;
        std::vector<int16_t> kp((size_t)n * 4);
        std::vector<int32_t> meta((size_t)n * META);
        k.fetch(kp.data(), t->buf.p_kp + P * 4, kp.size());
        k.fetch(meta.data(), t->buf.p_meta + P * META, meta.size());
        for (int i = 0; i < n && k.ok(); ++i) {
          int il = -1, ir = -1;   // ids by coordinates (one feature per pixel)
          for (int j = 0; j < nL; ++j) if (rcL[2 * j] == kp[4 * i + 1] && rcL[2 * j + 1] == kp[4 * i]) il = j;
          for (int j = 0; j < nR; ++j) if (rcR[2 * j] == kp[4 * i + 3] && rcR[2 * j + 1] == kp[4 * i + 2]) ir = j;
          out4[4 * i] = il; out4[4 * i + 1] = ir; out4[4 * i + 2] = meta[(size_t)i * META + M_DIST]; out4[4 * i + 3] = meta[(size_t)i * META + M_EPI];
        }
        rc = k.status();
      }
    }
  }
  scratch_put(c, t);
  return rc;
}

VS_API int vslam_stereo_recover(vslam_ctx* c, const uint8_t* imgL, const uint8_t* imgR, int32_t row_stride, const double w2c[12], int32_t n,
                                const uint8_t* has_lm, const double* lm, const uint8_t* pdL, const uint8_t* pdR, double tau_track, double tau_tri,
                                int32_t* n_rec, int32_t* rec_index, int32_t* rec_xy4, int32_t* rec_dist, uint8_t* rec_desc, double* rec_xyz) {
  int rc = entry_begin(c);
  if (rc != VSLAM_OK) return rc;
  if (!imgL || !imgR || !w2c || n < 0 || !n_rec || (n && (!has_lm || !lm || !pdL || !pdR || !rec_index || !rec_xy4 || !rec_dist || !rec_desc || !rec_xyz)))
    return fail(c, VSLAM_ERR_INVALID, "stereo_recover: bad argument");
  if (row_stride < c->cfg.c.cols) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than image width");
  *n_rec = 0;
  if (n == 0) return VSLAM_OK;
  vslam_ctx* t = nullptr;
  vslam_config cfg = c->cfg.c;
  cfg.det_rows = 1; cfg.det_cols = 1; cfg.max_keypoints = 64; cfg.max_points = (std::max(64, n) + 1023) & ~1023; cfg.max_history_frames = 2;
  rc = scratch_get(c, cfg, &t);
  if (rc != VSLAM_OK) return rc;
  const size_t P = t->cfg.MAXP;
  std::vector<uint8_t> desc((size_t)n * 64);
  std::vector<int32_t> meta((size_t)n * META, 0), lost((size_t)n);
  for (int i = 0; i < n; ++i) {
    std::memcpy(&desc[(size_t)64 * i], pdL + (size_t)32 * i, 32);
    std::memcpy(&desc[(size_t)64 * i + 32], pdR + (size_t)32 * i, 32);
    meta[(size_t)i * META + M_LMUP] = has_lm[i] ? 1 : 0;
    meta[(size_t)i * META + M_PREV] = -1;
    lost[i] = i;
  }
  hipStream_t q = t->stream_img;
  Call k(c, q);
  k.up_to(t->buf.p_desc, desc.data(), desc.size()); k.up_to(t->buf.p_meta, meta.data(), meta.size());
  k.up_to(t->buf.p_lm, lm, (size_t)n * 3); k.up_to(t->buf.lost, lost.data(), lost.size());
  rc = k.ok() ? set_inputs(t, imgL, imgR, row_stride, 0, false) : k.status();
  if (rc == VSLAM_OK) {
    if (t->cfg.c.descriptor_type == VSLAM_DESCRIPTOR_ORB)
      hipLaunchKernelGGL(k_gauss7, dim3(t->cfg.TX, (t->cfg.c.rows + VS_TILE_H - 1) / VS_TILE_H, 2), dim3(256), 0, q, t->cfg, t->buf, gauss7_of(t->cfg));
    else launch_fast_box(t, q, 2);
    RecoverAlone a;
    std::memcpy(a.w2c, w2c, sizeof a.w2c); a.tau_track = tau_track; a.tau_tri = tau_tri; a.n = n;
    hipLaunchKernelGGL(k_recover_alone, dim3(1), dim3(VS_WG), 0, q, t->cfg, t->buf, a);
    StreamState st;
    k.down(&st, t->buf.st, 1);
    if (k.finish() == VSLAM_OK && st.n_cur > 0) {     // also: the host staging vectors may go out of scope now
      const int m = st.n_cur;
      std::vector<int16_t> kp((size_t)m * 4);
      std::vector<int32_t> mt((size_t)m * META);
      k.fetch(kp.data(), t->buf.p_kp + P * 4, kp.size());
      k.fetch(mt.data(), t->buf.p_meta + P * META, mt.size());
      k.fetch(rec_desc, t->buf.p_desc + P * 64, (size_t)m * 64);
      k.fetch(rec_xyz, t->buf.p_cam + P * 3, (size_t)m * 3);
      for (int i = 0; i < m && k.ok(); ++i) {
        rec_index[i] = mt[(size_t)i * META + M_PREV]; rec_dist[i] = mt[(size_t)i * META + M_DIST];
        for (int j = 0; j < 4; ++j) rec_xy4[4 * i + j] = kp[4 * (size_t)i + j];
      }
      if (k.ok()) *n_rec = m;
    }
    rc = k.status();
  } else if (c->err.empty()) c->err = t->err;
  scratch_put(c, t);
  return rc;
}

// ---- cv::equalizeHist on one host image (kernels_equalize.h) --------------------------------------------------------
VS_API int vslam_equalize_hist_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, uint8_t* dst, uint32_t* hist256) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 0 || cols < 0) return fail(c, VSLAM_ERR_INVALID, "equalize_hist: negative size");
  if (rows == 0 || cols == 0) return VSLAM_OK;
  if (!src || !dst || row_stride < cols) return fail(c, VSLAM_ERR_INVALID, "equalize_hist: bad argument");
  if ((size_t)rows * (size_t)cols > (size_t)VS_EQ_MAX_PIXELS) return fail(c, VSLAM_ERR_INVALID, "equalize_hist: more than 2^24 pixels");
  Call k(c, c->stream);
  const size_t bytes = (size_t)(rows - 1) * row_stride + cols;
  const size_t off = (size_t)((uintptr_t)src & 15u);       // the device copy keeps the caller's alignment: rows start where they would in place
  uint8_t* ds = k.dev<uint8_t>(bytes + 16);
  k.up_to(ds + off, src, bytes);
  const int ostride = (cols + 15) & ~15;
  uint8_t* dd = k.dev<uint8_t>((size_t)rows * ostride);
  EqArgs ea{};
  place(ea, ds + off, row_stride, dd, ostride, rows, cols);
  ea.hist = k.dev<uint32_t>(256);
  if (k.ok()) k.note(equalize_enqueue(c->stream, ea));
  if (k.ok()) k.note(hipMemcpy2DAsync(dst, (size_t)cols, dd, (size_t)ostride, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
  if (hist256) k.down(hist256, ea.hist, 256);
  return k.finish();
}

// ---- a detection mask's eroded packed words from one host image (kernels_mask.h) ----------------------------------------
VS_API int vslam_mask_pack_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int32_t margin, uint64_t* words) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 0 || cols < 0) return fail(c, VSLAM_ERR_INVALID, "mask_pack: negative size");
  if (margin < 0 || margin > VS_MASK_MAX_MARGIN) return fail(c, VSLAM_ERR_INVALID, "mask_pack: margin outside 0 .. 64");
  if (rows == 0 || cols == 0) return VSLAM_OK;
  if (!src || !words || row_stride < cols || rows > 32767 || cols > 32767) return fail(c, VSLAM_ERR_INVALID, "mask_pack: bad argument");
  Call k(c, c->stream);
  const size_t bytes = (size_t)(rows - 1) * row_stride + cols;
  const size_t off = (size_t)((uintptr_t)src & 15u);       // the device copy keeps the caller's alignment: rows start where they would in place
  uint8_t* ds = k.dev<uint8_t>(bytes + 16);
  k.up_to(ds + off, src, bytes);
  MaskPackArgs a{};
  a.src[0] = ds + off; a.src_row_stride = row_stride; a.rows = rows; a.cols = cols; a.TX = (cols + 63) / 64; a.margin = margin; a.n = 1; a.sides = 1;
  const size_t nw = (size_t)rows * a.TX;
  a.dst = k.dev<unsigned long long>(nw);
  active_all(a.active, 1);
  if (k.ok()) mask_pack_enqueue(c->stream, a);
  k.launched();
  k.down(reinterpret_cast<unsigned long long*>(words), a.dst, nw);
  return k.finish();
}

// ---- the eroded packed validity words of one host remap map (kernels_mask.h, k_map_valid) -------------------------------
VS_API int vslam_map_validity_mask(vslam_ctx* c, const int16_t* map_xy, const uint16_t* map_a, int32_t rows, int32_t cols, int32_t raw_rows,
                                   int32_t raw_cols, int32_t margin, uint64_t* words) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 1 || cols < 1 || rows > 32767 || cols > 32767 || raw_rows < 1 || raw_cols < 1 || raw_rows > 32767 || raw_cols > 32767)
    return fail(c, VSLAM_ERR_INVALID, "map_validity_mask: sizes outside 1 .. 32767");
  if (margin < 0 || margin > VS_MASK_MAX_MARGIN) return fail(c, VSLAM_ERR_INVALID, "map_validity_mask: margin outside 0 .. 64");
  if (!map_xy || !map_a || !words) return fail(c, VSLAM_ERR_INVALID, "map_validity_mask: null argument");
  if (!rect_maps_ok(map_a, (size_t)rows * cols)) return fail(c, VSLAM_ERR_INVALID, "map_validity_mask: interpolation table index >= 1024");
  Call k(c, c->stream);
  RemapMaps m;
  m.rows = rows; m.cols = cols; m.raw_rows = raw_rows; m.raw_cols = raw_cols;
  m.stride = (cols + 3) & ~3;
  std::vector<int16_t> pxy;
  std::vector<uint16_t> pa;
  rect_pad_maps(map_xy, map_a, rows, cols, m.stride, pxy, pa);
  m.xy[0] = k.up(pxy.data(), pxy.size());
  m.a[0] = k.up(pa.data(), pa.size());
  const size_t nw = (size_t)rows * ((cols + 63) / 64);
  unsigned long long* dw = k.dev<unsigned long long>(nw);
  if (k.ok()) map_valid_enqueue(c->stream, m, 1, margin, dw);
  k.launched();
  k.down(reinterpret_cast<unsigned long long*>(words), dw, nw);
  return k.finish();
}

// ---- cv::CLAHE::apply on one host image (kernels_clahe.h) -------------------------------------------------------------
VS_API int vslam_clahe_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, double clip_limit, int32_t tiles_x,
                          int32_t tiles_y, uint8_t* dst, int32_t dst_row_stride, uint8_t* luts) {
  if (int rc = entry_begin(c)) return rc;
  ClaheArgs ca;
  std::memset(&ca, 0, sizeof ca);
  const char* why = "";
  if (!clahe_geometry(rows, cols, clip_limit, tiles_x, tiles_y, ca, &why)) return fail(c, VSLAM_ERR_INVALID, std::string("clahe_u8: ") + why);
  if (!src || !dst || row_stride < cols || dst_row_stride < cols || (dst == src && dst_row_stride != row_stride)) return fail(c, VSLAM_ERR_INVALID, "clahe_u8: bad argument");
  Call k(c, c->stream);
  // the device copies keep the caller's alignment: rows start where they would in place
  const size_t bytes = (size_t)(rows - 1) * row_stride + cols, off = (size_t)((uintptr_t)src & 15u);
  uint8_t* ds = k.dev<uint8_t>(bytes + 16);
  k.up_to(ds + off, src, bytes);
  const size_t doff = (size_t)((uintptr_t)dst & 15u);
  uint8_t* dd = dst == src ? ds + off : k.dev<uint8_t>((size_t)(rows - 1) * dst_row_stride + cols + 16) + doff;
  const size_t nl = (size_t)tiles_x * tiles_y * 256;
  place(ca, ds + off, row_stride, dd, dst_row_stride, rows, cols);
  ca.luts = k.dev<uint8_t>(nl);
  if (k.ok()) k.note(clahe_enqueue(c->stream, ca));
  if (k.ok()) k.note(hipMemcpy2DAsync(dst, (size_t)dst_row_stride, dd, (size_t)dst_row_stride, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
  if (luts) k.down(luts, ca.luts, nl);
  return k.finish();
}

// ---- the depth image's bilateral filter on one host image (kernels_bilateral.h) ----------------------------------------
VS_API int vslam_bilateral_depth_u16(vslam_ctx* c, const uint16_t* src, int32_t rows, int32_t cols, int32_t row_stride, double depth_scale,
                                     double sigma_color, double sigma_space, uint16_t* dst, int32_t dst_row_stride, float* lut4098) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 0 || cols < 0) return fail(c, VSLAM_ERR_INVALID, "bilateral_depth_u16: negative size");
  BilateralArgs ba;
  std::memset(&ba, 0, sizeof ba);
  const char* why = "";
  if (!bilateral_args(std::max(rows, 1), std::max(cols, 1), depth_scale, sigma_color, sigma_space, ba, &why)) return fail(c, VSLAM_ERR_INVALID, std::string("bilateral_depth_u16: ") + why);
  if (rows == 0 || cols == 0) return VSLAM_OK;
  if (!src || !dst || row_stride < cols || dst_row_stride < cols || (dst == src && dst_row_stride != row_stride)) return fail(c, VSLAM_ERR_INVALID, "bilateral_depth_u16: bad argument");
  if (!c->bl_cells) {                                                    // the first call allocates and arms the cells; every call leaves them armed
    uint32_t* cells = nullptr;
    HIP_TRY(c, dalloc(c, &cells, 4));
    HIP_TRY(c, bilateral_arm(cells, 1, c->stream));
    c->bl_cells = cells;
  }
  Call k(c, c->stream);
  // the device copies keep the caller's 4-byte phase: the filter stores words where the caller's image would take them.  Source and
  // destination are two buffers on the device also when they are one on the host: a tile reads its neighbours' pixels
  const size_t ne = (size_t)(rows - 1) * row_stride + cols, nd = (size_t)(rows - 1) * dst_row_stride + cols;
  uint16_t* ds = k.dev<uint16_t>(ne + 2) + (((uintptr_t)src & 3u) >> 1);
  k.up_to(ds, src, ne);
  uint16_t* dd = k.dev<uint16_t>(nd + 2) + (((uintptr_t)dst & 3u) >> 1);
  ba.src = ds; ba.src_row_stride = row_stride; ba.dst = dd; ba.dst_row_stride = dst_row_stride; ba.n = 1;
  ba.cells = c->bl_cells; ba.lut = k.dev<float>(VS_BL_LUT);
  if (k.ok()) bilateral_enqueue(c->stream, ba);
  if (k.ok()) k.note(hipMemcpy2DAsync(dst, (size_t)dst_row_stride * 2, dd, (size_t)dst_row_stride * 2, (size_t)cols * 2, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
  if (lut4098) k.down(lut4098, ba.lut, VS_BL_LUT);
  return k.finish();
}

// ---- interleaved 8-bit colour to grey on one host image (kernels_gray.h) --------------------------------------------
VS_API int vslam_gray_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int format, uint8_t* dst) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 0 || cols < 0) return fail(c, VSLAM_ERR_INVALID, "gray_u8: negative size");
  if (format < VSLAM_PIXEL_BGR8 || format > VSLAM_PIXEL_RGBA8) return fail(c, VSLAM_ERR_INVALID, "gray_u8: unknown pixel format");
  if (rows == 0 || cols == 0) return VSLAM_OK;
  const int64_t wb = (int64_t)gray_channels(format) * cols;
  if (!src || !dst || (int64_t)row_stride < wb) return fail(c, VSLAM_ERR_INVALID, "gray_u8: bad argument");
  Call k(c, c->stream);
  const size_t bytes = (size_t)(rows - 1) * row_stride + (size_t)wb;
  const size_t off = (size_t)((uintptr_t)src & 15u);       // the device copy keeps the caller's alignment: rows start where they would in place
  uint8_t* ds = k.dev<uint8_t>(bytes + 16);
  k.up_to(ds + off, src, bytes);
  const int ostride = (cols + 15) & ~15;
  uint8_t* dd = k.dev<uint8_t>((size_t)rows * ostride);
  GrayArgs ga{};
  place(ga, ds + off, row_stride, dd, ostride, rows, cols);
  ga.format = format;
  if (k.ok()) k.note(gray_enqueue(c->stream, ga));
  if (k.ok()) k.note(hipMemcpy2DAsync(dst, (size_t)cols, dd, (size_t)ostride, (size_t)cols, (size_t)rows, hipMemcpyDeviceToHost, c->stream));
  return k.finish();
}

// ---- integer-factor reduction of one host image / depth image (kernels_downscale.h) -------------------------------------
// the checks the two entries share; *empty: a zero-size call, nothing to do
static int downscale_entry_check(vslam_ctx* c, const char* who, const void* src, int32_t rows, int32_t cols, int32_t row_stride, int32_t factor, const void* dst,
                                 int32_t dst_row_stride, bool* empty) {
  *empty = false;
  const std::string w(who);
  if (rows < 0 || cols < 0) return fail(c, VSLAM_ERR_INVALID, w + ": negative size");
  if (!ds_factor_ok(factor)) return fail(c, VSLAM_ERR_INVALID, w + ": factor outside 2 .. 4");
  if (rows == 0 || cols == 0) { *empty = true; return VSLAM_OK; }
  if (!ds_size_ok(rows, cols, factor)) return fail(c, VSLAM_ERR_INVALID, w + ": full size outside 1 .. 32767 or below one block");
  if (!src || !dst || row_stride < cols || dst_row_stride < ds_out(cols, factor)) return fail(c, VSLAM_ERR_INVALID, w + ": bad argument");
  return VSLAM_OK;
}
VS_API int vslam_downscale_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int32_t factor, uint8_t* dst,
                              int32_t dst_row_stride) {
  if (int rc = entry_begin(c)) return rc;
  bool empty;
  if (int rc = downscale_entry_check(c, "downscale_u8", src, rows, cols, row_stride, factor, dst, dst_row_stride, &empty)) return rc;
  if (empty) return VSLAM_OK;
  const int orows = ds_out(rows, factor), ocols = ds_out(cols, factor);
  Call k(c, c->stream);
  // the device copies keep the caller's alignment: rows start where they would in place.  Only what the blocks cover is copied.
  const size_t bytes = (size_t)(orows * factor - 1) * row_stride + (size_t)ocols * factor, nd = (size_t)(orows - 1) * dst_row_stride + ocols;
  uint8_t* ds = k.dev<uint8_t>(bytes + 16) + (size_t)((uintptr_t)src & 15u);
  k.up_to(ds, src, bytes);
  uint8_t* dd = k.dev<uint8_t>(nd + 16) + (size_t)((uintptr_t)dst & 15u);
  DownscaleArgs da{};
  place(da, ds, row_stride, dd, dst_row_stride, orows, ocols);
  da.factor = factor;
  if (k.ok()) k.note(downscale_enqueue(c->stream, da));
  if (k.ok()) k.note(hipMemcpy2DAsync(dst, (size_t)dst_row_stride, dd, (size_t)dst_row_stride, (size_t)ocols, (size_t)orows, hipMemcpyDeviceToHost, c->stream));
  return k.finish();
}
VS_API int vslam_downscale_depth_u16(vslam_ctx* c, const uint16_t* src, int32_t rows, int32_t cols, int32_t row_stride, int32_t factor, uint16_t* dst,
                                     int32_t dst_row_stride) {
  if (int rc = entry_begin(c)) return rc;
  bool empty;
  if (int rc = downscale_entry_check(c, "downscale_depth_u16", src, rows, cols, row_stride, factor, dst, dst_row_stride, &empty)) return rc;
  if (empty) return VSLAM_OK;
  const int orows = ds_out(rows, factor), ocols = ds_out(cols, factor);
  Call k(c, c->stream);
  // the device copies keep the caller's 4-byte phase: the kernel chooses its loads by it
  const size_t ne = (size_t)(orows * factor - 1) * row_stride + (size_t)ocols * factor, nd = (size_t)(orows - 1) * dst_row_stride + ocols;
  uint16_t* ds = k.dev<uint16_t>(ne + 2) + (((uintptr_t)src & 3u) >> 1);
  k.up_to(ds, src, ne);
  uint16_t* dd = k.dev<uint16_t>(nd + 2) + (((uintptr_t)dst & 3u) >> 1);
  DownscaleDepthArgs da{};
  da.src = ds; da.src_row_stride = row_stride; da.dst = dd; da.dst_row_stride = dst_row_stride; da.rows = orows; da.cols = ocols; da.n = 1; da.factor = factor;
  if (k.ok()) k.note(downscale_depth_enqueue(c->stream, da));
  if (k.ok()) k.note(hipMemcpy2DAsync(dst, (size_t)dst_row_stride * 2, dd, (size_t)dst_row_stride * 2, (size_t)ocols * 2, (size_t)orows, hipMemcpyDeviceToHost, c->stream));
  return k.finish();
}

// ---- Gaussian / median smoothing of one host image (kernels_smooth.h): dense dst ----------------------------------------
VS_API int vslam_smooth_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int mode, int32_t ksize, uint8_t* dst) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 0 || cols < 0) return fail(c, VSLAM_ERR_INVALID, "smooth_u8: negative size");
  if (mode != VSLAM_SMOOTH_GAUSSIAN && mode != VSLAM_SMOOTH_MEDIAN) return fail(c, VSLAM_ERR_INVALID, "smooth_u8: unknown mode");
  if (!smooth_mode_ok(mode, ksize)) return fail(c, VSLAM_ERR_INVALID, "smooth_u8: a ksize the mode does not have");
  if (rows == 0 || cols == 0) return VSLAM_OK;
  std::string why;
  if (const int rc = smooth_check("smooth_u8", mode, ksize, rows, cols, &why)) return fail(c, rc, why);
  if (!src || !dst || row_stride < cols) return fail(c, VSLAM_ERR_INVALID, "smooth_u8: bad argument");
  Call k(c, c->stream);
  // the device copies keep the caller's alignment: source rows and destination dwords start where they would in place
  const size_t bytes = (size_t)(rows - 1) * row_stride + (size_t)cols;
  uint8_t* ds = k.dev<uint8_t>(bytes + 16) + (size_t)((uintptr_t)src & 15u);
  k.up_to(ds, src, bytes);
  uint8_t* dd = k.dev<uint8_t>((size_t)rows * cols + 16) + (size_t)((uintptr_t)dst & 15u);
  SmoothArgs sa{};
  place(sa, ds, row_stride, dd, cols, rows, cols);
  sa.mode = mode; sa.ksize = ksize;
  if (k.ok()) k.note(smooth_enqueue(c->stream, sa));
  k.down(dst, dd, (size_t)rows * cols);
  return k.finish();
}

// ---- the colour of n pixels of one host image, direct or through a remap map pair (kernels_map_color.h) --------------
VS_API int vslam_sample_color_u8(vslam_ctx* c, const uint8_t* src, int32_t rows, int32_t cols, int32_t row_stride, int format, const int16_t* map_xy,
                                 const uint16_t* map_a, int32_t map_rows, int32_t map_cols, const int16_t* xy, int32_t n, uint8_t* rgb) {
  if (int rc = entry_begin(c)) return rc;
  if (rows < 0 || cols < 0 || n < 0) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: negative size");
  if (format < VSLAM_PIXEL_BGR8 || format > VSLAM_PIXEL_RGBA8) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: unknown pixel format");
  if ((map_xy == nullptr) != (map_a == nullptr)) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: both maps or none");
  const bool mapped = map_xy != nullptr;
  if (mapped && (map_rows < 0 || map_cols < 0)) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: negative map size");
  const int64_t wb = (int64_t)gray_channels(format) * cols;
  if ((int64_t)row_stride < wb || (!src && rows > 0 && cols > 0)) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: bad argument");
  if (n == 0) return VSLAM_OK;
  if (!xy || !rgb) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: bad argument");
  const size_t nm = mapped ? (size_t)map_rows * (size_t)map_cols : 0;
  if (mapped && !rect_maps_ok(map_a, nm)) return fail(c, VSLAM_ERR_INVALID, "sample_color_u8: interpolation table index >= 1024");
  Call k(c, c->stream);
  const bool empty = rows == 0 || cols == 0;
  const size_t bytes = empty ? 0 : (size_t)(rows - 1) * row_stride + (size_t)wb;
  const size_t off = (size_t)((uintptr_t)src & 15u);       // the device copy keeps the caller's alignment: rows start where they would in place
  uint8_t* ds = k.dev<uint8_t>(bytes + 16);
  k.up_to(ds + off, src, bytes);
  ColorSrc cs{};
  cs.img = ds + off; cs.row_stride = row_stride; cs.rows = rows; cs.cols = cols; cs.format = format;
  if (mapped) { cs.map_xy = k.up(map_xy, nm * 2); cs.map_a = k.up(map_a, nm); cs.map_stride = map_cols; cs.map_rows = map_rows; cs.map_cols = map_cols; }
  const int16_t* dxy = k.up(xy, (size_t)n * 2);
  uint32_t* dw = k.dev<uint32_t>((size_t)n);
  if (k.ok()) hipLaunchKernelGGL(k_sample_color, dim3((n + 255) / 256), dim3(256), 0, c->stream, cs, dxy, n, dw);
  std::vector<uint32_t> w((size_t)n);
  k.down(w.data(), dw, (size_t)n);
  const int rc = k.finish();
  if (rc != VSLAM_OK) return rc;
  for (int32_t i = 0; i < n; ++i) { rgb[3 * i] = (uint8_t)w[i]; rgb[3 * i + 1] = (uint8_t)(w[i] >> 8); rgb[3 * i + 2] = (uint8_t)(w[i] >> 16); }
  return VSLAM_OK;
}
