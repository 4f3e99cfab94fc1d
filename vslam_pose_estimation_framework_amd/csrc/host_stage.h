// host_stage.h — the stage entries (the reference's plug-in virtuals one C call each; control flow stays with the caller), the setters
// between them, and the stage reports: the pinned report buffer, what the last launch on the frame queue packed into it, and the four
// views that read it.  Host code, included by vslam_hip.hip after host_frame.h (inputs, launch sequences, report_launch).
#pragma once

// ---- stage entry points (the reference's plug-in virtuals; control flow stays with the caller) ----------
// what the LAST launch on the frame queue packed into the report buffer: a view of exactly that needs no launch of its own
static void report_note(vslam_ctx* c, int what, int in_progress, int stream, int seq) {
  c->report_have = what; c->report_have_ip = in_progress; c->report_have_stream = stream; c->report_have_seq = seq;
}
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
    report_note(c, report, in_progress, 0, io.seq);
  }
  return io;
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
    const int seq = report_launch(c, c->stream, buf_set(c, c->last_set), 0, VS_REPORT_KEYPOINTS, 0);
    HIP_TRY(c, hipGetLastError());
    report_note(c, VS_REPORT_KEYPOINTS, 0, 0, seq);
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
      const int seq = report_launch(c, c->stream, buf_set(c, c->last_set), 0, VS_REPORT_POINTS, 0);
      HIP_TRY(c, hipGetLastError());
      report_note(c, VS_REPORT_POINTS, 0, 0, seq);
    }
    return frame_done(c);
  }
  int rc = launch_stage(c, VS_STAGE_COMPUTE, 0, VS_REPORT_POINTS, 0);
  return rc == VSLAM_OK ? frame_done(c) : rc;
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
// A report's completion flag (its seq, stored last with system-scope release) is polled in the pinned buffer: the caller's thread sees
// the stage end a few microseconds after the kernel's last store instead of waiting for the runtime's own completion path (~10-15 us per
// synchronisation, five per frame).  Bounded: after ~0.1 s without the flag the queue is synchronised the ordinary way (an inactive
// stream never writes a report: the callers' STATE error)
static int report_wait(vslam_ctx* c, const int32_t* flag, int seq) {
  for (long spin = 0; spin < 4000000L; ++spin) {
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return VSLAM_OK;
    __builtin_ia32_pause();
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
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
    seq = report_launch(c, c->stream, buf_set(c, c->last_set), s, what, in_progress);
    HIP_TRY(c, hipGetLastError());
    report_note(c, what, in_progress, s, seq);
  }
  const ReportHeader* h = reinterpret_cast<const ReportHeader*>(c->report);
  rc = report_wait(c, &h->seq, seq);
  if (rc) return rc;
  *hdr = h;
  if (__atomic_load_n(&h->seq, __ATOMIC_ACQUIRE) != seq || h->what != what) return fail(c, VSLAM_ERR_STATE, "stage report is stale (the stream is inactive?)");
  if ((*hdr)->info.error_flags) c->err = "device buffer capacity exceeded (error_flags != 0)";
  return VSLAM_OK;
}
// the keypoint lists of a report; with_desc false: the early report, whose descriptors are not there yet (vslam_view_keypoints brings them)
static void keypoints_view_fill(const vslam_ctx* c, const ReportHeader* h, bool with_desc, vslam_keypoints_view* out) {
  for (int d = 0; d < 2; ++d) {
    out->n[d] = std::min(h->n_kp[d], c->cfg.NMAX);
    out->xy[d] = reinterpret_cast<const int16_t*>(c->report + c->rl.kp_xy[d]);
    out->score[d] = c->report + c->rl.kp_score[d];
    out->desc[d] = with_desc ? c->report + c->rl.desc[d] : nullptr;
  }
}
VS_API int vslam_view_keypoints(vslam_ctx* c, int s, vslam_keypoints_view* out) {
  if (!c || !out) return VSLAM_ERR_INVALID;
  const ReportHeader* h = nullptr;
  int rc = report_run(c, s, VS_REPORT_KEYPOINTS, 0, &h);
  if (rc) return rc;
  keypoints_view_fill(c, h, true, out);
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
  keypoints_view_fill(c, h, false, out);
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
