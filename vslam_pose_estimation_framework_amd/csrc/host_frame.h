// host_frame.h — one frame on a context: where its input images come from (device pointers, host uploads through pinned staging), its
// routing through the input stages (route_frame, from the route of stage_plan.h), the image pipeline and the frame's launch sequence, and the fused entries
// vslam_process_*.  Host code, included by vslam_hip.hip after host_switches.h.
#pragma once

// ---- launches ------------------------------------------------------------------------------------
// workgroups of k_report by what it packs (kernels_report.h)
static int report_blocks(int what) {
  return what == VS_REPORT_KEYPOINTS ? 32 : what == VS_REPORT_POINTS ? 16 : what == VS_REPORT_KEYPOINTS_XY ? 8 : 4;
}
// one stage report of stream s on queue q, stamped with the next sequence number (returned: the report's header carries it back)
static int report_launch(vslam_ctx* c, hipStream_t q, const DevBuf& bs, int s, int what, int in_progress) {
  const int seq = ++c->report_seq;
  hipLaunchKernelGGL(k_report, dim3(report_blocks(what)), dim3(256), 0, q, c->cfg, bs, s, what, in_progress, seq, c->rl, c->report_dev, c->report_done);
  return seq;
}
static int launch_image_pipeline(vslam_ctx* c) {
  const DevCfg& d = c->cfg;
  const int set = c->parity;
  const int n = c->B;
  hipStream_t st = c->img_override ? c->img_override : c->stream_img;
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
  // the input stages as route_frame has laid them out (the slabs they write are those the wait above has freed)
  HIP_TRY(c, prestage_enqueue(st, c->pre, c->rect.maps, c->eq, n, 2, c->buf.active));
  // detection masks (kernels_mask.h): nothing while none is set
  const bool masked = c->dmask.pending || c->dmask.stat[0] || c->dmask.stat[1];
  if (masked) { if (const int rc = mask_prepare(c, st)) return rc; } else c->dmask.last = 0;
  const DevBuf bs = buf_set(c, set, c->img_override ? c->q0_frm : c->q0_img);
  dim3 g1(d.TX, (d.c.rows + VS_TILE_H - 1) / VS_TILE_H, 2 * n);
  const bool orb = d.c.descriptor_type == VSLAM_DESCRIPTOR_ORB;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (coarse && c->timers) { e0 = ev_get(c); (void)hipEventRecord(e0, st); }
  { KernelTimer t(c, 0, st, true, !coarse); hipLaunchKernelGGL(k_fast_box, g1, dim3(256), VS_FB_DYN_LDS, st, c->cfg, bs); }
  { KernelTimer t(c, 1, st, true, !coarse); if (masked) mask_enqueue(c, st, bs); launch_emit(st, c->cfg, bs, n, 2, orb ? (int)VSLAM_ORB_BORDER : (int)VSLAM_BRIEF_BORDER, 1); }
  if (e0) { e1 = ev_get(c); (void)hipEventRecord(e1, st); c->evrec.push_back({e0, e1, 0, true}); c->kern_n[1] += 1; }
  if (c->img_override && c->report && c->B == 1) {
    // stage path with a view reader: coordinates and scores leave for the host as soon as k_emit has written them, so that the caller
    // builds its cv::KeyPoint lists while k_brief / k_stereo_dist / k_begin still run (vslam_view_keypoints_xy)
    // — read through report_xy_seq only: what report_note records about the frame queue's last report is left alone
    c->report_xy_seq = report_launch(c, st, bs, 0, VS_REPORT_KEYPOINTS_XY, 0);
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
  if (c->eq.on) c->eq.have_frame = true;
  if (c->col.format != VSLAM_PIXEL_GRAY8) c->col.have_frame = true;
  if (c->ds.factor > 1) c->ds.have_frame = true;
  if (c->sm.mode) c->sm.have_frame = true;
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
// this frame's left colour image as k_map_color reads it: the raw image behind the left rectification map while rectifying; while
// downscaling the full-size image, tapped by block averages at the reduced size
static ColorSrc map_color_src(const vslam_ctx* c) {
  const PrePlan& p = c->pre;
  const bool ds = p.factor > 1;
  return color_src(p.color, ds ? p.red_rows : p.in_rows, ds ? p.red_cols : p.in_cols, c->col.format, c->rect.on ? &c->rect.maps : nullptr, p.factor);
}
static int launch_frame(vslam_ctx* c) {
  const int n = c->B;
  hipStream_t st = c->stream;
  const DevBuf bs = buf_set(c, c->last_set, c->q0_frm);
  ConstDevCfg* kc = (ConstDevCfg*)c->d_cfg;
  ConstDevBuf* kb = (ConstDevBuf*)(c->d_bufs + c->last_set);
  // the frame's motion prior, ahead of the candidate kernel that reads it (nothing under CONSTANT_VELOCITY)
  if (const int rc = launch_motion_prior(c)) return rc;
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
  // the map's colours, from this frame's left colour image (through the left rectification map when rectifying) at the ids of this frame
  if (c->mapcol.rgb) hipLaunchKernelGGL(k_map_color, dim3(n), dim3(VS_MAP_COLOR_WG), 0, st, c->cfg, bs, c->map.d, map_color_src(c), c->mapcol.rgb);
  HIP_TRY(c, hipGetLastError());
  return frame_done(c);
}
// Host images of all streams (rows x cols each) into the device slabs dst[left/right] (dst_stride bytes per row, dst_stream_stride per
// stream); *out receives where they landed: one copy per side keeps the caller's strides.
static int upload_to(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, int rows, int cols,
                     uint8_t* const dst[2], int32_t dst_stride, size_t dst_stream_stride, ImgPlanes* out) {
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
// This frame's routing through the input stages: the plan's route (stage_plan.h, which alone decides it) turned into c->pre,
// the slot's src / dst, and DevBuf::img, which the detector reads.  `in`: where the incoming pair lies — the slab the upload filled, at the
// strides upload_to left it with, or the caller's device memory.  Every stage reads where the one before it left the pair.
static void route_frame(vslam_ctx* c, const StageSwitches& sw, const StageRoute& r, const ImgPlanes& in) {
  const int set = c->parity;
  PrePlan& p = c->pre;
  p.format = c->col.format; p.remap = sw.remap; p.factor = sw.factor;
  p.rows = sw.rows; p.cols = sw.cols;
  p.red_rows = sw.remap ? sw.raw_rows : sw.rows; p.red_cols = sw.remap ? sw.raw_cols : sw.cols;
  stage_in_size(sw, &p.in_rows, &p.in_cols);
  p.smooth_mode = c->sm.mode; p.smooth_ksize = c->sm.ksize;
  ImgPlanes cur = in;                                  // where the pair lies behind the stages so far
  auto hop = [&](const StageHop& h, ImgPlanes& src, ImgPlanes& dst) {
    if (!h.on) return;
    src = cur;
    dst = h.src == h.dst ? cur : slab_planes(c, h.dst, set);     // in place (the slot alone): a host upload keeps the caller's strides
    cur = dst;
  };
  hop(r.gray, p.color, p.gray);
  hop(r.down, p.full, p.reduced);
  hop(r.remap, p.raw, p.mapped);
  hop(r.smooth, p.unsmoothed, p.smoothed);
  hop(r.slot, c->eq.src, c->eq.dst);
  buf_set_planes(c->buf, cur);
}
// A frame's input pair.  Host images go to the slab of this step's parity that the plan names (the colour slabs take channels * width
// bytes per row); device images are read in place, by the first stage alone (and, colour, by k_map_color behind the frame's last launch
// while map colours are on).
static int set_inputs(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, bool on_device) {
  const StageSwitches sw = stage_switches(c);
  const StageRoute r = stage_route(sw, on_device);
  const bool colour = sw.channels != 0;
  int rows, cols;
  stage_in_size(sw, &rows, &cols);
  const int wb = colour ? sw.channels * cols : cols;
  if (!L || !R) return fail(c, VSLAM_ERR_INVALID, "called with empty frame");  // stereo_framepoint_generator.cpp:75-78
  if (row_stride < wb)
    return fail(c, VSLAM_ERR_INVALID, colour ? "row stride smaller than channels * image width" : sw.factor > 1 ? "row stride smaller than the full image width" : sw.remap ? "row stride smaller than the raw image width" : "row stride smaller than image width");
  ImgPlanes in = {{L, R}, row_stride, image_stride};
  if (!on_device) {
    // map colours: k_map_color read this parity's slab on the FRAME queue two steps ago, and the upload below is issued ahead of the wait in
    // launch_image_pipeline — it waits for that frame here (without the switch k_gray_u8, on the image queue itself, is the slab's last reader).
    // Every queue upload_to may copy on: its dense path takes img_override when set (the stage path of one stream: the frame queue itself,
    // already in order behind k_map_color, hence skipped), its strided paths always the image queue.
    if (colour && c->mapcol.rgb && c->frm_pending[c->parity]) {
      hipStream_t up[2] = {c->img_override ? c->img_override : c->stream_img, c->stream_img};
      for (int k = 0; k < 2; ++k)
        if (up[k] != c->stream && (k == 0 || up[k] != up[0])) HIP_TRY(c, hipStreamWaitEvent(up[k], c->ev_frm[c->parity], 0));
    }
    const ImgPlanes to = slab_planes(c, r.upload, c->parity);
    uint8_t* const dst[2] = {const_cast<uint8_t*>(to.p[0]), const_cast<uint8_t*>(to.p[1])};
    if (const int rc = upload_to(c, L, R, row_stride, image_stride, rows, wb, dst, to.row_stride, to.stream_stride, &in)) return rc;
  }
  route_frame(c, sw, r, in);
  return VSLAM_OK;
}

// the fused frame.  Host images: the context's device is made current first.  Device images: the caller's current device is left as it
// is (a caller such as torch may rely on that; the images already live on the context's device).
static int process_frame(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, bool on_device) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->sticky != VSLAM_OK) return c->sticky;
  if (!on_device) HIP_TRY(c, hipSetDevice(c->device));
  int rc = set_inputs(c, L, R, row_stride, image_stride, on_device);
  if (rc != VSLAM_OK) return rc;
  rc = flush_pending(c);
  if (rc != VSLAM_OK) return rc;
  rc = launch_image_pipeline(c);
  if (rc != VSLAM_OK) return rc;
  return launch_frame(c);
}
VS_API int vslam_process_device(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride) {
  return process_frame(c, L, R, row_stride, image_stride, true);
}
VS_API int vslam_process_host(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride) {
  return process_frame(c, L, R, row_stride, image_stride, false);
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
