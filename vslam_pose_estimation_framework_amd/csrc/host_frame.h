// host_frame.h — one frame on a context: where its input images come from (device pointers, host uploads through pinned staging, raw
// pairs of a rectifying context), the image pipeline and the frame's launch sequence, the fused entries vslam_process_*, and the
// rectification, equalisation and colour-input switches.  Host code, included by vslam_hip.hip after host_ctx.h.
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
  if (c->col.format != VSLAM_PIXEL_GRAY8) {
    // colour pair -> grey pair where the next stage reads (set_color_inputs has chosen: the rectifier's raw slabs or upload[set])
    const vslam_ctx::Col& q = c->col;
    GrayArgs ga;
    for (int k = 0; k < 2; ++k) { ga.src[k] = q.src[k]; ga.dst[k] = q.out[k]; }
    ga.src_row_stride = q.src_row_stride; ga.src_stream_stride = q.src_stream_stride;
    ga.dst_row_stride = q.out_row_stride; ga.dst_stream_stride = q.out_stream_stride;
    ga.rows = q.out_rows; ga.cols = q.out_cols; ga.n = n; ga.sides = 2; ga.format = q.format;
    std::memcpy(ga.active, c->buf.active, sizeof ga.active);
    HIP_TRY(c, gray_enqueue(st, ga));
  }
  if (c->rect.on) {
    // raw pair -> rectified pair in upload[set] (the slab the wait above has freed), ahead of the detector
    const vslam_ctx::Rect& q = c->rect;
    RectArgs ra;
    // (with equalisation on as well: in slabs of its own, the equalised pair goes to upload[set])
    for (int k = 0; k < 2; ++k) { ra.src[k] = q.src[k]; ra.map_xy[k] = q.map_xy[k]; ra.map_a[k] = q.map_a[k]; ra.dst[k] = c->eq.keep[0] ? c->eq.keep[k] : c->upload[set][k]; }
    ra.src_stream_stride = q.src_stream_stride; ra.src_row_stride = q.src_row_stride; ra.src_rows = q.raw_rows; ra.src_cols = q.raw_cols;
    ra.map_stride = q.map_stride; ra.dst_stream_stride = c->up_stream_stride; ra.dst_row_stride = c->up_stride;
    ra.rows = d.c.rows; ra.cols = d.c.cols; ra.s0 = 0; ra.n = n; ra.sides = 2;
    std::memcpy(ra.active, c->buf.active, sizeof ra.active);
    hipLaunchKernelGGL(k_rectify, dim3((d.c.cols + 255) / 256, (d.c.rows + 3) / 4, 2 * ((n + VS_RECT_SB - 1) / VS_RECT_SB)), dim3(256), 0, st, ra);
  }
  if (c->eq.on) {
    // equalised pair in upload[set]: in place when the input is already there (host upload), written there from the rectified pair's own
    // slabs or from the caller's device images, which these two kernels alone read; everything downstream reads upload[set]
    vslam_ctx::Eq& q = c->eq;
    const bool in_place = !c->rect.on && c->buf.img[0] == c->upload[set][0];
    // one placement for both modes of the slot: global equalisation (k_hist_u8, k_equalize_apply) or CLAHE (k_clahe_lut, k_clahe_apply)
    const int32_t dst_row_stride = in_place ? c->buf.img_row_stride : c->up_stride;
    const size_t dst_stream_stride = in_place ? c->buf.img_stream_stride : c->up_stream_stride;
    auto place = [&](auto& x) {
      for (int k = 0; k < 2; ++k) { x.src[k] = c->rect.on ? q.keep[k] : c->buf.img[k]; x.dst[k] = c->upload[set][k]; }
      x.src_row_stride = c->rect.on ? c->up_stride : c->buf.img_row_stride;
      x.src_stream_stride = c->rect.on ? c->up_stream_stride : c->buf.img_stream_stride;
      x.dst_row_stride = dst_row_stride; x.dst_stream_stride = dst_stream_stride;
      x.rows = d.c.rows; x.cols = d.c.cols; x.n = n; x.sides = 2;
      std::memcpy(x.active, c->buf.active, sizeof x.active);
    };
    if (q.clahe) { ClaheArgs ca = q.geo; place(ca); ca.luts = q.luts; HIP_TRY(c, clahe_enqueue(st, ca)); }
    else { EqArgs ea; place(ea); ea.hist = q.hist; HIP_TRY(c, equalize_enqueue(st, ea)); }
    for (int k = 0; k < 2; ++k) { c->buf.img[k] = c->upload[set][k]; q.out[k] = c->upload[set][k]; }
    c->buf.img_row_stride = q.out_row_stride = dst_row_stride; c->buf.img_stream_stride = q.out_stream_stride = dst_stream_stride;
  }
  const DevBuf bs = buf_set(c, set, c->img_override ? c->q0_frm : c->q0_img);
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
// this frame's left colour image as k_map_color reads it: the raw image behind the left rectification map while rectifying
static ColorSrc map_color_src(const vslam_ctx* c) {
  const vslam_ctx::Col& q = c->col;
  ColorSrc s{};
  s.img = q.src[0]; s.stream_stride = q.src_stream_stride; s.row_stride = q.src_row_stride; s.rows = q.out_rows; s.cols = q.out_cols; s.format = q.format;
  if (c->rect.on) { s.map_xy = c->rect.map_xy[0]; s.map_a = c->rect.map_a[0]; s.map_stride = c->rect.map_stride; s.map_rows = c->cfg.c.rows; s.map_cols = c->cfg.c.cols; }
  return s;
}
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
  // the map's colours, from this frame's left colour image (through the left rectification map when rectifying) at the ids of this frame
  if (c->mapcol.rgb) hipLaunchKernelGGL(k_map_color, dim3(n), dim3(VS_MAP_COLOR_WG), 0, st, c->cfg, bs, c->map.d, map_color_src(c), c->mapcol.rgb);
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
// Colour input: host pairs go to the colour slabs of this step's parity (upload_to with the byte width as cols), device pairs are read in
// place (by k_gray_u8, and by k_map_color behind the frame's last launch while map colours are on).  The grey pair is written where the next stage reads: the rectifier's raw slabs when rectifying, else
// upload[parity]; DevBuf::img points at upload[parity] either way, as it does for a grey host frame.
static int set_color_inputs(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, bool on_device) {
  vslam_ctx::Col& q = c->col;
  vslam_ctx::Rect& rq = c->rect;
  const int rows = rq.on ? rq.raw_rows : c->cfg.c.rows, cols = rq.on ? rq.raw_cols : c->cfg.c.cols;
  const int wb = gray_channels(q.format) * cols;
  if (!L || !R) return fail(c, VSLAM_ERR_INVALID, "called with empty frame");
  if (row_stride < wb) return fail(c, VSLAM_ERR_INVALID, "row stride smaller than channels * image width");
  ImgLoc o = {{L, R}, row_stride, image_stride};
  if (!on_device) {
    // map colours: k_map_color read this parity's slab on the FRAME queue two steps ago, and the upload below is issued ahead of the wait in
    // launch_image_pipeline — it waits for that frame here (without the switch k_gray_u8, on the image queue itself, is the slab's last reader).
    // Every queue upload_to may copy on: its dense path takes img_override when set (the stage path of one stream: the frame queue itself,
    // already in order behind k_map_color, hence skipped), its strided paths always the image queue.
    if (c->mapcol.rgb && c->frm_pending[c->parity]) {
      hipStream_t up[2] = {c->img_override ? c->img_override : c->stream_img, c->stream_img};
      for (int k = 0; k < 2; ++k)
        if (up[k] != c->stream && (k == 0 || up[k] != up[0])) HIP_TRY(c, hipStreamWaitEvent(up[k], c->ev_frm[c->parity], 0));
    }
    const int rc = upload_to(c, L, R, row_stride, image_stride, rows, wb, q.slab[c->parity], q.stride, q.stream_stride, &o);
    if (rc != VSLAM_OK) return rc;
  }
  q.src[0] = o.p[0]; q.src[1] = o.p[1]; q.src_row_stride = o.row_stride; q.src_stream_stride = o.stream_stride;
  q.out_rows = rows; q.out_cols = cols;
  for (int k = 0; k < 2; ++k) q.out[k] = rq.on ? rq.raw[c->parity][k] : c->upload[c->parity][k];
  q.out_row_stride = rq.on ? rq.raw_stride : c->up_stride;
  q.out_stream_stride = rq.on ? rq.raw_stream_stride : c->up_stream_stride;
  if (rq.on) { rq.src[0] = q.out[0]; rq.src[1] = q.out[1]; rq.src_row_stride = q.out_row_stride; rq.src_stream_stride = q.out_stream_stride; }
  return set_images_device(c, c->upload[c->parity][0], c->upload[c->parity][1], c->up_stride, c->up_stream_stride);
}
static int set_inputs(vslam_ctx* c, const uint8_t* L, const uint8_t* R, int32_t row_stride, size_t image_stride, bool on_device) {
  if (c->col.format != VSLAM_PIXEL_GRAY8) return set_color_inputs(c, L, R, row_stride, image_stride, on_device);
  if (c->rect.on) return set_raw_inputs(c, L, R, row_stride, image_stride, on_device);
  return on_device ? set_images_device(c, L, R, row_stride, image_stride) : upload_images(c, L, R, row_stride, image_stride);
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
  if (off) { (void)eq_keep_sync(c); return col_slab_sync(c) == hipSuccess ? VSLAM_OK : fail(c, VSLAM_ERR_HIP, "vslam_set_rectification: colour slabs"); }
  vslam_ctx::Rect& q = c->rect;
  q.raw_rows = raw_rows; q.raw_cols = raw_cols;
  q.raw_stride = (raw_cols + 63) & ~63;
  q.raw_stream_stride = (size_t)raw_rows * q.raw_stride;
  q.map_stride = (cols + 3) & ~3;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {
    e = q.mem.alloc(&q.map_xy[k], (size_t)rows * q.map_stride * 2);
    if (e == hipSuccess) e = q.mem.alloc(&q.map_a[k], (size_t)rows * q.map_stride);
    for (int p = 0; p < 2 && e == hipSuccess; ++p) e = q.mem.alloc(&q.raw[p][k], (size_t)c->B * q.raw_stream_stride);
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
  e = eq_keep_sync(c);
  if (e == hipSuccess) e = col_slab_sync(c);
  if (e != hipSuccess) { rect_free(c); return fail(c, VSLAM_ERR_HIP, std::string("vslam_set_rectification: ") + hipGetErrorString(e)); }
  return VSLAM_OK;
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
VS_API int vslam_get_rectified_images(vslam_ctx* c, int s, uint8_t* left, uint8_t* right) {
  const int rc = check_stream(c, s);
  if (rc != VSLAM_OK) return rc;
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_rectified_images: null output");
  if (!c->rect.on || !c->rect.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_rectified_images: no frame has been rectified since vslam_set_rectification");
  const int rows = c->cfg.c.rows, cols = c->cfg.c.cols;
  for (int k = 0; k < 2; ++k)
    HIP_TRY(c, hipMemcpy2D(k ? right : left, cols, (c->eq.keep[0] ? c->eq.keep[k] : c->upload[c->last_set][k]) + (size_t)s * c->up_stream_stride,
                           c->up_stride, cols, rows, hipMemcpyDeviceToHost));
  return VSLAM_OK;
}

// ---- histogram equalisation of the input pair (kernels_equalize.h) -------------------------------
// The slot's switch.  geo null: global equalisation, else CLAHE with what clahe_geometry made of the caller's arguments.  The two modes
// exclude each other; switching one off while the other is on changes nothing.
static int eq_switch(vslam_ctx* c, const char* who, bool on, const ClaheArgs* geo, double clip_limit) {
  const bool clahe = geo != nullptr;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, std::string(who) + " called inside a frame");
  if (c->eq.on && c->eq.clahe != clahe)
    return !on ? VSLAM_OK : fail(c, VSLAM_ERR_STATE, std::string(who) + (clahe ? ": global equalisation is on (vslam_set_equalization)" : ": CLAHE is on (vslam_set_clahe)"));
  const bool same = !clahe || (c->eq.clip_limit == clip_limit && c->eq.geo.tiles_x == geo->tiles_x && c->eq.geo.tiles_y == geo->tiles_y);
  if (on ? (c->eq.on && same) : !c->eq.on) return VSLAM_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  sync_all(c);                     // the frames in flight still read the tables and the slabs
  eq_free(c);
  if (!on) return VSLAM_OK;
  hipError_t e;
  if (!clahe) {
    e = c->eq.mem.alloc(&c->eq.hist, (size_t)c->B * 2 * 256);
    if (e == hipSuccess) e = hipMemset(c->eq.hist, 0, (size_t)c->B * 2 * 256 * sizeof(uint32_t));
  } else {
    c->eq.geo = *geo; c->eq.clip_limit = clip_limit;
    const size_t nl = (size_t)c->B * 2 * geo->tiles_x * geo->tiles_y * 256;
    e = c->eq.mem.alloc(&c->eq.luts, nl);
    if (e == hipSuccess) e = hipMemset(c->eq.luts, 0, nl);
  }
  c->eq.on = e == hipSuccess;
  c->eq.clahe = c->eq.on && clahe;
  if (e == hipSuccess) e = eq_keep_sync(c);
  if (e != hipSuccess) { eq_free(c); return fail(c, VSLAM_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }
  return VSLAM_OK;
}
VS_API int vslam_set_equalization(vslam_ctx* c, int on) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_equalization called inside a frame");
  if ((size_t)c->cfg.c.rows * c->cfg.c.cols > (size_t)VS_EQ_MAX_PIXELS) return fail(c, VSLAM_ERR_INVALID, "vslam_set_equalization: more than 2^24 pixels per image");
  return eq_switch(c, "vslam_set_equalization", on != 0, nullptr, 0);
}

// ---- CLAHE of the input pair: the second mode of the equalisation slot (kernels_clahe.h) ----------
VS_API int vslam_set_clahe(vslam_ctx* c, int on, double clip_limit, int tiles_x, int tiles_y) {
  if (!c) return VSLAM_ERR_INVALID;
  if (c->frame_begun) return fail(c, VSLAM_ERR_STATE, "vslam_set_clahe called inside a frame");
  ClaheArgs geo;
  std::memset(&geo, 0, sizeof geo);
  const char* why = "";
  if (on && !clahe_geometry(c->cfg.c.rows, c->cfg.c.cols, clip_limit, tiles_x, tiles_y, geo, &why)) return fail(c, VSLAM_ERR_INVALID, std::string("vslam_set_clahe: ") + why);
  return eq_switch(c, "vslam_set_clahe", on != 0, &geo, clip_limit);
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
  const vslam_ctx::Col& q = c->col;
  if (q.format == VSLAM_PIXEL_GRAY8 || !q.have_frame) return fail(c, VSLAM_ERR_STATE, "vslam_get_gray_images: no frame has been converted since vslam_set_color_input");
  if (!left || !right) return fail(c, VSLAM_ERR_INVALID, "vslam_get_gray_images: null output");
  for (int k = 0; k < 2; ++k)
    HIP_TRY(c, hipMemcpy2D(k ? right : left, q.out_cols, q.out[k] + (size_t)s * q.out_stream_stride, q.out_row_stride, q.out_cols, q.out_rows,
                           hipMemcpyDeviceToHost));
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
