// kernels_frame2.h — second half of the frame kernel: the PoseTracker3D control flow that strings prune, recovery (kernels_recover.h), landmark
// refinement (kernels_frame_lm.h) and the stereo step (kernels_stereo.h) together, the frame's closing step, and the one-thread resets and setters.
#pragma once
#include "kernels_stereo.h"
#include "kernels_report.h"
#include "kernels_frame_lm.h"

// ==============================================================================================
// K5: PoseTracker3D::compute for one stream (pose_tracker_3d.cpp:32-222)
// ==============================================================================================
__device__ __forceinline__ void set_pose(const DevCfg& c, const DevBuf& b, int s, int f, const double* c2w) {
  double* hp = hpose_of(c, b, s, f);
  for (int k = 0; k < 12; ++k) hp[k] = c2w[k];
  tf_inverse(c2w, hp + 12);
}


// The frame's closing step, by one thread: the current frame's point count, what the stream carries to the next frame, the frame's report and the pose
// log.  The fused frame passes the values of its FrameCarry, the stage path those of its StreamState; what only one of them reports stays with it.
__device__ __forceinline__ void frame_close(const DevCfg& c, const DevBuf& b, int s, StreamState& st, vslam_frame_info& info, const FrameShared& sh, int pb_cur,
                                            int f, int status, int n_active, int win, double tau_track, double tau_tri, const double* prior) {
  const double* c2w = hpose_of(c, b, s, f);
  *pts_of(c, b, s, pb_cur).n = sh.n_cur;
  st.n_tracked_landmarks_prev = n_active;
  st.frame_count = f + 1; st.has_prev = 1; st.cur = pb_cur;
  info.frame_index = f + 1; info.status = status;
  info.n_keypoints_left = b.n_kp[s * 2]; info.n_keypoints_right = b.n_kp[s * 2 + 1];
  int rl = 0, rr = 0;
  for (int r = 0; r < c.n_regions; ++r) { rl += b.iinfo[s].raw_count[0][r]; rr += b.iinfo[s].raw_count[1][r]; info.thresholds[r] = b.iinfo[s].thr_after[r]; }
  for (int r = c.n_regions; r < VSLAM_MAX_REGIONS; ++r) info.thresholds[r] = 0;
  info.n_detected_left = rl; info.n_detected_right = rr;
  info.n_new_stereo = sh.n_cand; info.n_points = sh.n_cur; info.window_pixels = win;
  info.error_flags = ld_relaxed(&st.error_flags); info.tau_track = tau_track; info.tau_triangulation = tau_tri;
  for (int k = 0; k < 12; ++k) { info.camera_left_to_world[k] = c2w[k]; info.previous_to_current[k] = prior[k]; }
  if (f < VS_POSE_LOG) { double* pl = b.pose_log + ((size_t)s * VS_POSE_LOG + f) * 12; for (int k = 0; k < 12; ++k) pl[k] = c2w[k]; }
}

// Phase 2 of the frame (status switch, stereo sweep + binning + emission, the frame's closing step): the end of k_frame, and the frame workgroups of
// k_tail_lm.  sh.n_cur / sh.n_cand are set by the caller.
__device__ __forceinline__ void frame_phase2(const DevCfg& c, const DevBuf& b, int s, StreamState& st, vslam_frame_info& info, FrameCarry& fc, FrameShared& sh,
                                             int pb_cur, int f, unsigned char* arena) {
  const int tid = threadIdx.x;
  const int n_active = fc.n_active;
  int status = fc.status;
  if (n_active > c.c.minimum_number_of_landmarks_to_track) status = VSLAM_TRACKING;
  const double tau_tri2 = fc.tau_tri;
  const unsigned long long ts = wall_clock64();
  wg_stereo(c, b, s, sh, pb_cur, tau_tri2, f, arena);
  if (tid == 0) {
    st.ticks[4] += wall_clock64() - ts;
    // the dead-reckoning limit (no reference counterpart): frames in a row whose pose is not an accepted aligner result;
    // at the limit a Tracking stream localizes again — pose and prior stay
    const int dr = fc.moved ? 0 : min(st.dr_count, 0x3fffffff) + 1;     // saturates: a stream may stand still for ever
    st.dr_count = dr;
    if (c.dead_reckoning_limit > 0 && dr >= c.dead_reckoning_limit && status == VSLAM_TRACKING) status = VSLAM_LOCALIZING;
    const double* c2w = hpose_of(c, b, s, f);
    st.status = status; st.win = fc.win; st.tau_track = fc.tau_track; st.tau_tri = tau_tri2;
    for (int k = 0; k < 12; ++k) { st.prior[k] = fc.prior[k]; st.pose[k] = c2w[k]; }
    st.aligner_valid = fc.aligner_valid;
    info.status_at_start = fc.status0;
    info.track_attempts = fc.attempts; info.n_after_prune = fc.n_after_prune; info.n_recovered = fc.n_recovered;
    info.n_active_landmarks = n_active; info.track_broken = fc.broken; info.fallback = fc.fallback;
    frame_close(c, b, s, st, info, sh, pb_cur, f, status, n_active, fc.win, fc.tau_track, tau_tri2, fc.prior);
    st.dbg[8] += wall_clock64() - fc.t0;
  }
}

// The landmark-team workgroups that run beside the frame workgroups of a launch (k_tail_lm, k_stage_lm): workgroup i of G per stream
__device__ __forceinline__ void lm_team_workgroup(const DevCfg& c, const DevBuf& b, int i, int G, FrameShared& sh, unsigned char* arena) {
  const int sl = i / G, s = b.s0 + sl;
  if (!vs_active(b, s)) return;
  lm_teams_body(c, b, s, i - sl * G, G, arena, sh.flag, sh.n_proj);
}

// The frame's steps:
//   phase 0  track resolution, registration (aligner, recursion, fallback / break), prune, recovery projection
//   phase 1  recovery BRIEF + append, history publication
//   phase 2  landmark creation / refinement, status switch, stereo sweep + binning + emission, report
// phase < 0 runs everything in one launch (launch sequence 0, many streams).  Launch sequence 4 (up to VS_SPLIT4_MAX_STREAMS streams) runs
//   phase 0      this kernel
//   [k_recover_brief]  BRIEF of the projected lost points, all streams, one wavefront each (the ~140 recovery patches of a frame spread over
//                      the idle CUs: 67 -> 9 us)
//   phase 4      this kernel: phase 1 without the BRIEF, plus the count of active landmarks
//   [k_tail_lm]  phase 2 with the landmark refinement in workgroups of its own BESIDE it (nothing of phase 2 reads what the refinement
//                writes — landmark coordinates and update counts of the tracked points; the next frame's phase 0 does)
// The configuration and the buffer table arrive as pointers into the CONSTANT address space (device-resident copies the
// context uploads once): passed by value, the ~60 pointers of DevBuf are all loaded in the prologue, cannot stay in the
// 100-odd SGPRs and are parked in VGPR lanes — 1900 v_readlane instructions kernel-wide, ~190 in every aligner round.
// Through the constant address space each use is a scalar load next to where it is needed.
typedef const DevCfg __attribute__((address_space(4))) ConstDevCfg;
typedef const DevBuf __attribute__((address_space(4))) ConstDevBuf;
__global__ VS_FRAME_BOUNDS void k_frame(ConstDevCfg* cp, ConstDevBuf* bp, int phase) {
  const DevCfg& c = *(const DevCfg*)cp;
  const DevBuf& b = *(const DevBuf*)bp;
  __shared__ FrameShared sh;
  __shared__ __align__(16) unsigned char arena[VS_ARENA];
  const int s = b.s0 + xcd_local_stream(blockIdx.x, gridDim.x, b.xcd_rot), tid = threadIdx.x;
  if (!vs_active(b, s)) return;
  StreamState& st = b.st[s];
  vslam_frame_info& info = b.info[s];
  const int f = st.frame_count;             // index of the frame being processed
  const int has_prev = st.has_prev;
  const int pb_prev = st.cur, pb_cur = st.cur ^ 1;
  const int status0 = st.status;
  const int n_lm_prev = st.n_tracked_landmarks_prev;
  FrameCarry& fc = st.fc;
  if (phase <= 0) {   // ======================================= phase 0 =======================================
  if (tid == 0) {
    sh.status = status0; sh.win = st.win; sh.tau_track = st.tau_track; sh.attempts = 0; sh.broken = 0; sh.fallback = 0;
    sh.aligner_ran = 0; sh.n_trk = 0; sh.n_lost = 0; sh.n_lm = 0; sh.n_cur = 0; sh.n_cand = 0; sh.its = 0; sh.conv = 0; sh.n_proj = 0;
    sh.inl = 0; sh.outl = 0; sh.E = 0; sh.flag = 0;
    for (int k = 0; k < 12; ++k) sh.T[k] = 0;
    for (int k = 0; k < 36; ++k) sh.H[k] = 0;
    set_pose(c, b, s, f, st.pose);          // frame created at WorldMap::robot_to_world
  }
  const unsigned long long tK0 = wall_clock64();
  (void)tK0;
  // the motion prior lives in LDS (sh.prior), not in 24 VGPRs of every thread across the whole registration loop
  if (tid < 12) sh.prior[tid] = st.prior[tid];
  const double* prior = sh.prior;
  const double tau_tri = tau_tri_rule(c, status0, b.n_kp[s * 2]);
  int win = st.win;
  double tau_track = st.tau_track;          // tracker's _current_descriptor_distance_tracking
  double tau_gen = tau_track;               // generator's _maximum_descriptor_distance_tracking (last _track)
  __syncthreads();
  const double* prev_c2w = hpose_of(c, b, s, f > 0 ? f - 1 : 0);
  int n_tracked_landmarks = 0, n_after_prune = 0;
  bool aligner_valid = false;
  bool moved = false;                       // the pose is an accepted aligner result
  // CAMERA_ODOMETRY never breaks the track and never retries by appearance with an identity prior: it dead-reckons on the guess
  // (:316-341, :405-417, :555-559)
  const bool odometry = c.motion_model == VSLAM_MOTION_CAMERA_ODOMETRY;

  if (has_prev) {
    const PtView pv = pts_of(c, b, s, pb_prev);
    const int P = *pv.n;
    for (int i = tid; i < P; i += VS_WG) pv.meta[(size_t)i * META + M_NEXT] = 0;
    __syncthreads();
    // ---- up to three track/register attempts (_registerRecursive, :300-419) -----------------------
    int by_app = status0 == VSLAM_LOCALIZING;
    bool done = false;
    for (int attempt = 0; attempt < 3 && !done; ++attempt) {
      // _track (:225-298)
      if (by_app) win = c.c.maximum_projection_tracking_distance_pixels;
      tau_gen = tau_track;
      if (attempt > 0) {
        const unsigned long long tc = wall_clock64();
        // initialize(frame, false): fresh feature stores; candidates for the new prior / window / mode
        const int lane = tid % VS_CGL, w = tid / VS_CGL;
        for (int i = w; i < P; i += VS_WG / VS_CGL) candidates_wave(c, b, s, pb_prev, i, lane, reinterpret_cast<CandWave*>(arena) + w, prior, win, tau_gen, tau_tri, by_app);
        __syncthreads();
        if (tid == 0) st.ticks[0] += wall_clock64() - tc;
      }
      aligner_valid = false;
      unsigned long long t0 = wall_clock64();
      wg_track_resolve(c, b, s, sh, pb_prev, arena, win, tau_gen, tau_tri, by_app);
      if (tid == 0) st.ticks[0] += wall_clock64() - t0;
      const int n_trk = sh.n_trk;
      n_tracked_landmarks = sh.n_lm;
      {
        const double ratio = (double)n_trk / (double)P;
        const double lm_per_pt = (double)n_tracked_landmarks / (double)n_trk;
        const double succ = (double)n_trk / (double)c.target_kp;
        const int wmax = c.c.maximum_projection_tracking_distance_pixels, wmin = c.c.minimum_projection_tracking_distance_pixels;
        if (ratio < c.c.good_tracking_ratio / 2) {
          if (win < wmax) win = (int)fmin(win * 1 / c.c.tunnel_vision_ratio, (double)wmax);
        } else {
          if (win > wmin) win = (int)fmax(win * c.c.tunnel_vision_ratio, (double)wmin);
        }
        if (ratio < c.c.good_tracking_ratio || n_trk < c.c.aligner_minimum_number_of_inliers || (lm_per_pt < 0.5 && succ < 0.25)) {
          tau_track += 5;
          if (tau_track > c.c.maximum_descriptor_distance_tracking) tau_track = c.c.maximum_descriptor_distance_tracking;
        } else {
          tau_track -= 5;
          if (tau_track < c.c.minimum_descriptor_distance_tracking) tau_track = c.c.minimum_descriptor_distance_tracking;
        }
      }
      if (tid == 0) ++sh.attempts;
      // ---- registration ------------------------------------------------------------------------------
      bool accept = false, fall = false, brk = false;
      if (status0 == VSLAM_LOCALIZING) {
        // :103-161
        if (n_trk < c.c.minimum_number_of_landmarks_to_track) {
          fall = true;
        } else {
          const unsigned long long ta = wall_clock64();
          wg_align(c, b, s, sh, pb_prev, false, prior);
          if (tid == 0) st.ticks[1] += wall_clock64() - ta;
          aligner_valid = true;
          if (sh.inl < c.c.minimum_number_of_landmarks_to_track) fall = true; else accept = true;
        }
        done = true;
      } else {
        const double rel = (double)n_tracked_landmarks / (double)n_lm_prev;
        if (n_tracked_landmarks == 0 || rel < 0.1) {
          if (odometry) {
            // stick to the odometry guess (:323-328); on the third attempt _fallbackEstimate in the place of breakTrack (:333-336) — under
            // this model the same pose, previous · inverse(prior), with the prior kept (:555-559)
            fall = true; done = true;
          } else if (attempt < 2) {
            if (tid == 0) tf_identity(sh.prior);
            by_app = 1;
          } else {
            brk = true; done = true;
          }
        } else {
          const unsigned long long ta = wall_clock64();
          wg_align(c, b, s, sh, pb_prev, true, prior);
          if (tid == 0) st.ticks[1] += wall_clock64() - ta;
          aligner_valid = true;
          if (sh.inl > c.c.minimum_number_of_landmarks_to_track) {
            accept = true; done = true;
          } else if (attempt < 2) {
            if (win < c.c.maximum_projection_tracking_distance_pixels) ++win;
            by_app = 0;
          } else if (odometry) {
            fall = true; done = true;     // _fallbackEstimate in the place of breakTrack (:408-411)
          } else {
            brk = true; done = true;
          }
        }
      }
      bool move = false;     // the frame's pose is previous · inverse(prior)
      if (accept) {
        // accept-or-fallback on the size of the motion (:139-159, :372-388)
        const double dang = rotation_angle(sh.T);
        const double dtr = sqrt((sh.T[3] * sh.T[3] + sh.T[7] * sh.T[7]) + sh.T[11] * sh.T[11]);
        if (dang > c.c.minimum_delta_angular_for_movement || dtr > c.c.minimum_delta_translational_for_movement) {
          if (tid == 0) for (int k = 0; k < 12; ++k) sh.prior[k] = sh.T[k];
          move = true; moved = true;
        } else {
          fall = true;
        }
      }
      if (fall) {  // _fallbackEstimate (:551-566): under CAMERA_ODOMETRY the pose the guess gives, the prior kept (:555-559)
        if (tid == 0) sh.fallback = 1;
        if (odometry) move = true;
        else if (tid == 0) { tf_identity(sh.prior); set_pose(c, b, s, f, prev_c2w); }
      }
      if (move && tid == 0) {
        double inv[12], c2w[12];
        tf_inverse(sh.prior, inv);
        tf_mul(prev_c2w, inv, c2w);
        set_pose(c, b, s, f, c2w);
      }
      if (brk) {   // breakTrack (:422-435)
        if (tid == 0) { tf_identity(sh.prior); set_pose(c, b, s, f, prev_c2w); sh.broken = 1; sh.status = VSLAM_LOCALIZING; }
      }
      __syncthreads();
    }
    // report the final track() / converge() before their buffers are consumed
    if (tid == 0) {
      info.n_tracked = sh.n_trk; info.n_lost = sh.n_lost; info.n_tracked_landmarks = n_tracked_landmarks;
      info.aligner_ran = aligner_valid ? 1 : 0;
      info.aligner_iterations = aligner_valid ? sh.its : 0; info.aligner_converged = aligner_valid ? sh.conv : 0;
      info.n_inliers = aligner_valid ? sh.inl : 0; info.n_outliers = aligner_valid ? sh.outl : 0;
      info.total_error = aligner_valid ? sh.E : 0;
      st.al_n = aligner_valid ? sh.n_trk : 0;
      for (int k = 0; k < 12; ++k) st.al_T[k] = sh.T[k];
      for (int k = 0; k < 36; ++k) st.al_H[k] = sh.H[k];
    }
    VS_PHASE_BEGIN(tP);
    wg_prune(c, b, s, sh, pb_prev, pb_cur, aligner_valid);
    VS_PHASE_STAMP(6, tP);
    n_after_prune = sh.n_cur;
    if (c.c.enable_landmark_recovery) {
      if (phase < 0) wg_recover_project(c, b, s, sh.n_lost, pb_prev, hpose_of(c, b, s, f) + 12, reinterpret_cast<int32_t*>(arena + VS_RLIST_OFF), VS_RLIST_CAP, &sh.n_proj);
      else wg_recover_project(c, b, s, sh.n_lost, pb_prev, hpose_of(c, b, s, f) + 12);
    }
  } else if (tid == 0) {
    info.n_tracked = 0; info.n_lost = 0; info.n_tracked_landmarks = 0; info.aligner_ran = 0; info.aligner_iterations = 0;
    info.aligner_converged = 0; info.n_inliers = 0; info.n_outliers = 0; info.total_error = 0; st.al_n = 0;
  }
  __syncthreads();
  if (tid == 0) {
    fc.status = sh.status; fc.status0 = status0; fc.win = win; fc.attempts = sh.attempts; fc.broken = sh.broken; fc.fallback = sh.fallback;
    fc.n_after_prune = n_after_prune; fc.aligner_valid = aligner_valid ? 1 : 0; fc.n_tracked_landmarks = n_tracked_landmarks; fc.moved = moved ? 1 : 0;
    fc.n_cur = sh.n_cur; fc.n_lost = (has_prev && c.c.enable_landmark_recovery) ? sh.n_lost : 0; fc.n_recovered = 0; fc.n_active = 0;
    fc.tau_track = tau_track; fc.tau_gen = tau_gen; fc.tau_tri = tau_tri; fc.t0 = tK0;
    for (int k = 0; k < 12; ++k) fc.prior[k] = prior[k];
  }
  __syncthreads();
  if (phase == 0) return;
  }  // phase 0

  {   // ========================== phase 1 (4: + the count of active landmarks) ==========================
    if (tid == 0) { sh.n_cur = fc.n_cur; sh.n_lost = fc.n_lost; sh.flag = 0; }
    __syncthreads();
    if (has_prev && c.c.enable_landmark_recovery) {
      const unsigned long long tr = wall_clock64();
      if (phase < 0) {
        wg_recover_brief(c, b, s, pb_prev, sh.n_lost, sh.n_proj, fc.tau_gen, fc.tau_tri, arena);
        __syncthreads();
      }
      wg_recover_append(c, b, s, sh, pb_prev, pb_cur);
      if (tid == 0) { st.ticks[2] += wall_clock64() - tr; fc.n_recovered = sh.flag; }
    }
    wg_publish_history(c, b, s, sh.n_cur, pb_cur, f);
    if (tid == 0) { fc.n_cur = sh.n_cur; fc.n_active = 0; fc.lm_pb = pb_cur; fc.lm_f = f; }
    __syncthreads();
    if (phase == 4) {
      // the landmark kernel will run BESIDE phase 2: the number of active landmarks — what the status switch needs — is the number of points
      // whose track is long enough for a landmark (landmark_point returns false for nothing else)
      const int active = lm_count_active(c, b, s, pts_of(c, b, s, pb_cur), sh.n_cur);
      int total;
      block_exclusive_scan(active, sh.scan, &total);
      if (tid == 0) fc.n_active = total;
      return;
    }
  }

  // ========================================= phase 2 (fused) =========================================
  if (tid == 0) { sh.n_cur = fc.n_cur; sh.n_cand = 0; }
  __syncthreads();
  {
    const unsigned long long tu = wall_clock64();
    const int total = wg_landmarks_lds(c, b, s, sh, pb_cur, f, arena);
    if (tid == 0) { fc.n_active = total; st.ticks[3] += wall_clock64() - tu; }
    __syncthreads();
  }
  frame_phase2(c, b, s, st, info, fc, sh, pb_cur, f, arena);
}

// Launch sequence 4's last launch: the n frame workgroups run phase 2, G more workgroups per stream the landmark refinement (lm_teams_body) — ONE launch
// instead of a second queue with a fork and a join around it (each costs the frame queue ~7 us).  Nothing in phase 2 reads what the refinement writes.
// (Folding the recovery descriptors and phase 1 into the same launch as well — workgroups handing over through counters — was measured: every
// workgroup of a launch carries the frame workgroup's 140 KB of LDS, so the recovery workers own whole CUs and the next frame's image kernels lose
// them: 0.226 -> 0.232 ms for one stream, 0.292 -> 0.353 for eleven.)
__global__ VS_FRAME_BOUNDS void k_tail_lm(ConstDevCfg* cp, ConstDevBuf* bp, int n, int G) {
  const DevCfg& c = *(const DevCfg*)cp;
  const DevBuf& b = *(const DevBuf*)bp;
  __shared__ FrameShared sh;
  __shared__ __align__(16) unsigned char arena[VS_ARENA];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n) {
    const int s = b.s0 + xcd_local_stream(blockIdx.x, n, b.xcd_rot);
    if (!vs_active(b, s)) return;
    StreamState& st = b.st[s];
    FrameCarry& fc = st.fc;
    if (tid == 0) { sh.n_cur = fc.n_cur; sh.n_cand = 0; }
    __syncthreads();
    frame_phase2(c, b, s, st, b.info[s], fc, sh, st.cur ^ 1, st.frame_count, arena);
  } else {
    lm_team_workgroup(c, b, (int)blockIdx.x - n, G, sh, arena);
  }
}

// vslam_reset_stream, asynchronous: the stream state has an image-pipeline half (the detector thresholds, written by k_emit
// and read by k_fast_box on the image stream) and a tracker half (everything else, frame stream); each half is reset by a
// one-thread kernel queued on the HIP stream that owns it, so a stream restarts between two frames without a host sync.
struct ResetList { int32_t n; int32_t ids[63]; };   // streams restarted between two frames, one launch per half of the state
__global__ void k_reset_stream_img(const DevCfg c, const DevBuf b, const ResetList l) {
  if ((int)threadIdx.x >= l.n) return;
  const int s = l.ids[threadIdx.x];
  StreamState& st = b.st[s];
  for (int r = 0; r < VSLAM_MAX_REGIONS; ++r) st.thr[r] = r < c.n_regions ? c.c.detector_threshold_minimum : 0;
  atomicAnd(&st.error_flags, ~1);     // bit 0 (keypoint capacity) is raised by k_emit on this HIP stream
}
__global__ void k_reset_stream_trk(const DevCfg c, const DevBuf b, const ResetList l) {
  if ((int)threadIdx.x >= l.n) return;
  const int s = l.ids[threadIdx.x];
  StreamState& st = b.st[s];
  st.status = VSLAM_LOCALIZING; st.win = c.c.maximum_projection_tracking_distance_pixels; st.frame_count = 0; st.has_prev = 0;
  st.n_tracked_landmarks_prev = 0; st.cur = 0; st.aligner_valid = 0; atomicAnd(&st.error_flags, 1);
  st.tau_track = c.c.minimum_descriptor_distance_tracking; st.tau_tri = 0.1 * 256;
  tf_identity(st.prior); tf_identity(st.pose);
  tf_identity(st.guess); tf_identity(st.guess_prev); st.dr_count = 0;
  st.by_appearance = 0; st.n_trk = 0; st.n_lost = 0; st.n_tracked_landmarks = 0;
  st.al_n = 0; st.al_inliers = 0; st.al_outliers = 0; st.al_iterations = 0; st.al_converged = 0; st.al_wsize = 0; st.al_total_error = 0;
  st.tau_gen = 0; st.n_cur = 0; st.n_active = 0; st.n_after_prune = 0; st.n_recovered = 0; st.n_new = 0; st.track_calls = 0;
  b.n_points[s * 2] = 0; b.n_points[s * 2 + 1] = 0;
  vslam_frame_info& info = b.info[s];
  unsigned char* p = reinterpret_cast<unsigned char*>(&info);
  for (size_t k = 0; k < sizeof(vslam_frame_info); ++k) p[k] = 0;
}
// the current pose of every stream (camera_left_to_world of the frame just processed) -> dst[stream][12]
__global__ void k_gather_poses(const DevBuf b, int n, double* dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * 12) dst[i] = b.st[b.s0 + i / 12].pose[i % 12];
}

// setters of the tracker-owned state (one thread)
struct D12 { double v[12]; };   // a transform passed by value as a kernel argument (no staging buffer)
__global__ void k_set_tracker_state(const DevBuf b, int s, int status, int win, double tau, const D12 prior) {
  StreamState& st = b.st[s];
  st.status = status; st.win = win; st.tau_track = tau;
  for (int k = 0; k < 12; ++k) st.prior[k] = prior.v[k];
}
__global__ void k_set_pose(const DevBuf b, int s, const D12 pose) {
  StreamState& st = b.st[s];
  for (int k = 0; k < 12; ++k) st.pose[k] = pose.v[k];
}
