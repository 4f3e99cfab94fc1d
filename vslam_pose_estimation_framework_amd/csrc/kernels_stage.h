// kernels_stage.h — stage-granular entry points: the same device functions as the frame kernel, one reference virtual per launch, with the
// control flow left to the caller (shim/proslam_hip_plugin.h keeps the reference's PoseTracker3D logic).
#pragma once
#include "kernels_frame2.h"

enum { VS_STAGE_TRACK = 1, VS_STAGE_ALIGN = 2, VS_STAGE_PRUNE_RECOVER = 3, VS_STAGE_UPDATE = 4, VS_STAGE_STEREO = 5, VS_STAGE_COMPUTE = 6 /* UPDATE then STEREO */,
       VS_STAGE_PRUNE_PROJECT = 7, VS_STAGE_RECOVER_APPEND = 8 /* PRUNE_RECOVER as two launches around the wide k_recover_brief */,
       VS_STAGE_STEREO_COUNT = 9 /* STEREO + the COUNT of active landmarks: their refinement runs beside the stage in the same launch (k_stage_lm) */ };

// WorldMap::createFrame + the bookkeeping PoseTracker3D::compute does before initialize() (:36-77)
// the caller's setters folded into a stage launch (StageIo): applied by one lane before anything reads the stream state
__device__ __forceinline__ void stage_apply_set(StreamState& st, const StageIo& io) {
  if (io.set_flags & 1) { st.status = io.status; st.win = io.win; st.tau_track = io.tau; for (int k = 0; k < 12; ++k) st.prior[k] = io.prior[k]; }
  if (io.set_flags & 2) { for (int k = 0; k < 12; ++k) st.pose[k] = io.pose[k]; }
}
__global__ __launch_bounds__(256) void k_begin(const DevCfg c, const DevBuf b, const StageIo io) {
  const int s = b.s0 + xcd_local_stream(blockIdx.x, gridDim.x, b.xcd_rot), tid = threadIdx.x;
  if (!vs_active(b, s)) return;
  StreamState& st = b.st[s];
  if (io.set_flags) { if (tid == 0) stage_apply_set(st, io); __syncthreads(); }
  const int f = st.frame_count;
  if (st.has_prev) {
    const PtView pv = pts_of(c, b, s, st.cur);
    const int P = *pv.n;
    for (int i = tid; i < P; i += blockDim.x) pv.meta[(size_t)i * META + M_NEXT] = 0;
  }
  if (tid == 0) {
    set_pose(c, b, s, f, st.pose);
    st.tau_tri = tau_tri_rule(c, st.status, b.n_kp[s * 2]);
    st.n_trk = 0; st.n_lost = 0; st.n_tracked_landmarks = 0; st.n_cur = 0; st.n_active = 0; st.al_n = 0;
    st.aligner_valid = 0; st.n_after_prune = 0; st.n_recovered = 0; st.n_new = 0; st.track_calls = 0;
    st.al_inliers = 0; st.al_outliers = 0; st.al_iterations = 0; st.al_converged = 0; st.al_total_error = 0;
    vslam_frame_info& info = b.info[s];
    info.status_at_start = st.status; info.fallback = 0; info.track_broken = 0;
  }
}

__device__ __forceinline__ void stage_body(const DevCfg& c, const DevBuf& b, int stage, int arg, const StageIo& io, FrameShared& sh, unsigned char* arena, int bx, int gx) {
  const int s = b.s0 + xcd_local_stream(bx, gx, b.xcd_rot), tid = threadIdx.x;
  if (!vs_active(b, s)) return;
  StreamState& st = b.st[s];
  vslam_frame_info& info = b.info[s];
  if (io.set_flags) { if (tid == 0) stage_apply_set(st, io); __syncthreads(); }
  const int f = st.frame_count;
  const int pb_prev = st.cur, pb_cur = st.cur ^ 1;
  const bool has_prev = st.has_prev != 0;
  if (tid == 0) {
    sh.n_trk = st.n_trk; sh.n_lost = st.n_lost; sh.n_lm = st.n_tracked_landmarks; sh.n_cur = st.n_cur; sh.n_cand = 0;
    sh.E = st.al_total_error; sh.inl = st.al_inliers; sh.outl = st.al_outliers; sh.its = 0; sh.conv = 0; sh.flag = 0;
  }
  __syncthreads();
  if (stage == VS_STAGE_TRACK && has_prev) {
    const double tau = st.tau_track;
    const unsigned long long t0 = wall_clock64();
    wg_track_resolve(c, b, s, sh, pb_prev, arena, st.win, tau, st.tau_tri, arg);
    if (tid == 0) {
      st.ticks[0] += wall_clock64() - t0;
      st.n_trk = sh.n_trk; st.n_lost = sh.n_lost; st.n_tracked_landmarks = sh.n_lm; st.aligner_valid = 0; st.tau_gen = tau;
      st.al_n = 0; st.track_calls += 1;
      info.n_tracked = sh.n_trk; info.n_lost = sh.n_lost; info.n_tracked_landmarks = sh.n_lm; info.track_attempts = st.track_calls;
      info.aligner_ran = 0;
    }
  } else if (stage == VS_STAGE_ALIGN && has_prev) {
    double T0[12];
    for (int k = 0; k < 12; ++k) T0[k] = st.prior[k];
    const unsigned long long t0 = wall_clock64();
    wg_align(c, b, s, sh, pb_prev, arg != 0, T0);
    if (tid == 0) {
      st.ticks[1] += wall_clock64() - t0;
      st.al_n = sh.n_trk; st.al_inliers = sh.inl; st.al_outliers = sh.outl; st.al_iterations = sh.its; st.al_converged = sh.conv;
      st.al_total_error = sh.E; st.aligner_valid = 1;
      for (int k = 0; k < 12; ++k) st.al_T[k] = sh.T[k];
      for (int k = 0; k < 36; ++k) st.al_H[k] = sh.H[k];
      info.aligner_ran = 1; info.aligner_iterations = sh.its; info.aligner_converged = sh.conv; info.n_inliers = sh.inl;
      info.n_outliers = sh.outl; info.total_error = sh.E;
    }
  } else if (stage == VS_STAGE_PRUNE_RECOVER) {
    if (tid == 0) set_pose(c, b, s, f, st.pose);   // Frame::setRobotToWorld happened on the host side
    __syncthreads();
    if (has_prev) {
      wg_prune(c, b, s, sh, pb_prev, pb_cur, st.aligner_valid != 0);
      const int n_after = sh.n_cur;
      int n_rec = 0;
      const unsigned long long t0 = wall_clock64();
      if (arg) { wg_recover(c, b, s, sh, pb_prev, pb_cur, hpose_of(c, b, s, f) + 12, st.tau_gen, st.tau_tri, arena); n_rec = sh.flag; }
      if (tid == 0) {
        if (arg) st.ticks[2] += wall_clock64() - t0;
        st.n_cur = sh.n_cur; st.n_after_prune = n_after; st.n_recovered = n_rec;
        info.n_after_prune = n_after; info.n_recovered = n_rec; info.n_points = sh.n_cur;
      }
    }
  } else if (stage == VS_STAGE_PRUNE_PROJECT) {
    // _prunePoints, then the projection of the lost landmarks; their descriptors are computed by the wide k_recover_brief (one wavefront
    // per projected point over the whole chip instead of eight wavefronts behind one CU's memory pipe), which reads what it needs from fc
    if (tid == 0) set_pose(c, b, s, f, st.pose);   // Frame::setRobotToWorld happened on the host side
    __syncthreads();
    if (has_prev) {
      wg_prune(c, b, s, sh, pb_prev, pb_cur, st.aligner_valid != 0);
      const int n_after = sh.n_cur;
      __syncthreads();
      wg_recover_project(c, b, s, sh.n_lost, pb_prev, hpose_of(c, b, s, f) + 12);
      if (tid == 0) {
        st.n_cur = n_after; st.n_after_prune = n_after; st.n_recovered = 0;
        st.fc.n_lost = sh.n_lost; st.fc.tau_gen = st.tau_gen; st.fc.tau_tri = st.tau_tri;
        info.n_after_prune = n_after; info.n_recovered = 0; info.n_points = n_after;
      }
    } else if (tid == 0) {
      st.fc.n_lost = 0;
    }
  } else if (stage == VS_STAGE_RECOVER_APPEND) {
    if (has_prev) {
      const unsigned long long t0 = wall_clock64();
      wg_recover_append(c, b, s, sh, pb_prev, pb_cur);
      const int n_rec = sh.flag;
      if (tid == 0) {
        st.ticks[2] += wall_clock64() - t0;
        st.n_cur = sh.n_cur; st.n_recovered = n_rec;
        info.n_recovered = n_rec; info.n_points = sh.n_cur;
      }
    }
    if (arg & 2) {
      // the frame's point list is final: publish it to the history ring here, so that the landmark kernel of the next call (vslam_compute of a
      // one-stream context: lm_teams_body beside the stereo stage, k_stage_lm) finds what wg_update_points would have published first
      __syncthreads();
      wg_publish_history(c, b, s, sh.n_cur, pb_cur, f);
      if (tid == 0) { st.fc.n_cur = sh.n_cur; st.fc.lm_pb = pb_cur; st.fc.lm_f = f; }
    }
  } else if (stage == VS_STAGE_UPDATE || stage == VS_STAGE_STEREO || stage == VS_STAGE_COMPUTE || stage == VS_STAGE_STEREO_COUNT) {
    if (stage == VS_STAGE_STEREO_COUNT) {
      // _number_of_active_landmarks without the refinement: a point is active iff its track is long enough for a landmark
      const int active = lm_count_active(c, b, s, pts_of(c, b, s, pb_cur), sh.n_cur);
      int total;
      block_exclusive_scan(active, sh.scan, &total);
      if (tid == 0) { st.n_active = total; info.n_active_landmarks = total; }
      __syncthreads();
    } else
    if (stage != VS_STAGE_STEREO) {
      const unsigned long long t0 = wall_clock64();
      wg_update_points(c, b, s, sh, pb_cur, f, arena);
      if (tid == 0) { st.n_active = sh.n_lm; info.n_active_landmarks = sh.n_lm; st.ticks[3] += wall_clock64() - t0; }
    }
    if (stage == VS_STAGE_COMPUTE) {     // the two launches of compute() in one: the shared scalars start over as a new launch would read them
      __syncthreads();
      if (tid == 0) { sh.n_lm = st.n_tracked_landmarks; sh.n_cand = 0; sh.flag = 0; sh.n_cur = st.n_cur; }
      __syncthreads();
    }
    if (stage != VS_STAGE_UPDATE) {
      const unsigned long long t0 = wall_clock64();
      wg_stereo(c, b, s, sh, pb_cur, st.tau_tri, f, arena);
      if (tid == 0) {
        st.ticks[4] += wall_clock64() - t0;
        st.n_cur = sh.n_cur; st.n_new = sh.n_cand;
        frame_close(c, b, s, st, info, sh, pb_cur, f, st.status, st.n_active, st.win, st.tau_track, st.tau_tri, st.prior);
      }
    }
  }
  if (io.report && s == io.report_stream) {
    // the stage's results for the caller, packed by this workgroup into the pinned host buffer (kernels_report.h): the host
    // synchronises the frame queue once and reads them there
    __threadfence();
    __syncthreads();
    report_body(c, b, s, io.report, io.report_in_progress, io.seq, io.L, io.out, (size_t)tid, (size_t)blockDim.x, true, tid, (int)blockDim.x);
    __threadfence_system();
    __syncthreads();
    if (tid == 0) report_publish(io.out, io.seq);
  }
}
__global__ __launch_bounds__(VS_WG) void k_stage(const DevCfg c, const DevBuf b, int stage, int arg, const StageIo io) {
  __shared__ FrameShared sh;
  __shared__ __align__(16) unsigned char arena[VS_ARENA];
  stage_body(c, b, stage, arg, io, sh, arena, blockIdx.x, gridDim.x);
}
// vslam_compute of a context whose vslam_prune_recover has published the frame's history: the n stream workgroups run the stage (STEREO_COUNT: the
// stereo sweep with the active landmarks counted, not refined), G more workgroups per stream refine the landmarks beside it (lm_teams_body) — one launch
__global__ __launch_bounds__(VS_WG) void k_stage_lm(const DevCfg c, const DevBuf b, int stage, int arg, const StageIo io, int n, int G) {
  __shared__ FrameShared sh;
  __shared__ __align__(16) unsigned char arena[VS_ARENA];
  if ((int)blockIdx.x < n) stage_body(c, b, stage, arg, io, sh, arena, blockIdx.x, n);
  else lm_team_workgroup(c, b, (int)blockIdx.x - n, G, sh, arena);
}
