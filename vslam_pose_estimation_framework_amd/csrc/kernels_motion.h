// kernels_motion.h — the motion prior a frame starts with (PoseTracker3D::compute, pose_tracker_3d.cpp:40-66): the arithmetic of the
// CAMERA_ODOMETRY model, written once, the per-stream kernel that puts the prior into the stream state ahead of everything that reads it
// (k_track_candidates, k_frame), and the kernel behind the stand-alone entry vslam_motion_prior.  CONSTANT_VELOCITY launches nothing of
// this: it keeps the last refined motion (:44-48).
#pragma once
#include "dev_types.h"
#include "dev_math.h"

// _previous_to_current_camera = _camera_left_in_world_guess.inverse() * _camera_left_in_world_guess_previous (:55): the inverse first, then
// the product, each with the operation order of dev_math.h.  out may alias neither input.
VS_HD void motion_prior(const double* guess, const double* guess_prev, double* out) {
  double inv[12];
  tf_inverse(guess, inv);
  tf_mul(inv, guess_prev, out);
}

// What the host hands over for a frame: `dev` a caller's device array [n_streams][12] for every active stream (null: none), `host` /
// `mask` the context's own copy of the guesses set one stream at a time (mask[s] != 0: stream s has a new one; both null: none).  A
// stream set through both takes `host`.
struct GuessSrc { const double* dev; const double* host; const int32_t* mask; };

// Frame start of every active stream, one thread each: take the stream's new guess if one was set (a frame without one re-uses the last,
// as the reference's member does), then
//   NONE              prior = identity (:62-65)
//   CAMERA_ODOMETRY   prior = motion_prior(guess, guess_prev) if the stream has a previous frame (:54-56); afterwards, always,
//                     guess_prev = guess (:57)
// (never launched under CONSTANT_VELOCITY)
// A switched-off stream is neither read nor written: its guess state stays where it is.
__global__ __launch_bounds__(64) void k_motion_prior(const DevBuf b, int n, int model, const GuessSrc g) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = b.s0 + i;
  if (!vs_active(b, s)) return;
  StreamState& st = b.st[s];
  const double* src = (g.mask && g.mask[s]) ? g.host + (size_t)s * 12 : g.dev ? g.dev + (size_t)s * 12 : nullptr;
  if (src) for (int k = 0; k < 12; ++k) st.guess[k] = src[k];
  if (model == VSLAM_MOTION_NONE) {
    tf_identity(st.prior);
  } else if (model == VSLAM_MOTION_CAMERA_ODOMETRY) {
    double gc[12], gp[12], T[12];
    for (int k = 0; k < 12; ++k) { gc[k] = st.guess[k]; gp[k] = st.guess_prev[k]; }
    if (st.has_prev) {
      motion_prior(gc, gp, T);
      for (int k = 0; k < 12; ++k) st.prior[k] = T[k];
    }
    for (int k = 0; k < 12; ++k) st.guess_prev[k] = gc[k];
  }
}

// vslam_motion_prior: out[i] = motion_prior(guess[i], guess_prev[i]), one thread per transform
__global__ __launch_bounds__(256) void k_motion_prior_entry(int n, const double* guess, const double* guess_prev, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double gc[12], gp[12], T[12];
  for (int k = 0; k < 12; ++k) { gc[k] = guess[(size_t)i * 12 + k]; gp[k] = guess_prev[(size_t)i * 12 + k]; }
  motion_prior(gc, gp, T);
  for (int k = 0; k < 12; ++k) out[(size_t)i * 12 + k] = T[k];
}
