// landmark_math.h — the arithmetic of Landmark::update (types/landmark.cpp:66-167), written once: the robust 3x3 Gauss-Newton over the
// measurements of a track.  Its callers differ in where the measurements come from and who evaluates them: the stereo tracker's refinement
// (kernels_frame_lm.h: one lane or a team of eight per track), the RGB-D tracker's (kernels_rgbd.h: a team per track) and the stand-alone
// entry (kernels_landmark.h: one lane per caller-provided list).  All of them, and the CPU oracle, have to agree to the bit, so every
// expression below keeps the oracle's grouping (the library is built with -ffp-contract=off).
//
// R^T R of a world_to_camera (J^T J of a measurement, J = R) is symmetric to the bit: entry [r][c] and entry [c][r] are sums of the same
// commuting products in the same grouping.  A term therefore carries six products, and lm_add puts each off-diagonal one in both places.
#pragma once
#include <hip/hip_runtime.h>
#include "dev_math.h"

#define LM_TEAM_G 8   // lanes of a team (lm_team_add)
// one measurement's contribution; kind 0: behind the camera (an outlier, nothing added), 1: inlier, 2: outlier with the saturated kernel,
// -1: no measurement (a team lane beyond the list's end)
struct LmTerm { double e2, h[6], b[3]; int kind, pad; };
enum LmRound { LM_NEXT_ROUND, LM_KEEP, LM_ACCEPT, LM_RESET };

// entry e = 3 r + c of R^T R of world_to_camera W
__device__ __forceinline__ double lm_rtr_entry(const double* W, int e) {
  const int r = e / 3, c = e - 3 * r;
  return (W[r] * W[c] + W[4 + r] * W[4 + c]) + W[8 + r] * W[8 + c];
}
__device__ __forceinline__ void lm_rtr(const double* W, double* out9) {
#pragma unroll
  for (int e = 0; e < 9; ++e) out9[e] = lm_rtr_entry(W, e);
}
// projection, residual, saturated kernel, om * R^T R and om * R^T e of one measurement mc = x, y, z, 1 / z of the landmark estimate wv
__device__ __forceinline__ LmTerm lm_term(const double* W, const double* RtR, const double* mc, const double* wv, double kern) {
  LmTerm t;
  double sp[3];
  tf_apply(W, wv, sp);
  if (sp[2] <= 0) { t.kind = 0; return t; }
  const double e[3] = {sp[0] - mc[0], sp[1] - mc[1], sp[2] - mc[2]};
  double om = mc[3];
  t.e2 = om * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  t.kind = 1;
  if (t.e2 > kern) { om *= kern / t.e2; t.kind = 2; }
  t.h[0] = om * RtR[0]; t.h[1] = om * RtR[1]; t.h[2] = om * RtR[2]; t.h[3] = om * RtR[4]; t.h[4] = om * RtR[5]; t.h[5] = om * RtR[8];
#pragma unroll
  for (int r = 0; r < 3; ++r) t.b[r] = om * ((W[r] * e[0] + W[4 + r] * e[1]) + W[8 + r] * e[2]);
  return t;
}
// The thirteen additions of a term.  Only these have to happen in the order of the measurement list.
__device__ __forceinline__ void lm_add(const LmTerm& q, double* H, double* bv, double& err, int& n_out) {
  if (q.kind == 0) { ++n_out; return; }
  err += q.e2;
  if (q.kind == 2) ++n_out;
  H[0] += q.h[0]; H[4] += q.h[3]; H[8] += q.h[5];
  H[1] += q.h[1]; H[3] += q.h[1]; H[2] += q.h[2]; H[6] += q.h[2]; H[5] += q.h[4]; H[7] += q.h[4];
  bv[0] += q.b[0]; bv[1] += q.b[1]; bv[2] += q.b[2];
}
// a measurement of a frame whose R^T R is not staged, evaluated and added on the lane itself
__device__ __forceinline__ void lm_add_unstaged(const double* W, const double* mc, const double* wv, double kern, double* H, double* bv, double& err, int& n_out) {
  double rtr[9];
  lm_rtr(W, rtr);
  lm_add(lm_term(W, rtr, mc, wv, kern), H, bv, err, n_out);
}
// One batch of a team of LM_TEAM_G lanes: lane gl parks its term t, then every lane adds the batch's nb terms in list order into its own copy
// of the sums (no broadcast afterwards).  The first barrier: the previous batch's terms have been read by every lane of the team.  The reads
// are plain LDS loads, so that the next terms are on their way while one is being added (volatile reads cost one LDS round trip EACH: 88 per
// batch).
__device__ __forceinline__ void lm_team_add(LmTerm* terms, int gl, const LmTerm& t, int nb, double* H, double* bv, double& err, int& n_out) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  terms[gl] = t;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < LM_TEAM_G; ++u) {
    if (u < nb) { const LmTerm q = terms[u]; lm_add(q, H, bv, err, n_out); }
  }
}
// The end of a round: the Gauss-Newton step on wv, the convergence test (:134) and what becomes of the landmark (:138-155).  n_meas
// measurements, n_out of them outliers, `updates` inliers at the landmark's last accepted update (never negative in the trackers; a negative
// count from a stand-alone caller accepts nothing).  LM_ACCEPT: wv replaces the landmark with n_in updates; LM_RESET: the mean of the track's
// world coordinates does; LM_KEEP: the landmark stays.
__device__ __forceinline__ LmRound lm_round_end(const double* H, const double* bv, double* wv, double err, double err_prev, int it, int n_meas, int n_out, int updates, int& n_in) {
  double nb[3] = {-bv[0], -bv[1], -bv[2]}, dx[3];
  full_piv_solve_regs<3>(H, nb, dx);
  for (int q = 0; q < 3; ++q) wv[q] += dx[q];
  n_in = n_meas - n_out;
  if (!(fabs(err - err_prev) < 1e-5 || it == 999)) return LM_NEXT_ROUND;
  if ((unsigned)n_in > (unsigned)updates) return LM_ACCEPT;
  return n_in < n_out ? LM_RESET : LM_KEEP;
}
