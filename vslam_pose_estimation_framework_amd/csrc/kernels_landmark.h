// kernels_landmark.h — Landmark::update (types/landmark.cpp:66-167) on caller-provided measurement lists, stand-alone.
// The fused tracker runs the same refinement inside its frame kernel (kernels_frame_lm.h landmark_point, walking the history
// ring) on the same arithmetic (landmark_math.h); this entry exists so that the arithmetic is pinned by an independent fixture.
// One thread per landmark: a 3x3 Gauss-Newton over 3..100 measurements is latency-bound bookkeeping, the batch supplies the
// parallelism.
#pragma once
#include <hip/hip_runtime.h>
#include "landmark_math.h"

__global__ __launch_bounds__(256) void k_landmark_update(int n, const int32_t* offsets, const int32_t* frame_of, const double* w2c,
                                                         const double* c2w, const double* cam, double* world, int32_t* updates,
                                                         int max_iterations, double kernel) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int a = offsets[i], e = offsets[i + 1];
  if (e <= a) return;
  double wv[3] = {world[3 * (size_t)i], world[3 * (size_t)i + 1], world[3 * (size_t)i + 2]};
  const int updates0 = updates[i];
  double err_prev = 0;
  for (int it = 0; it < max_iterations; ++it) {
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0};
    double err = 0;
    int n_out = 0;
    for (int m = a; m < e; ++m) {
      const double* p = cam + 3 * (size_t)m;
      const double mc[4] = {p[0], p[1], p[2], 1 / p[2]};                            // :107 (Measurement::inverse_depth_meters)
      lm_add_unstaged(w2c + 12 * (size_t)frame_of[m], mc, wv, kernel, H, bv, err, n_out);   // :97-127, J = R
    }
    int n_in;
    const LmRound end = lm_round_end(H, bv, wv, err, err_prev, it, e - a, n_out, updates0, n_in);   // :131-155
    if (end == LM_ACCEPT) {
      for (int q = 0; q < 3; ++q) world[3 * (size_t)i + q] = wv[q];
      updates[i] = n_in;
    } else if (end == LM_RESET) {
      double acc[3] = {0, 0, 0};
      for (int m = a; m < e; ++m) {
        double wp[3];
        tf_apply(c2w + 12 * (size_t)frame_of[m], cam + 3 * (size_t)m, wp);
        for (int q = 0; q < 3; ++q) acc[q] += wp[q];
      }
      for (int q = 0; q < 3; ++q) world[3 * (size_t)i + q] = acc[q] / (double)(e - a);
    }
    if (end != LM_NEXT_ROUND) break;
    err_prev = err;
  }
}
