// bilateral_geometry.h — the index arithmetic of kernels_bilateral.h, host and device: the reflected border, the tile grid of
// k_bilateral_apply with its halo, and the taps of one sigma_space.  Plain C++ (no HIP header), so that the sanitizer walk
// (tests/cpp/bilateral_geometry_walk.cpp) runs exactly what the kernel runs.
#pragma once
#include <stdint.h>
#include <cmath>
#include "exp_fixed.h"

#define VS_BL_TILE 32             // k_bilateral_apply: a workgroup owns TILE x TILE pixels
#define VS_BL_MAX_RADIUS 8
#define VS_BL_MAX_TAPS 200        // 197 lattice points lie inside the circle of radius 8
#define VS_BL_HALO_MAX (VS_BL_TILE + 2 * VS_BL_MAX_RADIUS)
#define VS_BL_LUT 4098            // kExpNumBins + 2
#define VS_BL_MAX_PIXELS (1 << 24)

// borderInterpolate(p, n, BORDER_REFLECT_101): n >= 1; ends for every p (each round trip brings p closer to [0, n))
VS_XD inline int bl_reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}
// side of the staged square of a tile and the row pitch it is stored with (odd: two rows of a half-wave do not start on one bank)
VS_XD inline int bl_halo(int radius) { return VS_BL_TILE + 2 * radius; }
VS_XD inline int bl_pitch(int radius) { return bl_halo(radius) | 1; }
VS_XD inline int bl_tiles(int n) { return (n + VS_BL_TILE - 1) / VS_BL_TILE; }
// source index of staged element h (0 .. halo - 1) of tile t along an axis of length n
VS_XD inline int bl_staged(int t, int h, int radius, int n) { return bl_reflect101(t * VS_BL_TILE - radius + h, n); }

struct BlTaps {
  int32_t n, radius;
  float w[VS_BL_MAX_TAPS];        // space_weight, scan order: rows outer, columns inner
  int8_t di[VS_BL_MAX_TAPS], dj[VS_BL_MAX_TAPS];
};
// sigma <= 0 counts as 1 (cv::bilateralFilter)
inline double bl_sigma(double s) { return s > 0 ? s : 1.0; }
// false: the radius max(1, cvRound(sigma_space * 1.5)) lies above VS_BL_MAX_RADIUS (or sigma_space is not finite)
inline bool bl_make_taps(double sigma_space, BlTaps& t) {
  if (!std::isfinite(sigma_space)) return false;
  const double s = bl_sigma(sigma_space);
  const double rr = std::nearbyint(s * 1.5);           // ties to even, like cvRound
  if (rr > VS_BL_MAX_RADIUS) return false;
  const int radius = rr < 1 ? 1 : (int)rr;
  const double coeff = -0.5 / (s * s);
  t.n = 0; t.radius = radius;
  for (int i = -radius; i <= radius; ++i)
    for (int j = -radius; j <= radius; ++j) {
      if (std::sqrt((double)(i * i + j * j)) > radius) continue;
      t.w[t.n] = (float)exp_fixed((double)(i * i + j * j) * coeff);
      t.di[t.n] = (int8_t)i; t.dj[t.n] = (int8_t)j;
      ++t.n;
    }
  return true;
}
