// exp_fixed.h — exp(x) for x <= 0 in float64 from IEEE +, -, *, rint and ldexp only, so that the host compiler, the device and numpy
// (bilateral.py: exp_fixed, the same constants and the same grouping) agree on every bit.  Needs -ffp-contract=off: a fused multiply-add
// anywhere below is another function.  Plain C++ with no HIP header: the sanitizer walk (tests/cpp/bilateral_geometry_walk.cpp) builds it
// with the host compiler alone.
//   k = rint(x * (1 / ln 2)); r = (x - k * LN2_HI) - k * LN2_LO (fdlibm's split: LN2_HI has 21 trailing zero bits, k * LN2_HI is exact for
//   |k| < 2^11, and so is the first difference); |r| <= 0.35; p = the Taylor polynomial of degree 13 in Horner form (truncation below
//   0.35^14 / 14! e^0.35 < 7e-18); ldexp(p, k).  x < -746 gives 0 (exp(-746) < 2^-1076).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define VS_XD __host__ __device__
#else
#define VS_XD
#endif

VS_XD inline double exp_fixed(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (x < -746.0) return 0.0;
  const double k = rint(x * 1.4426950408889634);
  const double r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10;
  // 1 / j!, j = 13 .. 0: quotients of exactly representable integers, rounded once by the compiler as Python rounds them
  double p = 1.0 / 6227020800.0;
  p = 1.0 / 479001600.0 + r * p;
  p = 1.0 / 39916800.0 + r * p;
  p = 1.0 / 3628800.0 + r * p;
  p = 1.0 / 362880.0 + r * p;
  p = 1.0 / 40320.0 + r * p;
  p = 1.0 / 5040.0 + r * p;
  p = 1.0 / 720.0 + r * p;
  p = 1.0 / 120.0 + r * p;
  p = 1.0 / 24.0 + r * p;
  p = 1.0 / 6.0 + r * p;
  p = 1.0 / 2.0 + r * p;
  p = 1.0 + r * p;
  p = 1.0 + r * p;
  return ldexp(p, (int)k);
}
