// kernels_rectify.h — rectification of raw (distorted, non-parallel) stereo pairs ahead of the detector (gfx950).
//
// cv::remap(raw, out, map_xy, map_a, INTER_LINEAR, BORDER_CONSTANT, 0) on fixed-point maps in the CV_16SC2 + CV_16UC1 format of
// cv::convertMaps / initUndistortRectifyMap [recalled]:
//   map_xy[r][c] = (x0, y0), the integer part of the source coordinate;  map_a[r][c] = ay * 32 + ax, its fraction in 1/32 px.
//   w00 = (32 - ax)(32 - ay), w01 = ax (32 - ay), w10 = (32 - ax) ay, w11 = ax ay (OpenCV's table holds these times 32, sum 32768;
//   (32 S + 16384) >> 15 == (S + 512) >> 10 exactly), p_ij = raw[y0 + i][x0 + j] inside the raw image, 0 outside.
// Integer arithmetic only: bit-exact by construction.  A tap outside the raw image is never read.
//
// Shape: one lane = 4 consecutive output pixels of one row (one 16-B map_xy load, one 8-B map_a load, one 32-bit store), 64 lanes =
// a 256-px row segment, 4 rows per 256-thread workgroup; grid z = 2 sides x stream batches, each workgroup loops over VS_RECT_SB
// streams so that a map value is loaded once per batch.  The four taps are byte gathers: rectification maps are locally smooth, a
// wave's taps span 2-3 raw rows of ~260 B, which the L1 / L2 serve.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"

#ifndef VS_RECT_SB
#define VS_RECT_SB 8          // streams per workgroup
#endif

struct RectArgs {
  const uint8_t* src[2];      // raw images [left/right]: stream s at src[side] + s * src_stream_stride
  size_t src_stream_stride;
  int32_t src_row_stride, src_rows, src_cols;
  const int16_t* map_xy[2];   // [rows][map_stride][2]
  const uint16_t* map_a[2];   // [rows][map_stride], values < 1024
  int32_t map_stride;         // entries per map row, a multiple of 4 (the padding entries are never stored)
  uint8_t* dst[2];            // rectified images, stream s at dst[side] + s * dst_stream_stride; rows 4-byte aligned
  size_t dst_stream_stride;
  int32_t dst_row_stride;     // a multiple of 4
  int32_t rows, cols;         // rectified size
  int32_t s0, n;              // streams s0 .. s0 + n - 1
  int32_t sides;              // 2: grid z = 2 * batches (side = z & 1); 1: left only, grid z = batches
  uint32_t active[VS_MAX_STREAMS / 32];   // DevBuf::active: a switched-off stream is neither read nor written
};

__device__ __forceinline__ int rect_pixel(const uint8_t* __restrict__ src, const RectArgs& a, int x0, int y0, int ax, int ay) {
  const bool vx0 = (unsigned)x0 < (unsigned)a.src_cols, vx1 = (unsigned)(x0 + 1) < (unsigned)a.src_cols;
  const bool vy0 = (unsigned)y0 < (unsigned)a.src_rows, vy1 = (unsigned)(y0 + 1) < (unsigned)a.src_rows;
  const uint8_t* row0 = src + (ptrdiff_t)y0 * a.src_row_stride;
  const uint8_t* row1 = row0 + a.src_row_stride;
  const int p00 = vy0 && vx0 ? row0[x0] : 0;
  const int p01 = vy0 && vx1 ? row0[x0 + 1] : 0;
  const int p10 = vy1 && vx0 ? row1[x0] : 0;
  const int p11 = vy1 && vx1 ? row1[x0 + 1] : 0;
  const int s = (32 - ax) * (32 - ay) * p00 + ax * (32 - ay) * p01 + (32 - ax) * ay * p10 + ax * ay * p11;
  return (s + 512) >> 10;
}

__global__ __launch_bounds__(256) void k_rectify(RectArgs a) {
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x = blockIdx.x * 256 + (threadIdx.x & 63) * 4;
  const int side = a.sides == 2 ? (int)(blockIdx.z & 1) : 0;
  const int j0 = (a.sides == 2 ? (int)(blockIdx.z >> 1) : (int)blockIdx.z) * VS_RECT_SB;
  if (r >= a.rows || x >= a.cols) return;
  const size_t m = (size_t)r * a.map_stride + x;
  const int4 xy = *reinterpret_cast<const int4*>(a.map_xy[side] + 2 * m);
  const uint2 fr = *reinterpret_cast<const uint2*>(a.map_a[side] + m);
  const int xyw[4] = {xy.x, xy.y, xy.z, xy.w};
  const uint32_t fw[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
  int x0[4], y0[4], ax[4], ay[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x0[k] = (int)(int16_t)(xyw[k] & 0xffff);      // little endian: x in the low half, y in the high half
    y0[k] = xyw[k] >> 16;                         // arithmetic shift keeps the sign
    ax[k] = (int)(fw[k] & 31u);
    ay[k] = (int)((fw[k] >> 5) & 31u);
  }
  const int j1 = min(a.n, j0 + VS_RECT_SB);
  for (int j = j0; j < j1; ++j) {
    const int s = a.s0 + j;
    if (!((a.active[s >> 5] >> (s & 31)) & 1u)) continue;
    const uint8_t* src = a.src[side] + (size_t)s * a.src_stream_stride;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) word |= (uint32_t)rect_pixel(src, a, x0[k], y0[k], ax[k], ay[k]) << (8 * k);
    uint8_t* dst = a.dst[side] + (size_t)s * a.dst_stream_stride + (size_t)r * a.dst_row_stride + x;
    if (x + 4 <= a.cols) *reinterpret_cast<uint32_t*>(dst) = word;
    else
      for (int k = 0; x + k < a.cols; ++k) dst[k] = (uint8_t)(word >> (8 * k));
  }
}
