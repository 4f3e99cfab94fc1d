// kernels_undistort.h — undistortion of raw RGB-D frames ahead of the detector and the space map (gfx950).
//
// One fixed-point map pair (kernels_rectify.h's format: map_xy = integer source coordinate, map_a = ay * 32 + ax in 1/32 px) serves the
// image and the depth image registered to it.
//   image: k_rectify in its one-sided form (remap_enqueue of host_prestage.h fills its argument block): bilinear, rect_pixel's arithmetic.
//   depth: k_undistort_depth, nearest neighbour on the same maps, ties up — this repository's own rule, depth is never blended (a mix
//          across a depth edge invents a surface):
//            x = x0 + (ax >> 4), y = y0 + (ay >> 4), out = src[y][x] inside the raw image, else 0 (0 = no measurement: kernels_depth.h).
// Integer arithmetic only: bit-exact by construction.  A tap outside the raw image is never read.
//
// Shape of k_undistort_depth, as k_rectify: one lane = 4 consecutive output pixels of one row (one 16-B map_xy load, one 8-B map_a load,
// four 16-bit gathers per sequence, one 8-B store where the destination is 8-byte aligned, element stores otherwise and in the row
// tail), 64 lanes = a 256-px row segment, 4 rows per 256-thread workgroup; grid z = sequence batches, each workgroup loops over
// VS_RECT_SB sequences so that a map entry is loaded once per batch.
#pragma once
#include "kernels_rectify.h"

struct UndistortDepthArgs {
  const uint16_t* src;        // raw depth images: sequence s at src + s * src_stream_stride (elements)
  size_t src_stream_stride;
  int32_t src_row_stride, src_rows, src_cols;   // src_rows * src_row_stride < 2^31 (both <= 32767 wherever this is filled)
  const int16_t* map_xy;      // [rows][map_stride][2]
  const uint16_t* map_a;      // [rows][map_stride], values < 1024
  int32_t map_stride;         // entries per map row, a multiple of 4 (the padding entries are never stored)
  uint16_t* dst;              // undistorted depth images, sequence s at dst + s * dst_stream_stride (elements); any alignment
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  int32_t rows, cols;         // undistorted size
  int32_t n;                  // sequences 0 .. n - 1
};

__global__ __launch_bounds__(256) void k_undistort_depth(UndistortDepthArgs a) {
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x = blockIdx.x * 256 + (threadIdx.x & 63) * 4;
  const int j0 = (int)blockIdx.z * VS_RECT_SB;
  if (r >= a.rows || x >= a.cols) return;
  const size_t m = (size_t)r * a.map_stride + x;
  const int4 xy = *reinterpret_cast<const int4*>(a.map_xy + 2 * m);
  const uint2 fr = *reinterpret_cast<const uint2*>(a.map_a + m);
  const int xyw[4] = {xy.x, xy.y, xy.z, xy.w};
  const uint32_t fw[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
  int off[4];                                     // element offset of the tap in its image, -1: outside (never read)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int sx = (int)(int16_t)(xyw[k] & 0xffff) + (int)((fw[k] & 31u) >> 4);      // little endian: x in the low half, y in the high half
    const int sy = (xyw[k] >> 16) + (int)(((fw[k] >> 5) & 31u) >> 4);
    const bool inside = (unsigned)sx < (unsigned)a.src_cols && (unsigned)sy < (unsigned)a.src_rows;
    off[k] = inside ? sy * a.src_row_stride + sx : -1;
  }
  const int j1 = min(a.n, j0 + VS_RECT_SB);
  for (int j = j0; j < j1; ++j) {
    const uint16_t* src = a.src + (size_t)j * a.src_stream_stride;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = off[k] >= 0 ? (uint32_t)src[off[k]] : 0u;
    uint16_t* dst = a.dst + (size_t)j * a.dst_stream_stride + (size_t)r * a.dst_row_stride + x;
    if (x + 4 <= a.cols && (reinterpret_cast<uintptr_t>(dst) & 7u) == 0) *reinterpret_cast<uint2*>(dst) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    else
      for (int k = 0; k < 4 && x + k < a.cols; ++k) dst[k] = (uint16_t)v[k];
  }
}

// grid of k_undistort_depth, and of k_rectify per side, on n sequences
static inline dim3 undistort_grid(int32_t rows, int32_t cols, int32_t n) { return dim3((cols + 255) / 256, (rows + 3) / 4, (n + VS_RECT_SB - 1) / VS_RECT_SB); }
