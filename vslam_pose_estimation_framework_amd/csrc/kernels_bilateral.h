// kernels_bilateral.h — bilateral filtering of the 16-bit depth image ahead of the space map (gfx950): the optional first step of
// DepthFramePointGenerator::_computeDepthMap (depth_framepoint_generator.cpp:415-422, enable_bilateral_filtering).
//
// convertTo(CV_32F, depth_scale), cv::bilateralFilter(src, dst, -1, sigma_color, sigma_space) on one float channel, convertTo(CV_16U,
// 1 / depth_scale) [recalled; the definition with every order of operations fixed: bilateral.py]:
//   to metres  v = float(raw) * float(depth_scale)
//   radius     max(1, cvRound(sigma_space * 1.5)); sigmas <= 0 count as 1
//   taps       (i, j) over -radius .. radius, rows outer, kept when sqrt(i*i + j*j) <= radius, in that order;
//              space_weight = float(exp_fixed((i*i + j*j) * (-0.5 / sigma_space^2)))                          (bilateral_geometry.h)
//   borders    BORDER_REFLECT_101
//   range      lo, hi = min, max of v over the image (holes count); hi - lo < FLT_EPSILON: the filter is the identity on v
//   table      scale_index = 4096.f / (hi - lo); lut[i] = float(exp_fixed((i / scale_index)^2 * (-0.5 / sigma_color^2))), i = 0 .. 4097, in
//              double; once an entry has rounded to 0.f every later one is 0
//   per pixel  over the taps in order: alpha = |val - val0| * scale_index, idx = int(alpha), alpha -= idx,
//              w = space_weight * (lut[idx] + alpha * (lut[idx + 1] - lut[idx])), sum += val * w, wsum += w;  out = sum / wsum
//   to 16 bit  clamp(rint(out * float(1.0 / depth_scale)), 0, 65535)
// Every float operation is one of __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn / rintf, the doubles of the table are IEEE operations of a
// library built without contraction: the result is bit-exact against numpy by construction.
//
// Three kernels, the last grid dimension = streams:
//   k_depth_range      minimum and maximum of the raw image (float(raw) * scale is monotone: raw order is metre order), reduced in the
//                      wave by shuffles and across the four waves in LDS, then one atomicMin and one atomicMax per workgroup into cells[stream][0 .. 1]
//                      (at most 128 workgroups per stream, a wave per row, 16 B per lane where the row is aligned), which are armed
//                      (0xffffffff, 0) when allocated and re-armed by the next kernel
//   k_bilateral_lut    one workgroup per stream: reads and re-arms the two cells, writes the identity flag and scale_index to
//                      cells[stream][2 .. 3] and the table to lut[stream][4098].  The running-zero rule is a minimum: every thread
//                      reports the first index whose entry is 0.f (atomicMin in LDS), entries from there on are stored as 0.
//   k_bilateral_apply  a workgroup owns a 32 x 32 tile: it stages the (32 + 2 radius)^2 square around it in LDS as float metres with the
//                      reflection applied, the table (16392 B) and the taps, and every thread walks the taps for four pixels (two
//                      neighbours in each of two rows 16 apart) with the sums in registers.  A neighbour pair leaves as one 32-bit
//                      store where the destination is 4-byte aligned and both lie inside the image, as two 16-bit stores otherwise.
//                      src and dst must not overlap: a tile reads its neighbours' pixels.
//                      LDS: 16392 (table) + 48 * 49 * 4 = 9408 (square at radius 8) + 1600 (taps) = 27400 B: five workgroups fit a
//                      CU's 160 KB, two were asked for.  The gathers lut[idx], lut[idx + 1] hit whatever banks the image sends them
//                      to: accepted.
//
// Bounds, for every shape bilateral_args() accepts (rows, cols >= 1, rows * cols <= 2^24, radius 1 .. 8, <= 200 taps):
//   source reads   k_depth_range reads rows [0, rows) x columns [0, cols) (vectors over [head, head + 8 nvec) with head + 8 nvec <= cols); k_bilateral_apply reads src[bl_staged(..)]: bl_reflect101 returns
//                  an index in [0, n) for every p (walked over random sizes and radii by tests/cpp/bilateral_geometry_walk.cpp)
//   square         element (hy, hx), hy, hx < halo = 32 + 2 radius <= 48, at hy * pitch + hx with pitch = halo | 1 <= 49: below 48 * 49.  A
//                  pixel (py, px) of the tile, py, px < 32, reads (py + radius + di, px + radius + dj) with |di|, |dj| <= radius: inside
//                  [0, halo)
//   table          alpha = |val - val0| * scale_index <= (hi - lo) * fl(4096 / (hi - lo)) < 4097, so idx <= 4096 and idx + 1 <= 4097; idx is
//                  clamped into [0, 4096] as well, which changes nothing for accepted images
//   stores         only pixels with row < rows and column < cols; the 32-bit store needs both columns inside: padding is never written
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cfloat>
#include <cmath>
#include <algorithm>
#include <cstring>
#include <vector>
#include "bilateral_geometry.h"

struct BilateralArgs {
  const uint16_t* src;        // stream s at src + s * src_stream_stride (elements), any 2-byte alignment
  size_t src_stream_stride;
  int32_t src_row_stride;
  uint16_t* dst;              // null: range and table alone
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  int32_t rows, cols, n;
  float scale, inv_scale;     // float(depth_scale), float(1.0 / depth_scale)
  double color_coeff;         // -0.5 / sigma_color^2
  uint32_t* cells;            // [n][4]: raw minimum, raw maximum (armed: 0xffffffff, 0), identity flag, scale_index bits
  float* lut;                 // [n][VS_BL_LUT]
  BlTaps taps;
};

__global__ __launch_bounds__(256) void k_depth_range(BilateralArgs a) {
  const int s = blockIdx.y, tid = threadIdx.x;
  const uint16_t* img = a.src + (size_t)s * a.src_stream_stride;
  uint32_t lo = 0xffffffffu, hi = 0u;
  // a wave per row: 16 B (eight pixels) per lane over the row's aligned interior [head, head + 8 nvec), inside [0, cols); the fewer than
  // eight pixels ahead of its first 16-B boundary and behind the last whole vector by single lanes.  Padding is never read.
  const int lane = tid & 63;
  for (int r = blockIdx.x * 4 + (tid >> 6); r < a.rows; r += gridDim.x * 4) {
    const uint16_t* row = img + (size_t)r * a.src_row_stride;
    const int head = min(a.cols, (int)(((16u - (uint32_t)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (a.cols - head) >> 3;
    if (lane < head) { const uint32_t v = row[lane]; lo = min(lo, v); hi = max(hi, v); }
    const uint4* pv = reinterpret_cast<const uint4*>(row + head);
    for (int v = lane; v < nvec; v += 64) {
      const uint4 q = pv[v];
      const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo = min(lo, min(w[k] & 0xffffu, w[k] >> 16));
        hi = max(hi, max(w[k] & 0xffffu, w[k] >> 16));
      }
    }
    for (int c = head + 8 * nvec + lane; c < a.cols; c += 64) { const uint32_t v = row[c]; lo = min(lo, v); hi = max(hi, v); }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    lo = min(lo, (uint32_t)__shfl_down((int)lo, d, 64));
    hi = max(hi, (uint32_t)__shfl_down((int)hi, d, 64));
  }
  // the four waves' results meet in LDS, so that a workgroup costs the two cells one atomic each: every atomic of a stream lands on
  // the same two addresses and they serialise (one per wave of 480 one-row workgroups took 46 us at 640 x 480)
  __shared__ uint32_t part[8];
  if ((tid & 63) == 0) { part[tid >> 6] = lo; part[4 + (tid >> 6)] = hi; }
  __syncthreads();
  if (tid == 0) {
    lo = min(min(part[0], part[1]), min(part[2], part[3]));
    hi = max(max(part[4], part[5]), max(part[6], part[7]));
    if (lo <= hi) {
      atomicMin(&a.cells[4 * s], lo);
      atomicMax(&a.cells[4 * s + 1], hi);
    }
  }
}

__global__ __launch_bounds__(256) void k_bilateral_lut(BilateralArgs a) {
  __shared__ float tab[VS_BL_LUT];
  __shared__ uint32_t mm[2];
  __shared__ uint32_t first;
  const int s = blockIdx.x, tid = threadIdx.x;
  uint32_t* cell = a.cells + 4 * s;
  float* out = a.lut + (size_t)s * VS_BL_LUT;
  if (tid == 0) { mm[0] = cell[0]; mm[1] = cell[1]; first = VS_BL_LUT; }
  __syncthreads();
  if (tid == 0) { cell[0] = 0xffffffffu; cell[1] = 0u; }               // armed for the next frame's k_depth_range
  const float lo = __fmul_rn((float)mm[0], a.scale), hi = __fmul_rn((float)mm[1], a.scale);
  const float span = __fsub_rn(hi, lo);
  if (!(span >= FLT_EPSILON)) {                                         // a flat image (or none): no table
    for (int i = tid; i < VS_BL_LUT; i += 256) out[i] = 0.f;
    if (tid == 0) { cell[2] = 1u; cell[3] = 0u; }
    return;
  }
  const float scale_index = __fdiv_rn(4096.f, span);
  for (int i = tid; i < VS_BL_LUT; i += 256) {
    const double q = (double)i / (double)scale_index;
    const float e = (float)exp_fixed(q * q * a.color_coeff);
    tab[i] = e;
    if (e == 0.f) atomicMin(&first, (uint32_t)i);
  }
  __syncthreads();
  const uint32_t f = first;
  for (int i = tid; i < VS_BL_LUT; i += 256) out[i] = (uint32_t)i >= f ? 0.f : tab[i];
  if (tid == 0) { cell[2] = 0u; cell[3] = __float_as_uint(scale_index); }
}

__device__ __forceinline__ void bl_tap(float val, float val0, float scale_index, float sw, const float* lut, float& sum, float& wsum) {
  float alpha = __fmul_rn(fabsf(__fsub_rn(val, val0)), scale_index);
  const int idx = min(max((int)alpha, 0), VS_BL_LUT - 2);
  alpha = __fsub_rn(alpha, (float)idx);
  const float l0 = lut[idx], l1 = lut[idx + 1];
  const float w = __fmul_rn(sw, __fadd_rn(l0, __fmul_rn(alpha, __fsub_rn(l1, l0))));
  sum = __fadd_rn(sum, __fmul_rn(val, w));
  wsum = __fadd_rn(wsum, w);
}
__device__ __forceinline__ uint32_t bl_to_u16(float metres, float inv_scale) {
  const float m = rintf(__fmul_rn(metres, inv_scale));
  return (uint32_t)fminf(fmaxf(m, 0.f), 65535.f);
}

__global__ __launch_bounds__(256) void k_bilateral_apply(BilateralArgs a) {
  __shared__ float lut[VS_BL_LUT];
  __shared__ float sq[VS_BL_HALO_MAX * (VS_BL_HALO_MAX | 1)];
  __shared__ float tw[VS_BL_MAX_TAPS];
  __shared__ int32_t toff[VS_BL_MAX_TAPS];
  const int s = blockIdx.z, tid = threadIdx.x;
  const int radius = min(max(a.taps.radius, 1), VS_BL_MAX_RADIUS), ntaps = min(max(a.taps.n, 0), VS_BL_MAX_TAPS);
  const int halo = bl_halo(radius), pitch = bl_pitch(radius);
  const uint32_t* cell = a.cells + 4 * s;
  const bool identity = cell[2] != 0u;
  const float scale_index = __uint_as_float(cell[3]);
  const uint16_t* img = a.src + (size_t)s * a.src_stream_stride;
  for (int e = tid; e < halo * halo; e += 256) {
    const int hy = e / halo, hx = e - hy * halo;
    const int r = bl_staged(blockIdx.y, hy, radius, a.rows), c = bl_staged(blockIdx.x, hx, radius, a.cols);
    sq[hy * pitch + hx] = __fmul_rn((float)img[(size_t)r * a.src_row_stride + c], a.scale);
  }
  if (!identity) {
    const float* g = a.lut + (size_t)s * VS_BL_LUT;
    for (int i = tid; i < VS_BL_LUT; i += 256) lut[i] = g[i];
    if (tid < ntaps) { tw[tid] = a.taps.w[tid]; toff[tid] = (int)a.taps.di[tid] * pitch + (int)a.taps.dj[tid]; }
  }
  __syncthreads();
  const int px = (tid & 15) * 2, py = tid >> 4;                          // pixels (py, px), (py, px + 1), (py + 16, px), (py + 16, px + 1)
  const int c0 = blockIdx.x * VS_BL_TILE + px, r0 = blockIdx.y * VS_BL_TILE + py;
  if (c0 >= a.cols || r0 >= a.rows) return;
  const int base = (py + radius) * pitch + px + radius;
  const float v00 = sq[base], v01 = sq[base + 1], v10 = sq[base + 16 * pitch], v11 = sq[base + 16 * pitch + 1];
  float o00 = v00, o01 = v01, o10 = v10, o11 = v11;
  if (!identity) {
    float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f, w00 = 0.f, w01 = 0.f, w10 = 0.f, w11 = 0.f;
    for (int k = 0; k < ntaps; ++k) {
      const float sw = tw[k];
      const int o = base + toff[k];
      bl_tap(sq[o], v00, scale_index, sw, lut, s00, w00);
      bl_tap(sq[o + 1], v01, scale_index, sw, lut, s01, w01);
      bl_tap(sq[o + 16 * pitch], v10, scale_index, sw, lut, s10, w10);
      bl_tap(sq[o + 16 * pitch + 1], v11, scale_index, sw, lut, s11, w11);
    }
    o00 = __fdiv_rn(s00, w00); o01 = __fdiv_rn(s01, w01); o10 = __fdiv_rn(s10, w10); o11 = __fdiv_rn(s11, w11);
  }
  uint16_t* out = a.dst + (size_t)s * a.dst_stream_stride;
  const bool pair = c0 + 1 < a.cols;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = r0 + 16 * h;
    if (r >= a.rows) break;
    const uint32_t m0 = bl_to_u16(h ? o10 : o00, a.inv_scale), m1 = bl_to_u16(h ? o11 : o01, a.inv_scale);
    uint16_t* o = out + (size_t)r * a.dst_row_stride + c0;
    if (pair && ((uintptr_t)o & 3u) == 0) *reinterpret_cast<uint32_t*>(o) = m0 | (m1 << 16);
    else {
      o[0] = (uint16_t)m0;
      if (pair) o[1] = (uint16_t)m1;
    }
  }
}

// What the entries check and the kernels need of one (rows, cols, depth_scale, sigmas) combination: false with a reason for what is
// refused.  Fills the size, the two scales, the colour coefficient and the taps of a; images, cells, lut and n stay the caller's.
static bool bilateral_args(int rows, int cols, double depth_scale, double sigma_color, double sigma_space, BilateralArgs& a, const char** why) {
  if (rows < 1 || cols < 1) { *why = "empty image"; return false; }
  if ((size_t)rows * (size_t)cols > (size_t)VS_BL_MAX_PIXELS) { *why = "more than 2^24 pixels"; return false; }
  if (!(depth_scale > 0) || !std::isfinite(depth_scale)) { *why = "depth_scale must be positive and finite"; return false; }
  if (!std::isfinite(sigma_color)) { *why = "sigma_color is not finite"; return false; }
  if (!bl_make_taps(sigma_space, a.taps)) { *why = "radius above 8 (sigma_space * 1.5 rounds above it, or is not finite)"; return false; }
  const double sc = bl_sigma(sigma_color);
  a.rows = rows; a.cols = cols;
  a.scale = (float)depth_scale; a.inv_scale = (float)(1.0 / depth_scale);
  a.color_coeff = -0.5 / (sc * sc);
  return true;
}
// the two cells of n streams as k_depth_range expects them
static hipError_t bilateral_arm(uint32_t* cells, int n, hipStream_t st) {
  std::vector<uint32_t> h((size_t)n * 4, 0u);
  for (int s = 0; s < n; ++s) h[(size_t)4 * s] = 0xffffffffu;
  hipError_t e = hipMemcpyAsync(cells, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);                   // h leaves scope
  return e;
}
// range, table and (with a destination) the filter on queue st
static void bilateral_enqueue(hipStream_t st, const BilateralArgs& a) {
  hipLaunchKernelGGL(k_depth_range, dim3(std::min((a.rows + 3) / 4, std::max(8, std::min(128, 4096 / std::max(a.n, 1)))), a.n), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_bilateral_lut, dim3(a.n), dim3(256), 0, st, a);
  if (a.dst) hipLaunchKernelGGL(k_bilateral_apply, dim3(bl_tiles(a.cols), bl_tiles(a.rows), a.n), dim3(256), 0, st, a);
}
