// kernels_equalize.h — histogram equalisation of 8-bit images ahead of the detector (gfx950).
//
// cv::equalizeHist on one 8-bit image [recalled]:
//   h[256]  = counts of the rows x cols pixels (padding beyond cols never counted)
//   i0      = the first v with h[v] != 0
//   if h[i0] == rows*cols: output = input                          (a constant image stays as it is)
//   scale   = float(255) / float(rows*cols - h[i0])                IEEE single, one correctly rounded division
//   sum_v   = h[i0+1] + ... + h[v]                                 (integers)
//   lut[v]  = 0 for v <= i0, else min(255, rint(float(sum_v) * scale))    one single-precision multiply, ties to even
//   out     = lut[in]
// The two float operations are written with __fdiv_rn / __fmul_rn (no contraction, no reciprocal approximation) and rintf; everything else
// is integer, and rows * cols <= 2^24 keeps every count exact in float: the result is bit-exact by construction.
//
// Two kernels on one grid, x = row bands, y = sides, z = streams; a switched-off stream (DevBuf::active) is neither read nor written.
//   k_hist_u8         one wavefront per row of its band, 16 B per lane where the row is aligned (byte lanes for the unaligned head and the
//                     tail), 32-bit LDS counters in VS_EQ_COPIES copies per bin chosen by lane (copy-minor layout: the copies of one bin lie
//                     in different banks), equal neighbouring bytes of a lane's 16 merged into one add — a constant image costs one LDS add
//                     per 16 B instead of sixteen on one address; the band's counts leave with one vector integer atomic per non-empty bin
//                     into hist[stream][side][256], which the host zeroes on the same queue ahead of the launch.  Integer sums do not
//                     depend on the order of arrival.
//   k_equalize_apply  every workgroup rebuilds the LUT in LDS (first non-empty bin, 256-wide scan, the two float operations) and maps its
//                     band through it, 16 B per lane in and out; in place when dst == src.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"

#ifndef VS_EQ_COPIES
#define VS_EQ_COPIES 8        // LDS counter copies per bin (a power of two, <= 32)
#endif
#define VS_EQ_MAX_PIXELS (1 << 24)

struct EqArgs {
  const uint8_t* src[2];      // images [left/right]: stream s at src[side] + s * src_stream_stride, any alignment
  size_t src_stream_stride;
  int32_t src_row_stride;
  uint8_t* dst[2];            // equalised images (may be src: in place); null for a count alone
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  uint32_t* hist;             // [n][sides][256]
  int32_t rows, cols;
  int32_t n, sides;           // grid z = n, grid y = sides
  int32_t band;               // rows per workgroup
  uint32_t active[VS_MAX_STREAMS / 32];
};

// the bytes of one aligned 16-B load into the lane's counter copy, equal neighbours merged
__device__ __forceinline__ void eq_count16(uint32_t* cnt, const uint4& q, int copy) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  uint32_t cur = w[0] & 255u, run = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 255u;
    if (b == cur) ++run;
    else { atomicAdd(&cnt[cur * VS_EQ_COPIES + copy], run); cur = b; run = 1; }
  }
  atomicAdd(&cnt[cur * VS_EQ_COPIES + copy], run);
}

__global__ __launch_bounds__(256) void k_hist_u8(EqArgs a) {
  __shared__ uint32_t cnt[256 * VS_EQ_COPIES];
  const int s = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  for (int i = tid; i < 256 * VS_EQ_COPIES; i += 256) cnt[i] = 0;
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6, copy = lane & (VS_EQ_COPIES - 1);
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  const int r1 = min(a.rows, ((int)blockIdx.x + 1) * a.band);
  for (int r = blockIdx.x * a.band + wave; r < r1; r += 4) {
    const uint8_t* p = img + (size_t)r * a.src_row_stride;
    const int head = min(a.cols, (int)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u));
    if (lane < head) atomicAdd(&cnt[p[lane] * VS_EQ_COPIES + copy], 1u);
    const int nvec = (a.cols - head) >> 4;
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    for (int v = lane; v < nvec; v += 64) eq_count16(cnt, pv[v], copy);
    const int t0 = head + nvec * 16;                                    // fewer than 16 bytes are left
    if (t0 + lane < a.cols) atomicAdd(&cnt[p[t0 + lane] * VS_EQ_COPIES + copy], 1u);
  }
  __syncthreads();
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < VS_EQ_COPIES; ++j) sum += cnt[tid * VS_EQ_COPIES + ((j + tid) & (VS_EQ_COPIES - 1))];
  if (sum) atomicAdd(&a.hist[((size_t)s * a.sides + side) * 256 + tid], sum);
}

__device__ __forceinline__ uint32_t eq_map4(const uint8_t* lut, uint32_t w) {
  return (uint32_t)lut[w & 255u] | ((uint32_t)lut[(w >> 8) & 255u] << 8) | ((uint32_t)lut[(w >> 16) & 255u] << 16) | ((uint32_t)lut[w >> 24] << 24);
}

__global__ __launch_bounds__(256) void k_equalize_apply(EqArgs a) {
  __shared__ uint32_t scan[256];
  __shared__ uint8_t lut[256];
  __shared__ int first;
  const int s = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  const uint32_t h = a.hist[((size_t)s * a.sides + side) * 256 + tid];
  scan[tid] = h;
  if (tid == 0) first = 256;
  __syncthreads();
  if (h) atomicMin(&first, tid);
  for (int d = 1; d < 256; d <<= 1) {                                   // inclusive scan of the counts
    const uint32_t v = tid >= d ? scan[tid - d] : 0u;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int i0 = first;
  const uint32_t total = scan[255], base = i0 < 256 ? scan[i0] : 0u;    // base = h[i0]: every bin below it is empty
  if (i0 > 255 || base == total) lut[tid] = (uint8_t)tid;               // a constant image copies through
  else {
    const float scale = __fdiv_rn(255.f, (float)(total - base));
    const float m = __fmul_rn((float)(scan[tid] - base), scale);
    lut[tid] = tid <= i0 ? (uint8_t)0 : (uint8_t)min(255, (int)rintf(m));
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  uint8_t* out = a.dst[side] + (size_t)s * a.dst_stream_stride;
  const int r1 = min(a.rows, ((int)blockIdx.x + 1) * a.band);
  for (int r = blockIdx.x * a.band + wave; r < r1; r += 4) {
    const uint8_t* p = img + (size_t)r * a.src_row_stride;
    uint8_t* o = out + (size_t)r * a.dst_row_stride;
    const int head = min(a.cols, (int)((16u - (uint32_t)((uintptr_t)o & 15u)) & 15u));
    if (lane < head) o[lane] = lut[p[lane]];
    const int nvec = (a.cols - head) >> 4;
    uint4* ov = reinterpret_cast<uint4*>(o + head);
    if ((((uintptr_t)p ^ (uintptr_t)o) & 15u) == 0) {                   // source and destination rows aligned alike: 16 B in, 16 B out
      const uint4* pv = reinterpret_cast<const uint4*>(p + head);
      for (int v = lane; v < nvec; v += 64) {
        const uint4 q = pv[v];
        ov[v] = make_uint4(eq_map4(lut, q.x), eq_map4(lut, q.y), eq_map4(lut, q.z), eq_map4(lut, q.w));
      }
    } else {                                                            // a caller's image at another alignment: byte loads, 16-B stores
      for (int v = lane; v < nvec; v += 64) {
        const uint8_t* pb = p + head + 16 * v;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          w[k] = (uint32_t)lut[pb[4 * k]] | ((uint32_t)lut[pb[4 * k + 1]] << 8) | ((uint32_t)lut[pb[4 * k + 2]] << 16) | ((uint32_t)lut[pb[4 * k + 3]] << 24);
        ov[v] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
    const int t0 = head + nvec * 16;
    if (t0 + lane < a.cols) o[t0 + lane] = lut[p[t0 + lane]];
  }
}

// rows per workgroup: about 2048 workgroups in all, never fewer than one row per wavefront
static int equalize_band(int rows, int images) {
  const int bands = std::max(1, std::min((rows + 3) / 4, 2048 / std::max(images, 1)));
  return std::max(4, (rows + bands - 1) / bands);
}
// the table zeroed, the count, and (with a destination) the mapping, on queue st.  a.hist, the images, sizes, n, sides and active are the
// caller's; a.band is set here.
static hipError_t equalize_enqueue(hipStream_t st, EqArgs a) {
  a.band = equalize_band(a.rows, a.n * a.sides);
  const hipError_t e = hipMemsetAsync(a.hist, 0, (size_t)a.n * a.sides * 256 * sizeof(uint32_t), st);
  if (e != hipSuccess) return e;
  const dim3 grid((a.rows + a.band - 1) / a.band, a.sides, a.n);
  hipLaunchKernelGGL(k_hist_u8, grid, dim3(256), 0, st, a);
  if (a.dst[0]) hipLaunchKernelGGL(k_equalize_apply, grid, dim3(256), 0, st, a);
  return hipSuccess;
}
