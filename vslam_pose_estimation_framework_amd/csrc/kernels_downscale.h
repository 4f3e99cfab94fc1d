// kernels_downscale.h — integer-factor reduction of 8-bit images and 16-bit depth images (gfx950).  The index arithmetic is
// downscale_geometry.h's, shared with the host walk.
//
// Factor f = 2, 3 or 4; a full image of R x C gives R / f x C / f, the R % f bottom rows and C % f right columns are never read.
//   8 bit:  out[y][x] = (sum of the f x f block at (f y, f x) + f f / 2) / (f f), round half up, all integer.  At f = 2 that is
//           (a + b + c + d + 2) >> 2, which cv::resize(INTER_AREA) computes at an integer factor of 2 [recalled]; at 3 and 4 OpenCV goes
//           through a float reciprocal and may differ on ties: parity with it is not pinned.
//   depth:  never blended (a mix across a depth edge invents a surface, as for the nearest-neighbour depth remap): the v non-zero values
//           of the block in ascending order, out = element (v - 1) / 2, the lower median; 0 when v == 0.
//
// k_downscale_u8<f>, a kernel per factor: the grid of k_gray_u8 (x = bands of output rows, here four rows: one per wavefront, y = sides,
// z = streams; a switched-off stream is neither read nor written), a lane per group of four output pixels: per block row f dwords (8-byte loads at 2, three dwords
// at 3, 16-byte loads at 4) and one more when the row's phase is not 0, shifted into place with v_alignbyte_b32; sums by v_sad_u8 against
// zero; one 32-bit store; the loads of up to three groups of a lane (a whole row's at 1241 pixels) are issued before the first sum.  No byte outside [row, row + f * out_cols) of a block row is read and no byte beyond out_cols of a destination
// row is written: ds_groups admits a group to the wide path only when its whole dword window lies inside every one of its f block rows —
// that can fail for the first group (the rounding reaches below the row) and for the last (the extra dword reaches beyond it); those, the
// pixels ahead of the first aligned destination dword and the fewer than four behind the last go through byte loads of exactly their
// own f x f bytes.
// k_downscale_depth_u16<f>, a kernel per factor: one output pixel per lane (two per lane was not built: no comparison exists), the block in registers (dword loads where f is even and the rows are dword aligned,
// element loads otherwise), the order statistic by a fixed sorting network (ds_lower_median): no register array is indexed dynamically.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"
#include "downscale_geometry.h"

struct DownscaleArgs {
  const uint8_t* src[2];      // full images [left/right]: stream s at src[side] + s * src_stream_stride, any alignment
  size_t src_stream_stride;   // bytes
  int32_t src_row_stride;     // bytes, >= factor * cols
  uint8_t* dst[2];            // reduced images
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  int32_t rows, cols;         // the REDUCED size
  int32_t n, sides;           // grid z = n, grid y = sides
  int32_t band;               // output rows per workgroup
  int32_t factor;
  uint32_t active[VS_MAX_STREAMS / 32];
};

// output pixels [i0, i1) of one row by byte loads, a lane per pixel
template <int F>
__device__ __forceinline__ void downscale_bytes(const uint8_t* p, int stride, uint8_t* o, int i0, int i1, int lane) {
  for (int i = i0 + lane; i < i1; i += 64) {
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < F; ++k)
#pragma unroll
      for (int j = 0; j < F; ++j) s += p[(size_t)k * stride + F * i + j];
    o[i] = (uint8_t)ds_round(s, F);
  }
}

// the four sums of F dwords of one block row, added to s
template <int F>
__device__ __forceinline__ void downscale_sums(const uint32_t (&w)[F], uint32_t (&s)[4]) {
  if constexpr (F == 2) {
    s[0] = __builtin_amdgcn_sad_u8(w[0] & 0xffffu, 0u, s[0]); s[1] = __builtin_amdgcn_sad_u8(w[0] >> 16, 0u, s[1]);
    s[2] = __builtin_amdgcn_sad_u8(w[1] & 0xffffu, 0u, s[2]); s[3] = __builtin_amdgcn_sad_u8(w[1] >> 16, 0u, s[3]);
  } else if constexpr (F == 3) {
    s[0] = __builtin_amdgcn_sad_u8(w[0] & 0xffffffu, 0u, s[0]);
    s[1] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[1], w[0], 3u) & 0xffffffu, 0u, s[1]);
    s[2] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[2], w[1], 2u) & 0xffffffu, 0u, s[2]);
    s[3] = __builtin_amdgcn_sad_u8(w[2] >> 8, 0u, s[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = __builtin_amdgcn_sad_u8(w[k], 0u, s[k]);
  }
}

// one output row: p = the first byte of its first block row, o = its first destination byte
template <int F>
__device__ __forceinline__ void downscale_row(const uint8_t* p, int stride, uint8_t* o, int cols, int lane) {
  const int head = ds_head((uintptr_t)o, cols);
  uint32_t sh[F];
  int v_lo = 0, v_hi = (cols - head) >> 2;
#pragma unroll
  for (int k = 0; k < F; ++k) {
    int lo, hi;
    sh[k] = ds_shift((uintptr_t)(p + (size_t)k * stride), F, head);
    ds_groups(cols, F, head, sh[k], &lo, &hi);
    v_lo = max(v_lo, lo); v_hi = min(v_hi, hi);
  }
  if (v_hi <= v_lo) { downscale_bytes<F>(p, stride, o, 0, cols, lane); return; }
  downscale_bytes<F>(p, stride, o, 0, head + 4 * v_lo, lane);
  // U groups of a lane per round, every load of the round issued ahead of the first sum: a row holds few groups per lane (620 pixels are
  // 155 groups), so this puts the whole row's loads in flight at once
  constexpr int U = F == 2 ? 3 : F == 3 ? 2 : 1;      // 18, 24 and 20 dwords a round
  for (int v0 = v_lo + lane; v0 < v_hi; v0 += 64 * U) {
    uint32_t d[U][F][F + 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = v0 + 64 * u;
      if (v < v_hi) {
#pragma unroll
        for (int k = 0; k < F; ++k) {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(p + (size_t)k * stride + ds_window(F, head, sh[k], v));
#pragma unroll
          for (int j = 0; j < F; ++j) d[u][k][j] = q[j];
          d[u][k][F] = sh[k] ? q[F] : 0u;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int v = v0 + 64 * u;
      if (v < v_hi) {
        uint32_t s[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < F; ++k) {
          uint32_t w[F];
#pragma unroll
          for (int j = 0; j < F; ++j) w[j] = __builtin_amdgcn_alignbyte(d[u][k][j + 1], d[u][k][j], sh[k]);
          downscale_sums<F>(w, s);
        }
        *reinterpret_cast<uint32_t*>(o + head + 4 * v) = ds_round(s[0], F) | (ds_round(s[1], F) << 8) | (ds_round(s[2], F) << 16) | (ds_round(s[3], F) << 24);
      }
    }
  }
  downscale_bytes<F>(p, stride, o, head + 4 * v_hi, cols, lane);
}

// a kernel per factor: factor 2 holds 18 dwords a round and runs at the full eight waves per SIMD, which the registers of factor 4 would
// take from it in one kernel
template <int F>
__global__ __launch_bounds__(256, F == 2 ? 8 : 4) void k_downscale_u8(DownscaleArgs a) {
  const int s = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  const int lane = tid & 63, wave = tid >> 6;
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  uint8_t* out = a.dst[side] + (size_t)s * a.dst_stream_stride;
  const int r1 = min(a.rows, ((int)blockIdx.x + 1) * a.band);
  for (int r = blockIdx.x * a.band + wave; r < r1; r += 4) {
    const uint8_t* p = img + (size_t)r * F * a.src_row_stride;
    uint8_t* o = out + (size_t)r * a.dst_row_stride;
    downscale_row<F>(p, a.src_row_stride, o, a.cols, lane);
  }
}

// the reduction on queue st.  Images, strides, the reduced size, factor, n, sides and active are the caller's; a.band is set here: a row
// per wavefront.  (equalize_band's bands, cut for 2048 resident workgroups of 8 waves per SIMD, leave this kernel, which holds fewer, a
// second round that is a quarter full: measured, profiles/downscale_cost_mi355x.txt.)
static hipError_t downscale_enqueue(hipStream_t st, DownscaleArgs a) {
  a.band = 4;
  const dim3 grid((a.rows + a.band - 1) / a.band, a.sides, a.n);
  if (a.factor == 2) hipLaunchKernelGGL(k_downscale_u8<2>, grid, dim3(256), 0, st, a);
  else if (a.factor == 3) hipLaunchKernelGGL(k_downscale_u8<3>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_downscale_u8<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---- depth -------------------------------------------------------------------------------------------------------------
struct DownscaleDepthArgs {
  const uint16_t* src;        // full depth images: sequence s at src + s * src_stream_stride (elements), any 2-byte alignment
  size_t src_stream_stride;
  int32_t src_row_stride;     // elements, >= factor * cols
  uint16_t* dst;              // reduced depth images
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  int32_t rows, cols;         // the REDUCED size
  int32_t n;                  // grid z = n
  int32_t factor;
};

template <int F>
__device__ __forceinline__ uint32_t downscale_depth_pixel(const uint16_t* p, int stride, int x) {
  uint32_t v[F * F];
  const uint16_t* b = p + (size_t)F * x;
  // dword loads: F even, so the block's first element is a whole number of dwords into a row, and every block row dword aligned
  if (F != 3 && (((uintptr_t)p | (uintptr_t)(2 * stride)) & 3u) == 0) {
#pragma unroll
    for (int k = 0; k < F; ++k) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(b + (size_t)k * stride);
#pragma unroll
      for (int j = 0; j < F / 2; ++j) { const uint32_t w = q[j]; v[k * F + 2 * j] = w & 0xffffu; v[k * F + 2 * j + 1] = w >> 16; }
    }
  } else {
#pragma unroll
    for (int k = 0; k < F; ++k)
#pragma unroll
      for (int j = 0; j < F; ++j) v[k * F + j] = b[(size_t)k * stride + j];
  }
  return ds_lower_median<F>(v);
}

// a kernel per factor, like k_downscale_u8
template <int F>
__global__ __launch_bounds__(256) void k_downscale_depth_u16(DownscaleDepthArgs a) {
  const int r = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  if (r >= a.rows || x >= a.cols) return;
  const uint16_t* p = a.src + (size_t)blockIdx.z * a.src_stream_stride + (size_t)r * F * a.src_row_stride;
  a.dst[(size_t)blockIdx.z * a.dst_stream_stride + (size_t)r * a.dst_row_stride + x] = (uint16_t)downscale_depth_pixel<F>(p, a.src_row_stride, x);
}

static hipError_t downscale_depth_enqueue(hipStream_t st, const DownscaleDepthArgs& a) {
  const dim3 grid((a.cols + 63) / 64, (a.rows + 3) / 4, a.n);
  if (a.factor == 2) hipLaunchKernelGGL(k_downscale_depth_u16<2>, grid, dim3(256), 0, st, a);
  else if (a.factor == 3) hipLaunchKernelGGL(k_downscale_depth_u16<3>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_downscale_depth_u16<4>, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
