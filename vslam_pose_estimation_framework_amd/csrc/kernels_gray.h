// kernels_gray.h — interleaved 8-bit colour to grey ahead of everything else in the frame path (gfx950).
//
// cvtColor(CV_BGR2GRAY / CV_RGB2GRAY / CV_BGRA2GRAY / CV_RGBA2GRAY) on 8-bit images, 14 fractional bits [recalled: the OpenCV 3.x of the
// reference's image; io_formats.rgb_to_gray_opencv states the same]:
//   gray = (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14          all integer; the largest sum, 255 * 16384 + 8192, needs 22 bits
// Alpha is ignored.  The 15-bit coefficients of newer OpenCV (9798 / 19235 / 3735) are not built.
//
// One kernel, the grid of the equalisation pair: x = row bands, y = sides, z = streams; a switched-off stream (DevBuf::active) is neither
// read nor written.  One wavefront per row.  The row is cut at the DESTINATION's 16-byte borders: a lane owns one aligned group of 16 output
// pixels and stores it with one 16-byte store.  Its 48 (64) source bytes start at any address: the lane loads the 12 (16) dwords from the
// dword-aligned address below its first byte, and one more when that address is not its first byte, and shifts the pairs into place with
// v_alignbyte_b32 by (address & 3), which is the same for every group of a row (48 and 64 are multiples of 4).  Bytes leave the dwords by
// shift-and-mask and enter 24-bit multiply-adds.
// No load touches a byte outside [row, row + channels * cols) of its own row: a group takes the wide path only when its whole dword window
// [first byte rounded down to 4, + 48/64 (+ 4 when rounded)) lies inside the row — that can fail for the row's first group (the rounding
// reaches below the row) and for its last (the extra dword reaches beyond it), nowhere else; those groups, the pixels ahead of the first
// aligned group and the fewer than 16 behind the last go through byte loads of exactly their own three bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"
#include "kernels_equalize.h"     // equalize_band: the same grid

#define VS_GRAY_CR 4899u
#define VS_GRAY_CG 9617u
#define VS_GRAY_CB 1868u

struct GrayArgs {
  const uint8_t* src[2];      // colour images [left/right]: stream s at src[side] + s * src_stream_stride, any alignment
  size_t src_stream_stride;   // bytes
  int32_t src_row_stride;     // bytes, >= channels * cols
  uint8_t* dst[2];            // grey images
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  int32_t rows, cols;
  int32_t n, sides;           // grid z = n, grid y = sides
  int32_t band;               // rows per workgroup
  int32_t format;             // VSLAM_PIXEL_BGR8 .. VSLAM_PIXEL_RGBA8
  uint32_t active[VS_MAX_STREAMS / 32];
};

// channels of a pixel format (1 .. 4), and whether its first byte is red
static __host__ __device__ __forceinline__ int gray_channels(int format) { return format <= 2 ? 3 : 4; }
static __host__ __device__ __forceinline__ bool gray_red_first(int format) { return format == 2 || format == 4; }

__device__ __forceinline__ uint32_t gray_of(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t c0, uint32_t c2) {
  return (__umul24(b0, c0) + __umul24(b1, VS_GRAY_CG) + __umul24(b2, c2) + 8192u) >> 14;
}
__device__ __forceinline__ uint32_t gray_byte(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }

// pixels [i0, i1) of one row by byte loads, a lane per pixel
template <int CH>
__device__ __forceinline__ void gray_bytes(const uint8_t* p, uint8_t* o, int i0, int i1, int lane, uint32_t c0, uint32_t c2) {
  for (int i = i0 + lane; i < i1; i += 64) {
    const uint8_t* s = p + CH * i;
    o[i] = (uint8_t)gray_of(s[0], s[1], s[2], c0, c2);
  }
}

// one row: p = its first source byte, o = its first destination byte
template <int CH>
__device__ __forceinline__ void gray_row(const uint8_t* p, uint8_t* o, int cols, int lane, uint32_t c0, uint32_t c2) {
  constexpr int ND = 4 * CH;                                              // dwords of 16 pixels
  const int head = min(cols, (int)((16u - (uint32_t)((uintptr_t)o & 15u)) & 15u));
  const int nvec = (cols - head) >> 4;
  const uint32_t sh = (uint32_t)((uintptr_t)(p + CH * head) & 3u);       // of every group of this row
  const int extra = sh ? 4 : 0;
  // groups whose dword window lies inside the row: [v_lo, v_hi)
  int v_lo = (head == 0 && sh) ? 1 : 0;
  const int room = CH * (cols - head) + (int)sh - 4 * ND - extra;         // >= 16 * CH * v  <=>  group v's window ends inside the row
  int v_hi = room < 0 ? 0 : min(nvec, room / (16 * CH) + 1);
  if (v_hi <= v_lo) { gray_bytes<CH>(p, o, 0, cols, lane, c0, c2); return; }
  gray_bytes<CH>(p, o, 0, head + 16 * v_lo, lane, c0, c2);
  const uint8_t* a0 = p + CH * head - sh;                                 // dword aligned; >= p for every v >= v_lo
  for (int v = v_lo + lane; v < v_hi; v += 64) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a0 + (size_t)(16 * CH) * v);
    uint32_t d[ND + 1];
#pragma unroll
    for (int k = 0; k < ND; ++k) d[k] = q[k];
    d[ND] = sh ? q[ND] : 0u;
    uint32_t w[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) w[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
    uint32_t g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                         // four pixels per output dword
      uint32_t g0, g1, g2, g3;
      if (CH == 3) {
        const uint32_t a = w[3 * k], b = w[3 * k + 1], c = w[3 * k + 2];
        g0 = gray_of(gray_byte(a, 0), gray_byte(a, 1), gray_byte(a, 2), c0, c2);
        g1 = gray_of(gray_byte(a, 3), gray_byte(b, 0), gray_byte(b, 1), c0, c2);
        g2 = gray_of(gray_byte(b, 2), gray_byte(b, 3), gray_byte(c, 0), c0, c2);
        g3 = gray_of(gray_byte(c, 1), gray_byte(c, 2), gray_byte(c, 3), c0, c2);
      } else {
        const uint32_t x0 = w[4 * k], x1 = w[4 * k + 1], x2 = w[4 * k + 2], x3 = w[4 * k + 3];
        g0 = gray_of(gray_byte(x0, 0), gray_byte(x0, 1), gray_byte(x0, 2), c0, c2);
        g1 = gray_of(gray_byte(x1, 0), gray_byte(x1, 1), gray_byte(x1, 2), c0, c2);
        g2 = gray_of(gray_byte(x2, 0), gray_byte(x2, 1), gray_byte(x2, 2), c0, c2);
        g3 = gray_of(gray_byte(x3, 0), gray_byte(x3, 1), gray_byte(x3, 2), c0, c2);
      }
      g[k] = g0 | (g1 << 8) | (g2 << 16) | (g3 << 24);
    }
    *reinterpret_cast<uint4*>(o + head + 16 * v) = make_uint4(g[0], g[1], g[2], g[3]);
  }
  gray_bytes<CH>(p, o, head + 16 * v_hi, cols, lane, c0, c2);
}

__global__ __launch_bounds__(256) void k_gray_u8(GrayArgs a) {
  const int s = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  const int lane = tid & 63, wave = tid >> 6;
  const bool rf = gray_red_first(a.format);
  const uint32_t c0 = rf ? VS_GRAY_CR : VS_GRAY_CB, c2 = rf ? VS_GRAY_CB : VS_GRAY_CR;
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  uint8_t* out = a.dst[side] + (size_t)s * a.dst_stream_stride;
  const int r1 = min(a.rows, ((int)blockIdx.x + 1) * a.band);
  for (int r = blockIdx.x * a.band + wave; r < r1; r += 4) {
    const uint8_t* p = img + (size_t)r * a.src_row_stride;
    uint8_t* o = out + (size_t)r * a.dst_row_stride;
    if (gray_channels(a.format) == 3) gray_row<3>(p, o, a.cols, lane, c0, c2);
    else gray_row<4>(p, o, a.cols, lane, c0, c2);
  }
}

// the conversion on queue st.  Images, strides, sizes, format, n, sides and active are the caller's; a.band is set here.
static hipError_t gray_enqueue(hipStream_t st, GrayArgs a) {
  a.band = equalize_band(a.rows, a.n * a.sides);
  hipLaunchKernelGGL(k_gray_u8, dim3((a.rows + a.band - 1) / a.band, a.sides, a.n), dim3(256), 0, st, a);
  return hipGetLastError();
}
