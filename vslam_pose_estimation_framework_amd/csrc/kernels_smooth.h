// kernels_smooth.h — noise suppression on the 8-bit intensity image ahead of the equalisation slot and the detector (gfx950): a
// fixed-point Gaussian of 3, 5 or 7 taps and a median of 3 x 3 or 5 x 5.  All integer, bit-exact by definition (smooth.py restates it):
//   Gaussian: taps K in 1/256 — {64,128,64}, {16,64,96,64,16}, {8,28,56,72,56,28,8} — out = (sum_i sum_j K_i K_j p(y+i-r, x+j-r) + 32768) >> 16,
//             rows and columns reflected without edge duplication (index -1 -> 1); it needs rows > r and cols > r.
//   median:   element k k / 2 of the sorted k x k window, rows and columns clamped to the image (replicated border); any size.
//
// k_smooth<MODE, R>, a kernel per mode and radius, streams the image: no LDS.  grid z = stream * sides + side (a switched-off stream is
// neither read nor written), grid x = wavefronts / 4.  A wavefront owns `band` output rows of one 256-column chunk and walks down them; a
// lane owns four consecutive pixels, placed so that its destination dword is aligned wherever the destination's row stride allows it.
// The few groups of a row that cannot take the dword path belong to a wavefront of their own per band (above k_smooth).
// Per source row a lane loads the four aligned dwords that cover its columns x0 - 4 .. x0 + 7 and shifts them into place with v_alignbyte_b32; a row's loads are issued 2 r + 1 rows ahead of its arithmetic.  What a row leaves
// behind stays in registers for the 2 r rows after it (in place: the row loop is unrolled 2 r + 1 times): the Gaussian keeps its four row sums, two to a register (255 * 256 fits 16 bits; v_dot4_u32_u8 on the
// taps; the column pass is v_dot2_u32_u16), the median its columns as packed half-precision pairs (0x6400 | p is the exact half 1024 + p, ordered like p), so a source byte
// leaves memory about once per band (band + 2 r rows are read for band rows written).
// The 3 x 3 median sorts every column of three once (shared by the three windows it belongs to), then takes the median of {max of the
// lows, median of the mids, min of the highs}; the 5 x 5 median is a 99-exchange selection network on the 25 packed values, whose
// unused halves the compiler drops.  Both on v_pk_minimum3_f16 / v_pk_maximum3_f16 (pk_min3 / pk_max3 of kernels_image.h).
// Bounds: the dword path is taken by a lane only when x0 >= 7 and x0 + 12 <= cols, so that every aligned dword it loads lies inside
// [row, row + cols) whatever the row's phase; every other lane loads exactly the bytes of its taps, border-mapped and clamped into the
// row.  No byte beyond cols of a destination row is written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"

#define VS_SMOOTH_OFF 0
#define VS_SMOOTH_GAUSSIAN 1
#define VS_SMOOTH_MEDIAN 2

struct SmoothArgs {
  const uint8_t* src[2];      // images [left/right]: stream s at src[side] + s * src_stream_stride, any alignment
  size_t src_stream_stride;   // bytes
  int32_t src_row_stride;     // bytes, >= cols
  uint8_t* dst[2];            // never the source: the stage cannot work in place
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  int32_t rows, cols;
  int32_t n, sides;           // grid z = n * sides
  int32_t mode, ksize;        // VS_SMOOTH_*, 3 / 5 / 7
  int32_t band, chunks;       // output rows per wavefront; 256-column chunks per row (set by smooth_enqueue)
  uint32_t active[VS_MAX_STREAMS / 32];
};

// which (mode, ksize) pairs exist, and what they ask of the size (host and device)
__host__ __device__ inline bool smooth_mode_ok(int mode, int ksize) {
  return mode == VS_SMOOTH_GAUSSIAN ? (ksize == 3 || ksize == 5 || ksize == 7) : mode == VS_SMOOTH_MEDIAN ? (ksize == 3 || ksize == 5) : false;
}
__host__ __device__ inline bool smooth_size_ok(int mode, int ksize, int rows, int cols) {
  return rows >= 1 && cols >= 1 && (mode != VS_SMOOTH_GAUSSIAN || (rows > ksize / 2 && cols > ksize / 2));
}

// border: index p of n mapped into 0 .. n - 1 — reflected (Gaussian) or clamped (median); the final clamp only ever moves taps of
// pixels that are not written (n > r holds for the Gaussian)
template <int MODE>
__device__ __forceinline__ int smooth_border(int p, int n) {
  if (MODE == VS_SMOOTH_GAUSSIAN) p = p < 0 ? -p : (p >= n ? 2 * n - 2 - p : p);
  return min(max(p, 0), n - 1);
}

// one source row of a lane as loaded: d[0..3] aligned dwords to be shifted by sh bytes (dword path) or columns x0 - 4 .. x0 + 7 in
// d[0..2] with sh == 0 (byte path)
struct SmoothRaw { uint32_t d[4]; uint32_t sh; };

// STREAM (a streaming wavefront, cols >= 20): every lane loads its four dwords without a branch — a lane outside the dword path loads the
// nearest columns that are on it and its result is never stored —, so that the loads of the rows ahead stay counted (a load under a
// branch makes every wait a wait for all of them)
template <int MODE, int R, bool STREAM>
__device__ __forceinline__ SmoothRaw smooth_fetch(const uint8_t* row, int cols, int x0, bool wide, bool edge) {
  SmoothRaw w;
  if constexpr (STREAM) {
    const uint8_t* a = row + min(max(x0, 7), cols - 12) - 4;      // 7 .. cols - 12: the dword path's own range
    w.sh = (uint32_t)((uintptr_t)a & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - w.sh);
    w.d[0] = q[0]; w.d[1] = q[1]; w.d[2] = q[2]; w.d[3] = q[3];
    return w;
  }
  w.d[0] = w.d[1] = w.d[2] = w.d[3] = 0u; w.sh = 0u;
  if (wide) {
    // (pointer arithmetic, not an integer round trip: the loads stay global_load, which return in order and can be counted)
    const uint8_t* a = row + x0 - 4;
    w.sh = (uint32_t)((uintptr_t)a & 3u);
    const uint32_t* q = reinterpret_cast<const uint32_t*>(a - w.sh);
    // the fourth dword is needed only when sh != 0, but it lies inside the row either way (x0 + 12 <= cols) and a branch here would
    // keep the loads from being counted
    w.d[0] = q[0]; w.d[1] = q[1]; w.d[2] = q[2]; w.d[3] = q[3];
  } else if (edge) {
#pragma unroll
    for (int k = 4 - R; k < 8 + R; ++k)
      w.d[k >> 2] |= (uint32_t)row[smooth_border<MODE>(x0 - 4 + k, cols)] << (8 * (k & 3));
  }
  return w;
}
// columns x0 - 4 .. x0 - 1, x0 .. x0 + 3, x0 + 4 .. x0 + 7
__device__ __forceinline__ void smooth_lcr(const SmoothRaw& w, uint32_t* L, uint32_t* C, uint32_t* Rr) {
  *L = __builtin_amdgcn_alignbyte(w.d[1], w.d[0], w.sh);
  *C = __builtin_amdgcn_alignbyte(w.d[2], w.d[1], w.sh);
  *Rr = __builtin_amdgcn_alignbyte(w.d[3], w.d[2], w.sh);
}
// the dword at byte offset OFF (0 .. 8) of the twelve bytes L C R
template <int OFF>
__device__ __forceinline__ uint32_t smooth_window(uint32_t L, uint32_t C, uint32_t Rr) {
  if constexpr (OFF == 0) return L;
  else if constexpr (OFF < 4) return __builtin_amdgcn_alignbyte(C, L, (uint32_t)OFF);
  else if constexpr (OFF == 4) return C;
  else if constexpr (OFF < 8) return __builtin_amdgcn_alignbyte(Rr, C, (uint32_t)(OFF - 4));
  else return Rr;
}

// ---- Gaussian ---------------------------------------------------------------------------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
template <int R> struct SmoothTaps;
template <> struct SmoothTaps<1> { static constexpr uint32_t k[3] = {64, 128, 64}; };
template <> struct SmoothTaps<2> { static constexpr uint32_t k[5] = {16, 64, 96, 64, 16}; };
template <> struct SmoothTaps<3> { static constexpr uint32_t k[7] = {8, 28, 56, 72, 56, 28, 8}; };

// taps FIRST .. FIRST + 3 (those that exist) as the bytes of a dword, tap FIRST at byte AT
template <int R, int FIRST, int AT>
__device__ __forceinline__ constexpr uint32_t smooth_tap_word() {
  uint32_t w = 0;
  for (int t = 0; t < 4; ++t)
    if (FIRST + t <= 2 * R && AT + t < 4) w |= SmoothTaps<R>::k[FIRST + t] << (8 * (AT + t));
  return w;
}
// the row sum of pixel J of the lane's four: taps at bytes 4 + J - R .. 4 + J + R of L C R
template <int R, int J>
__device__ __forceinline__ uint32_t smooth_row_sum(uint32_t L, uint32_t C, uint32_t Rr) {
  constexpr int F = 4 + J - R;
  uint32_t s = __builtin_amdgcn_udot4(smooth_window<F>(L, C, Rr), smooth_tap_word<R, 0, 0>(), 0u, false);
  if constexpr (R > 1) {
    constexpr int F2 = F + 4 < 8 ? F + 4 : 8;        // taps 4 .. 2 R sit at bytes F + 4 - F2 .. of this dword
    s = __builtin_amdgcn_udot4(smooth_window<F2>(L, C, Rr), smooth_tap_word<R, 4, F + 4 - F2>(), s, false);
  }
  return s;
}

// ---- median -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ h16x2 smooth_h(uint32_t v) { return __builtin_bit_cast(h16x2, v | 0x64006400u); }
__device__ __forceinline__ uint32_t smooth_u(h16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ h16x2 smooth_min(h16x2 a, h16x2 b) { return pk_min3(a, b, b); }
__device__ __forceinline__ h16x2 smooth_max(h16x2 a, h16x2 b) { return pk_max3(a, b, b); }
__device__ __forceinline__ h16x2 smooth_med3(h16x2 a, h16x2 b, h16x2 c) { return smooth_max(smooth_min(a, b), smooth_min(smooth_max(a, b), c)); }
// (hi half of lo, lo half of hi): the pair one column to the right of lo
__device__ __forceinline__ h16x2 smooth_between(h16x2 lo, h16x2 hi) { return __builtin_bit_cast(h16x2, __builtin_amdgcn_alignbit(smooth_u(hi), smooth_u(lo), 16u)); }
// two packed results -> four bytes
__device__ __forceinline__ uint32_t smooth_pack(h16x2 p01, h16x2 p23) { return __builtin_amdgcn_perm(smooth_u(p23), smooth_u(p01), 0x06040200u); }

// median of 25 by 99 exchanges (the selection network published with N. Devillard's "Fast median search", 1998; checked over all 2^25
// 0/1 inputs by tests/test_smooth_host.py, which reads this table)
// clang-format off
#define VS_SMOOTH_MED25_NET \
  {0,1},{3,4},{2,4},{2,3},{6,7},{5,7},{5,6},{9,10},{8,10},{8,9},{12,13},{11,13},{11,12},{15,16},{14,16},{14,15},{18,19},{17,19},{17,18},{21,22},{20,22},{20,21}, \
  {23,24},{2,5},{3,6},{0,6},{0,3},{4,7},{1,7},{1,4},{11,14},{8,14},{8,11},{12,15},{9,15},{9,12},{13,16},{10,16},{10,13},{20,23},{17,23},{17,20},{21,24},{18,24}, \
  {18,21},{19,22},{8,17},{9,18},{0,18},{0,9},{10,19},{1,19},{1,10},{11,20},{2,20},{2,11},{12,21},{3,21},{3,12},{13,22},{4,22},{4,13},{14,23},{5,23},{5,14},{15,24}, \
  {6,24},{6,15},{7,16},{7,19},{13,21},{15,23},{7,13},{7,15},{1,9},{3,11},{5,17},{11,17},{9,17},{4,10},{6,12},{7,14},{4,6},{4,7},{12,14},{10,14},{6,7},{10,12}, \
  {6,10},{6,17},{12,17},{7,17},{7,10},{12,18},{7,12},{10,18},{12,20},{10,20},{10,12}
// clang-format on
__device__ __forceinline__ h16x2 smooth_med25(h16x2 (&p)[25]) {
  constexpr uint8_t net[99][2] = {VS_SMOOTH_MED25_NET};
#pragma unroll
  for (int e = 0; e < 99; ++e) {
    const h16x2 a = p[net[e][0]], b = p[net[e][1]];
    p[net[e][0]] = smooth_min(a, b);
    p[net[e][1]] = smooth_max(a, b);
  }
  return p[12];
}

// ---- the kernel -------------------------------------------------------------------------------------------------------------
// Output rows y0 .. y1 - 1 of the lane's pixels x0 .. x0 + 3.  edge: the lane has pixels at all; wide: it takes the dword path; whole:
// all four pixels are inside the image.
template <int MODE, int R, bool STREAM>
__device__ __forceinline__ void smooth_walk(const SmoothArgs& a, const uint8_t* img, uint8_t* out, int x0, int y0, int y1, bool edge, bool wide, bool whole) {
  const int rows = a.rows, cols = a.cols;

  // what the last 2 R + 1 source rows left behind.  The row loop is unrolled 2 R + 1 times, so that the newest row's slot, and with it
  // every slot's age, is known at compile time and no register moves; the 5 x 5 median, whose body is some 400 instructions, shifts its
  // sixteen registers instead.  AGE(a): the slot of the row a rows below the oldest.
  constexpr int N = 2 * R + 1;
  constexpr int KEEP = MODE == VS_SMOOTH_GAUSSIAN ? 2 : (R == 1 ? 3 : 4);
  constexpr bool ROTATE = MODE == VS_SMOOTH_GAUSSIAN || R == 1;
  constexpr int UNROLL = ROTATE ? N : 1;
  uint32_t ring[N][KEEP];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int k = 0; k < KEEP; ++k) ring[i][k] = 0u;

  // UNROLL source rows are in flight per lane: a row's loads are issued UNROLL rows ahead of its arithmetic
  const int last = y1 - 1 + R;
  SmoothRaw ahead[UNROLL];
#pragma unroll
  for (int ph = 0; ph < UNROLL; ++ph)
    ahead[ph] = smooth_fetch<MODE, R, STREAM>(img + (size_t)smooth_border<MODE>(min(y0 - R + ph, last), rows) * a.src_row_stride, cols, x0, wide && y0 - R + ph <= last, edge && y0 - R + ph <= last);
  for (int sy0 = y0 - R; sy0 <= last; sy0 += UNROLL) {
#pragma unroll
  for (int ph = 0; ph < UNROLL; ++ph) {
    const int sy = sy0 + ph;
    if (sy > last) break;
    const SmoothRaw cur = ahead[ph];
    // (streaming: beyond the band's last row that row again, which the cache holds, instead of a branch)
    if (STREAM || sy + UNROLL <= last) ahead[ph] = smooth_fetch<MODE, R, STREAM>(img + (size_t)smooth_border<MODE>(min(sy + UNROLL, last), rows) * a.src_row_stride, cols, x0, wide, edge);
    uint32_t L, C, Rr;
    smooth_lcr(cur, &L, &C, &Rr);
    if constexpr (!ROTATE) {
#pragma unroll
      for (int i = 0; i < N - 1; ++i)
#pragma unroll
        for (int k = 0; k < KEEP; ++k) ring[i][k] = ring[i + 1][k];
    }
#define VS_SMOOTH_AGE(a) (ROTATE ? (ph + 1 + (a)) % N : (a))
    uint32_t* nw = ring[VS_SMOOTH_AGE(N - 1)];
    if constexpr (MODE == VS_SMOOTH_GAUSSIAN) {
      // row sums are below 2^16: two to a register
      nw[0] = smooth_row_sum<R, 0>(L, C, Rr) | (smooth_row_sum<R, 1>(L, C, Rr) << 16);
      nw[1] = smooth_row_sum<R, 2>(L, C, Rr) | (smooth_row_sum<R, 3>(L, C, Rr) << 16);
    } else if constexpr (R == 1) {     // columns (-1, 0), (1, 2), (3, 4)
      nw[0] = __builtin_amdgcn_perm(C, L, 0x0c040c03u); nw[1] = __builtin_amdgcn_perm(0u, C, 0x0c020c01u); nw[2] = __builtin_amdgcn_perm(Rr, C, 0x0c040c03u);
    } else {                           // columns (-2, -1), (0, 1), (2, 3), (4, 5)
      nw[0] = __builtin_amdgcn_perm(0u, L, 0x0c030c02u); nw[1] = __builtin_amdgcn_perm(0u, C, 0x0c010c00u);
      nw[2] = __builtin_amdgcn_perm(0u, C, 0x0c030c02u); nw[3] = __builtin_amdgcn_perm(0u, Rr, 0x0c010c00u);
    }
    const int y = sy - R;
    if (y < y0 || !edge) continue;

    uint32_t px;
    if constexpr (MODE == VS_SMOOTH_GAUSSIAN) {
      uint32_t o[4];
#pragma unroll
      for (int q = 0; q < 2; ++q) {      // v_dot2_u32_u16 with the tap in one half and zero in the other picks a pixel's row sum out of its pair
        uint32_t lo = 32768u, hi = 32768u;
#pragma unroll
        for (int i = 0; i < N; ++i) {
          lo = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, ring[VS_SMOOTH_AGE(i)][q]), __builtin_bit_cast(u16x2, SmoothTaps<R>::k[i]), lo, false);
          hi = __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, ring[VS_SMOOTH_AGE(i)][q]), __builtin_bit_cast(u16x2, SmoothTaps<R>::k[i] << 16), hi, false);
        }
        o[2 * q] = lo >> 16; o[2 * q + 1] = hi >> 16;
      }
      px = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
    } else if constexpr (R == 1) {
      h16x2 lo[5], mid[5], hi[5];      // per column pair: 0, 2, 4 as loaded, 1, 3 between them
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const h16x2 r0 = smooth_h(ring[0][k]), r1 = smooth_h(ring[1][k]), r2 = smooth_h(ring[2][k]);
        lo[2 * k] = pk_min3(r0, r1, r2); hi[2 * k] = pk_max3(r0, r1, r2); mid[2 * k] = smooth_med3(r0, r1, r2);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        lo[2 * k + 1] = smooth_between(lo[2 * k], lo[2 * k + 2]); mid[2 * k + 1] = smooth_between(mid[2 * k], mid[2 * k + 2]);
        hi[2 * k + 1] = smooth_between(hi[2 * k], hi[2 * k + 2]);
      }
      h16x2 res[2];
#pragma unroll
      for (int k = 0; k < 2; ++k)
        res[k] = smooth_med3(pk_max3(lo[2 * k], lo[2 * k + 1], lo[2 * k + 2]), smooth_med3(mid[2 * k], mid[2 * k + 1], mid[2 * k + 2]),
                             pk_min3(hi[2 * k], hi[2 * k + 1], hi[2 * k + 2]));
      px = smooth_pack(res[0], res[1]);
    } else {
      h16x2 res[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {    // pixels (0, 1) from column pairs 0 .. 2 of the ring rows, pixels (2, 3) from pairs 1 .. 3
        h16x2 p[25];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const h16x2 e0 = smooth_h(ring[i][k]), e1 = smooth_h(ring[i][k + 1]), e2 = smooth_h(ring[i][k + 2]);
          p[5 * i] = e0; p[5 * i + 1] = smooth_between(e0, e1); p[5 * i + 2] = e1; p[5 * i + 3] = smooth_between(e1, e2); p[5 * i + 4] = e2;
        }
        res[k] = smooth_med25(p);
      }
      px = smooth_pack(res[0], res[1]);
    }
#undef VS_SMOOTH_AGE
    uint8_t* o = out + (size_t)y * a.dst_row_stride + x0;
    if (whole && ((uintptr_t)o & 3u) == 0) {
      *reinterpret_cast<uint32_t*>(o) = px;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j >= 0 && x0 + j < cols) o[j] = (uint8_t)(px >> (8 * j));
    }
  }
  }
}

// The lanes' grid: pixels x0 = 4 g - pad .. x0 + 3 for group g, pad = the destination's byte phase, so that out + x0 is dword aligned in
// row 0 and in every row whose offset is a multiple of 4.  Main wavefronts (band, chunk) own the groups of their 256 columns that take
// the dword path, down the whole band, with scalar row arithmetic and no byte path taken.  One more wavefront per band owns the
// groups that cannot — the first four and the last four, less those that can —: lane & 7 picks the group, lane >> 3 an eighth of the
// band's rows, so that the byte path's cost stays out of the streaming wavefronts.
template <int MODE, int R>
__global__ __launch_bounds__(256) void k_smooth(SmoothArgs a) {
  const int z = blockIdx.z, s = z / a.sides, side = z - s * a.sides;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int bands = (a.rows + a.band - 1) / a.band, mains = bands * a.chunks;
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  uint8_t* out = a.dst[side] + (size_t)s * a.dst_stream_stride;
  const int cols = a.cols, pad = (int)((uintptr_t)out & 3u);
  if (w < mains) {
    const int bi = w / a.chunks, chunk = w - bi * a.chunks;
    const int y0 = bi * a.band, y1 = min(a.rows, y0 + a.band);
    const int x0 = 4 * (chunk * 64 + lane) - pad;
    const bool wide = x0 >= 7 && x0 + 12 <= cols;
    if (cols >= 20) smooth_walk<MODE, R, true>(a, img, out, x0, y0, y1, wide, wide, true);
    else smooth_walk<MODE, R, false>(a, img, out, x0, y0, y1, wide, wide, true);
  } else if (w - mains < bands) {
    const int bi = w - mains, e = lane & 7, per = a.band >> 3;
    const int groups = (cols + pad + 3) >> 2;
    const int g = e < 4 ? e : groups - 1 - (e - 4);
    const int x0 = 4 * g - pad;
    const bool mine = g >= 0 && g < groups && (e < 4 || g >= 4) && !(x0 >= 7 && x0 + 12 <= cols) && x0 < cols && x0 + 4 > 0;
    const int y0 = bi * a.band + (lane >> 3) * per, y1 = max(y0, min(min(a.rows, (bi + 1) * a.band), y0 + per));
    smooth_walk<MODE, R, false>(a, img, out, x0, y0, y1, mine && y1 > y0, false, x0 >= 0 && x0 + 4 <= cols);
  }
}

// 256-column chunks of a row, for any phase of the destination (the lanes' grid starts up to three pixels ahead of column 0)
static inline int smooth_chunks(int cols) { return (cols + 3 + 255) / 256; }
// output rows per wavefront: band + 2 r rows are read for band rows written, so long bands; shorter ones where the image alone would
// not fill the chip (about two rounds of 8 wavefronts per SIMD over 256 CUs)
static inline int smooth_band(int rows, int cols, int images) {
  int band = 32;
  while (band > 8 && (long long)((rows + band - 1) / band) * smooth_chunks(cols) * images < 16384) band >>= 1;
  return band;
}
// the stage on queue st.  Images, strides, size, mode, ksize, n, sides and active are the caller's (checked: smooth_mode_ok,
// smooth_size_ok); a.band and a.chunks are set here.
static hipError_t smooth_enqueue(hipStream_t st, SmoothArgs a) {
  a.chunks = smooth_chunks(a.cols);
  a.band = smooth_band(a.rows, a.cols, a.n * a.sides);
  const int waves = ((a.rows + a.band - 1) / a.band) * (a.chunks + 1);       // a band's chunks, and its border wavefront
  const dim3 grid((waves + 3) / 4, 1, a.n * a.sides);
  const int r = a.ksize / 2;
  if (a.mode == VS_SMOOTH_GAUSSIAN) {
    if (r == 1) hipLaunchKernelGGL((k_smooth<VS_SMOOTH_GAUSSIAN, 1>), grid, dim3(256), 0, st, a);
    else if (r == 2) hipLaunchKernelGGL((k_smooth<VS_SMOOTH_GAUSSIAN, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_smooth<VS_SMOOTH_GAUSSIAN, 3>), grid, dim3(256), 0, st, a);
  } else {
    if (r == 1) hipLaunchKernelGGL((k_smooth<VS_SMOOTH_MEDIAN, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_smooth<VS_SMOOTH_MEDIAN, 2>), grid, dim3(256), 0, st, a);
  }
  return hipGetLastError();
}
