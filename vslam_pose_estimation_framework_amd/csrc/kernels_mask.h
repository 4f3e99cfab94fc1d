// kernels_mask.h — detection masks: keep keypoints off masked pixels (gfx950).
//
// cv::Feature2D::detect(image, keypoints, mask) [recalled]: the detector runs on the whole image, non-maximum suppression included, and
// KeyPointsFilter::runByPixelsMask then drops every keypoint whose pixel reads 0 in the 8-bit mask.  k_fast_box leaves one corner bit per
// pixel in DevBuf::mask (rows x TX 64-bit words per image, bit = column mod 64) and k_emit derives keypoints, the row / cell CSR and the
// controller's counts from nothing but those words, so ANDing a packed keep-mask into the words between the two launches is that filter.
//
// Packed form (mask.py): TX = (cols + 63) / 64 little-endian words per row, bit b of word t = column 64 t + b, non-zero byte = keep, bits
// beyond cols 0.  `margin` m (0 .. 64) erodes the keep-mask by the (2m+1) x (2m+1) square; pixels outside the image count as kept.
//
//   k_mask_pack   u8 rows (any row stride, any byte phase) -> eroded packed words.  A workgroup owns VS_MASK_BR output rows x VS_MASK_CW
//                 words: it forms the raw words of its rows +- m and words +- 1 by wave ballots over 256 consecutive pixels (four per
//                 lane: 32-bit loads, the four ballots' bits put in pixel order by mask_gather4) into LDS, erodes every row horizontally on the 192-bit value (previous,
//                 own, next word) by window doubling, and ANDs the 2m+1 rows of every output word out of LDS.  A mask byte leaves HBM
//                 once per band (plus the halo rows, and the halo word on either side when m > 0).  One launch covers both sides and all
//                 streams (grid z = stream * sides + side).  With `corner` set it is the frame-mask path fused: the eroded word is ANDed
//                 with the static word and into the corner word, and the effective word is kept for vslam_get_detection_mask — one pass
//                 over the mask bytes, no intermediate buffer.
//   k_mask_apply  corner_word &= static_word, two words (16 B) per lane, the static words loaded once per VS_MASK_SB streams (or, with a
//                 stream stride, every stream's own words: the RGB-D frame masks' effective words).
//   k_map_valid   the validity of a remap map's output pixels (every tap of non-zero weight inside the raw image), packed and eroded by
//                 k_mask_pack's own tile (mask_pack_tile) with the map entries as its pixel source.
// A switched-off stream (DevBuf::active) is neither read nor written.  Integer logic only: bit-exact by construction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"

#define VS_MASK_MAX_MARGIN 64
#define VS_MASK_BR 32         // output rows per workgroup
#define VS_MASK_CW 10         // output words per workgroup and row (KITTI: 20 words = two workgroups)
#define VS_MASK_SB 8          // streams per workgroup of k_mask_apply
#define VS_MASK_INFLIGHT 4    // items (256 pixels each) a wave loads before it ballots the first

// ---- the horizontal erosion of one word (host and device: tests/cpp runs it against a scalar loop) ------------------------------------
struct MaskW3 { unsigned long long w[3]; };       // 192 columns, w[0] the lowest
// x >> k over the 192 bits, 1 <= k <= 128; ones enter at the top (columns nobody reads: see mask_erode_word)
__host__ __device__ inline MaskW3 mask_shr(const MaskW3& x, int k) {
  const int ws = k >> 6, bs = k & 63;
  const unsigned long long ones = ~0ull;
  const unsigned long long a = ws == 0 ? x.w[0] : ws == 1 ? x.w[1] : x.w[2];
  const unsigned long long b = ws == 0 ? x.w[1] : ws == 1 ? x.w[2] : ones;
  const unsigned long long c = ws == 0 ? x.w[2] : ones;
  MaskW3 r;
  if (bs == 0) { r.w[0] = a; r.w[1] = b; r.w[2] = c; }
  else {
    r.w[0] = (a >> bs) | (b << (64 - bs));
    r.w[1] = (b >> bs) | (c << (64 - bs));
    r.w[2] = (c >> bs) | (ones << (64 - bs));
  }
  return r;
}
// bit b of the result = AND of the columns b - m .. b + m of `own`, borrowing from the previous and the next word of the row.
// F_L(p) = AND of the L columns from p upwards, by doubling: F_1 = x, F_2k = F_k & (F_k >> k), F_L = F_a & (F_a >> (L - a)) with a the
// largest power of two <= L = 2m + 1; the result is F_L at the positions 64 - m .. 127 - m, whose windows end at column 127 + m <= 191.
__host__ __device__ inline unsigned long long mask_erode_word(unsigned long long prev, unsigned long long own, unsigned long long next, int m) {
  if (m == 0) return own;
  MaskW3 f = {{prev, own, next}};
  const int L = 2 * m + 1;
  int a = 1;
  while (2 * a <= L) {
    const MaskW3 s = mask_shr(f, a);
    for (int i = 0; i < 3; ++i) f.w[i] &= s.w[i];
    a *= 2;
  }
  if (L > a) {
    const MaskW3 s = mask_shr(f, L - a);
    for (int i = 0; i < 3; ++i) f.w[i] &= s.w[i];
  }
  return m == 64 ? f.w[0] : (f.w[0] >> (64 - m)) | (f.w[1] << m);
}
// Four ballots over lanes that hold four consecutive pixels each: bit l of b[e] = pixel 4 l + e of 256.  Word k of the four (pixels 64 k
// .. 64 k + 63) takes bit 4 i + e from bit 16 k + i of b[e]: sixteen bits of each ballot, spread to every fourth position.
__host__ __device__ inline unsigned long long mask_spread16(unsigned long long x) {
  x &= 0xffffull;
  x = (x | (x << 24)) & 0x000000ff000000ffull;
  x = (x | (x << 12)) & 0x000f000f000f000full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}
__host__ __device__ inline unsigned long long mask_gather4(unsigned long long b0, unsigned long long b1, unsigned long long b2, unsigned long long b3, int k) {
  const int sh = 16 * k;
  return mask_spread16(b0 >> sh) | (mask_spread16(b1 >> sh) << 1) | (mask_spread16(b2 >> sh) << 2) | (mask_spread16(b3 >> sh) << 3);
}
// the bits of word t whose column lies inside the image
__host__ __device__ inline unsigned long long mask_cols_word(int t, int cols) {
  const int left = cols - 64 * t;
  return left >= 64 ? ~0ull : left <= 0 ? 0ull : ((1ull << left) - 1ull);
}

struct MaskPackArgs {
  const uint8_t* src[2];      // masks [left/right]: stream s at src[side] + s * src_stream_stride; null (fused path only): the side is all-keep
  size_t src_stream_stride;
  int32_t src_row_stride;
  int32_t rows, cols, TX;     // TX = (cols + 63) / 64 words per row
  int32_t margin;
  int32_t n, sides;           // streams 0 .. n - 1, grid z = n * sides
  unsigned long long* dst;    // [n][sides][rows][TX]; fused: the effective words [n][2][rows][TX]
  const unsigned long long* stat[2];   // the static words [rows][TX] of each side, ANDed into what is stored and applied; null: none
  unsigned long long* corner; // fused: DevBuf::mask [n][corner_sides][rows][TX]; null: nothing is applied
  int32_t corner_sides;       // images per stream of `corner`: 2 (DevBuf::mask), whichever `sides` are packed
  uint32_t active[VS_MAX_STREAMS / 32];
};

// The pixel source of k_mask_pack: an 8-bit image.  load4: the keep bytes (non-zero = keep) of the pixels x .. x + 3 of `row`, x any
// multiple of four from -256 on; what it returns for a pixel outside the image (or with !row_ok) is overridden by the caller.
struct MaskSrcU8 {
  const uint8_t* src; int32_t row_stride;
  __device__ __forceinline__ uint32_t load4(int row, int x, bool row_ok, int cols) const {
    // one aligned 32-bit load when the row starts on a multiple of four bytes, two funnelled into one otherwise (a loaded word always
    // holds a byte of the row, so it lies inside the caller's allocation)
    const uint8_t* at = src + (size_t)(row_ok ? row : 0) * row_stride + x;
    const int sh = (int)((uintptr_t)at & 3u);
    const uint32_t* al = reinterpret_cast<const uint32_t*>(at - sh);
    // pixels x .. x + 3 - sh come from the first aligned word, x + 4 - sh .. x + 3 from the second
    const bool lo_ok = row_ok && x + 3 - sh >= 0 && x < cols;
    const bool hi_ok = row_ok && sh > 0 && x + 3 >= 0 && x + 4 - sh < cols;
    const uint32_t lo = lo_ok ? al[0] : 0u, hi = hi_ok ? al[1] : 0u;
    return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo;
  }
};

typedef unsigned long long (*MaskRawRows)[VS_MASK_CW + 2];
typedef unsigned long long (*MaskHorRows)[VS_MASK_CW];

// One workgroup's tile of image (s, side): pack `from` (have: there is a source, workgroup-uniform; else all-keep), erode, AND with the
// static words, apply and store.  Written once for every pixel source (k_mask_pack: 8-bit images, k_map_valid: remap map entries).
template <class Src>
__device__ __forceinline__ void mask_pack_tile(const MaskPackArgs& a, const Src& from, bool have, int s, int side, MaskRawRows raw, MaskHorRows hor) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = a.margin;
  const int t0 = blockIdx.x * VS_MASK_CW, r0 = blockIdx.y * VS_MASK_BR;
  const int cw = min(VS_MASK_CW, a.TX - t0), nout = min(VS_MASK_BR, a.rows - r0);
  const int nr = nout + 2 * m;                      // staged rows: r0 - m .. r0 + nout + m - 1
  if (have) {                                       // workgroup-uniform
    // raw words, four at a time: item (j, g) = row r0 - m + j, words tb + 4 g .. tb + 4 g + 3, where tb = t0 - 1 (raw[j][0]) when the
    // halo words matter (m > 0), else t0 (raw[j][1]).  Lane l takes the four pixels 64 (tb + 4 g) + 4 l .. + 3 of the 256 (Src::load4),
    // four ballots give the bits pixel-interleaved, and lanes 0 .. 3 put one word each in order (mask_gather4).  Outside the image
    // everything is kept.  VS_MASK_INFLIGHT items of a wave are loaded before the first ballot waits: the loop is bound by load latency
    // otherwise.
    const int tb = m > 0 ? t0 - 1 : t0, k0 = m > 0 ? 0 : 1, nk = m > 0 ? cw + 2 : cw;
    const int ng = (nk + 3) >> 2, items = nr * ng;
    for (int i0 = wave; i0 < items; i0 += 4 * VS_MASK_INFLIGHT) {     // wave-uniform: every lane takes part in the ballots
      uint32_t v[VS_MASK_INFLIGHT];
#pragma unroll
      for (int u = 0; u < VS_MASK_INFLIGHT; ++u) {
        const int i = i0 + 4 * u;
        const int j = i / ng, g = i - j * ng;
        const int row = r0 - m + j, x = 64 * (tb + 4 * g) + 4 * lane;
        const bool row_ok = i < items && row >= 0 && row < a.rows;
        uint32_t px = from.load4(row, x, row_ok, a.cols);
        // a pixel outside the image (or the row) counts as kept
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (!(row_ok && x + e >= 0 && x + e < a.cols)) px |= 1u << (8 * e);
        v[u] = px;
      }
#pragma unroll
      for (int u = 0; u < VS_MASK_INFLIGHT; ++u) {
        const int i = i0 + 4 * u;
        const unsigned long long b0 = __ballot((v[u] & 0xffu) != 0), b1 = __ballot((v[u] & 0xff00u) != 0);
        const unsigned long long b2 = __ballot((v[u] & 0xff0000u) != 0), b3 = __ballot((v[u] & 0xff000000u) != 0);
        const int j = i / ng, g = i - j * ng;
        if (i < items && lane < 4 && 4 * g + lane < nk) raw[j][k0 + 4 * g + lane] = mask_gather4(b0, b1, b2, b3, lane);
      }
    }
    __syncthreads();
    for (int i = tid; i < nr * cw; i += 256) {
      const int j = i / cw, k = i - j * cw;
      hor[j][k] = mask_erode_word(raw[j][k], raw[j][k + 1], raw[j][k + 2], m);
    }
    __syncthreads();
  }
  for (int i = tid; i < nout * cw; i += 256) {
    const int r = i / cw, k = i - r * cw;
    unsigned long long acc = ~0ull;
    if (have)
      for (int j = r; j <= r + 2 * m; ++j) acc &= hor[j][k];
    const int row = r0 + r, t = t0 + k;
    acc &= mask_cols_word(t, a.cols);
    if (a.stat[side]) acc &= a.stat[side][(size_t)row * a.TX + t];
    // the corner words lie [n][corner_sides][rows][TX]: DevBuf::mask keeps two images per stream whichever sides are in use
    if (a.corner) a.corner[(((size_t)s * a.corner_sides + side) * a.rows + row) * a.TX + t] &= acc;
    a.dst[(((size_t)s * a.sides + side) * a.rows + row) * a.TX + t] = acc;
  }
}

__global__ __launch_bounds__(256) void k_mask_pack(MaskPackArgs a) {
  __shared__ unsigned long long raw[VS_MASK_BR + 2 * VS_MASK_MAX_MARGIN][VS_MASK_CW + 2];
  __shared__ unsigned long long hor[VS_MASK_BR + 2 * VS_MASK_MAX_MARGIN][VS_MASK_CW];
  const int s = (int)blockIdx.z / a.sides, side = (int)blockIdx.z - s * a.sides;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  const uint8_t* src = a.src[side];
  const MaskSrcU8 from{src ? src + (size_t)s * a.src_stream_stride : nullptr, a.src_row_stride};
  mask_pack_tile(a, from, src != nullptr, s, side, raw, hor);
}

// ---- validity of a remap map's output pixels (kernels_rectify.h: BORDER_CONSTANT fills every tap outside the raw image with 0) -------
// A map entry (x0, y0), ax = a & 31, ay = (a >> 5) & 31 is valid iff every tap of non-zero weight lies inside the raw image:
//   x0 >= 0 and x0 + (ax > 0) <= raw_cols - 1 and y0 >= 0 and y0 + (ay > 0) <= raw_rows - 1.
// k_map_valid packs that bit per entry and erodes it: k_mask_pack's tile with the map as its pixel source.  The loads are k_rectify's: one
// lane takes four consecutive entries (16 B of map_xy, 8 B of map_a; rows padded to map_stride, a multiple of four, so that a load that
// starts inside the image ends inside the row).  The padding entries are outside the image: they erode as kept and never become bits
// (mask_cols_word).  Grid (word groups, row bands, sides); once per setter call, not per frame.
struct MapValidArgs {
  const int16_t* map_xy[2];   // [rows][map_stride][2]
  const uint16_t* map_a[2];   // [rows][map_stride]
  int32_t map_stride, raw_rows, raw_cols;
  int32_t rows, cols, TX, margin, sides;
  unsigned long long* dst;    // [sides][rows][TX]
};
struct MaskSrcMap {
  const int16_t* xy; const uint16_t* fa; int32_t map_stride, raw_rows, raw_cols;
  __device__ __forceinline__ uint32_t load4(int row, int x, bool row_ok, int cols) const {
    if (!(row_ok && x >= 0 && x < cols)) return 0u;
    const size_t m = (size_t)row * map_stride + x;
    const int4 q = *reinterpret_cast<const int4*>(xy + 2 * m);
    const uint2 fr = *reinterpret_cast<const uint2*>(fa + m);
    const int xyw[4] = {q.x, q.y, q.z, q.w};
    const uint32_t fw[4] = {fr.x & 0xffffu, fr.x >> 16, fr.y & 0xffffu, fr.y >> 16};
    uint32_t px = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x0 = (int)(int16_t)(xyw[k] & 0xffff), y0 = xyw[k] >> 16;      // as k_rectify unpacks them
      const int ax = (int)(fw[k] & 31u), ay = (int)((fw[k] >> 5) & 31u);
      const bool ok = x0 >= 0 && x0 + (ax > 0) <= raw_cols - 1 && y0 >= 0 && y0 + (ay > 0) <= raw_rows - 1;
      px |= (ok ? 1u : 0u) << (8 * k);
    }
    return px;
  }
};
__global__ __launch_bounds__(256) void k_map_valid(MapValidArgs v) {
  __shared__ unsigned long long raw[VS_MASK_BR + 2 * VS_MASK_MAX_MARGIN][VS_MASK_CW + 2];
  __shared__ unsigned long long hor[VS_MASK_BR + 2 * VS_MASK_MAX_MARGIN][VS_MASK_CW];
  const int side = blockIdx.z;
  MaskPackArgs a{};
  a.rows = v.rows; a.cols = v.cols; a.TX = v.TX; a.margin = v.margin; a.n = 1; a.sides = v.sides; a.dst = v.dst;
  const MaskSrcMap from{v.map_xy[side], v.map_a[side], v.map_stride, v.raw_rows, v.raw_cols};
  mask_pack_tile(a, from, true, 0, side, raw, hor);
}

struct MaskApplyArgs {
  const unsigned long long* stat[2];   // static words [nw] of each side, null: the side is unmasked
  size_t stat_stream_stride;           // words between the streams' own words [n][nw] (one side); 0: every stream shares stat[side]
  unsigned long long* corner;          // DevBuf::mask: image (s, side) at corner + (s * 2 + side) * nw
  int32_t nw;                          // rows * TX
  int32_t n, sides;                    // streams 0 .. n - 1; sides 1: the left image only (RGB-D)
  uint32_t active[VS_MAX_STREAMS / 32];
};

// grid (word pairs / 256, sides, stream groups)
__global__ __launch_bounds__(256) void k_mask_apply(MaskApplyArgs a) {
  const int side = blockIdx.y;
  const unsigned long long* stat = a.stat[side];
  if (!stat) return;
  const int i = 2 * (blockIdx.x * 256 + threadIdx.x);
  if (i >= a.nw) return;
  const bool pair = !(a.nw & 1);       // every image starts 16-byte aligned (hipMalloc'ed bases, an even word count per image)
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  u64x2 sw;
  if (pair) sw = *reinterpret_cast<const u64x2*>(stat + i);
  else { sw.x = stat[i]; sw.y = i + 1 < a.nw ? stat[i + 1] : ~0ull; }
  const int j0 = blockIdx.z * VS_MASK_SB, j1 = min(a.n, j0 + VS_MASK_SB);
  for (int s = j0; s < j1; ++s) {
    if (!((a.active[s >> 5] >> (s & 31)) & 1u)) continue;
    if (a.stat_stream_stride) {        // the stream's own words (uniform over the launch)
      const unsigned long long* own = stat + (size_t)s * a.stat_stream_stride + i;
      if (pair) sw = *reinterpret_cast<const u64x2*>(own);
      else { sw.x = own[0]; sw.y = i + 1 < a.nw ? own[1] : ~0ull; }
    }
    unsigned long long* cw = a.corner + ((size_t)s * 2 + side) * a.nw + i;
    if (pair) {
      u64x2 v = *reinterpret_cast<u64x2*>(cw);
      v.x &= sw.x; v.y &= sw.y;
      *reinterpret_cast<u64x2*>(cw) = v;
    } else {
      cw[0] &= sw.x;
      if (i + 1 < a.nw) cw[1] &= sw.y;
    }
  }
}
