// kernels_clahe.h — contrast-limited adaptive histogram equalisation of 8-bit images ahead of the detector (gfx950).
//
// cv::createCLAHE(clipLimit, Size(tilesX, tilesY))->apply on one 8-bit image [recalled]:
//   extension  if cols % tilesX == 0 && rows % tilesY == 0 the image is used as it is; otherwise it grows at the bottom by tilesY - rows % tilesY
//              rows AND at the right by tilesX - cols % tilesX columns with BORDER_REFLECT_101 (index i >= n reads 2 (n - 1) - i): a dimension
//              that divides still gets a full tilesY (tilesX) extra lines when the other one does not.
//              tw = ext_cols / tilesX, th = ext_rows / tilesY, area = tw * th
//   clip       clipLimit > 0 ? max((int)(clipLimit * area / 256), 1) : 0       double arithmetic on the host; the kernels receive the integer
//   per tile   h[256] = counts; with clip > 0: clipped = sum of h[k] - clip over the bins above clip, those bins = clip, batch = clipped / 256,
//              residual = clipped - 256 * batch, every bin += batch, and with step = max(256 / residual, 1) bin k gets one more exactly when
//              k % step == 0 && k / step < residual (the closed form of the reference's loop: always `residual` bins)
//   table      lut[k] = clamp(rint(float(h[0] + .. + h[k]) * (float(255) / float(area))), 0, 255), ties to even
//   per pixel  txf = float(x) * (1.f / float(tw)) - 0.5f, tx1 = floor(txf), tx2 = tx1 + 1, xa = txf - float(tx1), xa1 = 1.f - xa, then
//              tx1 = max(tx1, 0), tx2 = min(tx2, tilesX - 1); the same in y;
//              res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya
//              dst = clamp(rint(res), 0, 255)
// Every float operation is one of __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn / rintf / floorf, everything else is integer, and
// rows * cols <= 2^24 keeps every count exact in float: the result is bit-exact by construction.
//
// Two kernels, y = sides, z = streams; a switched-off stream (DevBuf::active) is neither read nor written.
//   k_clahe_lut    x = tile.  Sixteen lanes per tile row: the part of the row inside the image is one contiguous run of the source row
//                  (a reflected ROW is a whole source row at another index), counted 16 B per lane over its aligned interior with
//                  eq_count16's run merging into the lane's counter copy, byte lanes for its head and tail; the columns that come from the
//                  reflected border are byte lanes.  Then one thread per bin: the copies summed, the clip, a workgroup sum of the excess,
//                  the closed-form redistribution, the 256-wide inclusive scan, the two float operations, one byte to
//                  luts[stream][side][tile][256].  No global atomics, nothing to zero: every entry has one writer.
//   k_clahe_apply  x = (tilesY + 1) row segments x `sub` parts.  Segment g holds the rows whose floor(tyf) is g - 1, so every row of it blends
//                  tile rows max(g - 1, 0) and min(g, tilesY - 1): at most two, 2 * tilesX * 256 B <= 16 KB of LDS.  A thread owns 16 columns
//                  (its tx1 / tx2 / xa computed once, in registers) and walks its rows: 16 B in where the source is aligned, 16 B out
//                  where the destination is, bytes otherwise; the columns ahead of the first 16-B boundary of row 0 and behind the last
//                  whole 16 go by byte lanes.  In place when dst == src: a pixel is read and written by one thread, read first.
//
// Bounds, for every shape clahe_geometry() accepts (1 <= tilesX, tilesY <= 32, cols > tilesX, rows > tilesY, rows * cols <= 2^24):
//   reflected indices   an extended index i lies in [n, n + tiles - 1], so 2 (n - 1) - i lies in [n - 1 - tiles, n - 2], inside [0, n) because
//                       n > tiles.  The kernels clamp the result into [0, n - 1] as well, which changes nothing for accepted shapes.
//   source reads        k_clahe_lut reads columns [x0, x0 + len) with len = clamp(cols - x0, 0, tw), and reflected columns as above;
//                       k_clahe_apply reads and writes columns [0, cols) only, vectors over [h0, h0 + 16 nvec) with h0 + 16 nvec <= cols.
//                       Padding bytes beyond cols are never read.
//   tile indices        tx1, tx2, and the tile rows of a segment, are clamped into [0, tiles - 1] on both sides before they index a table.
//   segments            row_start[] is non-decreasing with row_start[0] = 0 and row_start[tilesY + 1] = rows (clahe_geometry builds it with
//                       the float arithmetic of the definition), so every row belongs to exactly one segment and none lies outside
//                       [0, rows).  Were host and device floats to disagree, a row would blend with another segment's weights: a wrong
//                       value, never a wrong address.
//   tables              luts holds n * sides * tilesX * tilesY * 256 bytes; a tile row of tables is tilesX * 256 contiguous bytes at a
//                       multiple of 256 from a base that is 16-B aligned (checked by clahe_enqueue).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "dev_types.h"
#include "kernels_equalize.h"     // eq_count16, VS_EQ_COPIES, VS_EQ_MAX_PIXELS

#define VS_CLAHE_MAX_TILES 32

struct ClaheArgs {
  const uint8_t* src[2];      // images [left/right]: stream s at src[side] + s * src_stream_stride, any alignment
  size_t src_stream_stride;
  int32_t src_row_stride;
  uint8_t* dst[2];            // processed images (may be src: in place); null for the tables alone
  size_t dst_stream_stride;
  int32_t dst_row_stride;
  uint8_t* luts;              // [n][sides][tilesY][tilesX][256]
  int32_t rows, cols;
  int32_t n, sides;           // grid z = n, grid y = sides
  int32_t tiles_x, tiles_y, tw, th, clip;
  float inv_tw, inv_th;       // 1.f / float(tw), 1.f / float(th)
  int32_t sub;                // workgroups per row segment of k_clahe_apply
  int32_t row_start[VS_CLAHE_MAX_TILES + 2];   // segment g = rows [row_start[g], row_start[g + 1]), g = 0 .. tilesY
  uint32_t active[VS_MAX_STREAMS / 32];
};

__device__ __forceinline__ int clahe_reflect(int i, int n) { return min(max(i < n ? i : 2 * (n - 1) - i, 0), n - 1); }

__global__ __launch_bounds__(256) void k_clahe_lut(ClaheArgs a) {
  __shared__ uint32_t cnt[256 * VS_EQ_COPIES];
  __shared__ uint32_t scan[256];
  __shared__ uint32_t part[4];
  const int s = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  for (int i = tid; i < 256 * VS_EQ_COPIES; i += 256) cnt[i] = 0;
  __syncthreads();
  const int tile = blockIdx.x, tj = tile / a.tiles_x, ti = tile - tj * a.tiles_x;
  const int x0 = ti * a.tw, y0 = tj * a.th;
  const int len = min(max(a.cols - x0, 0), a.tw);                        // columns of the tile inside the image: [x0, x0 + len)
  const int l16 = tid & 15, copy = tid & (VS_EQ_COPIES - 1);
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  for (int r = tid >> 4; r < a.th; r += 16) {
    const uint8_t* row = img + (size_t)clahe_reflect(y0 + r, a.rows) * a.src_row_stride;
    const uint8_t* p = row + x0;
    const int head = min(len, (int)((16u - (uint32_t)((uintptr_t)p & 15u)) & 15u));
    if (l16 < head) atomicAdd(&cnt[p[l16] * VS_EQ_COPIES + copy], 1u);
    const int nvec = (len - head) >> 4;
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    for (int v = l16; v < nvec; v += 16) eq_count16(cnt, pv[v], copy);
    const int t0 = head + nvec * 16;                                     // fewer than 16 bytes are left
    if (t0 + l16 < len) atomicAdd(&cnt[p[t0 + l16] * VS_EQ_COPIES + copy], 1u);
    for (int x = x0 + len + l16; x < x0 + a.tw; x += 16)                 // the reflected border: x >= cols
      atomicAdd(&cnt[row[clahe_reflect(x, a.cols)] * VS_EQ_COPIES + copy], 1u);
  }
  __syncthreads();
  uint32_t h = 0;
#pragma unroll
  for (int j = 0; j < VS_EQ_COPIES; ++j) h += cnt[tid * VS_EQ_COPIES + ((j + tid) & (VS_EQ_COPIES - 1))];
  if (a.clip > 0) {
    const uint32_t clip = (uint32_t)a.clip;
    uint32_t ex = h > clip ? h - clip : 0u;
    h = min(h, clip);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) ex += __shfl_down(ex, d, 64);
    if ((tid & 63) == 0) part[tid >> 6] = ex;
    __syncthreads();
    const uint32_t clipped = part[0] + part[1] + part[2] + part[3];
    const uint32_t batch = clipped >> 8, residual = clipped & 255u;
    const uint32_t step = residual ? max(256u / residual, 1u) : 1u;
    h += batch + ((uint32_t)tid % step == 0 && (uint32_t)tid / step < residual ? 1u : 0u);
  }
  scan[tid] = h;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                                    // inclusive scan of the counts
    const uint32_t v = tid >= d ? scan[tid - d] : 0u;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const float scale = __fdiv_rn(255.f, (float)(a.tw * a.th));
  const int m = (int)rintf(__fmul_rn((float)scan[tid], scale));
  a.luts[(((size_t)s * a.sides + side) * (size_t)(a.tiles_x * a.tiles_y) + tile) * 256 + tid] = (uint8_t)min(max(m, 0), 255);
}

// column x: its two table offsets (tx1 * 256 in the low half, tx2 * 256 in the high half) and the weight of the second one
__device__ __forceinline__ void clahe_column(const ClaheArgs& a, int x, uint32_t& off, float& xa) {
  const float txf = __fsub_rn(__fmul_rn((float)x, a.inv_tw), 0.5f);
  const float f = floorf(txf);
  xa = __fsub_rn(txf, f);
  const int t1 = (int)f;
  const int tx1 = min(max(t1, 0), a.tiles_x - 1), tx2 = max(min(t1 + 1, a.tiles_x - 1), 0);
  off = (uint32_t)(tx1 << 8) | ((uint32_t)(tx2 << 8) << 16);
}
__device__ __forceinline__ uint32_t clahe_pixel(const uint8_t* t1, const uint8_t* t2, uint32_t v, uint32_t off, float xa, float ya, float ya1) {
  const uint32_t o1 = (off & 0xffffu) + v, o2 = (off >> 16) + v;
  const float xa1 = __fsub_rn(1.f, xa);
  const float top = __fadd_rn(__fmul_rn((float)t1[o1], xa1), __fmul_rn((float)t1[o2], xa));
  const float bot = __fadd_rn(__fmul_rn((float)t2[o1], xa1), __fmul_rn((float)t2[o2], xa));
  const int m = (int)rintf(__fadd_rn(__fmul_rn(top, ya1), __fmul_rn(bot, ya)));
  return (uint32_t)min(max(m, 0), 255);
}

__global__ __launch_bounds__(256) void k_clahe_apply(ClaheArgs a) {
  __shared__ uint4 tab4[2 * VS_CLAHE_MAX_TILES * 16];                    // two tile rows of tables, 256 B each
  const int s = blockIdx.z, side = blockIdx.y, tid = threadIdx.x;
  if (!((a.active[s >> 5] >> (s & 31)) & 1u)) return;
  const int g = (int)blockIdx.x / a.sub, part = (int)blockIdx.x - g * a.sub;
  const int seg0 = a.row_start[g], seg1 = a.row_start[g + 1];
  const int per = (seg1 - seg0 + a.sub - 1) / a.sub;
  const int r0 = seg0 + part * per, r1 = min(seg1, r0 + per);
  if (r0 >= r1) return;
  const int ty1 = min(max(g - 1, 0), a.tiles_y - 1), ty2 = max(min(g, a.tiles_y - 1), 0);
  const int row_u4 = a.tiles_x * 16;                                     // uint4 per tile row of tables
  const uint4* lut4 = reinterpret_cast<const uint4*>(a.luts + ((size_t)s * a.sides + side) * (size_t)(a.tiles_x * a.tiles_y) * 256);
  for (int i = tid; i < row_u4; i += 256) tab4[i] = lut4[(size_t)ty1 * row_u4 + i];
  if (ty2 != ty1) for (int i = tid; i < row_u4; i += 256) tab4[row_u4 + i] = lut4[(size_t)ty2 * row_u4 + i];
  __syncthreads();
  const uint8_t* t1 = reinterpret_cast<const uint8_t*>(tab4);
  const uint8_t* t2 = t1 + (ty2 != ty1 ? a.tiles_x * 256 : 0);
  const uint8_t* img = a.src[side] + (size_t)s * a.src_stream_stride;
  uint8_t* out = a.dst[side] + (size_t)s * a.dst_stream_stride;
  // the 16-column chunks start where row 0 of the destination meets a 16-B boundary; rows whose stride keeps that phase store 16 B
  const int h0 = min(a.cols, (int)((16u - (uint32_t)((uintptr_t)out & 15u)) & 15u));
  const int nvec = (a.cols - h0) >> 4;
  const int cw = min(max(nvec, 1), 256), nph = 256 / cw, ph = tid / cw;
  if (ph < nph) {
    for (int v = tid - ph * cw; v < nvec; v += cw) {
      const int c0 = h0 + 16 * v;
      uint32_t off[16]; float xa[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) clahe_column(a, c0 + k, off[k], xa[k]);
      for (int r = r0 + ph; r < r1; r += nph) {
        const float tyf = __fsub_rn(__fmul_rn((float)r, a.inv_th), 0.5f);
        const float ya = __fsub_rn(tyf, floorf(tyf)), ya1 = __fsub_rn(1.f, ya);
        const uint8_t* p = img + (size_t)r * a.src_row_stride + c0;
        uint8_t* o = out + (size_t)r * a.dst_row_stride + c0;
        uint32_t w[4];
        if (((uintptr_t)p & 15u) == 0) {
          const uint4 q = *reinterpret_cast<const uint4*>(p);
          w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        }
        uint32_t m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k)
          m[k >> 2] |= clahe_pixel(t1, t2, (w[k >> 2] >> (8 * (k & 3))) & 255u, off[k], xa[k], ya, ya1) << (8 * (k & 3));
        if (((uintptr_t)o & 15u) == 0) *reinterpret_cast<uint4*>(o) = make_uint4(m[0], m[1], m[2], m[3]);
        else {
#pragma unroll
          for (int k = 0; k < 16; ++k) o[k] = (uint8_t)(m[k >> 2] >> (8 * (k & 3)));
        }
      }
    }
  }
  // the columns ahead of the first chunk and behind the last one: fewer than 32 in all, one lane each, eight rows at a time
  const int t0 = h0 + 16 * nvec, nedge = h0 + (a.cols - t0), e = tid & 31;
  if (e < nedge) {
    const int x = e < h0 ? e : t0 + (e - h0);
    uint32_t off; float xa;
    clahe_column(a, x, off, xa);
    for (int r = r0 + (tid >> 5); r < r1; r += 8) {
      const float tyf = __fsub_rn(__fmul_rn((float)r, a.inv_th), 0.5f);
      const float ya = __fsub_rn(tyf, floorf(tyf)), ya1 = __fsub_rn(1.f, ya);
      const uint32_t v = img[(size_t)r * a.src_row_stride + x];
      out[(size_t)r * a.dst_row_stride + x] = (uint8_t)clahe_pixel(t1, t2, v, off, xa, ya, ya1);
    }
  }
}

// floor(float(y) * inv - 0.5f) with the arithmetic of the definition (the library is built without contraction)
static int clahe_floor(int y, float inv) { return (int)std::floor((float)y * inv - 0.5f); }
// What the entries check and the kernels need of one (rows, cols, clipLimit, tiles) combination: false with a reason for what is refused.
// Fills the tile sizes, the clip, the reciprocals and the row segments of a; images, tables, n, sides and active stay the caller's.
static bool clahe_geometry(int rows, int cols, double clip_limit, int tiles_x, int tiles_y, ClaheArgs& a, const char** why) {
  if (tiles_x < 1 || tiles_x > VS_CLAHE_MAX_TILES || tiles_y < 1 || tiles_y > VS_CLAHE_MAX_TILES) { *why = "tiles outside 1 .. 32"; return false; }
  if (cols <= tiles_x || rows <= tiles_y) { *why = "the image must be larger than the tile grid"; return false; }
  if ((size_t)rows * (size_t)cols > (size_t)VS_EQ_MAX_PIXELS) { *why = "more than 2^24 pixels"; return false; }
  if (!std::isfinite(clip_limit)) { *why = "clip_limit is not finite"; return false; }
  const bool whole = cols % tiles_x == 0 && rows % tiles_y == 0;
  const int ext_rows = whole ? rows : rows + tiles_y - rows % tiles_y, ext_cols = whole ? cols : cols + tiles_x - cols % tiles_x;
  a.rows = rows; a.cols = cols; a.tiles_x = tiles_x; a.tiles_y = tiles_y;
  a.tw = ext_cols / tiles_x; a.th = ext_rows / tiles_y;
  const double area = (double)a.tw * a.th;
  // no bin holds more than area, so a larger clip is the same as area (and stays inside int)
  a.clip = clip_limit > 0 ? (int)std::max(std::min(clip_limit * area / 256.0, area), 1.0) : 0;
  a.inv_tw = 1.f / (float)a.tw; a.inv_th = 1.f / (float)a.th;
  // row_start[g]: the first row whose floor(tyf) is at least g - 1; the floor is non-decreasing in the row, so an estimate is walked
  // to the boundary
  a.row_start[0] = 0;
  for (int g = 1; g <= tiles_y; ++g) {
    int y = std::min(rows, std::max(a.row_start[g - 1], (int)(((double)g - 0.5) * a.th)));
    while (y > a.row_start[g - 1] && clahe_floor(y - 1, a.inv_th) >= g - 1) --y;
    while (y < rows && clahe_floor(y, a.inv_th) < g - 1) ++y;
    a.row_start[g] = y;
  }
  for (int g = tiles_y + 1; g < VS_CLAHE_MAX_TILES + 2; ++g) a.row_start[g] = rows;
  return true;
}
// the tables, and (with a destination) the mapping, on queue st.  Everything but a.sub is the caller's (clahe_geometry + images, luts, n,
// sides, active).
static hipError_t clahe_enqueue(hipStream_t st, ClaheArgs a) {
  if ((uintptr_t)a.luts & 15u) return hipErrorInvalidValue;
  const int images = std::max(a.n * a.sides, 1);
  a.sub = std::max(1, std::min((a.th + 7) / 8, 2048 / (images * (a.tiles_y + 1))));
  hipLaunchKernelGGL(k_clahe_lut, dim3(a.tiles_x * a.tiles_y, a.sides, a.n), dim3(256), 0, st, a);
  if (a.dst[0]) hipLaunchKernelGGL(k_clahe_apply, dim3((a.tiles_y + 1) * a.sub, a.sides, a.n), dim3(256), 0, st, a);
  return hipSuccess;
}
