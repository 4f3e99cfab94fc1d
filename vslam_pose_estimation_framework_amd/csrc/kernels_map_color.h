// kernels_map_color.h — the colour of every landmark of the device map (opt-in, gfx950): vslam_enable_map_colors,
// vslam_rgbd_enable_map_colors, vslam_sample_color_u8.
//
// Definition (color.sample_rgb is the numpy restatement): a landmark's colour is the colour of its keypoint's pixel in the frame's colour
// image — the LEFT image of a stereo pair — at the landmark's last update, stored as (r, g, b, 0) whatever the input's channel order.
//   direct:        the pixel (x, y) of the colour image; outside the image: (0, 0, 0).
//   through a map: the keypoint lies in the rectified / undistorted image, the colour image is the raw one.  Each colour plane is remapped
//                  with k_rectify's arithmetic (kernels_rectify.h) at destination pixel (y, x): map_xy = (x0, y0), map_a = ay * 32 + ax,
//                  taps (y0, x0) .. (y0 + 1, x0 + 1), weights (32 - ax)(32 - ay) .. ax ay, (sum + 512) >> 10, a tap outside the raw image
//                  counts as 0 and is never read; a pixel outside the map: (0, 0, 0).
//   float pixels:  (RgbdList::xy: recovered points sit at sub-pixel projections) rounded half to even in float32 and clamped to the pixel
//                  grid (the map's when there is one) first.
// Integer arithmetic only: bit-exact by construction.
//
// k_map_color runs directly behind k_map_commit (and k_obs_append) on the frame queue and writes the colour of every point of the finished
// frame that carries an id (ids_cur[i] >= 0: the set for which k_map_commit writes last_frame).  k_rgbd_map_color runs directly behind
// k_rgbd_map_commit on the frame's one queue and writes the colour exactly when that kernel writes the entry's row (RGBD_F_LM on the
// current list and an id), once per frame under the commit's rule with a per-sequence mark of its own (RgbdMapColor::colored: the commit
// has already moved RgbdMap::committed when this kernel runs).
//
// Shape: one 1024-thread workgroup per stream, the frame's points in chunks of 1024, like the commit kernels: a chain of dependent loads
// per point (id -> keypoint -> map entry -> taps) and one 32-bit vector store.  No LDS, no atomics; two points of a frame never share an
// id.  The taps are byte gathers (3 per tap: an interleaved pixel has no alignment), 12 through a map; the points of a frame are spread
// over the image, so every tap is a cache line of its own and the kernel is bound by the latency of that chain, not by bytes.
// Nothing here is read by the tracker.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"
#include "kernels_frame.h"
#include "kernels_map.h"
#include "kernels_rgbd_map.h"
#include "downscale_geometry.h"   // ds_round: a tap's block average while the frames are downscaled

#define VS_MAP_COLOR_WG 1024

// where colours come from: one colour image per stream (img + stream * stream_stride), optionally behind one remap map pair shared by all streams
struct ColorSrc {
  const uint8_t* img;
  size_t stream_stride;
  int32_t row_stride, rows, cols;     // bytes per row; pixels of the grid the taps are addressed in (the reduced size while factor > 1)
  int32_t format;                     // VSLAM_PIXEL_BGR8 .. VSLAM_PIXEL_RGBA8
  const int16_t* map_xy;              // [map_rows][map_stride][2], null: direct
  const uint16_t* map_a;              // [map_rows][map_stride], values < 1024
  int32_t map_stride, map_rows, map_cols;
  int32_t factor;                     // > 1: img is the full-size image, a tap is the rounded average of its factor x factor block
};

// the three colour bytes of pixel (x, y) in file order, byte k in bits 8k .. 8k + 7; 0 outside the image (nothing is read then)
__device__ __forceinline__ uint32_t color_tap(const uint8_t* __restrict__ img, const ColorSrc& s, int ch, int x, int y) {
  if ((unsigned)x >= (unsigned)s.cols || (unsigned)y >= (unsigned)s.rows) return 0u;
  if (s.factor > 1) {               // the downscale stage's arithmetic (kernels_downscale.h), per channel, on the full-size image
    const int f = s.factor;
    const uint8_t* p = img + (size_t)y * f * (size_t)s.row_stride + (size_t)x * f * ch;
    uint32_t sum[3] = {0u, 0u, 0u};
    for (int k = 0; k < f; ++k)
      for (int j = 0; j < f; ++j) {
        const uint8_t* q = p + (size_t)k * (size_t)s.row_stride + (size_t)j * ch;
        sum[0] += q[0]; sum[1] += q[1]; sum[2] += q[2];
      }
    return ds_round(sum[0], f) | (ds_round(sum[1], f) << 8) | (ds_round(sum[2], f) << 16);
  }
  const uint8_t* p = img + (size_t)y * (size_t)s.row_stride + (size_t)x * ch;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}
// (r, g, b, 0) of pixel (x, y) of the pixel grid (the map's when there is one)
__device__ __forceinline__ uint32_t color_sample(const uint8_t* __restrict__ img, const ColorSrc& s, int x, int y) {
  const int ch = s.format <= 2 ? 3 : 4;
  uint32_t v;
  if (!s.map_xy) v = color_tap(img, s, ch, x, y);
  else {
    if ((unsigned)x >= (unsigned)s.map_cols || (unsigned)y >= (unsigned)s.map_rows) return 0u;
    const size_t m = (size_t)y * s.map_stride + x;
    const int xy = *reinterpret_cast<const int*>(s.map_xy + 2 * m);      // little endian: x in the low half, y in the high half
    const int x0 = (int)(int16_t)(xy & 0xffff), y0 = xy >> 16;           // arithmetic shift keeps the sign
    const int fa = s.map_a[m];
    const int ax = fa & 31, ay = (fa >> 5) & 31;
    const uint32_t p00 = color_tap(img, s, ch, x0, y0), p01 = color_tap(img, s, ch, x0 + 1, y0);
    const uint32_t p10 = color_tap(img, s, ch, x0, y0 + 1), p11 = color_tap(img, s, ch, x0 + 1, y0 + 1);
    const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
    v = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int sh = 8 * k;
      const int sum = w00 * (int)((p00 >> sh) & 255u) + w01 * (int)((p01 >> sh) & 255u) + w10 * (int)((p10 >> sh) & 255u) + w11 * (int)((p11 >> sh) & 255u);
      v |= (uint32_t)((sum + 512) >> 10) << sh;
    }
  }
  // file order -> r, g, b: BGR8 (1) and BGRA8 (3) swap bytes 0 and 2
  return (s.format & 1) ? ((v & 0x00ff00u) | ((v & 0xffu) << 16) | ((v >> 16) & 0xffu)) : v;
}

// ---- stereo: behind k_map_commit --------------------------------------------------------------------------------------
__global__ __launch_bounds__(VS_MAP_COLOR_WG) void k_map_color(const DevCfg c, const DevBuf b, const DevMap m, const ColorSrc src, uint32_t* __restrict__ rgb) {
  const int s = b.s0 + (int)blockIdx.x, tid = threadIdx.x;
  if (!vs_active(b, s)) return;
  const StreamState& st = b.st[s];
  const int f = st.frame_count - 1, pb = st.cur;     // the frame k_map_commit has just labelled and its point buffer
  if (f < 0) return;
  const PtView cv = pts_of(c, b, s, pb);
  const int n = min(*cv.n, c.MAXP);
  const int32_t* ids_cur = m.ids + ((size_t)pb * m.B + s) * c.MAXP;
  const uint8_t* img = src.img + (size_t)s * src.stream_stride;
  uint32_t* out = rgb + (size_t)s * m.cap;
  for (int i = tid; i < n; i += VS_MAP_COLOR_WG) {
    const int id = ids_cur[i];
    if (id < 0 || id >= m.cap) continue;
    const int xy = *reinterpret_cast<const int*>(cv.kp + 4 * (size_t)i);      // (xL, yL)
    out[id] = color_sample(img, src, (int)(int16_t)(xy & 0xffff), xy >> 16);
  }
}

// ---- RGB-D: behind k_rgbd_map_commit ----------------------------------------------------------------------------------
struct RgbdMapColor {
  uint32_t* rgb;       // [B][cap]  (r, g, b, 0)
  int32_t* colored;    // [B]       RgbdState::frame_count after the last frame this kernel served
};

__global__ __launch_bounds__(VS_MAP_COLOR_WG) void k_rgbd_map_color(const RgbdBuf all, const RgbdMap m, const ColorSrc src, const RgbdMapColor mc) {
  const int sq = blockIdx.x, tid = threadIdx.x;
  const RgbdBuf r = rgbd_stream(all, sq);
  const RgbdState& st = *r.st;
  const int fc = st.frame_count;
  const bool skip = !st.tail_done || mc.colored[sq] == fc;
  __syncthreads();                                         // every lane has read the mark before lane 0 may move it
  if (skip) return;
  const int f = fc - 1;                                    // the frame k_rgbd_map_commit has just labelled
  const RgbdList cur = rgbd_pick(r, (f & 1) != 0);
  const int np = min(st.last_points, r.MAXP);
  const int32_t* ids_cur = m.ids + ((size_t)(f & 1) * m.B + sq) * r.MAXP;
  const uint8_t* img = src.img + (size_t)sq * src.stream_stride;
  uint32_t* out = mc.rgb + (size_t)sq * m.cap;
  const int gw = src.map_xy ? src.map_cols : src.cols, gh = src.map_xy ? src.map_rows : src.rows;
  for (int i = tid; i < np; i += VS_MAP_COLOR_WG) {
    const int id = ids_cur[i];
    if (id < 0 || id >= m.cap || !(cur.flags[i] & RGBD_F_LM)) continue;
    const float2 p = *reinterpret_cast<const float2*>(cur.xy + 2 * (size_t)i);
    const int x = min(max(__float2int_rn(p.x), 0), max(gw - 1, 0)), y = min(max(__float2int_rn(p.y), 0), max(gh - 1, 0));     // half to even, then clamped
    out[id] = color_sample(img, src, x, y);
  }
  if (tid == 0) mc.colored[sq] = fc;
}

// ---- stand-alone: n integer pixels of one image (vslam_sample_color_u8) -----------------------------------------------
__global__ __launch_bounds__(256) void k_sample_color(const ColorSrc src, const int16_t* __restrict__ xy, int n, uint32_t* __restrict__ rgb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = *reinterpret_cast<const int*>(xy + 2 * (size_t)i);
  rgb[i] = color_sample(src.img, src, (int)(int16_t)(p & 0xffff), p >> 16);
}
