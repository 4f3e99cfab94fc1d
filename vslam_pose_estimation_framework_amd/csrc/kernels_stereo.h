// kernels_stereo.h — the stereo step of a frame, compute() (stereo_framepoint_generator.cpp:135-462): the sweep that pairs left and right features row by
// row for every epipolar offset, the bin competition among its matches, and the emission of the winners as new framepoints.
#pragma once
#include "kernels_recover.h"

// right features of the x-sorted row [g0, g1) with x <= xl, at most 255: binary search, 6 dependent loads instead of up to 255
template <class XR>
__device__ __forceinline__ int stereo_count_le(int g0, int g1, int xl, XR xr) {
  int lo = g0, hi = g1;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (xl - xr(mid) >= 0) lo = mid + 1; else hi = mid; }
  return min(lo - g0, 255);
}

// sdist[i][k], k < 16: Hamming distance of left feature i to right feature g0 + w0 + k of its row [g0, g1), where the
// window [w0, m) holds the (up to 16) nearest right features at or left of the left feature: m = number of right
// features of the row with x <= xl, w0 = max(m - 16, 0).  Nothing is written for m = 0 or m >= 255.
template <class XR>
__device__ __forceinline__ void stereo_dist_row(const uint8_t* descL, const uint8_t* descR, int i, int g0, int g1, int xl, XR xr,
                                                uint8_t* sdist) {
  const int m = stereo_count_le(g0, g1, xl, xr);
  if (m == 0 || m >= 255) return;
  const int w0 = max(m - 16, 0), mw = m - w0;
  const uint4 la = reinterpret_cast<const uint4*>(descL + (size_t)32 * i)[0], lb = reinterpret_cast<const uint4*>(descL + (size_t)32 * i)[1];
  uint32_t pk[4] = {0, 0, 0, 0};
  // four right descriptors in flight per step (the window is a contiguous index range)
  for (int k0 = 0; k0 < mw; k0 += 4) {
    uint4 ra[4], rb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint4* rp = reinterpret_cast<const uint4*>(descR + (size_t)32 * (g0 + w0 + min(k0 + u, mw - 1)));
      ra[u] = rp[0]; rb[u] = rp[1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int h = __popc(la.x ^ ra[u].x) + __popc(la.y ^ ra[u].y) + __popc(la.z ^ ra[u].z) + __popc(la.w ^ ra[u].w) +
                    __popc(lb.x ^ rb[u].x) + __popc(lb.y ^ rb[u].y) + __popc(lb.z ^ rb[u].z) + __popc(lb.w ^ rb[u].w);
      if (k0 + u < mw) pk[k0 >> 2] |= (uint32_t)(h > 255 ? 255 : h) << (8 * u);
    }
  }
  *reinterpret_cast<uint4*>(sdist + (size_t)i * 16) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
}

// L-R Hamming distances of the first epipolar pass for every left feature of every stream (image pipeline): the window
// the sweep's step A reads.  One thread per left feature.
__global__ __launch_bounds__(256) void k_stereo_dist(const DevCfg c, const DevBuf b) {
  int bx, sy;
  xcd_stream_block(&bx, &sy, b.xcd_rot);
  const int s = b.s0 + sy;
  if (!vs_active(b, s)) return;
  const int i = bx * blockDim.x + threadIdx.x;
  const int nL = b.n_kp[s * 2];
  if (i >= nL) return;
  const int16_t* kxyL = kpxy_of(c, b, s, 0);
  const int16_t* kxyR = kpxy_of(c, b, s, 1);
  const int rows = c.c.rows, CW1 = c.CW + 1, o = c.offsets[0];
  const int rr = kxyL[2 * i + 1] - o;
  if (rr < 0 || rr >= rows) return;
  const int32_t* rcR = rowcell_of(c, b, s, 1);
  stereo_dist_row(desc_of(c, b, s, 0), desc_of(c, b, s, 1), i, rcR[(size_t)rr * CW1], rcR[(size_t)rr * CW1 + c.CW], kxyL[2 * i],
                  [&](int g) { return (int)kxyR[2 * g]; }, b.sdist + (size_t)s * c.NMAX * 16);
}

// ---- the sweep (:235-360) ------------------------------------------------------------------------------------------------------
// It is sequential per image row only through the right cursor (a match at right feature g forbids g and everything left of it to
// later left features of the row).  A band of rows [r0, r1) owns the contiguous left features [l0, l1) and the right features
// [g0, g1) of the rows r - o; the band routine stages these slices in LDS (local index = global index minus l0 / g0) and runs
//  (A) every left feature, in parallel: over the window of its (up to 16) nearest right features at or left of it — whose
//      descriptor distances k_stereo_dist precomputed (offset 0) or the routine recomputes (later offsets) — the first-minimum
//      right feature for EVERY possible cursor position (a suffix-argmin table, 16 nibbles);
//  (B) one thread per row replays the cursor with one table lookup per left feature.  Only a cursor left of the window (more than
//      16 unconsumed right features behind the left feature, or 255 and more right features behind it at all) needs the
//      reference's explicit scan;
//  then appends the band's matches in sorted-left order.  The whole image is the band [0, rows) with all bases zero.
//
// Phase clock of the step (profiling builds, tools/probe/phase_clocks_per_stream.py): stamps 0 sweep, 1 append, 2 bin lists, 3 bin replay, 4 emission;
// b, s and tq travel into the routines below for VS_PHASE_STAMP alone.
struct StereoView {   // one stream's features as the sweep reads and writes them
  const int32_t *rcL, *rcR;       // row starts (rowcell), left / right
  const int16_t *kxyL, *kxyR;
  const uint8_t *descL, *descR;
  uint8_t *usedL, *usedR, *sdist;
  int32_t *sc, *match;            // candidates (left, right, distance, offset); HBM stand-in for the LDS match array
  int nL, nR, itau;               // itau: integer h < tau_tri  <=>  h < ceil(tau_tri)
};
#define VS_SD_TAG 0x200   // a match's distance field with this bit: "sdist[i][low nibble]", resolved by the parallel append (Hamming distances are <= 256)

__device__ __forceinline__ size_t stereo_stage_bytes(int n_rows, int nl, int nr) {
  return (size_t)4 * 2 * ((n_rows + 8) & ~7) + (size_t)(8 + 4 + 4 + 2 + 1 + 1) * ((nl + 7) & ~7) + (size_t)(2 + 1) * ((nr + 7) & ~7);
}
// start of row r in the left / right feature list; rows past the image start at the end of the list
__device__ __forceinline__ int stereo_row_start(const DevCfg& c, const int32_t* rc, int r) {
  return r < c.c.rows ? rc[(size_t)r * (c.CW + 1)] : rc[(size_t)(c.c.rows - 1) * (c.CW + 1) + c.CW];
}

// the reference's explicit scan from the cursor: first minimum below itau among the unused right features [cur, g1) with x <= xl, as
// distance << 16 | right feature, or -1
template <class XR, class UR>
__device__ __forceinline__ int stereo_scan(const StereoView& v, int i, int xl, int cur, int g1, XR xr, UR used) {
  const uint4 la = reinterpret_cast<const uint4*>(v.descL + (size_t)32 * i)[0], lb = reinterpret_cast<const uint4*>(v.descL + (size_t)32 * i)[1];
  int bg = -1, best = v.itau;
  for (int g = cur; g < g1; ++g) {
    if (used(g)) continue;
    if (xl - xr(g) < 0) break;
    const uint4 ra = reinterpret_cast<const uint4*>(v.descR + (size_t)32 * g)[0], rb = reinterpret_cast<const uint4*>(v.descR + (size_t)32 * g)[1];
    const int h = __popc(la.x ^ ra.x) + __popc(la.y ^ ra.y) + __popc(la.z ^ ra.z) + __popc(la.w ^ ra.w) +
                  __popc(lb.x ^ rb.x) + __popc(lb.y ^ rb.y) + __popc(lb.z ^ rb.z) + __popc(lb.w ^ rb.w);
    if (h < best) { best = h; bg = g; }
  }
  return bg < 0 ? -1 : (best << 16) | bg;
}

// append the matches of the left features [l0, l1) at offset o in sorted-left order and mark both features used; returns the new candidate count.
// res(i) = -1 or distance << 16 | right feature, dist_of(i, k) = sdist[i][k] for a VS_SD_TAG distance
template <class RES, class DIST>
__device__ __forceinline__ int stereo_append(const StereoView& v, FrameShared& sh, int o, int l0, int l1, int n_cand, RES res, DIST dist_of) {
  const int per = (l1 - l0 + VS_WG - 1) / VS_WG;
  const int i0 = l0 + threadIdx.x * per, i1 = min(i0 + per, l1);
  int cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += res(i) >= 0 ? 1 : 0;
  int total;
  int off = n_cand + block_exclusive_scan(cnt, sh.scan, &total);
  for (int i = i0; i < i1; ++i) {
    const int sm = res(i);
    if (sm < 0) continue;
    const int g = sm & 0xFFFF;
    int dist = sm >> 16;
    if (dist & VS_SD_TAG) dist = dist_of(i, dist & 15);
    reinterpret_cast<int4*>(v.sc)[off] = make_int4(i, g, dist, o);
    v.usedL[i] = 1; v.usedR[g] = 1;
    ++off;
  }
  return n_cand + total;
}

// One band at epipolar offset o.  WHOLE: the band is the image, its bases are compile-time zero.  SD: the distance rows ride along in LDS (whole image,
// first offset, when they fit) — an instantiation of its own, because a run-time pointer select between LDS and HBM would turn every access into a
// FLAT instruction, which waits on both the LDS and the HBM counters.
template <bool WHOLE, bool SD>
__device__ __forceinline__ int stereo_band(const DevCfg& c, const DevBuf& b, int s, unsigned long long& tq, const StereoView& v, FrameShared& sh, unsigned char* arena,
                                           bool recompute, int o, int r0_, int r1, int l0_, int l1, int g0_, int g1, int n_cand) {
  static_assert(WHOLE || !SD, "only the whole image carries its distance rows");
  const int tid = threadIdx.x, rows = c.c.rows;
  const int r0 = WHOLE ? 0 : r0_, l0 = WHOLE ? 0 : l0_, g0 = WHOLE ? 0 : g0_;
  const int nLp = ((l1 - l0) + 7) & ~7, nRp = ((g1 - g0) + 7) & ~7, rbn = r1 - r0, rowsp = (rbn + 8) & ~7;
  unsigned long long* ssuf = reinterpret_cast<unsigned long long*>(arena);   // step A: suffix-argmin nibbles
  int32_t* srL = reinterpret_cast<int32_t*>(ssuf + nLp);     // left row starts of rows r0 .. r1 (global indices)
  int32_t* srR = srL + rowsp;                                // right row starts of rows r0 - o .. r1 - o
  uint32_t* sxyL = reinterpret_cast<uint32_t*>(srR + rowsp); // x | y << 16
  int32_t* smatch = reinterpret_cast<int32_t*>(sxyL + nLp);  // sweep result per left feature: -1 or distance << 16 | right index
  uint16_t* sval = reinterpret_cast<uint16_t*>(smatch + nLp);// step A: bit c = a candidate exists at window position >= c
  int16_t* sxR = reinterpret_cast<int16_t*>(sval + nLp);
  uint8_t* suL = reinterpret_cast<uint8_t*>(sxR + nRp);      // used flags
  uint8_t* suR = suL + nLp;
  uint8_t* smL = suR + nRp;                                  // right features of the row at or left of the left feature (<= 255)
  uint4* sd4 = reinterpret_cast<uint4*>(arena + ((stereo_stage_bytes(rbn, l1 - l0, g1 - g0) + 15) & ~(size_t)15));
  for (int q = tid; q <= rbn; q += VS_WG) {
    srL[q] = stereo_row_start(c, v.rcL, r0 + q);
    srR[q] = stereo_row_start(c, v.rcR, min(max(r0 + q - o, 0), rows));
  }
#pragma unroll 4
  for (int i = l0 + tid; i < l1; i += VS_WG) { sxyL[i - l0] = reinterpret_cast<const uint32_t*>(v.kxyL)[i]; suL[i - l0] = v.usedL[i]; }
#pragma unroll 4
  for (int g = g0 + tid; g < g1; g += VS_WG) { sxR[g - g0] = v.kxyR[2 * g]; suR[g - g0] = v.usedR[g]; }
  if constexpr (SD) {
#pragma unroll 4
    for (int i = tid; i < l1; i += VS_WG) sd4[i] = reinterpret_cast<const uint4*>(v.sdist)[i];
  }
  __syncthreads();
  // distances of the first pass came from k_stereo_dist (image pipeline); later offsets recompute them here
  if (recompute) {
    for (int i = l0 + tid; i < l1; i += VS_WG) {
      if (suL[i - l0]) continue;
      const uint32_t xy = sxyL[i - l0];
      const int q = (int)(xy >> 16) - r0, rr = r0 + q - o;
      if (rr < 0 || rr >= rows) continue;
      stereo_dist_row(v.descL, v.descR, i, srR[q], srR[q + 1], (int)(xy & 0xFFFFu), [&](int g) { return (int)sxR[g - g0]; }, v.sdist);
    }
    __syncthreads();
  }
  // ---- step A ---------------------------------------------------------------------------------------------------
  for (int i = l0 + tid; i < l1; i += VS_WG) {
    unsigned long long suf = 0;
    unsigned val = 0;
    int m = 0;
    const uint32_t xy = sxyL[i - l0];
    const int q = (int)(xy >> 16) - r0, rr = r0 + q - o;
    if (!suL[i - l0] && rr >= 0 && rr < rows) {
      const int h0 = srR[q], h1 = srR[q + 1];
      m = stereo_count_le(h0, h1, (int)(xy & 0xFFFFu), [&](int g) { return (int)sxR[g - g0]; });
      if (m > 0 && m < 255) {
        const int w0 = max(m - 16, 0), mw = m - w0;
        uint4 dq;
        if constexpr (SD) dq = sd4[i]; else dq = *reinterpret_cast<const uint4*>(v.sdist + (size_t)i * 16);
        const unsigned long long d01 = ((unsigned long long)dq.y << 32) | dq.x, d23 = ((unsigned long long)dq.w << 32) | dq.z;
        int bh = 0, bj = -1;
        for (int k = mw - 1; k >= 0; --k) {
          const int h = (int)(((k < 8 ? d01 : d23) >> (8 * (k & 7))) & 255ull);
          if (!suR[h0 + w0 + k - g0] && h < v.itau && (bj < 0 || h <= bh)) { bh = h; bj = k; }
          if (bj >= 0) { suf |= (unsigned long long)bj << (4 * k); val |= 1u << k; }
        }
      }
    }
    ssuf[i - l0] = suf; sval[i - l0] = (uint16_t)val; smL[i - l0] = (uint8_t)m;
  }
  __syncthreads();
  // ---- step B: one thread per row ---------------------------------------------------------------------------------
  for (int q = tid; q < rbn; q += VS_WG) {
    const int rr = r0 + q - o;  // right row: L.row == R.row + o
    const bool rv = rr >= 0 && rr < rows;
    const int a0 = srL[q], a1 = srL[q + 1];
    const int h0 = rv ? srR[q] : 0, h1 = rv ? srR[q + 1] : 0;
    int cur = h0;
    for (int i = a0; i < a1; ++i) {
      const int m = smL[i - l0];
      int bg = -1, best = 0;
      // (m = 255 stands for "255 or more": the right features beyond the 255th are the explicit scan's to find)
      if (m > 0 && (cur < h0 + m || m == 255)) {
        const int w0 = max(m - 16, 0), cpos = cur - h0 - w0;
        if (m < 255 && cpos >= 0) {
          const unsigned val = sval[i - l0];
          if ((val >> cpos) & 1u) {
            const int k = (int)((ssuf[i - l0] >> (4 * cpos)) & 15ull);
            bg = h0 + w0 + k;
            best = VS_SD_TAG | k;   // the distance is fetched by the parallel append: no HBM round trip in this loop
          }
        } else {
          // cursor left of the window
          const int sm = stereo_scan(v, i, (int)(sxyL[i - l0] & 0xFFFFu), cur, h1, [&](int g) { return (int)sxR[g - g0]; }, [&](int g) { return suR[g - g0]; });
          if (sm >= 0) { bg = sm & 0xFFFF; best = sm >> 16; }
        }
      }
      int res = -1;
      if (bg >= 0 && !((double)((int)(sxyL[i - l0] & 0xFFFFu) - sxR[bg - g0]) < c.c.minimum_disparity_pixels)) {
        res = (best << 16) | bg;
        cur = bg + 1;
      }
      smatch[i - l0] = res;   // LDS: a global store here would put an HBM round trip into every step of the replay
    }
  }
  __syncthreads();
  if constexpr (WHOLE) VS_PHASE_STAMP(0, tq);
  return stereo_append(v, sh, o, l0, l1, n_cand, [&](int i) { return smatch[i - l0]; }, [&](int i, int k) -> int {
    if constexpr (SD) return reinterpret_cast<const uint8_t*>(sd4 + i)[k]; else return v.sdist[(size_t)i * 16 + k];
  });
}

// A single row whose slices exceed the arena (beyond ~5600 features in one row; the image may be 32767 wide): the reference's loop on HBM by one thread
__device__ __forceinline__ int stereo_row_hbm(const DevCfg& c, const StereoView& v, FrameShared& sh, int o, int r0, int l0, int l1, int g0, int g1, int n_cand) {
  const int tid = threadIdx.x;
  for (int i = l0 + tid; i < l1; i += VS_WG) v.match[i] = -1;
  __syncthreads();
  const int rr = r0 - o;
  if (tid == 0 && rr >= 0 && rr < c.c.rows) {
    int cur = g0;
    for (int i = l0; i < l1 && cur < g1; ++i) {
      if (v.usedL[i]) continue;
      const int xl = v.kxyL[2 * i];
      const int sm = stereo_scan(v, i, xl, cur, g1, [&](int g) { return (int)v.kxyR[2 * g]; }, [&](int g) { return v.usedR[g]; });
      if (sm >= 0 && !((double)(xl - v.kxyR[2 * (sm & 0xFFFF)]) < c.c.minimum_disparity_pixels)) { v.match[i] = sm; cur = (sm & 0xFFFF) + 1; }
    }
  }
  __syncthreads();
  return stereo_append(v, sh, o, l0, l1, n_cand, [&](int i) { return v.match[i]; }, [&](int, int) { return 0; });
}

// The staging does not fit the arena as a whole (very large feature counts): band by band.  Rows are independent and a band appends its matches
// before the next one starts: same results, same order.
__device__ __forceinline__ int stereo_sweep_banded(const DevCfg& c, const DevBuf& b, int s, unsigned long long& tq, const StereoView& v, FrameShared& sh, unsigned char* arena,
                                                   bool recompute, int o, int n_cand) {
  // There is no third form for an arena too small to band in: k_tail, the small-LDS kernel that passed one, is gone, and every caller has this arena.
  static_assert(VS_ARENA >= 8192, "the banded sweep needs an arena that holds at least a sparse row");
  const int rows = c.c.rows;
  auto rsR = [&](int r) { return stereo_row_start(c, v.rcR, min(max(r - o, 0), rows)); };
  int rb = max(1, (int)((size_t)rows * (size_t)VS_ARENA * 3 / (4 * stereo_stage_bytes(rows, v.nL, v.nR))));   // first guess: average density, 25 % slack
  for (int r0 = 0, r1; r0 < rows; r0 = r1) {
    int l0, l1, g0, g1;
    size_t need;
    for (;;) {   // shrink the band until its slices fit
      r1 = min(r0 + rb, rows);
      l0 = stereo_row_start(c, v.rcL, r0); l1 = stereo_row_start(c, v.rcL, r1);
      g0 = rsR(r0); g1 = rsR(r1);
      need = stereo_stage_bytes(r1 - r0, l1 - l0, g1 - g0);
      if (need <= (size_t)VS_ARENA || rb == 1) break;
      rb = max(1, rb / 2);
    }
    if (need > (size_t)VS_ARENA) { n_cand = stereo_row_hbm(c, v, sh, o, r0, l0, l1, g0, g1, n_cand); continue; }
    __syncthreads();   // the previous band's arrays are dead
    n_cand = stereo_band<false, false>(c, b, s, tq, v, sh, arena, recompute, o, r0, r1, l0, l1, g0, g1, n_cand);
  }
  __syncthreads();
  VS_PHASE_STAMP(0, tq);
  return n_cand;
}

// ---- the bin competition (:147-155, :371-394, :435-456) --------------------------------------------------------------------------
__device__ __forceinline__ int bin_of_pixel(const DevCfg& c, int x, int y) {
  const double bin = (double)c.c.bin_size_pixels;
  return min((int)rint((double)y / bin), c.rows_bin - 1) * c.cols_bin + min((int)rint((double)x / bin), c.cols_bin - 1);
}
// a candidate takes a bin that is empty, or whose holder has a smaller disparity and no smaller distance (not an argmax: order matters)
__device__ __forceinline__ bool bin_takes(int win, int disp, int dist, int wdisp, int wdist) { return win < 0 || (disp > wdisp && dist <= wdist); }
#define VS_BIN_EMPTY (-1)
#define VS_BIN_OCCUPIED (-2)   // by a tracked point: never replaced

// The competition's tables, three ways.  Per bin: a cursor (count, then start, then fill cursor: after the fill bin k's list is [cur(k - 1), cur(k)))
// and an occupant (VS_BIN_EMPTY, VS_BIN_OCCUPIED or the winning candidate).  Per candidate: its bin, disparity << 16 | distance, and a slot of the
// per-bin lists; the winners in bin order land in `out`.
template <bool LDS>   // 32-bit tables, in LDS or in HBM (cursors and lists written through atomics or by other waves are read past the vector L1)
struct BinTables32 {
  int32_t *occ_, *cur_, *items_, *cand_, *out_;   // [nb], [nb], [n], [n][2], [n]
  __device__ __forceinline__ static int ld(const int32_t* p) { if constexpr (LDS) return *p; else return ld_relaxed(p); }
  __device__ __forceinline__ void clear(int nb) const { for (int k = threadIdx.x; k < nb; k += VS_WG) { occ_[k] = VS_BIN_EMPTY; cur_[k] = 0; } }
  __device__ __forceinline__ void set_occ(int k, int v) const { occ_[k] = v; }
  __device__ __forceinline__ int occ(int k) const { return ld(occ_ + k); }
  __device__ __forceinline__ void set_cand(int q, int k, int pk) const { cand_[2 * q] = k; cand_[2 * q + 1] = pk; }
  __device__ __forceinline__ int cand_bin(int q) const { return cand_[2 * q]; }
  __device__ __forceinline__ int cand_pk(int q) const { return cand_[2 * q + 1]; }
  __device__ __forceinline__ int bump(int k) const { return atomicAdd(cur_ + k, 1); }
  __device__ __forceinline__ int cur(int k) const { return ld(cur_ + k); }
  __device__ __forceinline__ void set_cur(int k, int v) const { __hip_atomic_store(cur_ + k, v, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void set_item(int u, int q) const { items_[u] = q; }
  __device__ __forceinline__ int item(int u) const { return ld(items_ + u); }
  __device__ __forceinline__ void set_out(int t, int q) const { out_[t] = q; }
  __device__ __forceinline__ int out(int t) const { return out_[t]; }
};
// 16-bit tables in LDS (cursors two to a word, lists as u16), for grids too fine for the 32-bit ones: 4 (nb + 2) + 8 n + a few bytes
struct BinTables16 {
  uint32_t* cw; int words, n;   // cursors [words], then occupants [words], disparity | distance [n], lists [n], bins [n]
  __device__ __forceinline__ int16_t* occs() const { return reinterpret_cast<int16_t*>(cw + words); }
  __device__ __forceinline__ uint32_t* pks() const { return cw + 2 * words; }
  __device__ __forceinline__ uint16_t* items() const { return reinterpret_cast<uint16_t*>(cw + 2 * words + n); }
  __device__ __forceinline__ static size_t bytes(int nb, int n) { return ((size_t)((nb + 2) / 2) * 2 + (size_t)n) * 4 + (size_t)n * 4 + 16; }
  __device__ __forceinline__ void clear(int) const {
    for (int k = threadIdx.x; k < words; k += VS_WG) { cw[k] = 0u; cw[words + k] = 0xFFFFFFFFu; }
  }
  __device__ __forceinline__ void set_occ(int k, int v) const { occs()[k] = (int16_t)v; }
  __device__ __forceinline__ int occ(int k) const { return occs()[k]; }
  __device__ __forceinline__ void set_cand(int q, int k, int pk) const { items()[n + q] = (uint16_t)k; pks()[q] = (uint32_t)pk; }
  __device__ __forceinline__ int cand_bin(int q) const { return items()[n + q]; }
  __device__ __forceinline__ int cand_pk(int q) const { return (int)pks()[q]; }
  __device__ __forceinline__ int bump(int k) const { return (int)((atomicAdd(cw + (k >> 1), 1u << (16 * (k & 1))) >> (16 * (k & 1))) & 0xFFFFu); }
  __device__ __forceinline__ int cur(int k) const { return (int)((__hip_atomic_load(cw + (k >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (16 * (k & 1))) & 0xFFFFu); }
  __device__ __forceinline__ void set_cur(int k, int v) const { reinterpret_cast<uint16_t*>(cw)[k] = (uint16_t)v; }
  __device__ __forceinline__ void set_item(int u, int q) const { items()[u] = (uint16_t)q; }
  __device__ __forceinline__ int item(int u) const { return items()[u]; }
  __device__ __forceinline__ void set_out(int t, int q) const { items()[t] = (uint16_t)q; }   // (the emit scan's barriers retire every reader of the lists)
  __device__ __forceinline__ int out(int t) const { return items()[t]; }
};

// Tracked points seed the grid, the candidates are sorted into per-bin lists, one thread per bin replays its list in sweep order, and the winners are
// listed in bin-grid row-major order: t.out(0 ..).  Returns their number.
template <class T>
__device__ __forceinline__ int bin_competition(const DevCfg& c, const DevBuf& b, int s, unsigned long long& tq, FrameShared& sh, const StereoView& v,
                                               const PtView& cv, const T t, int n_tracked, int n_cand) {
  const int tid = threadIdx.x, nb = c.rows_bin * c.cols_bin;
  const int per = (nb + VS_WG - 1) / VS_WG, k0 = tid * per, k1 = min(k0 + per, nb);
  __syncthreads();
  t.clear(nb);
  __syncthreads();
  for (int j = tid; j < n_tracked; j += VS_WG) t.set_occ(bin_of_pixel(c, cv.kp[4 * (size_t)j], cv.kp[4 * (size_t)j + 1]), VS_BIN_OCCUPIED);
  for (int q = tid; q < n_cand; q += VS_WG) {            // bin id / disparity / distance of every candidate, once; per-bin counts
    const int4 e = *reinterpret_cast<const int4*>(v.sc + 4 * q);
    const int lxy = *reinterpret_cast<const int32_t*>(v.kxyL + 2 * e.x);
    const int xl = (int16_t)(lxy & 0xFFFF), yl = lxy >> 16;
    const int k = bin_of_pixel(c, xl, yl);
    t.set_cand(q, k, (int)(((uint32_t)(xl - v.kxyR[2 * e.y]) << 16) | (uint32_t)(e.z & 0xFFFF)));
    t.bump(k);
  }
  __syncthreads();
  VS_PHASE_STAMP(2, tq);
  {   // counts -> exclusive starts, in place
    int cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += t.cur(k);
    int total;
    int off = block_exclusive_scan(cnt, sh.scan, &total);
    for (int k = k0; k < k1; ++k) { const int m = t.cur(k); t.set_cur(k, off); off += m; }
  }
  __syncthreads();
  for (int q = tid; q < n_cand; q += VS_WG) t.set_item(t.bump(t.cand_bin(q)), q);   // fill: the cursor of bin k moves from its start to its end
  __syncthreads();
  for (int k = tid; k < nb; k += VS_WG) {
    if (t.occ(k) != VS_BIN_EMPTY) continue;
    const int i0 = k ? t.cur(k - 1) : 0, m = t.cur(k) - i0;
    int win = -1, wdisp = 0, wdist = 0, last = -1;
    for (int u = 0; u < m; ++u) {
      // next candidate in ascending sweep order (arrival order inside a list is arbitrary): smallest q greater than the last one taken
      int q = 0x7FFFFFFF;
      for (int w = 0; w < m; ++w) { const int x = t.item(i0 + w); if (x > last && x < q) q = x; }
      last = q;
      const int pk = t.cand_pk(q);
      if (bin_takes(win, pk >> 16, pk & 0xFFFF, wdisp, wdist)) { win = q; wdisp = pk >> 16; wdist = pk & 0xFFFF; }
    }
    t.set_occ(k, win);
  }
  __syncthreads();
  VS_PHASE_STAMP(3, tq);
  int cnt = 0;
  for (int k = k0; k < k1; ++k) cnt += t.occ(k) >= 0 ? 1 : 0;
  int total;
  int off = block_exclusive_scan(cnt, sh.scan, &total);
  for (int k = k0; k < k1; ++k) { const int q = t.occ(k); if (q >= 0) t.set_out(off++, q); }
  __syncthreads();
  return total;
}

// compute(): the sweep per epipolar offset, the bin competition (or plain emission), the history of the appended points, the shared counters
__device__ __forceinline__ void wg_stereo(const DevCfg& c, const DevBuf& b, int s, FrameShared& sh, int pb_cur, double tau_tri, int f, unsigned char* arena) {
  const int tid = threadIdx.x;
  const PtView cv = pts_of(c, b, s, pb_cur);
  const StereoView v = {rowcell_of(c, b, s, 0), rowcell_of(c, b, s, 1), kpxy_of(c, b, s, 0), kpxy_of(c, b, s, 1), desc_of(c, b, s, 0), desc_of(c, b, s, 1),
                        used_of(c, b, s, 0), used_of(c, b, s, 1), b.sdist + (size_t)s * c.NMAX * 16, b.sc + (size_t)s * c.NMAX * 4,
                        b.st_match + (size_t)s * c.NMAX * 3, b.n_kp[s * 2], b.n_kp[s * 2 + 1], (int)ceil(tau_tri)};
  const int n_tracked = sh.n_cur;
  const size_t stage_bytes = stereo_stage_bytes(c.c.rows, v.nL, v.nR);
  const bool staged = stage_bytes <= (size_t)VS_ARENA;
  // the distance rows of the first pass (from k_stereo_dist of the image pipeline) ride along when they fit
  const bool sd_lds = staged && ((stage_bytes + 15) & ~(size_t)15) + (size_t)16 * v.nL <= (size_t)VS_ARENA;
  int n_cand = 0;
#ifdef VS_PROFILE_PHASES
  unsigned long long tq = wall_clock64();
#else
  unsigned long long tq = 0;   // the stamps compile to nothing
#endif
#define DBG_STAMP(k) do { __syncthreads(); VS_PHASE_STAMP(k, tq); } while (0)
  for (int oi = 0; oi < c.n_offsets; ++oi) {
    const int o = c.offsets[oi];
    if (!staged) n_cand = stereo_sweep_banded(c, b, s, tq, v, sh, arena, oi > 0, o, n_cand);
    else if (oi == 0 && sd_lds) n_cand = stereo_band<true, true>(c, b, s, tq, v, sh, arena, false, o, 0, c.c.rows, 0, v.nL, 0, v.nR, n_cand);
    else n_cand = stereo_band<true, false>(c, b, s, tq, v, sh, arena, oi > 0, o, 0, c.c.rows, 0, v.nL, 0, v.nR, n_cand);
    DBG_STAMP(1);
  }
  // the competition's tables: in LDS (the sweep's staging is dead by now) when they fit, 32-bit before 16-bit, else in HBM
  const int nb = c.rows_bin * c.cols_bin;
  int32_t* const p = reinterpret_cast<int32_t*>(arena);
  int32_t* const aux = b.bin_aux + (size_t)s * (2 * ((size_t)nb + 1) + c.NMAX);
  const BinTables32<true> lds32 = {p, p + (nb + 1), p + 2 * (nb + 1), p + 2 * (nb + 1) + n_cand, p + 2 * (nb + 1) + 3 * n_cand};
  const BinTables16 lds16 = {reinterpret_cast<uint32_t*>(arena), (nb + 2) / 2, n_cand};
  const BinTables32<false> hbm = {b.bin_occ + (size_t)s * nb, aux, aux + 2 * ((size_t)nb + 1), v.match, v.match + 2 * (size_t)c.NMAX};
  enum { ALL, LDS32, LDS16, HBM } form = ALL;   // without binning every candidate becomes a point
  int added = n_cand;
  if (c.c.enable_keypoint_binning) {
    if (((size_t)3 * (nb + 1) + (size_t)4 * n_cand) * 4 <= (size_t)VS_ARENA) { form = LDS32; added = bin_competition(c, b, s, tq, sh, v, cv, lds32, n_tracked, n_cand); }
    else if (n_cand < 32767 && BinTables16::bytes(nb, n_cand) <= (size_t)VS_ARENA) { form = LDS16; added = bin_competition(c, b, s, tq, sh, v, cv, lds16, n_tracked, n_cand); }
    else { form = HBM; added = bin_competition(c, b, s, tq, sh, v, cv, hbm, n_tracked, n_cand); }
  }
  if (n_tracked + added > c.MAXP && tid == 0) atomicOr(&b.st[s].error_flags, 2);
  for (int u = tid; u < added && n_tracked + u < c.MAXP; u += VS_WG) {
    const int q = form == ALL ? u : form == LDS32 ? lds32.out(u) : form == LDS16 ? lds16.out(u) : hbm.out(u);
    const int4 e = *reinterpret_cast<const int4*>(v.sc + 4 * q);
    materialize_point(c, b, s, cv, n_tracked + u, e.x, e.y, e.z, e.w, -1, 0);
  }
  DBG_STAMP(4);
#undef DBG_STAMP
  const int n_final = min(n_tracked + added, c.MAXP);
  // history of the appended points
  double* hc = hcam_of(c, b, s, f);
  int32_t* hp = hprev_of(c, b, s, f);
  for (int j = n_tracked + tid; j < n_final; j += VS_WG) {
    { const double x = cv.cam[3 * (size_t)j], y = cv.cam[3 * (size_t)j + 1], z = cv.cam[3 * (size_t)j + 2];
      reinterpret_cast<double2*>(hc + 4 * (size_t)j)[0] = make_double2(x, y); reinterpret_cast<double2*>(hc + 4 * (size_t)j)[1] = make_double2(z, 1 / z); }
    hp[j] = -1;
    if (c.trail) *reinterpret_cast<uint4*>(cv.trail + (size_t)j * VS_TRAIL) = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);   // a track starts here
  }
  if (tid == 0) { sh.n_cand = added; sh.n_cur = n_final; }
  __syncthreads();
}
