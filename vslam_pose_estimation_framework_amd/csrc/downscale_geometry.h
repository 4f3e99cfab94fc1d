// downscale_geometry.h — the index arithmetic of kernels_downscale.h, host and device: the output size, the cut of an output row into
// byte pixels and groups of four, the dword window of a group in a block row, the rounded block average and the lower median of a depth
// block.  Plain C++ (no HIP header), so that the sanitizer walk (tests/cpp/downscale_geometry_walk.cpp) runs exactly what the kernels run.
//
// Factor f is 2, 3 or 4.  Output pixel (y, x) owns the f x f block whose corner is (f y, f x); the full % f bottom rows and right columns
// belong to no block and are never read.  Block row k of output row y is full row f y + k, of which the bytes [0, f * out_cols) are used.
#pragma once
#include <stdint.h>
#include "exp_fixed.h"            // VS_XD

#define VS_DS_MIN_FACTOR 2
#define VS_DS_MAX_FACTOR 4
#define VS_DS_MAX_SIZE 32767      // of a full image, either direction

VS_XD inline bool ds_factor_ok(int f) { return f >= VS_DS_MIN_FACTOR && f <= VS_DS_MAX_FACTOR; }
VS_XD inline int ds_out(int full, int f) { return full / f; }
// what the setters and the stand-alone entries ask of a full size: both in 1 .. 32767 and at least one block in each direction
VS_XD inline bool ds_size_ok(int full_rows, int full_cols, int f) {
  return full_rows >= 1 && full_cols >= 1 && full_rows <= VS_DS_MAX_SIZE && full_cols <= VS_DS_MAX_SIZE && ds_out(full_rows, f) >= 1 && ds_out(full_cols, f) >= 1;
}
// (sum of an f x f block + f f / 2) / (f f): round half up
VS_XD inline uint32_t ds_round(uint32_t sum, int f) { return (sum + (uint32_t)(f * f) / 2u) / (uint32_t)(f * f); }

// ---- an output row of the 8-bit kernel --------------------------------------------------------------------------------
// The row is cut at the DESTINATION's dword borders: `head` pixels ahead of the first aligned one, then groups of four output pixels (one
// 32-bit store each), then fewer than four.  Group v of block row k starts at source byte f * (head + 4 v) of that row, at any address: a
// lane loads the f dwords from the dword-aligned address below it, and one more when that address is not its first byte (shift sh = the
// address & 3, the same for every group of the block row since 4 f is a multiple of 4).  A group takes this wide path only when its whole
// window [first byte - sh, + 4 f (+ 4 when sh)) lies inside [0, f * out_cols) of the block row, for each of the f block rows; every other
// pixel goes through byte loads of exactly its own f x f bytes.
VS_XD inline int ds_head(uintptr_t dst_row, int out_cols) {
  const int h = (int)((4u - (uint32_t)(dst_row & 3u)) & 3u);
  return h < out_cols ? h : out_cols;
}
VS_XD inline uint32_t ds_shift(uintptr_t src_row, int f, int head) { return (uint32_t)((src_row + (uintptr_t)(f * head)) & 3u); }
// byte offset in the block row at which group v's window begins (>= 0 for v >= *v_lo of ds_groups)
VS_XD inline int ds_window(int f, int head, uint32_t sh, int v) { return f * head + 4 * f * v - (int)sh; }
// groups of a block row with shift sh whose window lies inside the row: [*v_lo, *v_hi), possibly empty
VS_XD inline void ds_groups(int out_cols, int f, int head, uint32_t sh, int* v_lo, int* v_hi) {
  const int nvec = (out_cols - head) >> 2;
  const int extra = sh ? 4 : 0;
  *v_lo = f * head < (int)sh ? 1 : 0;                                     // the rounding would reach below the row
  const int room = f * (out_cols - head) + (int)sh - 4 * f - extra;       // >= 4 f v  <=>  group v's window ends inside the row
  const int hi = room < 0 ? 0 : room / (4 * f) + 1;
  *v_hi = hi < nvec ? hi : nvec;
}

// ---- the lower median of a depth block --------------------------------------------------------------------------------
// A hole (0) becomes 65536, above every value; a fixed network (Batcher's merge exchange) sorts the f f numbers ascending, so the v
// values come first; the answer is element (v - 1) / 2, or 0 when v == 0.  Everything is indexed by constants once unrolled.
struct DsPair { uint8_t a, b; };
template <int N> struct DsNet;
template <> struct DsNet<4> {
  static constexpr int n = 5;
  static constexpr DsPair ce[5] = {{0, 1}, {2, 3}, {0, 2}, {1, 3}, {1, 2}};
};
template <> struct DsNet<9> {
  static constexpr int n = 28;
  static constexpr DsPair ce[28] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {1, 2}, {5, 6}, {0, 4}, {1, 5}, {2, 6}, {3, 7},
                                    {2, 4}, {3, 5}, {1, 2}, {3, 4}, {5, 6}, {0, 8}, {4, 8}, {2, 4}, {3, 5}, {6, 8}, {1, 2}, {3, 4}, {5, 6}, {7, 8}};
};
template <> struct DsNet<16> {
  static constexpr int n = 63;
  static constexpr DsPair ce[63] = {{0, 1}, {2, 3}, {4, 5}, {6, 7}, {8, 9}, {10, 11}, {12, 13}, {14, 15}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {8, 10},
                                    {9, 11}, {12, 14}, {13, 15}, {1, 2}, {5, 6}, {9, 10}, {13, 14}, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {8, 12}, {9, 13},
                                    {10, 14}, {11, 15}, {2, 4}, {3, 5}, {10, 12}, {11, 13}, {1, 2}, {3, 4}, {5, 6}, {9, 10}, {11, 12}, {13, 14}, {0, 8},
                                    {1, 9}, {2, 10}, {3, 11}, {4, 12}, {5, 13}, {6, 14}, {7, 15}, {4, 8}, {5, 9}, {6, 10}, {7, 11}, {2, 4}, {3, 5},
                                    {6, 8}, {7, 9}, {10, 12}, {11, 13}, {1, 2}, {3, 4}, {5, 6}, {7, 8}, {9, 10}, {11, 12}, {13, 14}};
};
// ascending, in place
template <int N>
VS_XD inline void ds_sort(uint32_t (&u)[N]) {
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
  for (int c = 0; c < DsNet<N>::n; ++c) {
    constexpr const DsPair* ce = DsNet<N>::ce;
    const uint32_t lo = u[ce[c].a] < u[ce[c].b] ? u[ce[c].a] : u[ce[c].b];
    const uint32_t hi = u[ce[c].a] < u[ce[c].b] ? u[ce[c].b] : u[ce[c].a];
    u[ce[c].a] = lo; u[ce[c].b] = hi;
  }
}
// v: the f f raw values of a block in any order (destroyed)
template <int F>
VS_XD inline uint32_t ds_lower_median(uint32_t (&v)[F * F]) {
  constexpr int N = F * F;
  int valid = 0;
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i < N; ++i) { valid += v[i] != 0u; v[i] = v[i] ? v[i] : 65536u; }
  ds_sort<N>(v);
  const int k = (valid - 1) >> 1;                                         // -1 when there is no value: no element is picked
  uint32_t out = 0u;
#if defined(__HIPCC__) || defined(__clang__)
#pragma unroll
#endif
  for (int i = 0; i <= (N - 1) / 2; ++i) out = k == i ? v[i] : out;
  return out;
}
