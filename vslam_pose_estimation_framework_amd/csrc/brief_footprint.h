// brief_footprint.h — which elements of the 49 x 49 box patch around a point the 512 taps of a BRIEF pattern read, and the list of 16-byte
// loads that covers them.  The pattern is run-time data (vslam_set_brief_pattern), so the table is derived from whatever pattern is loaded:
// brief_footprint() is the one builder, constexpr so that the built-in pattern's table is a static initialiser, plain C++ so that a host
// test can call it.  Reader: recover_brief_patch (the work list); the row bounds were tried on k_brief's staging and changed nothing.
//
// A staged patch row holds 56 u16 = 7 chunks of 16 bytes and begins at the image column (x - 24) & ~7, so the tap at column offset dx sits
// at row element a + 24 + dx with a = (x - 24) & 7.  The list is point-independent: a row with taps in [lo, hi] gets the chunks
// (24 + lo) >> 3 .. (31 + hi) >> 3, which cover every alignment a = 0 .. 7 and end at chunk 6 at most (hi <= 24) — no load leaves the
// 49 x 56 window —, and an item carries lo and hi, so the reader drops a chunk that lies wholly beside the taps at ITS alignment
// (brief_footprint_needs).
#pragma once
#include <stdint.h>
#include "../../include/vslam_brief_pattern.h"

#define VS_FP_ROWS (2 * VSLAM_BRIEF_PATCH_HALF + 1)    // 49 patch rows, row r = row offset r - 24
#define VS_FP_CPR 7                                    // 16-byte chunks per staged patch row
#define VS_FP_MAX_ITEMS (VS_FP_ROWS * VS_FP_CPR)       // the full rectangle: every row sampled at both ends
#define VS_FP_NO_ITEM (63u << 9)                       // lo = 63, hi = 0: needed at no alignment (fills a reader's unused slots)

struct BriefFootprint {
  int8_t col_lo[VS_FP_ROWS], col_hi[VS_FP_ROWS];       // first / last sampled column offset of a patch row; empty row: lo > hi
  int8_t row_lo, row_hi;                               // first / last non-empty row, as row offsets -24 .. 24
  int16_t n_items;
  uint32_t item[VS_FP_MAX_ITEMS];                      // row-major: row | chunk << 6 | (24 + lo) << 9 | (24 + hi) << 15
};

constexpr int brief_footprint_row(uint32_t item) { return (int)(item & 63u); }
constexpr int brief_footprint_chunk(uint32_t item) { return (int)((item >> 6) & 7u); }
// does the chunk hold a sampled element when the row begins a = (x - 24) & 7 elements before the patch's first column?
constexpr bool brief_footprint_needs(uint32_t item, int a) {
  return 8 * brief_footprint_chunk(item) + 7 >= a + (int)((item >> 9) & 63u) && 8 * brief_footprint_chunk(item) <= a + (int)((item >> 15) & 63u);
}

// pairs: 256 x {y1, x1, y2, x2}, every offset within +-24 (pattern_io checks a caller's table before it gets here)
constexpr BriefFootprint brief_footprint(const int8_t (*pairs)[4]) {
  BriefFootprint f{};
  for (int r = 0; r < VS_FP_ROWS; ++r) { f.col_lo[r] = VSLAM_BRIEF_PATCH_HALF + 1; f.col_hi[r] = -VSLAM_BRIEF_PATCH_HALF - 1; }
  for (int i = 0; i < 256; ++i)
    for (int k = 0; k < 4; k += 2) {
      const int r = pairs[i][k] + VSLAM_BRIEF_PATCH_HALF;
      const int8_t x = pairs[i][k + 1];
      if (x < f.col_lo[r]) f.col_lo[r] = x;
      if (x > f.col_hi[r]) f.col_hi[r] = x;
    }
  f.row_lo = VSLAM_BRIEF_PATCH_HALF + 1; f.row_hi = -VSLAM_BRIEF_PATCH_HALF - 1;
  int n = 0;
  for (int r = 0; r < VS_FP_ROWS; ++r) {
    if (f.col_lo[r] > f.col_hi[r]) continue;
    if (f.row_lo > VSLAM_BRIEF_PATCH_HALF) f.row_lo = (int8_t)(r - VSLAM_BRIEF_PATCH_HALF);
    f.row_hi = (int8_t)(r - VSLAM_BRIEF_PATCH_HALF);
    const int lo = VSLAM_BRIEF_PATCH_HALF + f.col_lo[r], hi = VSLAM_BRIEF_PATCH_HALF + f.col_hi[r];
    for (int c = lo >> 3; c <= (hi + 7) >> 3; ++c) f.item[n++] = (uint32_t)r | (uint32_t)c << 6 | (uint32_t)lo << 9 | (uint32_t)hi << 15;
  }
  f.n_items = (int16_t)n;
  return f;
}
