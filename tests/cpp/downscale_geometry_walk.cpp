// downscale_geometry_walk.cpp — the host side of csrc/downscale_geometry.h under the sanitizers, a program of its own (no device, no
// Python), built and run by hand from the repository's root (a few seconds):
//   g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I vslam_pose_estimation_framework_amd/csrc -o tests/cpp/downscale_geometry_walk tests/cpp/downscale_geometry_walk.cpp && tests/cpp/downscale_geometry_walk
// Over random full sizes 1 .. 700, the three factors, source phases 0 .. 3 and destination phases 0 .. 3 it walks every output row of
// k_downscale_u8 as the kernel does — the byte pixels, and per group of four the f (+ 1) dwords of each block row through ds_window — on
// buffers of exactly the rows' sizes (so that an index outside them is the sanitizer's finding), and checks that every byte read lies
// inside [0, f * out_cols) of its block row and at a dword-aligned address, that every output pixel is written exactly once and never
// beyond out_cols, and that the value is the definition's.  The depth kernel's block origin is walked on the same sizes; its sorting
// networks are checked on every 0-1 input (which proves them) and ds_lower_median against std::sort on random blocks with holes.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "downscale_geometry.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static std::mt19937 rng(20241021u);

// the definition, written apart from the helpers
static uint8_t mean_ref(const std::vector<uint8_t>& img, int stride, int f, int y, int x) {
  unsigned s = 0;
  for (int k = 0; k < f; ++k)
    for (int j = 0; j < f; ++j) s += img.at((size_t)(f * y + k) * stride + f * x + j);
  return (uint8_t)((s + f * f / 2) / (f * f));
}

// one image: full_rows x full_cols with `stride` bytes per row, its first byte at address phase `sp` (mod 4), the destination's first byte
// at phase `dp`, destination rows dstride bytes apart
static void walk_u8(int full_rows, int full_cols, int f, int stride, int sp, int dstride, int dp) {
  const int rows = ds_out(full_rows, f), cols = ds_out(full_cols, f);
  if (rows < 1 || cols < 1) { CHECK(!ds_size_ok(full_rows, full_cols, f), "size %d x %d / %d accepted", full_rows, full_cols, f); return; }
  CHECK(ds_size_ok(full_rows, full_cols, f), "size %d x %d / %d refused", full_rows, full_cols, f);
  std::vector<uint8_t> img((size_t)full_rows * stride);
  for (auto& b : img) b = (uint8_t)rng();
  std::vector<uint8_t> row((size_t)f * cols);                    // exactly what a block row may be read of
  std::vector<uint8_t> out(cols), written(cols);
  for (int y = 0; y < rows; ++y) {
    const uintptr_t o = (uintptr_t)dp + (uintptr_t)y * dstride;  // addresses as the kernel sees them, modulo what matters
    const int head = ds_head(o, cols);
    CHECK(head >= 0 && head <= cols && (head == cols || ((o + head) & 3u) == 0), "head %d", head);
    uint32_t sh[4];
    int v_lo = 0, v_hi = (cols - head) >> 2;
    for (int k = 0; k < f; ++k) {
      int lo, hi;
      sh[k] = ds_shift((uintptr_t)sp + (uintptr_t)(f * y + k) * stride, f, head);
      ds_groups(cols, f, head, sh[k], &lo, &hi);
      v_lo = std::max(v_lo, lo); v_hi = std::min(v_hi, hi);
    }
    std::fill(written.begin(), written.end(), 0);
    auto bytes = [&](int i0, int i1) {
      for (int i = i0; i < i1; ++i) {
        unsigned s = 0;
        for (int k = 0; k < f; ++k) {
          std::memcpy(row.data(), &img.at((size_t)(f * y + k) * stride), row.size());
          for (int j = 0; j < f; ++j) s += row.at((size_t)f * i + j);
        }
        out.at(i) = (uint8_t)ds_round(s, f);
        ++written.at(i);
      }
    };
    if (v_hi <= v_lo) bytes(0, cols);
    else {
      bytes(0, head + 4 * v_lo);
      for (int v = v_lo; v < v_hi; ++v) {
        unsigned s[4] = {0, 0, 0, 0};
        for (int k = 0; k < f; ++k) {
          std::memcpy(row.data(), &img.at((size_t)(f * y + k) * stride), row.size());
          const int w0 = ds_window(f, head, sh[k], v), nd = f + (sh[k] ? 1 : 0);
          CHECK(w0 >= 0 && w0 + 4 * nd <= f * cols, "window [%d, %d) outside [0, %d): f %d head %d sh %u v %d", w0, w0 + 4 * nd, f * cols, f, head, sh[k], v);
          CHECK((((uintptr_t)sp + (uintptr_t)(f * y + k) * stride + (uintptr_t)w0) & 3u) == 0, "window not dword aligned");
          uint8_t d[20];
          for (int b = 0; b < 4 * nd; ++b) d[b] = row.at((size_t)w0 + b);              // the dword loads
          for (int px = 0; px < 4; ++px)
            for (int j = 0; j < f; ++j) s[px] += d[sh[k] + f * px + j];                 // v_alignbyte_b32 by sh, then the byte sums
        }
        for (int px = 0; px < 4; ++px) { out.at((size_t)head + 4 * v + px) = (uint8_t)ds_round(s[px], f); ++written.at((size_t)head + 4 * v + px); }
        CHECK(((o + head + 4 * v) & 3u) == 0, "store not dword aligned");
      }
      bytes(head + 4 * v_hi, cols);
    }
    for (int x = 0; x < cols; ++x) {
      CHECK(written[x] == 1, "pixel (%d, %d) of %d x %d / %d written %d times", y, x, full_rows, full_cols, f, (int)written[x]);
      CHECK(out[x] == mean_ref(img, stride, f, y, x), "pixel (%d, %d) of %d x %d / %d", y, x, full_rows, full_cols, f);
    }
  }
  // the depth kernel: one lane per output pixel, the block's elements [f x, f x + f) of rows f y .. f y + f - 1
  std::vector<uint8_t> seen((size_t)full_rows * full_cols, 0);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x)
      for (int k = 0; k < f; ++k)
        for (int j = 0; j < f; ++j) ++seen.at((size_t)(f * y + k) * full_cols + f * x + j);
  for (int r = 0; r < full_rows; ++r)
    for (int c = 0; c < full_cols; ++c)
      CHECK(seen[(size_t)r * full_cols + c] == (r < rows * f && c < cols * f ? 1 : 0), "element (%d, %d) of %d x %d / %d in %d blocks", r, c, full_rows, full_cols, f, (int)seen[(size_t)r * full_cols + c]);
}

template <int N>
static void walk_network() {
  for (uint32_t bits = 0; bits < (1u << N); ++bits) {
    uint32_t u[N];
    for (int i = 0; i < N; ++i) u[i] = (bits >> i) & 1u;
    ds_sort<N>(u);
    for (int i = 0; i + 1 < N; ++i) CHECK(u[i] <= u[i + 1], "network of %d on %x", N, bits);
  }
  for (int c = 0; c < DsNet<N>::n; ++c) CHECK(DsNet<N>::ce[c].a < DsNet<N>::ce[c].b && DsNet<N>::ce[c].b < N, "pair %d of network %d", c, N);
}
template <int F>
static void walk_median() {
  constexpr int N = F * F;
  int counts[N + 1] = {0};
  for (int it = 0; it < 200000; ++it) {
    uint32_t v[N];
    std::vector<uint32_t> valid;
    const int style = it % 4;                                    // random, few distinct values, mostly holes, extremes
    for (int i = 0; i < N; ++i) {
      uint32_t x = style == 1 ? 1 + rng() % 3 : style == 3 ? (rng() & 1 ? 65535u : 0u) : rng() & 0xffffu;
      if (rng() % (style == 2 ? 2 : 5) == 0) x = 0;
      v[i] = x;
      if (x) valid.push_back(x);
    }
    std::sort(valid.begin(), valid.end());
    const uint32_t want = valid.empty() ? 0u : valid[(valid.size() - 1) / 2];
    ++counts[valid.size()];
    CHECK(ds_lower_median<F>(v) == want, "median of a %d x %d block, %zu values", F, F, valid.size());
  }
  for (int n = 0; n <= N; ++n) CHECK(counts[n] > 0, "no block with %d values at factor %d", n, F);
}

int main() {
  for (int f = 2; f <= 4; ++f)
    for (uint32_t s = 0; s <= (uint32_t)(255 * f * f); ++s) {
      const uint32_t q = s / (f * f), r = s % (f * f);
      CHECK(ds_round(s, f) == q + (2 * r >= (uint32_t)(f * f) ? 1u : 0u), "ds_round(%u, %d)", s, f);
    }
  CHECK(!ds_factor_ok(1) && ds_factor_ok(2) && ds_factor_ok(4) && !ds_factor_ok(5) && !ds_factor_ok(0) && !ds_factor_ok(-2), "factors");
  CHECK(!ds_size_ok(32768, 8, 2) && ds_size_ok(32767, 32767, 4) && !ds_size_ok(3, 8, 4) && !ds_size_ok(8, 1, 2) && !ds_size_ok(0, 8, 2), "sizes");
  walk_network<4>(); walk_network<9>(); walk_network<16>();
  walk_median<2>(); walk_median<3>(); walk_median<4>();
  std::uniform_int_distribution<int> size(1, 700), pad(0, 9);
  for (int it = 0; it < 40; ++it) {
    const int R = size(rng), C = size(rng);
    for (int f = 2; f <= 4; ++f)
      for (int sp = 0; sp < 4; ++sp) walk_u8(R, C, f, C + pad(rng), sp, C / f + pad(rng), (int)(rng() & 3u));
  }
  // small widths: every path's borders, with dense odd strides (every row at another phase)
  for (int f = 2; f <= 4; ++f)
    for (int oc = 1; oc <= 24; ++oc)
      for (int rem = 0; rem < f; ++rem)
        for (int sp = 0; sp < 4; ++sp)
          for (int dp = 0; dp < 4; ++dp) walk_u8(3 * f + rem, oc * f + rem, f, oc * f + rem, sp, oc + (dp & 1), dp);
  std::printf(fails ? "%d checks failed\n" : "downscale geometry walk: ok\n", fails);
  return fails ? 1 : 0;
}
