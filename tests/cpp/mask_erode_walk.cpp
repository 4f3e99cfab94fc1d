// mask_erode_walk.cpp — mask_erode_word, mask_cols_word and mask_gather4 of csrc/kernels_mask.h (host-and-device code) against a scalar loop: every margin
// 0 .. 64 on random, mostly-kept, one-hole and all-kept word triples.  Built and run by tests/test_mask_host.py; by hand with the sanitizers:
//   hipcc -x hip -O1 -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -o mask_erode_walk mask_erode_walk.cpp && ./mask_erode_walk
#include "../../vslam_pose_estimation_framework_amd/csrc/kernels_mask.h"
#include <cstdio>
#include <cstdlib>
#include <random>
static int bit(const unsigned long long w[3], int p) { return p < 0 || p >= 192 ? 1 : (int)((w[p >> 6] >> (p & 63)) & 1); }
int main() {
  std::mt19937_64 rng(5);
  long bad = 0, n = 0;
  for (int m = 0; m <= 64; ++m)
    for (int it = 0; it < 400; ++it) {
      unsigned long long w[3];
      const int mode = it % 4;
      for (int i = 0; i < 3; ++i) {
        unsigned long long x = rng();
        if (mode == 1) x |= rng() | rng() | rng();          // mostly ones
        if (mode == 2) x = ~0ull & ~(1ull << (rng() % 64)); // one hole
        if (mode == 3) x = ~0ull;
        w[i] = x;
      }
      if (mode == 3) w[rng() % 3] &= ~(1ull << (rng() % 64));
      unsigned long long want = 0;
      for (int b = 0; b < 64; ++b) {
        int v = 1;
        for (int d = -m; d <= m; ++d) v &= bit(w, 64 + b + d);
        want |= (unsigned long long)v << b;
      }
      const unsigned long long got = mask_erode_word(w[0], w[1], w[2], m);
      ++n;
      if (got != want) { if (bad < 5) printf("m=%d mode=%d got %016llx want %016llx\n", m, mode, got, want); ++bad; }
    }
  for (int cols = 1; cols < 200; ++cols)
    for (int t = 0; t < 4; ++t) {
      unsigned long long want = 0;
      for (int b = 0; b < 64; ++b) if (64 * t + b < cols) want |= 1ull << b;
      if (mask_cols_word(t, cols) != want) { ++bad; printf("cols %d t %d\n", cols, t); }
    }
  // mask_gather4: four ballots over lanes that hold four consecutive pixels each, back into pixel order
  for (int it = 0; it < 2000; ++it) {
    unsigned long long px[4] = {rng(), rng() | rng(), rng() & rng(), it % 3 ? rng() : ~0ull}, b[4] = {0, 0, 0, 0};
    for (int l = 0; l < 64; ++l)
      for (int e = 0; e < 4; ++e) {
        const int p = 4 * l + e;
        b[e] |= ((px[p >> 6] >> (p & 63)) & 1ull) << l;
      }
    for (int k = 0; k < 4; ++k, ++n)
      if (mask_gather4(b[0], b[1], b[2], b[3], k) != px[k]) { ++bad; printf("gather4 word %d\n", k); }
  }
  printf("%ld cases, %ld bad\n", n, bad);
  return bad != 0;
}
