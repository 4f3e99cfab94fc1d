// bilateral_geometry_walk.cpp — the host side of csrc/exp_fixed.h and csrc/bilateral_geometry.h under the sanitizers, a program of its own
// (no device, no Python), built and run by hand from the repository's root (about 10 s):
//   g++ -O1 -g -std=c++17 -Wall -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I vslam_pose_estimation_framework_amd/csrc -o tests/cpp/bilateral_geometry_walk tests/cpp/bilateral_geometry_walk.cpp && tests/cpp/bilateral_geometry_walk
// Over random sizes 1 .. 700 and radii 1 .. 8 it walks every tile of k_bilateral_apply as the kernel does — every staged element of the square
// through bl_staged, every tap of every pixel through the square's pitch — into buffers of exactly the kernel's sizes (so that an index
// outside them is the sanitizer's finding), and checks that every staged index lies inside the image, that the staged value is the one
// the definition's reflection names, and that the tiles' pixels partition the image.  exp_fixed is walked over its whole domain; with
// arguments, their values are printed as bit patterns (to compare with bilateral.py by hand).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "bilateral_geometry.h"

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the definition's loop, written apart from the helper
static int reflect_ref(long p, long n) {
  if (n == 1) return 0;
  for (;;) {
    if (p >= 0 && p < n) return (int)p;
    p = p < 0 ? -p : 2 * n - 2 - p;
  }
}

static void walk_image(int rows, int cols, const BlTaps& t) {
  const int radius = t.radius, halo = bl_halo(radius), pitch = bl_pitch(radius);
  std::vector<int32_t> image((size_t)rows * cols);
  for (size_t i = 0; i < image.size(); ++i) image[i] = (int32_t)i;
  std::vector<uint8_t> owned((size_t)rows * cols, 0);
  std::vector<int32_t> sq((size_t)VS_BL_HALO_MAX * (VS_BL_HALO_MAX | 1));     // the kernel's array
  for (int ty = 0; ty < bl_tiles(rows); ++ty)
    for (int tx = 0; tx < bl_tiles(cols); ++tx) {
      for (int e = 0; e < halo * halo; ++e) {
        const int hy = e / halo, hx = e - hy * halo;
        const int r = bl_staged(ty, hy, radius, rows), c = bl_staged(tx, hx, radius, cols);
        CHECK(r >= 0 && r < rows && c >= 0 && c < cols, "staged (%d, %d) outside %d x %d", r, c, rows, cols);
        CHECK(r == reflect_ref((long)ty * VS_BL_TILE - radius + hy, rows) && c == reflect_ref((long)tx * VS_BL_TILE - radius + hx, cols), "reflection");
        sq.at((size_t)hy * pitch + hx) = image.at((size_t)r * cols + c);
      }
      for (int tid = 0; tid < 256; ++tid) {
        const int px = (tid & 15) * 2, py = tid >> 4;
        for (int h = 0; h < 2; ++h)
          for (int w = 0; w < 2; ++w) {
            const int r = ty * VS_BL_TILE + py + 16 * h, c = tx * VS_BL_TILE + px + w;
            if (r >= rows || c >= cols) continue;
            ++owned.at((size_t)r * cols + c);
            const int base = (py + 16 * h + radius) * pitch + px + w + radius;
            for (int k = 0; k < t.n; ++k) {
              const int o = base + (int)t.di[k] * pitch + (int)t.dj[k];
              const int32_t want = image.at((size_t)reflect_ref(r + t.di[k], rows) * cols + reflect_ref(c + t.dj[k], cols));
              CHECK(sq.at((size_t)o) == want, "tap %d of pixel (%d, %d) in %d x %d radius %d", k, r, c, rows, cols, radius);
            }
          }
      }
    }
  for (size_t i = 0; i < owned.size(); ++i) CHECK(owned[i] == 1, "pixel %zu of %d x %d owned %d times", i, rows, cols, (int)owned[i]);
}

int main(int argc, char** argv) {
  // exp_fixed: finite, inside [0, 1], non-increasing within an ulp-sized slack, over the whole domain and beyond its end
  double prev = 1.0;
  for (int i = 0; i <= 760 * 64; ++i) {
    const double x = -(double)i / 64.0, e = exp_fixed(x);
    CHECK(e >= 0.0 && e <= 1.0 && e <= prev * (1.0 + 1e-15), "exp_fixed(%g) = %g after %g", x, e, prev);
    prev = e;
  }
  CHECK(exp_fixed(0.0) == 1.0, "exp_fixed(0)");
  CHECK(exp_fixed(-1e300) == 0.0 && exp_fixed(-746.5) == 0.0, "exp_fixed underflow");
  for (int i = 1; i < argc; ++i) {
    const double x = std::atof(argv[i]), e = exp_fixed(x);
    uint64_t b;
    std::memcpy(&b, &e, 8);
    std::printf("exp_fixed(%.17g) = %016" PRIx64 "\n", x, b);
  }
  // the taps of every radius: their count, their order, the refusal above 8
  static const int counts[9] = {0, 5, 13, 29, 49, 81, 113, 149, 197};
  BlTaps taps[9];
  for (int radius = 1; radius <= 8; ++radius) {
    BlTaps& t = taps[radius];
    CHECK(bl_make_taps(radius / 1.5 + 1e-9, t), "radius %d refused", radius);
    CHECK(t.radius == radius && t.n == counts[radius] && t.n <= VS_BL_MAX_TAPS, "radius %d: %d taps at radius %d", radius, t.n, t.radius);
    for (int k = 1; k < t.n; ++k) CHECK(t.di[k] > t.di[k - 1] || (t.di[k] == t.di[k - 1] && t.dj[k] > t.dj[k - 1]), "tap order");
  }
  BlTaps none;
  CHECK(!bl_make_taps(5.7, none) && !bl_make_taps(1e308, none) && bl_make_taps(-3.0, none) && none.radius == 2, "radius refusals");
  std::mt19937 rng(20240611u);
  std::uniform_int_distribution<int> size(1, 700), rad(1, 8);
  for (int it = 0; it < 60; ++it) walk_image(size(rng), size(rng), taps[rad(rng)]);
  for (int radius = 1; radius <= 8; ++radius)
    for (int n : {1, 2, 3, 31, 32, 33}) { walk_image(n, 65, taps[radius]); walk_image(65, n, taps[radius]); walk_image(n, n, taps[radius]); }
  std::printf(fails ? "%d checks failed\n" : "bilateral geometry walk: ok\n", fails);
  return fails ? 1 : 0;
}
