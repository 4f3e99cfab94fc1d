// orb_plan.h — the OrbDetector's pyramid plan and the index arithmetic of the feature store that holds its keypoints.  Plain C++ that the
// host, the kernels of kernels_rgbd_orb.h and a stand-alone program (tests/cpp/orb_store_walk.cpp) all compile: nothing here touches HIP.
//
// The plan is cv::ORB's computeKeyPoints bookkeeping (orb.cpp [recalled]) as vslam_orb_detect has always evaluated it: level l is the image
// scaled by 1 / scale_factor^l (float power, float quotient, rounded half to even), the pyramid ends at the first level smaller than
// 2 * edge + 8 in either direction, and the per-level quotas are a geometric series over ALL nlevels in float arithmetic.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#define VS_ORB_HD __host__ __device__
#else
#define VS_ORB_HD
#endif

#define VS_ORB_MAX_LEVELS 16
struct OrbPlan {
  int32_t n_levels;                       // levels that exist (<= nlevels)
  int32_t rows[VS_ORB_MAX_LEVELS], cols[VS_ORB_MAX_LEVELS];
  int32_t quota[VS_ORB_MAX_LEVELS];       // retainBest(quota) on the Harris response, retainBest(2 * quota) on the FAST score before it
  float scale[VS_ORB_MAX_LEVELS];         // (float)pow(scale_factor, l)
};
// rows x cols: the image the detector sees (a detector region's view).  nlevels <= VS_ORB_MAX_LEVELS.
static inline OrbPlan orb_plan(int rows, int cols, int nfeatures, float scale_factor, int nlevels, int edge) {
  OrbPlan p;
  for (int l = 0; l < VS_ORB_MAX_LEVELS; ++l) { p.rows[l] = p.cols[l] = p.quota[l] = 0; p.scale[l] = 1.f; }
  {
    const float factor = (float)(1.0 / scale_factor);
    float nd = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; ++l) { p.quota[l] = (int)lrint(nd); sum += p.quota[l]; nd *= factor; }
    p.quota[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;
  }
  p.n_levels = 0;
  for (int l = 0; l < nlevels; ++l) {
    const float sc = (float)pow((double)scale_factor, (double)l);
    const int nr = l ? (int)lrint(rows / sc) : rows, nc = l ? (int)lrint(cols / sc) : cols;
    if (l > 0 && (nr < 2 * edge + 8 || nc < 2 * edge + 8)) break;
    p.rows[l] = nr; p.cols[l] = nc; p.scale[l] = sc;
    p.n_levels = l + 1;
  }
  return p;
}

// ---- the feature store's index arithmetic -------------------------------------------------------------------------------------------------
// A frame's keypoint VECTOR (keypointsLeft(): detections appended attempt after attempt, region-major, level-major inside a region) is kept
// as arrays sorted by lattice pixel, with `order` mapping vector positions to sorted indices and `fvis` marking, per pixel, the feature the
// reference's lattice ends up pointing at: the last one written in vector order (intensity_feature_matcher.cpp:48-70).
//
// key of a keypoint: its lattice pixel ((int)y, (int)x), row-major
VS_ORB_HD static inline uint32_t orbd_pixel_key(float x, float y) { return ((uint32_t)(uint16_t)(int)y << 16) | (uint32_t)(uint16_t)(int)x; }
// true when the n levels, in vector order, never decrease (cv::ORB::compute leaves such a vector alone)
VS_ORB_HD static inline bool orbd_level_sorted(const uint8_t* level, int n) {
  for (int i = 1; i < n; ++i) if (level[i] < level[i - 1]) return false;
  return true;
}
// position of vector element v after the stable level-major regroup
VS_ORB_HD static inline int orbd_regroup_pos(const uint8_t* level, int n, int v) {
  const int lv = level[v];
  int at = 0;
  for (int u = 0; u < n; ++u) at += (level[u] < lv || (level[u] == lv && u < v)) ? 1 : 0;
  return at;
}
// rank of vector element v among `members` (m indices into key[] / vp[]; null: elements 0 .. m - 1 themselves): row-major by key, equal pixels
// in the order of their (final) vector positions vp[]; *visible: no member on the same pixel sits later in the vector.  Over the whole vector
// this is v's sorted index; the kernel asks it over the members of v's image ROW and adds the row's start (keys order rows first).
VS_ORB_HD static inline int orbd_rank(const uint32_t* key, const int32_t* vp, const int32_t* members, int m, int v, bool* visible) {
  const uint32_t k = key[v];
  const int p = vp[v];
  int at = 0;
  bool last = true;
  for (int j = 0; j < m; ++j) {
    const int u = members ? members[j] : j;
    const uint32_t ku = key[u];
    at += (ku < k || (ku == k && vp[u] < p)) ? 1 : 0;
    last = last && !(ku == k && vp[u] > p);
  }
  *visible = last;
  return at;
}
// row / cell CSR entry: sorted keys[0 .. n) below pixel (row, x)
VS_ORB_HD static inline int orbd_lower_bound(const uint32_t* sorted_key, int n, uint32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) { const int m = (lo + hi) >> 1; if (sorted_key[m] < key) lo = m + 1; else hi = m; }
  return lo;
}
