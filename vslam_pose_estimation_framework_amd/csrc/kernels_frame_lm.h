// kernels_frame_lm.h — the stereo tracker's landmark creation and refinement (_updatePoints' landmark part, pose_tracker_3d.cpp:475-520):
// history ring and trails, the per-track refinement by one lane or a team of eight, and the workgroup bodies that stage the poses, build the
// work lists and hand the tracks out.  The Gauss-Newton arithmetic itself is landmark_math.h's.
#pragma once
#include "kernels_frame.h"
#include "landmark_math.h"

// Creation = mean of the track's world coordinates (Landmark::Landmark, landmark.cpp:19-31), otherwise Gauss-Newton refinement over all
// measurements of the track (Landmark::update, :66-167).  Measurements are reached by walking the per-frame `prev` links of the history ring
// (frame f, index i) -> (f-1, prev[i]).
// The poses of the last VS_LM_NP frames are staged in LDS once per workgroup and the first VS_LM_CN measurements of the point's track once per
// point (the chain walk is a chase of dependent HBM loads, and the Gauss-Newton rounds would repeat it); longer tracks continue in HBM from where
// the cache ends.  Same order of accumulation, same bits.
#ifndef VS_LM_CN
#define VS_LM_CN 6
#endif
#define VS_LM_NP 48   // world_to_camera of the last VS_LM_NP frames staged in LDS (one copy for all points of the frame)
// The trail addresses measurements 0 .. VS_TRAIL of a track directly; everything older goes through the ring's `prev` links and reads the ring.
// The directly addressed part therefore never leaves the staged window (nor, in a team, the lanes' measurement slots: see landmark_team).
static_assert(VS_TRAIL + 1 <= VS_LM_NP, "the directly addressed measurements must lie inside the staged pose window");
struct LmCache { double w2c[VS_LM_NP][12]; double rtr[VS_LM_NP][9]; double cam[VS_WG][VS_LM_CN][4]; };
// Long tracks go to a team of eight lanes (landmark_team).
#define VS_LM_TEAM_G LM_TEAM_G  // lanes per team
#ifndef VS_LM_TEAM_WAVES
#define VS_LM_TEAM_WAVES 2      // wavefronts of the workgroup that run teams when the frame has long tracks (16 teams at a time)
#endif
#ifndef VS_LM_TEAM_MIN
#define VS_LM_TEAM_MIN 9        // measurements from which a track goes to a team
#endif
#define VS_LM_TEAM_LDS (VS_LM_TEAM_WAVES * (64 / VS_LM_TEAM_G) * VS_LM_TEAM_G * (int)sizeof(LmTerm))

// The poses of the last VS_LM_NP frames and their R^T R (J^T J of every measurement taken in that frame: a property of the frame) into the
// cache, by the whole workgroup; the caller synchronises before the cache is read.
__device__ __forceinline__ void lm_stage_poses(const DevCfg& c, const DevBuf& b, int s, int f, LmCache* lc) {
  for (int t = threadIdx.x; t < VS_LM_NP * 12; t += VS_WG) { const int k = t / 12; if (f - k >= 0 && k < c.HCAP) lc->w2c[k][t - 12 * k] = hpose_of(c, b, s, f - k)[12 + t - 12 * k]; }
  __syncthreads();
  for (int t = threadIdx.x; t < VS_LM_NP * 9; t += VS_WG) { const int k = t / 9; if (f - k >= 0 && k < c.HCAP) lc->rtr[k][t - 9 * k] = lm_rtr_entry(lc->w2c[k], t - 9 * k); }
}
// Sum of the world coordinates along the track of point i of frame f, newest first, at most len points; returns how many the track had.
__device__ __forceinline__ int lm_chain_sum(const DevCfg& c, const DevBuf& b, int s, int f, int i, int len, double* acc) {
  acc[0] = acc[1] = acc[2] = 0;
  int k = 0;
  while (k < len) {
    double wp[3];
    tf_apply(hpose_of(c, b, s, f), hcam_of(c, b, s, f) + 4 * (size_t)i, wp);
    for (int q = 0; q < 3; ++q) acc[q] += wp[q];
    i = hprev_of(c, b, s, f)[i];
    --f; ++k;
    if (i < 0) break;
  }
  return k;
}
// Measurement k of the track (frame f - k): index i for k = 0, the trail's entry k - 1 up to k = VS_TRAIL, then the `prev` links of the history
// ring.  Returns n_direct = measurements addressed without a link walk; a 0xFFFF entry (the track starts there: `ended`) ends the list like a
// negative `prev` link does.
__device__ __forceinline__ int lm_trail_scan(const uint16_t* tr, int len, bool& ended) {
  int n_direct = 1;
  const int want = min(len, VS_TRAIL + 1);
  for (int q0 = 0; q0 < VS_TRAIL && n_direct < want && !ended; q0 += 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(tr + q0);
    const uint32_t wv4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const uint32_t ent = (wv4[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
      if (!ended && n_direct < want) { if (ent == 0xFFFFu) ended = true; else ++n_direct; }
    }
  }
  return n_direct;
}
__device__ __forceinline__ int lm_index_at(const uint16_t* tr, int i, int k) { return k == 0 ? i : (int)tr[k - 1]; }   // k < n_direct
// where the link walk continues after the directly addressed measurements (only tracks longer than VS_TRAIL + 1): frame ff, index ii
__device__ __forceinline__ void lm_walk_from(const DevCfg& c, const DevBuf& b, int s, int f, int i, const uint16_t* tr, int n_direct, int len, int& ff, int& ii, bool& ended) {
  if (!ended && n_direct < len) { ff = f - (n_direct - 1); ii = hprev_of(c, b, s, ff)[lm_index_at(tr, i, n_direct - 1)]; --ff; if (ii < 0) ended = true; }
  else ended = true;
}
// measurements k .. len - 1 along the `prev` links from (ff, ii): poses and measurements from the ring
__device__ __forceinline__ void lm_walk(const DevCfg& c, const DevBuf& b, int s, int ff, int ii, int k, int len, const double* wv, double kern, double* H, double* bv, double& err, int& n_out) {
  for (; k < len; ++k) {
    lm_add_unstaged(hpose_of(c, b, s, ff) + 12, hcam_of(c, b, s, ff) + 4 * (size_t)ii, wv, kern, H, bv, err, n_out);
    ii = hprev_of(c, b, s, ff)[ii];
    --ff;
    if (ii < 0) break;
  }
}

// Framepoint i of the current frame on one lane: staged slots for its first VS_LM_CN measurements, four loads in flight beyond them.  Returns
// true when the point carries an active landmark afterwards.
__device__ __forceinline__ bool landmark_point(const DevCfg& c, const DevBuf& b, int s, const PtView& cv, int f, int i, LmCache* lc) {
  int32_t* m = cv.meta + (size_t)i * META;
  const int tlen = m[M_TLEN];
  if (tlen < c.c.minimum_track_length_for_landmark_creation) return false;
  const int lmup0 = m[M_LMUP];
  int len = tlen + 1;
  if (len > c.HCAP) { len = c.HCAP; atomicOr(&b.st[s].error_flags, 4); }
  double wpos[3];
  if (lmup0 == 0) {
    // Landmark::Landmark: average of the world coordinates along the track, which may be shorter than its length says
    double acc[3];
    len = lm_chain_sum(c, b, s, f, i, len, acc);
    for (int q = 0; q < 3; ++q) wpos[q] = acc[q] / (double)len;
    m[M_LMUP] = len;
  } else {
    // Landmark::update
    double wv[3] = {cv.lm[3 * (size_t)i], cv.lm[3 * (size_t)i + 1], cv.lm[3 * (size_t)i + 2]};
    for (int q = 0; q < 3; ++q) wpos[q] = wv[q];
    double err_prev = 0;
    const double kern = c.c.landmark_maximum_error_squared_meters;
    const uint16_t* tr = cv.trail + (size_t)i * VS_TRAIL;
    bool ended = false;
    const int n_direct = c.trail ? lm_trail_scan(tr, len, ended) : 1;
    // the first VS_LM_CN measurements into the thread's LDS slots, once
    int ncache = 0, ffc = f, iic = i;
    double (*slot)[4] = lc->cam[threadIdx.x];
    if (c.trail) {
      const int nc = min(min(len, VS_LM_CN), n_direct);
      double mv[VS_LM_CN][4];
#pragma unroll
      for (int k = 0; k < VS_LM_CN; ++k)
        if (k < nc) { const double* mc = hcam_of(c, b, s, f - k) + 4 * (size_t)lm_index_at(tr, i, k); mv[k][0] = mc[0]; mv[k][1] = mc[1]; mv[k][2] = mc[2]; mv[k][3] = mc[3]; }
#pragma unroll
      for (int k = 0; k < VS_LM_CN; ++k)
        if (k < nc) { slot[k][0] = mv[k][0]; slot[k][1] = mv[k][1]; slot[k][2] = mv[k][2]; slot[k][3] = mv[k][3]; }
      ncache = nc;
      lm_walk_from(c, b, s, f, i, tr, n_direct, len, ffc, iic, ended);
    } else {
      for (int k = 0; k < len && k < VS_LM_CN; ++k) {
        const double* mc = hcam_of(c, b, s, ffc) + 4 * (size_t)iic;
        slot[k][0] = mc[0]; slot[k][1] = mc[1]; slot[k][2] = mc[2]; slot[k][3] = mc[3];
        ++ncache;
        iic = hprev_of(c, b, s, ffc)[iic];
        --ffc;
        if (iic < 0) { ended = true; break; }
      }
    }
    for (int it = 0; it < c.c.landmark_maximum_number_of_iterations; ++it) {
      double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0};
      double err = 0;
      int n_out = 0;
      for (int k = 0; k < ncache; ++k) lm_add(lm_term(lc->w2c[k], lc->rtr[k], slot[k], wv, kern), H, bv, err, n_out);   // frame f - k
      if (c.trail) {
        // directly addressed measurements, four at a time: their (independent) loads are in flight together
        constexpr int NB = 4;     // loads in flight together
        for (int k0 = ncache; k0 < n_direct; k0 += NB) {
          double mc[NB][4];
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int k = min(k0 + u, n_direct - 1);
            const double* src = hcam_of(c, b, s, f - k) + 4 * (size_t)lm_index_at(tr, i, k);
            mc[u][0] = src[0]; mc[u][1] = src[1]; mc[u][2] = src[2]; mc[u][3] = src[3];
          }
#pragma unroll
          for (int u = 0; u < NB; ++u) {
            const int k = k0 + u;
            if (k < n_direct) lm_add(lm_term(lc->w2c[k], lc->rtr[k], mc[u], wv, kern), H, bv, err, n_out);   // k < n_direct <= VS_TRAIL + 1: inside the staged window
          }
        }
      }
      if (!ended) lm_walk(c, b, s, ffc, iic, c.trail ? n_direct : ncache, len, wv, kern, H, bv, err, n_out);
      int n_in;
      const LmRound end = lm_round_end(H, bv, wv, err, err_prev, it, len, n_out, lmup0, n_in);
      if (end == LM_ACCEPT) {
        for (int q = 0; q < 3; ++q) wpos[q] = wv[q];
        m[M_LMUP] = n_in;
      } else if (end == LM_RESET) {
        double acc[3];
        lm_chain_sum(c, b, s, f, i, len, acc);
        for (int q = 0; q < 3; ++q) wpos[q] = acc[q] / (double)len;
      }
      if (end != LM_NEXT_ROUND) break;
      err_prev = err;
    }
  }
  for (int q = 0; q < 3; ++q) cv.lm[3 * (size_t)i + q] = wpos[q];
  tf_apply(hpose_of(c, b, s, f) + 12, wpos, cv.camlm + 3 * (size_t)i);
  return true;
}

// Landmark::update of a LONG track by a team of eight lanes.  One lane per landmark walks a chain of ~65 dependent fp64 operations per
// measurement and round; the longest track of the frame (dozens of measurements, three rounds) kept the phase waiting for one wavefront.
// Only the thirteen ADDITIONS into H, b and the error have to happen in the list's order: the eight lanes evaluate eight consecutive
// measurements at once (lm_term), park the terms in LDS, and every lane adds the eight terms in list order into its own copy of the sums
// (lm_team_add) — the same operations on the same operands in the same order as landmark_point's serial loop, an eighth of the
// multiplications on the critical path.  Measurements beyond the trail (k >= n_direct: only reachable through the `prev` links) follow
// serially on every lane alike.
// classification used by the work lists: an update (not a creation) of a track with VS_LM_TEAM_MIN or more measurements
__device__ __forceinline__ bool landmark_is_long(const DevCfg& c, const int32_t* m) {
  return m[M_LMUP] != 0 && min(m[M_TLEN] + 1, c.HCAP) >= VS_LM_TEAM_MIN && c.trail;
}
__device__ __forceinline__ void landmark_team(const DevCfg& c, const DevBuf& b, int s, const PtView& cv, int f, int i, LmCache* lc, LmTerm* terms, int gl) {
  int32_t* m = cv.meta + (size_t)i * META;
  const int lmup0 = m[M_LMUP];
  int len = m[M_TLEN] + 1;
  if (len > c.HCAP) { len = c.HCAP; if (gl == 0) atomicOr(&b.st[s].error_flags, 4); }
  double wpos[3];
  double wv[3] = {cv.lm[3 * (size_t)i], cv.lm[3 * (size_t)i + 1], cv.lm[3 * (size_t)i + 2]};
  for (int q = 0; q < 3; ++q) wpos[q] = wv[q];
  const double kern = c.c.landmark_maximum_error_squared_meters;
  const uint16_t* tr = cv.trail + (size_t)i * VS_TRAIL;
  bool ended = false;
  const int n_direct = lm_trail_scan(tr, len, ended);
  // this lane's measurements of the directly addressed part (k = gl, gl + 8, ...) into its LDS slots, all loads in flight, once
  constexpr int NG = VS_LM_CN;                       // groups whose measurements have a slot (k < 8 * NG)
  static_assert(VS_TRAIL + 1 <= VS_LM_TEAM_G * NG, "every directly addressed measurement needs a slot");
  double (*slot)[4] = lc->cam[threadIdx.x];
  {
    double mv[NG][4];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int k = VS_LM_TEAM_G * g + gl;
      if (k < n_direct) {
        const double* mc = hcam_of(c, b, s, f - k) + 4 * (size_t)lm_index_at(tr, i, k);
        mv[g][0] = mc[0]; mv[g][1] = mc[1]; mv[g][2] = mc[2]; mv[g][3] = mc[3];
      }
    }
#pragma unroll
    for (int g = 0; g < NG; ++g)
      if (VS_LM_TEAM_G * g + gl < n_direct) { slot[g][0] = mv[g][0]; slot[g][1] = mv[g][1]; slot[g][2] = mv[g][2]; slot[g][3] = mv[g][3]; }
  }
  int ffc = f, iic = i;
  lm_walk_from(c, b, s, f, i, tr, n_direct, len, ffc, iic, ended);
  double err_prev = 0;
  for (int it = 0; it < c.c.landmark_maximum_number_of_iterations; ++it) {
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bv[3] = {0, 0, 0};
    double err = 0;
    int n_out = 0;
    for (int k0 = 0; k0 < n_direct; k0 += VS_LM_TEAM_G) {
      const int k = k0 + gl;
      LmTerm t;
      t.kind = -1;
      if (k < n_direct) {
        double mc[4];
        const int g = k0 / VS_LM_TEAM_G;
        mc[0] = slot[g][0]; mc[1] = slot[g][1]; mc[2] = slot[g][2]; mc[3] = slot[g][3];      // k < n_direct: every directly addressed measurement has a slot
        t = lm_term(lc->w2c[k], lc->rtr[k], mc, wv, kern);                                    // ... and its frame lies inside the staged window
      }
      lm_team_add(terms, gl, t, min(VS_LM_TEAM_G, n_direct - k0), H, bv, err, n_out);
    }
    if (!ended) lm_walk(c, b, s, ffc, iic, n_direct, len, wv, kern, H, bv, err, n_out);
    int n_in;
    const LmRound end = lm_round_end(H, bv, wv, err, err_prev, it, len, n_out, lmup0, n_in);
    if (end == LM_ACCEPT) {
      for (int q = 0; q < 3; ++q) wpos[q] = wv[q];
      if (gl == 0) m[M_LMUP] = n_in;
    } else if (end == LM_RESET) {
      double acc[3];
      lm_chain_sum(c, b, s, f, i, len, acc);
      for (int q = 0; q < 3; ++q) wpos[q] = acc[q] / (double)len;
    }
    if (end != LM_NEXT_ROUND) break;
    err_prev = err;
  }
  if (gl == 0) {
    for (int q = 0; q < 3; ++q) cv.lm[3 * (size_t)i + q] = wpos[q];
    tf_apply(hpose_of(c, b, s, f) + 12, wpos, cv.camlm + 3 * (size_t)i);
  }
}

// The active landmarks of a frame counted without refining them, for the callers whose refinement runs BESIDE them in the same launch (k_tail_lm,
// k_stage_lm): a point is active iff its track is long enough for a landmark.  Called by the whole workgroup; returns this thread's share.
// A track that outgrew the history ring raises error bit 4 here as well: the refinement's own atomicOr (landmark_point / landmark_team) is not
// ordered against the report its neighbour workgroup writes, and the frame that truncates first must show the bit under every launch sequence.
__device__ __forceinline__ int lm_count_active(const DevCfg& c, const DevBuf& b, int s, const PtView& cvc, int n_cur) {
  int active = 0, cut = 0;
  for (int i = threadIdx.x; i < n_cur; i += VS_WG) {
    const int tlen = cvc.meta[(size_t)i * META + M_TLEN];
    if (tlen >= c.c.minimum_track_length_for_landmark_creation) { ++active; cut |= tlen + 1 > c.HCAP ? 1 : 0; }
  }
  cut = __syncthreads_or(cut);
  if (cut && threadIdx.x == 0) atomicOr(&b.st[s].error_flags, 4);
  return active;
}

// Besides the history ring (camera coordinates and `prev` link of every point of frame f), every point gets its trail: the
// indices of its track's points in frames f-1 .. f-VS_TRAIL (its predecessor, then the predecessor's own trail shifted by one;
// 0xFFFF where the track starts before that).  The landmark refinement then addresses its measurements directly instead of
// walking the links, a chain of dependent HBM loads per measurement.
__device__ __forceinline__ void wg_publish_history(const DevCfg& c, const DevBuf& b, int s, int n, int pb_cur, int f) {
  const PtView cv = pts_of(c, b, s, pb_cur);
  const PtView pv = pts_of(c, b, s, pb_cur ^ 1);
  double* hc = hcam_of(c, b, s, f);
  int32_t* hp = hprev_of(c, b, s, f);
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    { const double x = cv.cam[3 * (size_t)i], y = cv.cam[3 * (size_t)i + 1], z = cv.cam[3 * (size_t)i + 2];
      reinterpret_cast<double2*>(hc + 4 * (size_t)i)[0] = make_double2(x, y); reinterpret_cast<double2*>(hc + 4 * (size_t)i)[1] = make_double2(z, 1 / z); }   // Measurement::inverse_depth_meters
    const int ip = cv.meta[(size_t)i * META + M_PREV];
    hp[i] = ip;
    if (c.trail) {
      uint4* dst = reinterpret_cast<uint4*>(cv.trail + (size_t)i * VS_TRAIL);
      if (ip < 0) {
        dst[0] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);   // only entry 0 is ever reached: len = 1
      } else {
        const uint4* src = reinterpret_cast<const uint4*>(pv.trail + (size_t)ip * VS_TRAIL);
        uint32_t w[VS_TRAIL / 2];
#pragma unroll
        for (int q = 0; q < VS_TRAIL / 8; ++q) { const uint4 v = src[q]; w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w; }
        uint32_t o[VS_TRAIL / 2];
        o[0] = (uint32_t)ip | (w[0] << 16);
#pragma unroll
        for (int q = 1; q < VS_TRAIL / 2; ++q) o[q] = (w[q - 1] >> 16) | (w[q] << 16);
#pragma unroll
        for (int q = 0; q < VS_TRAIL / 8; ++q) dst[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
      }
    }
  }
}

// Share g of G of the landmark creation / refinement of frame f's n_cur points by one workgroup: the poses of the last VS_LM_NP frames and
// every lane's first measurements staged in the LDS arena, short tracks one lane each, long tracks a team of eight lanes.  The share is the
// points i with i % G == g (the lists' order depends on the order of the atomics: a share must not be defined through it); a frame too large
// for the lists is handed out lane by lane, without teams.  n_short / n_long_sh: two counters in LDS.  adapt_team_waves: only as many
// wavefronts run teams as the share's long tracks fill, the others take short tracks (otherwise always VS_LM_TEAM_WAVES).  Returns this
// thread's number of active landmarks; history of frame f must have been published (wg_publish_history).
__device__ __forceinline__ int lm_refine_share(const DevCfg& c, const DevBuf& b, int s, const PtView& cvu, int n_cur, int f, int g, int G, unsigned char* arena,
                                               int& n_short, int& n_long_sh, bool adapt_team_waves) {
  const int tid = threadIdx.x;
  int active = 0;
  static_assert(sizeof(LmCache) + VS_LM_TEAM_LDS + 4096 <= VS_ARENA, "landmark cache + team terms must leave room for the work lists");
  constexpr int LIST_CAP = (VS_ARENA - (int)sizeof(LmCache) - VS_LM_TEAM_LDS) / 2;
  LmCache* lc = reinterpret_cast<LmCache*>(arena);
  LmTerm* team_terms = reinterpret_cast<LmTerm*>(arena + VS_ARENA - VS_LM_TEAM_LDS);
  uint16_t* work = reinterpret_cast<uint16_t*>(arena + sizeof(LmCache));
  lm_stage_poses(c, b, s, f, lc);
  if (tid == 0) { n_short = 0; n_long_sh = 0; }
  __syncthreads();
  if (n_cur <= LIST_CAP && n_cur <= 65535) {
    // The points that carry a landmark (track long enough: creation or refinement) are compacted into work lists first: ~40 % of the frame's
    // points, one per thread in a single round instead of two half-empty ones (a thread's refinement is a serial chain).  Short tracks from
    // the front of the list, long ones from its end.
    for (int i0 = 0; i0 < n_cur; i0 += VS_WG) {
      const int i = i0 + tid;
      const int32_t* mi = cvu.meta + (size_t)min(i, n_cur - 1) * META;
      const bool need = i < n_cur && (i % G) == g && mi[M_TLEN] >= c.c.minimum_track_length_for_landmark_creation;
      const bool lng = need && landmark_is_long(c, mi);
      const unsigned long long m = __ballot(need && !lng), ml = __ballot(lng);
      int base = 0, basel = 0;
      if ((tid & 63) == 0 && m) base = atomicAdd(&n_short, __popcll(m));
      if ((tid & 63) == 0 && ml) basel = atomicAdd(&n_long_sh, __popcll(ml));
      base = __builtin_amdgcn_readfirstlane(base); basel = __builtin_amdgcn_readfirstlane(basel);
      if (need && !lng) work[base + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))] = (uint16_t)i;
      if (lng) work[LIST_CAP - 1 - (basel + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(ml >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ml, 0u)))] = (uint16_t)i;
    }
    __syncthreads();
    const int n_work = n_short, n_long = n_long_sh;
    constexpr int WT = 64 / VS_LM_TEAM_G;      // teams of a wavefront
    const int team_waves = adapt_team_waves ? min(VS_LM_TEAM_WAVES, (n_long + WT - 1) / WT) : VS_LM_TEAM_WAVES;
    if ((tid >> 6) < team_waves) {
      const int team = tid / VS_LM_TEAM_G, gl = tid % VS_LM_TEAM_G;
      for (int q = team; q < n_long; q += team_waves * WT) {
        landmark_team(c, b, s, cvu, f, work[LIST_CAP - 1 - q], lc, team_terms + team * VS_LM_TEAM_G, gl);
        active += gl == 0 ? 1 : 0;
      }
    } else {
      for (int q = tid - 64 * team_waves; q < n_work; q += VS_WG - 64 * team_waves) active += landmark_point(c, b, s, cvu, f, work[q], lc) ? 1 : 0;
    }
  } else {
    for (int i = g * VS_WG + tid; i < n_cur; i += G * VS_WG) active += landmark_point(c, b, s, cvu, f, i, lc) ? 1 : 0;
  }
  return active;
}

// The whole frame in the stream's own workgroup (PoseTracker3D::_updatePoints' landmark part); returns the number of active landmarks
// (block-uniform).  Used by k_frame's fused launches and by the stage path's UPDATE / COMPUTE stages.
__device__ __forceinline__ int wg_landmarks_lds(const DevCfg& c, const DevBuf& b, int s, FrameShared& sh, int pb_cur, int f, unsigned char* arena) {
  // sh.n_proj (recovery is over): the count of long tracks
  const int active = lm_refine_share(c, b, s, pts_of(c, b, s, pb_cur), sh.n_cur, f, 0, 1, arena, sh.flag, sh.n_proj, true);
  int total;
  block_exclusive_scan(active, sh.scan, &total);
  __syncthreads();
  if (threadIdx.x == 0) sh.flag = 0;
  __syncthreads();
  return total;
}

__device__ __forceinline__ void wg_update_points(const DevCfg& c, const DevBuf& b, int s, FrameShared& sh, int pb_cur, int f, unsigned char* arena) {
  // publish the current frame's cam/prev to the history ring first (chains start here)
  wg_publish_history(c, b, s, sh.n_cur, pb_cur, f);
  __syncthreads();
  const int total = wg_landmarks_lds(c, b, s, sh, pb_cur, f, arena);     // the fused launch's refinement (LDS-cached, teams): 31 us per KITTI-sized frame where one thread per track took 80
  if (threadIdx.x == 0) sh.n_lm = total;  // _number_of_active_landmarks
  __syncthreads();
}

// The same refinement spread over G workgroups per stream, each with the frame workgroup's own machinery, i.e. the operations of k_frame's
// landmark phase in the same order: launch sequence 4 (k_tail_lm) and the stage path of a one-stream context (k_stage_lm) run it beside the
// frame's last phase / stage, inside the same launch, where a wide one-thread-per-track kernel (56 us for one KITTI-sized stream) would be longer
// than what it hides behind.  The share-0 workgroup adds its duration to the stream's landmark chronometer (neither caller is timed by HIP events).
__device__ __forceinline__ void lm_teams_body(const DevCfg& c, const DevBuf& b, int s, int g, int G, unsigned char* arena, int& n_short, int& n_long_sh) {
  const unsigned long long t_begin = wall_clock64();
  StreamState& st = b.st[s];
  lm_refine_share(c, b, s, pts_of(c, b, s, st.fc.lm_pb), st.fc.n_cur, st.fc.lm_f, g, G, arena, n_short, n_long_sh, false);
  if (g == 0 && threadIdx.x == 0) st.ticks[3] += wall_clock64() - t_begin;
}
