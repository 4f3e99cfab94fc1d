// kernels_recover.h — what the frame does with the previous frame's points once the pose is known: prune (the surviving tracked points become the
// current frame's first points) and recovery of the lost ones (projection, descriptors at the projections, append).
#pragma once
#include "kernels_frame.h"

// write one framepoint (Frame::createFramepoint, types/frame.cpp:61-84) from a left/right feature pair
__device__ __forceinline__ void materialize_point(const DevCfg& c, const DevBuf& b, int s, const PtView& cv, int j, int fl,
                                                  int fr, int dist, int epi, int prev, int tlen) {
  const int16_t* kxyL = kpxy_of(c, b, s, 0);
  const int16_t* kxyR = kpxy_of(c, b, s, 1);
  const int xL = kxyL[2 * fl], yL = kxyL[2 * fl + 1], xR = kxyR[2 * fr], yR = kxyR[2 * fr + 1];
  cv.kp[4 * (size_t)j] = (int16_t)xL; cv.kp[4 * (size_t)j + 1] = (int16_t)yL;
  cv.kp[4 * (size_t)j + 2] = (int16_t)xR; cv.kp[4 * (size_t)j + 3] = (int16_t)yR;
  // the record moves in 16-byte pieces (descriptors) and 8-byte pieces (meta: 24 bytes a point): a quarter of the memory instructions
  const uint4* dl = reinterpret_cast<const uint4*>(desc_of(c, b, s, 0) + (size_t)32 * fl);
  const uint4* dr = reinterpret_cast<const uint4*>(desc_of(c, b, s, 1) + (size_t)32 * fr);
  uint4* o = reinterpret_cast<uint4*>(cv.desc + (size_t)64 * j);
  const uint4 l0 = dl[0], l1 = dl[1], r0 = dr[0], r1 = dr[1];
  o[0] = l0; o[1] = l1; o[2] = r0; o[3] = r1;
  static_assert(META == 6 && M_DIST == 0 && M_EPI == 1 && M_PREV == 2 && M_TLEN == 3 && M_LMUP == 4 && M_NEXT == 5, "meta is written as three pairs");
  int2* m = reinterpret_cast<int2*>(cv.meta + (size_t)j * META);
  m[0] = make_int2(dist, epi); m[1] = make_int2(prev, tlen); m[2] = make_int2(0, 0);
  triangulate(c, xL, yL, xR, yR, cv.cam + 3 * (size_t)j);
  for (int k = 0; k < 3; ++k) { cv.camlm[3 * (size_t)j + k] = 0; cv.lm[3 * (size_t)j + k] = 0; }
}

// _prunePoints (pose_tracker_3d.cpp:437-472) fused with the materialisation of the surviving tracked
// points into the current frame's point arrays.  Quirk B.3: aligner not run on these points -> drop all.
__device__ __forceinline__ void wg_prune(const DevCfg& c, const DevBuf& b, int s, FrameShared& sh, int pb_prev, int pb_cur, bool aligner_valid) {
  const int tid = threadIdx.x;
  const int n = sh.n_trk;
  const PtView pv = pts_of(c, b, s, pb_prev);
  const PtView cv = pts_of(c, b, s, pb_cur);
  const int32_t* trk = b.trk + (size_t)s * c.MAXP * 4;
  const double* chi = b.al_chi + (size_t)s * c.MAXP;
  const uint8_t* inl = b.al_inl + (size_t)s * c.MAXP;
  const int16_t* kxyL = kpxy_of(c, b, s, 0);
  const int16_t* kxyR = kpxy_of(c, b, s, 1);
  const bool by_inlier = aligner_valid && (sh.E / (double)n < c.c.aligner_maximum_error_kernel);
  const int per = (n + VS_WG - 1) / VS_WG;
  const int u0 = tid * per, u1 = min(u0 + per, n);
  int cnt = 0;
  for (int u = u0; u < u1; ++u) {
    bool keep = false;
    if (aligner_valid) keep = by_inlier ? (inl[u] != 0) : (chi[u] != -1 && chi[u] < 100 * c.c.aligner_maximum_error_kernel);
    if (keep) ++cnt;
  }
  int total;
  int off = block_exclusive_scan(cnt, sh.scan, &total);
  for (int u = u0; u < u1; ++u) {
    bool keep = false;
    if (aligner_valid) keep = by_inlier ? (inl[u] != 0) : (chi[u] != -1 && chi[u] < 100 * c.c.aligner_maximum_error_kernel);
    const int ip = trk[4 * u];
    if (keep) {
      const int fl = trk[4 * u + 1], fr = trk[4 * u + 2];
      materialize_point(c, b, s, cv, off, fl, fr, trk[4 * u + 3], kxyR[2 * fr + 1] - kxyL[2 * fl + 1], ip,
                        pv.meta[(size_t)ip * META + M_TLEN] + 1);
      // the landmark travels with the track (origin()->landmark())
      cv.meta[(size_t)off * META + M_LMUP] = pv.meta[(size_t)ip * META + M_LMUP];
      for (int k = 0; k < 3; ++k) cv.lm[3 * (size_t)off + k] = pv.lm[3 * (size_t)ip + k];
      ++off;
    } else {
      pv.meta[(size_t)ip * META + M_NEXT] = 0;  // FramePoint::clear unlinks previous->next
    }
  }
  if (tid == 0) sh.n_cur = min(total, c.MAXP);
  __syncthreads();
}

// recoverPoints (stereo_framepoint_generator.cpp:683-869) in three steps:
//   project : one thread per lost point: landmark -> both image planes, depth and border gates (:704-764)
//   brief   : one wavefront per surviving point: BRIEF at both projections from the box images, the three
//             descriptor gates and the disparity gate (:773-842).  Runs inside the workgroup (stage path) or as
//             the wide kernel k_recover_brief over all streams (fused path).
//   append  : survivors are appended in lost-list order (:844-864)
// rec[6q] : 0 = rejected, 2 = projected (needs BRIEF), 1 = recovered; then xL, yL, xR, yR, Hamming L-R
// `list` (LDS, optional): compact work list of the projected points for the in-workgroup BRIEF step — 6 ints per entry
// (q, previous point, xL, yL, xR, yR), count in *n_list — so that step does not chase rec[] through HBM point by point.
__device__ __forceinline__ void wg_recover_project(const DevCfg& c, const DevBuf& b, int s, int n_lost, int pb_prev, const double* w2c,
                                                   int32_t* list = nullptr, int list_cap = 0, int* n_list = nullptr) {
  const PtView pv = pts_of(c, b, s, pb_prev);
  const int32_t* lost = b.lost + (size_t)s * c.MAXP;
  int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
  for (int q = threadIdx.x; q < n_lost; q += blockDim.x) {
    const int ip = lost[q];
    int ok = pv.meta[(size_t)ip * META + M_LMUP] > 0 ? 2 : 0;
    int xL = 0, yL = 0, xR = 0, yR = 0;
    if (ok) {
      double pc[3], uL[3], uR[3];
      tf_apply(w2c, pv.lm + 3 * (size_t)ip, pc);
      mat3_mul_vec(c.c.K, pc, uL);
      for (int k = 0; k < 3; ++k) uR[k] = uL[k] + c.c.baseline_h[k];
      if (uL[2] < c.c.minimum_depth_meters || uL[2] > c.c.maximum_depth_meters || uR[2] < c.c.minimum_depth_meters ||
          uR[2] > c.c.maximum_depth_meters) ok = 0;
      if (ok) {
        const float pLx = (float)rint(uL[0] / uL[2]), pLy = (float)rint(uL[1] / uL[2]);
        const float pRx = (float)rint(uR[0] / uR[2]), pRy = (float)rint(uR[1] / uR[2]);
        const float border = 35.f;  // 5 * keypoint.size (FAST: 7)
        if (pLx < border + 1 || pLx > c.c.cols - border - 1 || pRx < border + 1 || pRx > c.c.cols - border - 1 ||
            pLy < border + 1 || pLy > c.c.rows - border - 1 || pRy < border + 1 || pRy > c.c.rows - border - 1) ok = 0;
        xL = (int)pLx; yL = (int)pLy; xR = (int)pRx; yR = (int)pRy;
      }
    }
    rec[6 * q] = ok; rec[6 * q + 1] = xL; rec[6 * q + 2] = yL; rec[6 * q + 3] = xR; rec[6 * q + 4] = yR; rec[6 * q + 5] = 0;
    if (ok && list) {
      const int k = atomicAdd(n_list, 1);
      if (k < list_cap) { int32_t* e = list + 6 * k; e[0] = q; e[1] = ip; e[2] = xL; e[3] = yL; e[4] = xR; e[5] = yR; }
    }
  }
}

__device__ __forceinline__ void recover_brief_wave(const DevCfg& c, const DevBuf& b, int s, int pb_prev, int q, int lane,
                                                   double tau_track, double tau_tri) {
  int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
  if (rec[6 * q] != 2) return;   // wave-uniform
  const PtView pv = pts_of(c, b, s, pb_prev);
  const int ip = (b.lost + (size_t)s * c.MAXP)[q];
  const int xL = rec[6 * q + 1], yL = rec[6 * q + 2], xR = rec[6 * q + 3], yR = rec[6 * q + 4];
  const uint16_t* boxL = box_of(c, b, s, 0);
  const uint16_t* boxR = box_of(c, b, s, 1);
  // both descriptors in (uniform) registers: the 16 box gathers of a lane are issued together, then 8 ballots
  int aL[4], bL[4], aR[4], bR[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = j * 64 + lane;
    aL[j] = boxL[(size_t)(yL + c_brief[i][0]) * c.bstride + (xL + c_brief[i][1])];
    bL[j] = boxL[(size_t)(yL + c_brief[i][2]) * c.bstride + (xL + c_brief[i][3])];
    aR[j] = boxR[(size_t)(yR + c_brief[i][0]) * c.bstride + (xR + c_brief[i][1])];
    bR[j] = boxR[(size_t)(yR + c_brief[i][2]) * c.bstride + (xR + c_brief[i][3])];
  }
  unsigned long long dL[4], dR[4];
  const unsigned long long* pd = reinterpret_cast<const unsigned long long*>(pv.desc + (size_t)64 * ip);
  int hL = 0, hR = 0, dist = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    dL[j] = __builtin_bswap64(__brevll(__ballot(aL[j] < bL[j])));
    dR[j] = __builtin_bswap64(__brevll(__ballot(aR[j] < bR[j])));
    hL += __popcll(dL[j] ^ pd[j]);
    hR += __popcll(dR[j] ^ pd[4 + j]);
    dist += __popcll(dL[j] ^ dR[j]);
  }
  int ok = 1;
  if ((double)hL > tau_track) ok = 0;
  if (ok && (double)((float)xL - (float)xR) < c.c.minimum_disparity_pixels) ok = 0;
  if (ok && (double)hR > tau_track) ok = 0;
  if (ok && (double)dist > tau_tri) ok = 0;
  if (lane == 0) {
    rec[6 * q] = ok; rec[6 * q + 5] = dist;
    if (ok) {
      unsigned long long* dl = reinterpret_cast<unsigned long long*>(b.rec_desc + ((size_t)s * c.MAXP + q) * 64);
#pragma unroll
      for (int j = 0; j < 4; ++j) { dl[j] = dL[j]; dl[4 + j] = dR[j]; }
    }
  }
}

// recoverPoints with the ORB extractor (descriptor_type 1): the steered tests of both projections straight from the
// Gaussian-blurred images (the extractor runs on the 71 x 71 region around the projection upstream,
// stereo_framepoint_generator.cpp:773-812; the pattern stays >= 14 px inside it, so the region's own border handling never
// reaches a tap).  Gates as in recover_brief_wave.
__device__ __forceinline__ void recover_orb_wave(const DevCfg& c, const DevBuf& b, int s, int pb_prev, int q, int ip, int xL, int yL, int xR, int yR,
                                                 int lane, double tau_track, double tau_tri, const OrbTaps& taps) {
  int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
  const PtView pv = pts_of(c, b, s, pb_prev);
  unsigned long long dL[4], dR[4];
  orb_wave(blur_of(c, b, s, 0) + (size_t)yL * c.bstride + xL, taps, dL);
  orb_wave(blur_of(c, b, s, 1) + (size_t)yR * c.bstride + xR, taps, dR);
  const unsigned long long* pd = reinterpret_cast<const unsigned long long*>(pv.desc + (size_t)64 * ip);
  int hL = 0, hR = 0, dist = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { hL += __popcll(dL[j] ^ pd[j]); hR += __popcll(dR[j] ^ pd[4 + j]); dist += __popcll(dL[j] ^ dR[j]); }
  int ok = 1;
  if ((double)hL > tau_track) ok = 0;
  if (ok && (double)((float)xL - (float)xR) < c.c.minimum_disparity_pixels) ok = 0;
  if (ok && (double)hR > tau_track) ok = 0;
  if (ok && (double)dist > tau_tri) ok = 0;
  if (lane == 0) {
    rec[6 * q] = ok; rec[6 * q + 5] = dist;
    if (ok) {
      unsigned long long* dl = reinterpret_cast<unsigned long long*>(b.rec_desc + ((size_t)s * c.MAXP + q) * 64);
#pragma unroll
      for (int j = 0; j < 4; ++j) { dl[j] = dL[j]; dl[4 + j] = dR[j]; }
    }
  }
}

// Same computation with the two 49 x 49 box patches staged in LDS by coalesced 16-byte row loads (7 lanes per row):
// the 1024 scattered 2-byte gathers per point of recover_brief_wave keep the CU's texture-address unit busy for ~1000
// cycles; a dozen wide loads at most take a fraction of that.  `patch` = this wavefront's LDS area, VS_RPATCH bytes.
// Only the chunks the loaded pattern samples are fetched (c_brief_fp, brief_footprint.h; with the built-in pattern 142 - 147 loads per
// side, by alignment, against the rectangle's 343): the phase is bound by the bytes a workgroup pulls through its CU's memory pipe, and
// the taps read nothing else.
#define VS_RP_W (8 * VS_FP_CPR)
#define VS_RP_H VS_FP_ROWS
#define VS_RPATCH (2 * VS_RP_H * VS_RP_W * 2)
#define VS_RP_NLD ((VS_FP_MAX_ITEMS + 63) / 64)   // 6: loads per lane and side when the pattern samples the whole rectangle
// a lane's share of the footprint's work list, items lane, lane + 64, ...: the same for every point, so it is fetched once per recovery
struct RecoverItems { uint32_t it[VS_RP_NLD]; };
__device__ __forceinline__ RecoverItems recover_items(int lane) {
  RecoverItems w;
#pragma unroll
  for (int u = 0; u < VS_RP_NLD; ++u) w.it[u] = lane + 64 * u < c_brief_fp.n_items ? c_brief_fp.item[lane + 64 * u] : VS_FP_NO_ITEM;
  return w;
}
__device__ __forceinline__ void recover_brief_patch(const DevCfg& c, const DevBuf& b, int s, int pb_prev, int q, int ip, int xL, int yL,
                                                    int xR, int yR, int lane, double tau_track, double tau_tri, uint16_t* patch,
                                                    const RecoverItems& w) {
  int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
  const PtView pv = pts_of(c, b, s, pb_prev);
  const int xy[2][2] = {{xL, yL}, {xR, yR}};
  uint4 v[2][VS_RP_NLD];
  int cx[2];
#pragma unroll
  for (int sd = 0; sd < 2; ++sd) {
    const int col0 = (xy[sd][0] - VSLAM_BRIEF_PATCH_HALF) & ~7;   // 16-byte aligned; the patch ends at col0 + 55 at most
    cx[sd] = xy[sd][0] - col0;
    const uint16_t* base = box_of(c, b, s, sd) + (size_t)(xy[sd][1] - VSLAM_BRIEF_PATCH_HALF) * c.bstride + col0;
#pragma unroll
    for (int u = 0; u < VS_RP_NLD; ++u) {
      const int row = brief_footprint_row(w.it[u]), seg = brief_footprint_chunk(w.it[u]);   // row < VS_RP_H, seg < VS_FP_CPR by construction
      v[sd][u] = make_uint4(0u, 0u, 0u, 0u);
      if (brief_footprint_needs(w.it[u], cx[sd] - VSLAM_BRIEF_PATCH_HALF)) v[sd][u] = *reinterpret_cast<const uint4*>(base + (size_t)row * c.bstride + 8 * seg);
    }
  }
  unsigned long long pd[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) pd[j] = reinterpret_cast<const unsigned long long*>(pv.desc + (size_t)64 * ip)[j];
#pragma unroll
  for (int sd = 0; sd < 2; ++sd)
#pragma unroll
    for (int u = 0; u < VS_RP_NLD; ++u) {
      const int row = brief_footprint_row(w.it[u]), seg = brief_footprint_chunk(w.it[u]);
      if (brief_footprint_needs(w.it[u], cx[sd] - VSLAM_BRIEF_PATCH_HALF)) *reinterpret_cast<uint4*>(patch + (sd * VS_RP_H + row) * VS_RP_W + 8 * seg) = v[sd][u];
    }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  unsigned long long dL[4], dR[4];
  int hL = 0, hR = 0, dist = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = j * 64 + lane;
    const int oa = (VSLAM_BRIEF_PATCH_HALF + c_brief[i][0]) * VS_RP_W + c_brief[i][1], ob = (VSLAM_BRIEF_PATCH_HALF + c_brief[i][2]) * VS_RP_W + c_brief[i][3];
    const uint16_t* pl = patch + cx[0];
    const uint16_t* pr = patch + VS_RP_H * VS_RP_W + cx[1];
    dL[j] = __builtin_bswap64(__brevll(__ballot(pl[oa] < pl[ob])));
    dR[j] = __builtin_bswap64(__brevll(__ballot(pr[oa] < pr[ob])));
    hL += __popcll(dL[j] ^ pd[j]);
    hR += __popcll(dR[j] ^ pd[4 + j]);
    dist += __popcll(dL[j] ^ dR[j]);
  }
  __builtin_amdgcn_wave_barrier();
  int ok = 1;
  if ((double)hL > tau_track) ok = 0;
  if (ok && (double)((float)xy[0][0] - (float)xy[1][0]) < c.c.minimum_disparity_pixels) ok = 0;
  if (ok && (double)hR > tau_track) ok = 0;
  if (ok && (double)dist > tau_tri) ok = 0;
  if (lane == 0) {
    rec[6 * q] = ok; rec[6 * q + 5] = dist;
    if (ok) {
      unsigned long long* dl = reinterpret_cast<unsigned long long*>(b.rec_desc + ((size_t)s * c.MAXP + q) * 64);
#pragma unroll
      for (int j = 0; j < 4; ++j) { dl[j] = dL[j]; dl[4 + j] = dR[j]; }
    }
  }
}

// in-workgroup BRIEF step: the LDS work list first, then (list overflow only) the remaining points through rec[]
#define VS_RLIST_OFF ((VS_WG / 64) * VS_RPATCH)
// builds whose LDS arena is too small for the patches (co-scheduling experiments: a frame workgroup that fits into the hole one
// image-kernel workgroup leaves) gather the 2 x 512 taps of a point straight from the box images instead, like k_recover_brief
#define VS_RPATCH_IN_LDS (VS_RLIST_OFF + 24 * 64 <= VS_ARENA)
#define VS_RLIST_CAP (VS_RPATCH_IN_LDS ? (VS_ARENA - VS_RLIST_OFF) / 24 : 0)
__device__ __forceinline__ void wg_recover_brief(const DevCfg& c, const DevBuf& b, int s, int pb_prev, int n_lost, int n_list,
                                                 double tau_track, double tau_tri, unsigned char* arena) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if constexpr (!VS_RPATCH_IN_LDS) {
    if (c.c.descriptor_type == VSLAM_DESCRIPTOR_ORB) {
      const OrbTaps taps = orb_taps(lane, c.orb_cos, c.orb_sin, c.bstride);
      const int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
      const int32_t* lost = b.lost + (size_t)s * c.MAXP;
      for (int q = w; q < n_lost; q += VS_WG / 64) {
        if (rec[6 * q] != 2) continue;   // wave-uniform
        recover_orb_wave(c, b, s, pb_prev, q, lost[q], rec[6 * q + 1], rec[6 * q + 2], rec[6 * q + 3], rec[6 * q + 4], lane, tau_track, tau_tri, taps);
      }
    } else {
      for (int q = w; q < n_lost; q += VS_WG / 64) recover_brief_wave(c, b, s, pb_prev, q, lane, tau_track, tau_tri);
    }
    return;
  }
  uint16_t* patch = reinterpret_cast<uint16_t*>(arena + (size_t)w * VS_RPATCH);
  const int32_t* list = reinterpret_cast<const int32_t*>(arena + VS_RLIST_OFF);
  if (c.c.descriptor_type == VSLAM_DESCRIPTOR_ORB) {
    const OrbTaps taps = orb_taps(lane, c.orb_cos, c.orb_sin, c.bstride);
    const int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
    const int32_t* lost = b.lost + (size_t)s * c.MAXP;
    for (int q = w; q < n_lost; q += VS_WG / 64) {
      if (rec[6 * q] != 2) continue;   // wave-uniform
      recover_orb_wave(c, b, s, pb_prev, q, lost[q], rec[6 * q + 1], rec[6 * q + 2], rec[6 * q + 3], rec[6 * q + 4], lane, tau_track, tau_tri, taps);
    }
    return;
  }
  const RecoverItems items = recover_items(lane);
  if (n_list <= VS_RLIST_CAP) {
    for (int k = w; k < n_list; k += VS_WG / 64) {
      const int32_t* e = list + 6 * k;
      recover_brief_patch(c, b, s, pb_prev, e[0], e[1], e[2], e[3], e[4], e[5], lane, tau_track, tau_tri, patch, items);
    }
  } else {
    const int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
    const int32_t* lost = b.lost + (size_t)s * c.MAXP;
    for (int q = w; q < n_lost; q += VS_WG / 64) {
      if (rec[6 * q] != 2) continue;   // wave-uniform
      recover_brief_patch(c, b, s, pb_prev, q, lost[q], rec[6 * q + 1], rec[6 * q + 2], rec[6 * q + 3], rec[6 * q + 4], lane, tau_track, tau_tri, patch, items);
    }
  }
}

__device__ __forceinline__ void wg_recover_append(const DevCfg& c, const DevBuf& b, int s, FrameShared& sh, int pb_prev, int pb_cur) {
  const int tid = threadIdx.x;
  const PtView pv = pts_of(c, b, s, pb_prev);
  const PtView cv = pts_of(c, b, s, pb_cur);
  const int32_t* lost = b.lost + (size_t)s * c.MAXP;
  const int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
  const uint8_t* rdesc = b.rec_desc + (size_t)s * c.MAXP * 64;
  const int nl = sh.n_lost;
  const int per = (nl + VS_WG - 1) / VS_WG;
  const int q0 = tid * per, q1 = min(q0 + per, nl);
  int cnt = 0;
  for (int q = q0; q < q1; ++q) cnt += rec[6 * q] == 1 ? 1 : 0;
  int total;
  int off = sh.n_cur + block_exclusive_scan(cnt, sh.scan, &total);
  for (int q = q0; q < q1; ++q) {
    if (rec[6 * q] != 1) continue;
    if (off < c.MAXP) {
      const int ip = lost[q], j = off;
      const int xL = rec[6 * q + 1], yL = rec[6 * q + 2], xR = rec[6 * q + 3], yR = rec[6 * q + 4];
      cv.kp[4 * (size_t)j] = (int16_t)xL; cv.kp[4 * (size_t)j + 1] = (int16_t)yL; cv.kp[4 * (size_t)j + 2] = (int16_t)xR; cv.kp[4 * (size_t)j + 3] = (int16_t)yR;
      const uint32_t* src = reinterpret_cast<const uint32_t*>(rdesc + (size_t)64 * q);
      uint32_t* dst = reinterpret_cast<uint32_t*>(cv.desc + (size_t)64 * j);
      for (int k = 0; k < 16; ++k) dst[k] = src[k];
      int32_t* m = cv.meta + (size_t)j * META;
      m[M_DIST] = rec[6 * q + 5]; m[M_EPI] = 0; m[M_PREV] = ip; m[M_TLEN] = pv.meta[(size_t)ip * META + M_TLEN] + 1;
      m[M_LMUP] = pv.meta[(size_t)ip * META + M_LMUP]; m[M_NEXT] = 0;
      triangulate(c, xL, yL, xR, yR, cv.cam + 3 * (size_t)j);
      for (int k = 0; k < 3; ++k) { cv.lm[3 * (size_t)j + k] = pv.lm[3 * (size_t)ip + k]; cv.camlm[3 * (size_t)j + k] = 0; }
      pv.meta[(size_t)ip * META + M_NEXT] = 1;
    } else {
      atomicOr(&b.st[s].error_flags, 2);
    }
    ++off;
  }
  __syncthreads();
  if (tid == 0) { sh.flag = total; sh.n_cur = min(sh.n_cur + total, c.MAXP); }
  __syncthreads();
}

// whole recovery inside one workgroup (stage path)
__device__ __forceinline__ void wg_recover(const DevCfg& c, const DevBuf& b, int s, FrameShared& sh, int pb_prev, int pb_cur, const double* w2c,
                           double tau_track, double tau_tri, unsigned char* arena) {
  if (threadIdx.x == 0) sh.n_proj = 0;
  __syncthreads();
  wg_recover_project(c, b, s, sh.n_lost, pb_prev, w2c, reinterpret_cast<int32_t*>(arena + VS_RLIST_OFF), VS_RLIST_CAP, &sh.n_proj);
  __syncthreads();
  wg_recover_brief(c, b, s, pb_prev, sh.n_lost, sh.n_proj, tau_track, tau_tri, arena);
  __syncthreads();
  wg_recover_append(c, b, s, sh, pb_prev, pb_cur);
}

// fused path: BRIEF of the projected lost points of ALL streams, one wavefront each
__global__ __launch_bounds__(256) void k_recover_brief(const DevCfg c, const DevBuf b) {
  int bx, sy;
  xcd_stream_block(&bx, &sy, b.xcd_rot);
  const int s = b.s0 + sy;
  if (!vs_active(b, s)) return;
  const StreamState& st = b.st[s];
  const int lane = threadIdx.x & 63;
  const int wave = bx * 4 + (threadIdx.x >> 6), nwaves = gridDim.x * 4;
  const int nl = st.fc.n_lost;
  if (c.c.descriptor_type == VSLAM_DESCRIPTOR_ORB) {
    const OrbTaps taps = orb_taps(lane, c.orb_cos, c.orb_sin, c.bstride);
    const int32_t* rec = b.rec + (size_t)s * c.MAXP * 6;
    const int32_t* lost = b.lost + (size_t)s * c.MAXP;
    for (int q = wave; q < nl; q += nwaves) {
      if (rec[6 * q] != 2) continue;   // wave-uniform
      recover_orb_wave(c, b, s, st.cur, q, lost[q], rec[6 * q + 1], rec[6 * q + 2], rec[6 * q + 3], rec[6 * q + 4], lane, st.fc.tau_gen, st.fc.tau_tri, taps);
    }
    return;
  }
  for (int q = wave; q < nl; q += nwaves) recover_brief_wave(c, b, s, st.cur, q, lane, st.fc.tau_gen, st.fc.tau_tri);
}

// recoverPoints on caller-provided lost points (vslam_stereo_recover): previous buffer 0 holds the lost points' descriptors,
// landmarks and landmark flags, the lost list is 0..n-1, survivors are appended to buffer 1 from its start.
struct RecoverAlone { double w2c[12]; double tau_track, tau_tri; int n; };
__global__ __launch_bounds__(VS_WG) void k_recover_alone(const DevCfg c, const DevBuf b, const RecoverAlone a) {
  __shared__ FrameShared sh;
  __shared__ __align__(16) unsigned char arena[VS_ARENA];
  __shared__ double w2c[12];
  const int s = b.s0, tid = threadIdx.x;
  if (tid < 12) w2c[tid] = a.w2c[tid];
  if (tid == 0) { sh.n_lost = a.n; sh.n_cur = 0; sh.flag = 0; }
  __syncthreads();
  wg_recover(c, b, s, sh, 0, 1, w2c, a.tau_track, a.tau_tri, arena);
  if (tid == 0) { b.st[s].n_cur = sh.n_cur; b.st[s].n_recovered = sh.flag; }
}
