// kernels_map.h — the open-loop landmark map kept on the device (WorldMap::_landmarks, world_map.h:116; opt-in, gfx950).
//
// k_frame creates and refines landmarks (PoseTracker3D::_updatePoints, Landmark::Landmark / Landmark::update) but keeps them only on
// the frame's points.  k_map_commit runs after a frame's last launch and copies every landmark the frame touched into a per-stream
// store indexed by a dense landmark id, so a landmark outlives the track that carried it.
//
// Identity is the track.  A point's M_PREV links it to its predecessor in the previous frame (recovered points included:
// wg_recover_append_t sets M_PREV to the lost point's index).  Per stream and frame, in the order of the frame's point list:
//   id[i] = id_prev[M_PREV[i]]     when the point has a predecessor and that predecessor carries an id;
//   else the next id               when the point carries a landmark (M_LMUP > 0: vslam_get_points' validity rule);
//   else -1.
// Ids start at 0 after vslam_enable_map or a reset and follow point order within a frame, as Landmark::identifier() does in a fresh
// reference process (_updatePoints creates landmarks in point order); that correspondence is the intent, it is not pinned here.
// The ids of the previous frame are only read when the stream has one (frame index > 0).
//
// Which points were updated this frame: landmark_point runs on every point whose track is long enough (M_TLEN >=
// minimum_track_length_for_landmark_creation) and leaves M_LMUP > 0 on each of them; a point with M_LMUP > 0 inherited it from a
// predecessor whose track was already long enough.  So "carries a landmark" and "its landmark was updated this frame" are the same
// set, M_LMUP > 0, and every point with an id is in it.  Each such point writes its landmark's slot: coordinates (p_lm), the update
// count (M_LMUP, Landmark::_number_of_updates), last_frame = this frame (_last_update) and the point's left descriptor (the last entry
// of Landmark::_descriptors); a landmark new this frame also writes first_frame.  Frame indices are 0-based per stream (the pose log's).
//
// Capacity: once a stream's counter would pass `cap`, no entry is created; the points asking keep -1 (and ask again on later frames:
// the counter never falls, so they are refused for the track's life).  The frame that refused one sets error bit 8 in the stream
// state and in the frame's report: phase 2 has already copied the state's flags into the report when this kernel runs.
//
// Shape: one 1024-thread workgroup per active stream, the frame's points in chunks of 1024; new ids by a workgroup prefix sum in point
// order (deterministic).  Nothing here is read by the tracker.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"
#include "kernels_frame.h"

#define VS_MAP_WG 1024       // a KITTI frame's ~1500 points in two rounds: each round is a chain of dependent loads (meta -> ids_prev)
#define VS_MAP_OVERFLOW 8      // vslam_frame_info.error_flags bit: map capacity

struct DevMap {
  double* xyz;        // [B][cap][3]  Landmark::coordinates() (world)
  int32_t* info;      // [B][cap][3]  first_frame, last_frame, updates
  uint8_t* desc;      // [B][cap][32] left descriptor of the last update
  int32_t* count;     // [B]          ids handed out
  int32_t* ids;       // [2][B][MAXP] landmark id of every point, by point buffer (StreamState::cur)
  int32_t cap, B;
};

__global__ __launch_bounds__(VS_MAP_WG) void k_map_commit(const DevCfg c, const DevBuf b, const DevMap m) {
  __shared__ int scan[17];
  __shared__ int base_sh, refused_sh;
  const int s = b.s0 + (int)blockIdx.x, tid = threadIdx.x;
  if (!vs_active(b, s)) return;
  const StreamState& st = b.st[s];
  const int f = st.frame_count - 1, pb = st.cur;     // the frame just finished and its point buffer
  if (f < 0) return;
  const PtView cv = pts_of(c, b, s, pb);
  const int n = min(*cv.n, c.MAXP);
  const int32_t* ids_prev = m.ids + ((size_t)(pb ^ 1) * m.B + s) * c.MAXP;
  int32_t* ids_cur = m.ids + ((size_t)pb * m.B + s) * c.MAXP;
  double* xyz = m.xyz + (size_t)s * m.cap * 3;
  int32_t* inf = m.info + (size_t)s * m.cap * 3;
  uint8_t* dsc = m.desc + (size_t)s * m.cap * 32;
  if (tid == 0) { base_sh = m.count[s]; refused_sh = 0; }
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += VS_MAP_WG) {
    const int i = i0 + tid;
    int id = -1, lmup = 0;
    if (i < n) {
      const int32_t* mi = cv.meta + (size_t)i * META;
      const int ip = mi[M_PREV];
      lmup = mi[M_LMUP];
      if (f > 0 && ip >= 0 && ip < c.MAXP) { id = ids_prev[ip]; if (id >= m.cap) id = -1; }
    }
    const bool ask = i < n && id < 0 && lmup > 0;
    int total;
    const int off = block_exclusive_scan(ask ? 1 : 0, scan, &total);
    const int base = base_sh;
    bool fresh = false;
    if (ask) {
      if (base + off < m.cap) { id = base + off; fresh = true; }
      else refused_sh = 1;
    }
    if (i < n) {
      ids_cur[i] = id;
      if (id >= 0) {
        const double* p = cv.lm + 3 * (size_t)i;
        double* o = xyz + 3 * (size_t)id;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        int32_t* q = inf + 3 * (size_t)id;
        if (fresh) q[0] = f;
        q[1] = f; q[2] = lmup;
        const uint4* sd = reinterpret_cast<const uint4*>(cv.desc + (size_t)64 * i);
        uint4* dd = reinterpret_cast<uint4*>(dsc + (size_t)32 * id);
        dd[0] = sd[0]; dd[1] = sd[1];
      }
    }
    __syncthreads();     // every lane has read base_sh
    if (tid == 0) base_sh = min(base + total, m.cap);
    __syncthreads();
  }
  if (tid == 0) {
    m.count[s] = base_sh;
    if (refused_sh) { atomicOr(&b.st[s].error_flags, VS_MAP_OVERFLOW); atomicOr(&b.info[s].error_flags, VS_MAP_OVERFLOW); }
  }
}
