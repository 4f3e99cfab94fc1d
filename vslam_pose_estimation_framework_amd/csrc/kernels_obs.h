// kernels_obs.h — the landmark observation log kept on the device (opt-in on top of the landmark map of kernels_map.h; gfx950).
//
// k_map_commit leaves the map id of every point of the finished frame in DevMap::ids (ids_cur), and overwrites it two frames later.
// k_obs_append runs behind it and appends, per stream, one 16-byte entry for every point that carries an id, in the order of the
// frame's point list:
//   int32 id      the landmark's map id (vslam_get_map entry `id`)
//   int32 frame   0-based per stream, as in the pose log and the map's first_frame / last_frame
//   int16 xL, yL, xR, yR   the point's keypoints (p_kp, what vslam_get_points reports as kp)
// A stream's log is therefore sorted by frame, then by point order, and is deterministic.  A landmark's observations start with the
// frame that created its map entry: the earlier points of its track (before minimum_track_length_for_landmark_creation was reached)
// carry no id and are not logged.
//
// Capacity: entries past `cap` are dropped, so a full log holds exactly the first `cap` entries of the unconstrained one.  The
// per-stream counter stops at cap; a frame that dropped an entry sets error bit 16 in the stream state and in the frame's report
// (phase 2 has already copied the state's flags into the report when this kernel runs, as for the map's bit 8).
//
// Shape: one 1024-thread workgroup per active stream, the frame's points in chunks of 1024.  Write offsets come from a workgroup prefix
// sum over id >= 0 in point order, so the append needs no atomics and the order does not depend on scheduling; the running base is the
// same in every lane (the scan's total is broadcast), so nothing but the scan goes through LDS.  Two rounds of dependent loads (stream
// state -> point count, ids and keypoints), one fewer than k_map_commit (which chases meta -> ids_prev).  Each entry leaves as one
// 16-byte store.  Nothing here is read by the tracker or by the map.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "dev_types.h"
#include "kernels_frame.h"
#include "kernels_map.h"

#define VS_OBS_WG 1024
#define VS_OBS_OVERFLOW 16     // vslam_frame_info.error_flags bit: observation log capacity

struct DevObs {
  uint4* log;         // [B][cap]  {id, frame, xL | yL << 16, xR | yR << 16}
  int32_t* count;     // [B]       entries written
  int32_t cap;
};

__global__ __launch_bounds__(VS_OBS_WG) void k_obs_append(const DevCfg c, const DevBuf b, const DevMap m, const DevObs o) {
  __shared__ int scan[17];
  const int s = b.s0 + (int)blockIdx.x, tid = threadIdx.x;
  if (!vs_active(b, s)) return;
  const StreamState& st = b.st[s];
  const int f = st.frame_count - 1, pb = st.cur;     // the frame k_map_commit has just labelled and its point buffer
  if (f < 0) return;
  const PtView cv = pts_of(c, b, s, pb);
  const int n = min(*cv.n, c.MAXP);
  const int32_t* ids = m.ids + ((size_t)pb * m.B + s) * c.MAXP;
  const uint2* kp = reinterpret_cast<const uint2*>(cv.kp);      // 4 x int16 per point, 8-byte aligned
  uint4* log = o.log + (size_t)s * o.cap;
  int base = o.count[s];                             // <= cap
  bool dropped = false;
  for (int i0 = 0; i0 < n; i0 += VS_OBS_WG) {
    const int i = i0 + tid;
    int id = -1;
    uint2 k = make_uint2(0u, 0u);
    if (i < n) { id = ids[i]; k = kp[i]; }
    int total;
    const int off = block_exclusive_scan(id >= 0 ? 1 : 0, scan, &total);
    if (id >= 0 && off < o.cap - base) log[base + off] = make_uint4((uint32_t)id, (uint32_t)f, k.x, k.y);
    if (total > o.cap - base) { dropped = true; base = o.cap; }
    else base += total;
  }
  if (tid == 0) {
    o.count[s] = base;
    if (dropped) { atomicOr(&b.st[s].error_flags, VS_OBS_OVERFLOW); atomicOr(&b.info[s].error_flags, VS_OBS_OVERFLOW); }
  }
}
