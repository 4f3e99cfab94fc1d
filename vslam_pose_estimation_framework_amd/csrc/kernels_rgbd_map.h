// kernels_rgbd_map.h — the landmark map and the observation log of the device-resident RGB-D loop (opt-in, gfx950).
//
// k_rgbd_landmarks creates and refines landmarks (PoseTracker3D::_updatePoints) but keeps them only on the frame lists (RgbdList::lmw,
// lmu): a landmark is gone when its track ends.  k_rgbd_map_commit runs behind k_rgbd_finish, once per frame and sequence, and
//   1. labels every point of the finished frame with a dense landmark id,
//   2. copies every landmark the frame created or updated into a per-sequence store indexed by that id,
//   3. when the log is on, appends one entry per labelled point.
//
// Identity is the track.  In the order of the frame's point list (what vslam_rgbd_get_points returns):
//   id[i] = id_prev[prev[i]]   when the point has a predecessor and the predecessor carries an id (prev indexes the previous frame's
//                              framepoints followed by its temporary points; a temporary point never carries an id);
//   else the next id           when the point's landmark was created or updated this frame;
//   else -1.
// Ids are dense from 0 after enabling or a reset.  _updatePoints creates landmarks in point order, so id k is the k-th landmark of a
// fresh reference process (tests/test_rgbd_map_gpu.py pins that against the checker loop).
//
// "Created or updated this frame" is RGBD_F_LM on the CURRENT list: k_rgbd_track and k_rgbd_recover_finish hand a new point
// RGBD_F_UNREL / RGBD_F_CHAIN of its predecessor only, compute()'s points start with 0, and k_rgbd_landmarks sets RGBD_F_LM on exactly the
// points it ran Landmark::Landmark or Landmark::update for.  No existing kernel had to change.  A labelled point WITHOUT that flag (a
// track that goes on without an update) keeps its id, is logged, and leaves the map entry as it was.
//
// Map row (64 bytes, four 16-byte stores): {x, y} {z, last_frame, updates} {descriptor 0..15} {descriptor 16..31}; first_frame lives in
// an array of its own, written once by the frame that creates the entry.  Log entry (48 bytes, three 16-byte stores):
// {id, frame, x, y} {cam x, cam y} {cam z, 0}; x, y are RgbdList::xy and cam is RgbdList::cam bit for bit (the measurement
// Landmark::update consumed).  Frame indices are 0-based per sequence, the pose log's.
//
// Capacity: once a sequence's id counter would pass `cap`, no entry is created; the points asking keep -1 and ask again on later frames
// (the counter never falls, so they are refused for the track's life).  Log entries past `ocap` are dropped, so a full log holds exactly
// the first `ocap` entries of the unconstrained one.  A frame that refused a landmark sets VS_MAP_OVERFLOW, one that dropped an entry
// VS_OBS_OVERFLOW — in RgbdState::info.error_flags only (k_rgbd_finish has filled the report; RgbdState::error_flags is sticky in this
// tracker, and "exactly the frames that refused" could not be read from it).  The host copies the state block out behind this kernel.
//
// Once per frame: the tail is enqueued after every registration attempt and skips itself until the registration is done; k_rgbd_finish
// then raises tail_done and advances frame_count.  This kernel runs when tail_done is up and its own per-sequence mark
// (RgbdMap::committed, the frame_count it last served) differs from frame_count — so a frame with two or three attempts is committed
// after its last attempt and not again by the launches of a later attempt that serves another sequence of the batch.
//
// Shape: one 1024-thread workgroup per sequence, the frame's points in chunks of 1024.  New ids AND log offsets come from ONE workgroup
// prefix sum per chunk in point order (the two 0/1 votes packed into one int: a chunk's totals stay below 2^16), so the append needs no
// atomics and nothing depends on scheduling; the running bases are the same in every lane (the scan's totals are broadcast).  Nothing
// here is read by the tracker.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels_rgbd.h"
#include "kernels_map.h"      // VS_MAP_OVERFLOW
#include "kernels_obs.h"      // VS_OBS_OVERFLOW

#define VS_RGBD_MAP_WG 1024

struct RgbdMap {
  uint4* rows;         // [B][cap][4]   map rows (layout above)
  int32_t* first;      // [B][cap]      first_frame
  int32_t* count;      // [B]           ids handed out
  int32_t* committed;  // [B]           RgbdState::frame_count after the last frame this kernel served
  int32_t* ids;        // [2][B][MAXP]  landmark id of every point (framepoints and temporary points), by frame list (frame parity)
  uint4* log;          // [B][ocap][3]  log entries (layout above); null while the log is off
  int32_t* ocount;     // [B]           entries written
  int32_t cap, ocap, B;
};

__device__ __forceinline__ uint4 rgbd_map_pack(double a, double b) {
  return make_uint4((uint32_t)__double2loint(a), (uint32_t)__double2hiint(a), (uint32_t)__double2loint(b), (uint32_t)__double2hiint(b));
}

__global__ __launch_bounds__(VS_RGBD_MAP_WG) void k_rgbd_map_commit(const RgbdBuf all, const RgbdMap m) {
  __shared__ int scan[17];
  const int sq = blockIdx.x, tid = threadIdx.x;
  const RgbdBuf r = rgbd_stream(all, sq);
  RgbdState& st = *r.st;
  const int fc = st.frame_count;
  if (!st.tail_done || m.committed[sq] == fc) return;
  const int f = fc - 1;                                    // the frame k_rgbd_finish has just closed
  const RgbdList cur = rgbd_pick(r, (f & 1) != 0);        // its list: rgbd_cur() before frame_count advanced
  const int P = r.MAXP;
  const int np = min(st.last_points, P), n_all = min(st.last_all, P);
  const int n_prev = f > 0 ? P : 0;                        // the first frame has no previous ids to read
  const int32_t* ids_prev = m.ids + ((size_t)((f & 1) ^ 1) * m.B + sq) * P;
  int32_t* ids_cur = m.ids + ((size_t)(f & 1) * m.B + sq) * P;
  uint4* rows = m.rows + (size_t)sq * m.cap * 4;
  int32_t* first = m.first + (size_t)sq * m.cap;
  uint4* log = m.log ? m.log + (size_t)sq * m.ocap * 3 : nullptr;
  int base = m.count[sq];                                  // <= cap
  int obase = log ? m.ocount[sq] : 0;                      // <= ocap
  bool refused = false, dropped = false;
  for (int i0 = 0; i0 < n_all; i0 += VS_RGBD_MAP_WG) {
    const int i = i0 + tid;
    int id = -1;
    bool upd = false;
    if (i < np) {
      const int ip = cur.prev[i];
      upd = (cur.flags[i] & RGBD_F_LM) != 0;
      if (ip >= 0 && ip < n_prev) { id = ids_prev[ip]; if (id >= m.cap) id = -1; }
    }
    const bool ask = upd && id < 0, had = id >= 0;
    int total;
    const int off = block_exclusive_scan((ask ? 1 : 0) | (had ? 1 << 16 : 0), scan, &total);
    const int room = m.cap - base;                         // >= 0
    const int off_ask = off & 0xffff, n_ask = total & 0xffff;
    const bool fresh = ask && off_ask < room;
    if (fresh) id = base + off_ask;
    if (i < n_all) ids_cur[i] = id;
    if (id >= 0) {
      if (upd) {
        const double* w = cur.lmw + 3 * (size_t)i;
        const uint4* sd = reinterpret_cast<const uint4*>(cur.desc + (size_t)32 * i);
        const double z = w[2];
        uint4* o = rows + 4 * (size_t)id;
        o[0] = rgbd_map_pack(w[0], w[1]);
        o[1] = make_uint4((uint32_t)__double2loint(z), (uint32_t)__double2hiint(z), (uint32_t)f, (uint32_t)cur.lmu[i]);
        o[2] = sd[0]; o[3] = sd[1];
        if (fresh) first[id] = f;
      }
      if (log) {
        // entries ahead of this one in the chunk: the inherited ids before it plus the fresh ids before it
        const int at = (off >> 16) + min(off_ask, room);
        if (at < m.ocap - obase) {
          const double* cm = cur.cam + 3 * (size_t)i;
          uint4* e = log + 3 * ((size_t)obase + at);
          e[0] = make_uint4((uint32_t)id, (uint32_t)f, __float_as_uint(cur.xy[2 * i]), __float_as_uint(cur.xy[2 * i + 1]));
          e[1] = rgbd_map_pack(cm[0], cm[1]);
          e[2] = rgbd_map_pack(cm[2], 0.0);
        }
      }
    }
    const int n_fresh = min(n_ask, room);
    if (n_ask > room) refused = true;
    if (log) {
      const int n_log = (total >> 16) + n_fresh;
      if (n_log > m.ocap - obase) { dropped = true; obase = m.ocap; }
      else obase += n_log;
    }
    base += n_fresh;
  }
  if (tid == 0) {
    m.count[sq] = base;
    if (log) m.ocount[sq] = obase;
    if (refused || dropped) st.info.error_flags |= (refused ? VS_MAP_OVERFLOW : 0) | (dropped ? VS_OBS_OVERFLOW : 0);
    m.committed[sq] = fc;
  }
}
