// stage_plan.h — the stereo context's input stages as a plan: which slabs exist and how a frame is routed through them, as a pure function of
// the switch state.  The ONE place that decides either; host_switches.h brings the slabs into agreement with it
// (stage_slabs_reconcile) and host_frame.h reads a frame's route from it.  Plain C++ that the host and two stand-alone programs
// (tests/cpp/stage_plan_walk.cpp, tests/cpp/test_stage_reconcile.cpp) compile: nothing here touches HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

// the slabs the stages own, then the two places that are not the plan's to allocate: upload[parity] (always there) and the caller's memory
enum StageSlab { SLAB_COLOR = 0, SLAB_FULL, SLAB_RAW, SLAB_SM_IN, SLAB_KEEP, SLAB_SM_OUT, SLAB_OWNED, SLAB_UPLOAD = SLAB_OWNED, SLAB_CALLER };

// the switch state.  up_stride: bytes between rows of upload[parity], a constant of the context
struct StageSwitches {
  int channels = 0;                              // colour input: bytes per pixel of the frames that come in, 0 while off
  int factor = 1, full_rows = 0, full_cols = 0;  // downscale: off while factor == 1
  bool remap = false; int raw_rows = 0, raw_cols = 0;
  bool smooth = false, slot = false;
  int rows = 0, cols = 0, up_stride = 0;         // the size the detector works on
};
// the size of the frames that come in: the full size while downscaling, else the raw size while remapping, else rows x cols
static inline void stage_in_size(const StageSwitches& s, int* rows, int* cols) {
  if (s.factor > 1) { *rows = s.full_rows; *cols = s.full_cols; }
  else if (s.remap) { *rows = s.raw_rows; *cols = s.raw_cols; }
  else { *rows = s.rows; *cols = s.cols; }
}

// ---- question 1: which slabs must exist -------------------------------------------------------------
// pairs: 2 one pair per step parity, 1 one pair, 0 the slab does not exist; every image of a pair holds B streams of rows x stride bytes
struct SlabGeom {
  int rows = 0, width = 0, stride = 0, pairs = 0;
  size_t stream_stride() const { return (size_t)rows * stride; }
  bool operator==(const SlabGeom& o) const { return rows == o.rows && width == o.width && stride == o.stride && pairs == o.pairs; }
};
static inline SlabGeom stage_slab_wide(int rows, int width, int pairs) { return {rows, width, (width + 63) & ~63, pairs}; }
static inline void stage_slabs(const StageSwitches& s, SlabGeom want[SLAB_OWNED]) {
  int in_rows, in_cols;
  stage_in_size(s, &in_rows, &in_cols);
  const SlabGeom processed = {s.rows, s.cols, s.up_stride, 2};
  for (int id = 0; id < SLAB_OWNED; ++id) want[id] = SlabGeom();
  if (s.channels) want[SLAB_COLOR] = stage_slab_wide(in_rows, s.channels * in_cols, 2);
  if (s.factor > 1) want[SLAB_FULL] = stage_slab_wide(s.full_rows, s.full_cols, 2);
  if (s.remap) want[SLAB_RAW] = stage_slab_wide(s.raw_rows, s.raw_cols, 2);
  if (s.smooth) want[SLAB_SM_IN] = processed;
  if (s.slot && s.remap && !s.smooth) { want[SLAB_KEEP] = processed; want[SLAB_KEEP].pairs = 1; }
  if (s.smooth && s.slot) { want[SLAB_SM_OUT] = processed; want[SLAB_SM_OUT].pairs = 1; }
}

// ---- question 2: a frame's route ----------------------------------------------------------------------
// A stage that runs reads `src` and writes `dst`; src is always where the stage before it (or the upload, or the caller) left the pair.
struct StageHop { bool on = false; int src = SLAB_CALLER, dst = SLAB_CALLER; };
struct StageRoute {
  int upload = SLAB_CALLER;            // where a host frame is copied to; SLAB_CALLER: the frame is the caller's device memory, read in place
  StageHop gray, down, remap, smooth, slot;
  int detector = SLAB_CALLER;          // what the detector reads
};
static inline StageRoute stage_route(const StageSwitches& s, bool device_source) {
  StageRoute r;
  const int after_remap = s.smooth ? SLAB_SM_IN : SLAB_UPLOAD;
  const int next = s.remap ? SLAB_RAW : after_remap;     // what the remap, else the smoothing, else the slot and the detector read
  if (!device_source) r.upload = s.channels ? SLAB_COLOR : s.factor > 1 ? SLAB_FULL : next;
  int cur = r.upload;
  auto hop = [&cur](StageHop& h, int dst) { h.on = true; h.src = cur; h.dst = dst; cur = dst; };
  if (s.channels) hop(r.gray, s.factor > 1 ? SLAB_FULL : next);
  if (s.factor > 1) hop(r.down, next);
  if (s.remap) hop(r.remap, s.smooth ? SLAB_SM_IN : s.slot ? SLAB_KEEP : SLAB_UPLOAD);
  if (s.smooth) hop(r.smooth, s.slot ? SLAB_SM_OUT : SLAB_UPLOAD);     // never in place
  if (s.slot) hop(r.slot, SLAB_UPLOAD);                                // in place when the pair already lies there (it keeps its strides)
  r.detector = cur;
  return r;
}

// ---- the slabs themselves -----------------------------------------------------------------------------
// Store: OwnedStore<Mem> of device_store.h, one per slab id, so that a slab goes as a whole.  p[id][parity][left/right]; a one-pair slab
// uses parity 0.  geo[id]: what is held (pairs == 0: nothing).
template <class Store>
struct StageSlabs {
  Store mem[SLAB_OWNED];
  SlabGeom geo[SLAB_OWNED];
  uint8_t* p[SLAB_OWNED][2][2] = {};
  void drop(int id) {
    mem[id].release();
    geo[id] = SlabGeom();
    for (int q = 0; q < 2; ++q) p[id][q][0] = p[id][q][1] = nullptr;
  }
  void release() { for (int id = 0; id < SLAB_OWNED; ++id) drop(id); }
};
// Brings the slabs into agreement with `want` for B streams: frees what is no longer wanted or has another geometry, then allocates what
// is missing; what is still right stays.  0, or the status of the allocation that failed — that slab is dropped whole, the ones behind it
// are still missing: the caller turns the switch it was changing off and reconciles again.
template <class Store>
static int stage_slabs_reconcile(StageSlabs<Store>& s, const SlabGeom want[SLAB_OWNED], int B) {
  for (int id = 0; id < SLAB_OWNED; ++id) if (s.geo[id].pairs && !(s.geo[id] == want[id])) s.drop(id);
  for (int id = 0; id < SLAB_OWNED; ++id) {
    if (!want[id].pairs || s.geo[id].pairs) continue;
    for (int q = 0; q < want[id].pairs; ++q)
      for (int k = 0; k < 2; ++k)
        if (const int e = (int)s.mem[id].alloc(&s.p[id][q][k], (size_t)B * want[id].stream_stride())) { s.drop(id); return e; }
    s.geo[id] = want[id];
  }
  return 0;
}
