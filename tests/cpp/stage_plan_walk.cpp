// stage_plan_walk.cpp — csrc/stage_plan.h over every switch state of the stereo context: colour off / 3 / 4 channels, factor 1 / 2, remap
// off / on, smoothing off / on, slot off / on, host / device source.  The wanted slabs against the six existence conditions and the route
// against the table of DESIGN.md 6.1, both restated literally here, plus the properties the kernels rely on.  Host code only, no GPU; built
// and run by tests/test_stage_plan_host.py.
#include <cstdio>
#include <initializer_list>

#include "stage_plan.h"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s  (channels %d factor %d remap %d smooth %d slot %d device %d)\n", __FILE__, __LINE__, #cond, \
                                                    ch, f, remap, smooth, slot, device); return 1; } } while (0)

static const int ROWS = 61, COLS = 83, RAW_ROWS = 70, RAW_COLS = 95, UP_STRIDE = 128;

static bool same(const StageHop& h, bool on, int src, int dst) { return h.on == on && (!on || (h.src == src && h.dst == dst)); }

int main() {
  int states = 0;
  for (int ch : {0, 3, 4}) for (int f : {1, 2}) for (int remap = 0; remap < 2; ++remap) for (int smooth = 0; smooth < 2; ++smooth)
    for (int slot = 0; slot < 2; ++slot) for (int device = 0; device < 2; ++device) {
      StageSwitches s;
      s.channels = ch; s.remap = remap; s.raw_rows = remap ? RAW_ROWS : 0; s.raw_cols = remap ? RAW_COLS : 0;
      s.smooth = smooth; s.slot = slot; s.rows = ROWS; s.cols = COLS; s.up_stride = UP_STRIDE;
      const int red_rows = remap ? RAW_ROWS : ROWS, red_cols = remap ? RAW_COLS : COLS;      // what the downscale hands on
      s.factor = f; s.full_rows = f > 1 ? red_rows * f + 1 : 0; s.full_cols = f > 1 ? red_cols * f + 1 : 0;
      const int in_rows = f > 1 ? s.full_rows : red_rows, in_cols = f > 1 ? s.full_cols : red_cols;
      int r2, c2;
      stage_in_size(s, &r2, &c2);
      CHECK(r2 == in_rows && c2 == in_cols);

      // ---- the wanted set: the six existence conditions, and today's geometry ----
      SlabGeom want[SLAB_OWNED];
      stage_slabs(s, want);
      const bool exists[SLAB_OWNED] = {ch != 0, f > 1, remap != 0, smooth != 0, slot && remap && !smooth, smooth && slot};
      for (int id = 0; id < SLAB_OWNED; ++id) CHECK((want[id].pairs != 0) == exists[id]);
      const SlabGeom wide[3] = {{in_rows, ch * in_cols, (ch * in_cols + 63) & ~63, 2}, {s.full_rows, s.full_cols, (s.full_cols + 63) & ~63, 2},
                                {RAW_ROWS, RAW_COLS, (RAW_COLS + 63) & ~63, 2}};
      for (int id = SLAB_COLOR; id <= SLAB_RAW; ++id) CHECK(!exists[id] || want[id] == wide[id]);
      for (int id = SLAB_SM_IN; id <= SLAB_SM_OUT; ++id) {
        const SlabGeom g = {ROWS, COLS, UP_STRIDE, id == SLAB_SM_IN ? 2 : 1};
        CHECK(!exists[id] || want[id] == g);      // upload[parity]'s strides: its stream stride is rows * up_stride (asserted by stage_switches, host_switches.h)
      }

      // ---- the route against the table, restated ----
      const StageRoute r = stage_route(s, device != 0);
      const int next = remap ? SLAB_RAW : smooth ? SLAB_SM_IN : SLAB_UPLOAD;
      const int lands = device ? SLAB_CALLER : ch ? SLAB_COLOR : f > 1 ? SLAB_FULL : remap ? SLAB_RAW : smooth ? SLAB_SM_IN : SLAB_UPLOAD;
      CHECK(r.upload == lands);
      int cur = lands;
      const int gray_dst = f > 1 ? SLAB_FULL : next;
      CHECK(same(r.gray, ch != 0, cur, gray_dst));
      if (ch) cur = gray_dst;
      CHECK(same(r.down, f > 1, cur, next));
      if (f > 1) cur = next;
      const int remap_dst = smooth ? SLAB_SM_IN : slot ? SLAB_KEEP : SLAB_UPLOAD;
      CHECK(same(r.remap, remap != 0, cur, remap_dst));
      if (remap) cur = remap_dst;
      const int smooth_dst = slot ? SLAB_SM_OUT : SLAB_UPLOAD;
      CHECK(same(r.smooth, smooth != 0, cur, smooth_dst));
      if (smooth) cur = smooth_dst;
      CHECK(same(r.slot, slot != 0, cur, SLAB_UPLOAD));      // cur already UPLOAD: in place
      if (slot) cur = SLAB_UPLOAD;
      CHECK(r.detector == cur);

      // ---- what the kernels and the getters rely on ----
      const StageHop* hops[5] = {&r.gray, &r.down, &r.remap, &r.smooth, &r.slot};
      bool ran = false;
      for (int h = 0; h < 5; ++h) {
        if (!hops[h]->on) continue;
        ran = true;
        for (int id : {hops[h]->src, hops[h]->dst}) CHECK(id == SLAB_UPLOAD || id == SLAB_CALLER || (id >= 0 && id < SLAB_OWNED && want[id].pairs));
        CHECK(hops[h]->dst != SLAB_CALLER);                              // caller memory is only read
        CHECK(hops[h]->src != hops[h]->dst || hops[h] == &r.slot);        // the slot alone works in place
      }
      CHECK(!r.smooth.on || r.smooth.src != r.smooth.dst);
      CHECK(r.upload == SLAB_UPLOAD || r.upload == SLAB_CALLER || want[r.upload].pairs);
      CHECK((r.upload == SLAB_CALLER) == (device != 0));
      CHECK(r.detector == (!ran && device ? SLAB_CALLER : SLAB_UPLOAD));
      ++states;
    }
  std::printf("stage plan walk: ok (%d states)\n", states);
  return states == 96 ? 0 : 1;
}
