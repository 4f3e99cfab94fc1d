// test_stage_reconcile.cpp — stage_slabs_reconcile of csrc/stage_plan.h, the one function that allocates and frees the stereo context's
// stage slabs, on counting malloc / free stand-ins for the HIP calls (as test_device_store.cpp runs device_store.h).  A seeded walk of
// 2000 single-switch flips in the shape every setter of host_switches.h has — change the switch, reconcile, on failure turn that switch
// off and reconcile again — with a failure injected at the k-th allocation of a flip, for every k a reconcile reaches.  After every
// flip the live allocations are exactly the plan's wanted set at the right byte counts; at the end everything was freed exactly once.
// Host code only, no GPU; built by tests/cpp/Makefile with -fsanitize=address,undefined.
#include <hip/hip_runtime_api.h>      // types and declarations only: nothing of the HIP runtime is called or linked

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

#include "../../vslam_pose_estimation_framework_amd/csrc/device_store.h"
#include "../../vslam_pose_estimation_framework_amd/csrc/stage_plan.h"

static std::map<void*, size_t> g_live;
static long g_calls = 0, g_allocs = 0, g_frees = 0, g_bad_frees = 0, g_fail_at = -1, g_fail_from = -1;   // get() calls counted from 0
struct CountingMemory {
  static hipError_t get(void** p, size_t bytes) {
    const long call = g_calls++;
    if (call == g_fail_at || (g_fail_from >= 0 && call >= g_fail_from)) return hipErrorOutOfMemory;
    ++g_allocs;
    *p = std::malloc(bytes);
    g_live[*p] = bytes;
    return hipSuccess;
  }
  static void put(void* p) {
    if (!g_live.erase(p)) { ++g_bad_frees; return; }
    ++g_frees;
    std::free(p);
  }
  static hipError_t fill(void* p, int byte, size_t bytes, hipStream_t) { std::memset(p, byte, bytes); return hipSuccess; }
};
using Slabs = StageSlabs<OwnedStore<CountingMemory>>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return false; } } while (0)

static const int B = 3, ROWS = 61, COLS = 83, UP_STRIDE = 128;
static const int RAW[2][2] = {{70, 95}, {66, 90}};       // two lenses: setting other maps changes the raw slabs' geometry

struct Ctx { StageSwitches sw; Slabs slabs; };
// the setters' shape (host_switches.h: slabs_reconcile, slabs_settle, slabs_follow)
static int reconcile(Ctx& c) {
  SlabGeom want[SLAB_OWNED];
  stage_slabs(c.sw, want);
  return stage_slabs_reconcile(c.slabs, want, B);
}
static void settle(Ctx& c) {
  if (reconcile(c) == 0) return;
  c.sw.channels = 0; c.sw.slot = false;
  (void)reconcile(c);
}
enum Switch { COLOUR, DOWNSCALE, REMAP, SMOOTH, SLOT, N_SWITCHES };
static void turn_off(StageSwitches& s, int which) {
  if (which == COLOUR) s.channels = 0;
  if (which == DOWNSCALE) { s.factor = 1; s.full_rows = s.full_cols = 0; }
  if (which == REMAP) { s.remap = false; s.raw_rows = s.raw_cols = 0; }
  if (which == SMOOTH) s.smooth = false;
  if (which == SLOT) s.slot = false;
}
static bool is_off(const StageSwitches& s, int which) {
  return which == COLOUR ? s.channels == 0 : which == DOWNSCALE ? s.factor == 1 : which == REMAP ? !s.remap : which == SMOOTH ? !s.smooth : !s.slot;
}
// live allocations == the plan's wanted set of c.sw, pointer by pointer and byte by byte; nothing dangling where nothing is wanted
static bool agrees(const Ctx& c) {
  SlabGeom want[SLAB_OWNED];
  stage_slabs(c.sw, want);
  size_t n = 0;
  for (int id = 0; id < SLAB_OWNED; ++id) {
    CHECK(c.slabs.geo[id] == want[id]);
    CHECK(c.slabs.mem[id].mem.size() == (size_t)want[id].pairs * 2);
    for (int q = 0; q < 2; ++q)
      for (int k = 0; k < 2; ++k) {
        uint8_t* p = c.slabs.p[id][q][k];
        if (q >= want[id].pairs) { CHECK(p == nullptr); continue; }
        const auto it = g_live.find(p);
        CHECK(it != g_live.end() && it->second == (size_t)B * want[id].rows * want[id].stride);
        ++n;
      }
  }
  CHECK(g_live.size() == n && g_bad_frees == 0);
  return true;
}
// one setter call: `next` is the state with one switch changed.  False when a check fails; *failed: the injected failure was hit.
static bool flip(Ctx& c, int which, const StageSwitches& next, long fail_k, bool* failed, long* made) {
  SlabGeom before[SLAB_OWNED], after[SLAB_OWNED];
  uint8_t* held[SLAB_OWNED];
  stage_slabs(c.sw, before);
  stage_slabs(next, after);
  for (int id = 0; id < SLAB_OWNED; ++id) held[id] = c.slabs.p[id][0][0];
  c.sw = next;
  const long calls = g_calls;
  g_fail_at = fail_k >= 0 ? g_calls + fail_k : -1;
  const int e = reconcile(c);
  g_fail_at = -1;
  *made = g_calls - calls;
  *failed = e != 0;
  if (e) {
    CHECK(e == (int)hipErrorOutOfMemory && fail_k >= 0);
    turn_off(c.sw, which);
    settle(c);
    CHECK(is_off(c.sw, which));
  } else {
    for (int id = 0; id < SLAB_OWNED; ++id) CHECK(!(before[id] == after[id]) || c.slabs.p[id][0][0] == held[id]);     // what is still right stays
  }
  return agrees(c);
}
static StageSwitches fresh() {
  StageSwitches s;
  s.rows = ROWS; s.cols = COLS; s.up_stride = UP_STRIDE;
  return s;
}
// a single-switch change that the contract allows from s: the downscale's full size reduces to what the next stage takes, so the raw
// size (the remap) changes only while the downscale is off
static StageSwitches pick(const StageSwitches& s, std::mt19937& rng, int* which) {
  StageSwitches n = s;
  *which = (int)(rng() % N_SWITCHES);
  if (*which == REMAP && s.factor > 1) *which = DOWNSCALE;
  if (*which == COLOUR) { const int ch[3] = {0, 3, 4}; do n.channels = ch[rng() % 3]; while (n.channels == s.channels); }
  if (*which == DOWNSCALE) {
    do n.factor = 1 + (int)(rng() % 3); while (n.factor == s.factor);
    const int rr = s.remap ? s.raw_rows : ROWS, rc = s.remap ? s.raw_cols : COLS;
    n.full_rows = n.factor > 1 ? rr * n.factor + 1 : 0; n.full_cols = n.factor > 1 ? rc * n.factor + 1 : 0;
  }
  if (*which == REMAP) {
    const int lens = (int)(rng() % 3);          // 2: off, or on at the other lens when it is off already
    n.remap = lens < 2 || !s.remap;
    const int* raw = RAW[lens < 2 ? lens : 0];
    n.raw_rows = n.remap ? raw[0] : 0; n.raw_cols = n.remap ? raw[1] : 0;
  }
  if (*which == SMOOTH) n.smooth = !s.smooth || rng() % 3 == 0;      // on -> on: another mode, the plan is the same
  if (*which == SLOT) n.slot = !s.slot;
  return n;
}

int main() {
  long reach = 0;                     // the most allocations one reconcile made
  for (long k = -1; k <= reach; ++k) {     // pass k: about every third flip has its k-th allocation fail (-1: none does)
    std::mt19937 rng(20240607u);
    Ctx c;
    c.sw = fresh();
    long hits = 0;
    for (int step = 0; step < 2000; ++step) {
      int which;
      const StageSwitches next = pick(c.sw, rng, &which);
      const bool armed = k >= 0 && rng() % 3 == 0;
      bool failed;
      long made;
      if (!flip(c, which, next, armed ? k : -1, &failed, &made)) { std::printf("pass %ld step %d switch %d\n", k, step, which); return 1; }
      if (failed) ++hits;
      else if (made > reach) reach = made;
    }
    if (k >= 0 && k < reach && hits == 0) { std::printf("FAILED: no flip reached allocation %ld\n", k); return 1; }
    c.slabs.release();
    if (!g_live.empty() || g_frees != g_allocs || g_bad_frees) { std::printf("FAILED: pass %ld leaked or freed twice\n", k); return 1; }
    std::printf("pass %ld: %ld failed flips\n", k, hits);
  }
  if (reach < 10) { std::printf("FAILED: the walk never made the 10 allocations of remap on beside colour and the slot (%ld)\n", reach); return 1; }
  {   // the failed flip's second reconcile fails as well: colour input and the slot go off with it, and what is left agrees again
    Ctx c;
    c.sw = fresh();
    c.sw.channels = 3; c.sw.slot = true; c.sw.remap = true; c.sw.raw_rows = RAW[0][0]; c.sw.raw_cols = RAW[0][1];
    if (reconcile(c) != 0 || !agrees(c)) return 1;
    c.sw.factor = 2; c.sw.full_rows = 2 * RAW[0][0]; c.sw.full_cols = 2 * RAW[0][1];
    g_fail_from = g_calls;          // the full-size slabs fail, then the colour slabs at the old size
    const int e = reconcile(c);
    turn_off(c.sw, DOWNSCALE);
    settle(c);
    g_fail_from = -1;
    if (e == 0 || c.sw.channels != 0 || c.sw.slot || !c.sw.remap || !agrees(c)) { std::printf("FAILED: double failure\n"); return 1; }
    c.slabs.release();
    c.slabs.release();
    if (!g_live.empty() || g_frees != g_allocs || g_bad_frees) { std::printf("FAILED: double failure leaked\n"); return 1; }
  }
  std::printf("stage slabs: live allocations follow the plan, every allocation freed exactly once\n");
  return 0;
}
