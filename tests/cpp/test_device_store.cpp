// test_device_store.cpp — csrc/device_store.h (the memory a switchable feature owns on the device) on counting malloc / free stand-ins for
// the HIP calls: whatever order a store is enabled, replaced, half built, released twice or destroyed in, every allocation is freed
// exactly once.  Host code only, no GPU; built by tests/cpp/Makefile with -fsanitize=address,undefined, which also sees a leak, a double
// free or a write past a block.
#include <hip/hip_runtime_api.h>      // types and declarations only: nothing of the HIP runtime is called or linked

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "../../vslam_pose_estimation_framework_amd/csrc/device_store.h"

static std::set<void*> g_live;
static int g_calls = 0, g_allocs = 0, g_frees = 0, g_bad_frees = 0, g_fail_at = -1;   // g_fail_at: the get() call (counted from 0) that fails
struct CountingMemory {
  static hipError_t get(void** p, size_t bytes) {
    if (g_calls++ == g_fail_at) return hipErrorOutOfMemory;
    ++g_allocs;
    *p = std::malloc(bytes);
    g_live.insert(*p);
    return hipSuccess;
  }
  static void put(void* p) {
    if (!g_live.erase(p)) { ++g_bad_frees; return; }
    ++g_frees;
    std::free(p);
  }
  static hipError_t fill(void* p, int byte, size_t bytes, hipStream_t) { std::memset(p, byte, bytes); return hipSuccess; }
};
using Store = OwnedStore<CountingMemory>;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

// a feature the way the library writes one: typed pointers beside the store; enable replaces, enable(0) turns off, a failure frees the half
struct Feature {
  int cap = 0;
  double* xyz = nullptr; int* count = nullptr; unsigned char* desc = nullptr;
  Store mem;
  void off() { mem.release(); xyz = nullptr; count = nullptr; desc = nullptr; cap = 0; }
  hipError_t enable(int n) {
    off();
    if (n == 0) return hipSuccess;
    hipError_t e = mem.alloc_fill(&xyz, (size_t)n * 3, 0, nullptr);
    if (e == hipSuccess) e = mem.alloc_fill(&count, 1, 0, nullptr);
    if (e == hipSuccess) e = mem.alloc_fill(&desc, (size_t)n * 32, 0xff, nullptr);
    if (e != hipSuccess) { off(); return e; }
    cap = n;
    return hipSuccess;
  }
};
static bool balanced() { return g_live.empty() && g_frees == g_allocs && g_bad_frees == 0; }
static void start() { g_calls = g_allocs = g_frees = g_bad_frees = 0; g_fail_at = -1; }

int main() {
  {   // enable, replace, disable
    start();
    Feature f;
    CHECK(f.enable(5) == hipSuccess && f.cap == 5 && g_live.size() == 3);
    CHECK(f.xyz[14] == 0 && f.count[0] == 0 && f.desc[0] == 0xff && f.desc[159] == 0xff);
    CHECK(f.enable(9) == hipSuccess && f.cap == 9 && g_live.size() == 3 && g_frees == 3);
    CHECK(f.enable(0) == hipSuccess && f.cap == 0 && !f.xyz);
    CHECK(balanced() && g_allocs == 6);
  }
  for (int k = 0; k < 3; ++k) {   // the k-th allocation fails, on a fresh feature and on one that replaces a live store
    for (int live = 0; live < 2; ++live) {
      start();
      Feature f;
      if (live) CHECK(f.enable(4) == hipSuccess);
      g_fail_at = g_calls + k;
      CHECK(f.enable(7) == hipErrorOutOfMemory && f.cap == 0 && !f.xyz && !f.count && !f.desc);
      CHECK(balanced());
      g_fail_at = -1;
      const int before = g_allocs;
      CHECK(f.enable(7) == hipSuccess && f.cap == 7);      // usable afterwards
      f.off();
      CHECK(balanced() && g_allocs == before + 3);
    }
  }
  {   // a zero count still yields a block of its own (the library's std::max(count, 1))
    start();
    Store s;
    char* p = nullptr; char* q = nullptr;
    CHECK(s.alloc(&p, 0) == hipSuccess && s.alloc(&q, 0) == hipSuccess && p && q && p != q);
    s.release();
    CHECK(balanced());
  }
  {   // double release
    start();
    Feature f;
    CHECK(f.enable(3) == hipSuccess);
    f.off();
    f.off();
    f.mem.release();
    CHECK(balanced() && g_frees == 3);
  }
  {   // destroy with stores live: the owner releases each of its stores, the one that was never enabled included
    start();
    struct Owner { Feature map, log, never; void destroy() { map.off(); log.off(); never.off(); } } o;
    CHECK(o.map.enable(6) == hipSuccess && o.log.enable(2) == hipSuccess && g_live.size() == 6);
    o.destroy();
    CHECK(balanced() && g_frees == 6);
  }
  std::printf("device store: every allocation freed exactly once\n");
  return 0;
}
