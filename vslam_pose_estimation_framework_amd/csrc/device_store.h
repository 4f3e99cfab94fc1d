// device_store.h — device memory that a switchable feature owns (the landmark map, the observation log, the rectification maps; the RGB-D
// tracker's map and log): allocated when the feature is turned on, released as a whole when it is turned off, replaced or its owner is
// destroyed.  The owner keeps the typed pointers; the store only remembers what to free.  Plain host C++: tests/cpp/test_device_store.cpp
// runs it on counting stand-ins for the three HIP calls.
#pragma once
#include <algorithm>
#include <vector>

struct HipDeviceMemory {
  static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void put(void* p) { (void)hipFree(p); }
  static hipError_t fill(void* p, int byte, size_t bytes, hipStream_t st) { return hipMemsetAsync(p, byte, bytes, st); }
};
template <class Mem = HipDeviceMemory>
struct OwnedStore {
  std::vector<void*> mem;
  template <typename T> hipError_t alloc(T** p, size_t count) {
    void* q = nullptr;
    const hipError_t e = Mem::get(&q, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) { mem.push_back(q); *p = (T*)q; }
    return e;
  }
  // allocation whose every byte is set to `byte` on stream st (the caller synchronises once, behind the last one)
  template <typename T> hipError_t alloc_fill(T** p, size_t count, int byte, hipStream_t st) {
    const hipError_t e = alloc(p, count);
    return e == hipSuccess ? Mem::fill(*p, byte, count * sizeof(T), st) : e;
  }
  void release() { for (void* p : mem) Mem::put(p); mem.clear(); }
};
using DeviceStore = OwnedStore<>;
