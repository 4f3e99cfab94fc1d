// pk3_rate.hip — what does a three-input packed half-precision minimum cost next to the two-input packed i16 one?
// Four chains of 4096 instructions per wavefront, timed with s_memtime, at one and at eight wavefronts per SIMD:
//   dep_i16    dependent v_pk_min_i16, each followed by the s_nop 0 the compiler puts between dependent packed-i16 operations
//   indep_i16  v_pk_min_i16 over eight independent registers
//   dep_min3   dependent v_pk_minimum3_f16
//   indep_min3 v_pk_minimum3_f16 over eight independent registers
// Prints the median over wavefronts of cycles per instruction per SIMD (wave cycles / instructions / wavefronts per SIMD).
// Workgroups of 256 threads, one per CU (96 KB of LDS each) or eight per CU (20 KB each); that eight are resident together is
// what the LDS sizes allow, it is not observed (the clocks of different CUs cannot be compared).
// Build: hipcc -O3 --offload-arch=gfx950 -o pk3_rate tools/probe/pk3_rate.hip ; runs a few milliseconds.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { std::printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); std::exit(1); } } while (0)
constexpr int TRIPS = 64, PER_TRIP = 64;   // .rept 8 x 8 instructions

template <int CHAIN>
__global__ __launch_bounds__(256) void k_chain(uint32_t* out, uint32_t seed) {
  extern __shared__ unsigned char lds_pad[];   // only sets how many workgroups share a CU
  uint32_t r0 = seed + threadIdx.x, r1 = r0 ^ 0x00110022u, r2 = r0 + 3, r3 = r0 + 5, r4 = r0 + 7, r5 = r0 + 11, r6 = r0 + 13, r7 = r0 + 17;
  uint32_t y = 0x64406480u, z = 0x64106420u;
  if (CHAIN >= 2) { r0 = (r0 & 0x00ff00ffu) | 0x64006400u; r1 = (r1 & 0x00ff00ffu) | 0x64006400u; r2 = (r2 & 0x00ff00ffu) | 0x64006400u; r3 = (r3 & 0x00ff00ffu) | 0x64006400u;
                    r4 = (r4 & 0x00ff00ffu) | 0x64006400u; r5 = (r5 & 0x00ff00ffu) | 0x64006400u; r6 = (r6 & 0x00ff00ffu) | 0x64006400u; r7 = (r7 & 0x00ff00ffu) | 0x64006400u; }
  __syncthreads();
  uint64_t t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t0));
#pragma unroll 1
  for (int trip = 0; trip < TRIPS; ++trip) {
    if (CHAIN == 0)
      asm volatile(".rept 64\n v_pk_min_i16 %0, %0, %1\n s_nop 0\n.endr" : "+v"(r0) : "v"(y));
    else if (CHAIN == 1)
      asm volatile(".rept 8\n v_pk_min_i16 %0, %0, %8\n v_pk_min_i16 %1, %1, %8\n v_pk_min_i16 %2, %2, %8\n v_pk_min_i16 %3, %3, %8\n"
                   " v_pk_min_i16 %4, %4, %8\n v_pk_min_i16 %5, %5, %8\n v_pk_min_i16 %6, %6, %8\n v_pk_min_i16 %7, %7, %8\n.endr"
                   : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7) : "v"(y));
    else if (CHAIN == 2)
      asm volatile(".rept 64\n v_pk_minimum3_f16 %0, %0, %1, %2\n.endr" : "+v"(r0) : "v"(y), "v"(z));
    else
      asm volatile(".rept 8\n v_pk_minimum3_f16 %0, %0, %8, %9\n v_pk_minimum3_f16 %1, %1, %8, %9\n v_pk_minimum3_f16 %2, %2, %8, %9\n v_pk_minimum3_f16 %3, %3, %8, %9\n"
                   " v_pk_minimum3_f16 %4, %4, %8, %9\n v_pk_minimum3_f16 %5, %5, %8, %9\n v_pk_minimum3_f16 %6, %6, %8, %9\n v_pk_minimum3_f16 %7, %7, %8, %9\n.endr"
                   : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7) : "v"(y), "v"(z));
  }
  uint64_t t1 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t1));
  const uint32_t keep = r0 ^ r1 ^ r2 ^ r3 ^ r4 ^ r5 ^ r6 ^ r7;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if ((threadIdx.x & 63) == 0) { out[2 * wave] = (uint32_t)(t1 - t0); out[2 * wave + 1] = keep; }
}

template <int CHAIN>
static double run(uint32_t* d_out, int cus, int waves_per_simd) {
  const int block = 256, per_cu = waves_per_simd;                // a workgroup is one wavefront on every SIMD
  const int lds = waves_per_simd == 1 ? 96 * 1024 : 20 * 1024;   // 160 KB per CU: one workgroup of 96 KB, eight of 20 KB
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_chain<CHAIN>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  const int grid = cus * per_cu, waves = grid * block / 64;
  std::vector<uint32_t> h(2 * waves);
  for (int rep = 0; rep < 2; ++rep) {   // the first launch loads the code object
    k_chain<CHAIN><<<grid, block, lds>>>(d_out, 12345u + rep);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
  }
  CK(hipMemcpy(h.data(), d_out, h.size() * 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> t(waves);
  for (int i = 0; i < waves; ++i) t[i] = h[2 * i];
  std::sort(t.begin(), t.end());
  return (double)t[waves / 2] / (TRIPS * PER_TRIP) / waves_per_simd;
}

int main() {
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  uint32_t* d_out; CK(hipMalloc(&d_out, (size_t)cus * 8 * 4 * 2 * 4));   // 8 workgroups x 4 wavefronts x 2 words per CU
  std::printf("%s, %d CUs; cycles per instruction per SIMD (s_memtime, median over wavefronts, %d instructions per wavefront)\n", prop.gcnArchName, cus, TRIPS * PER_TRIP);
  std::printf("%-28s %12s %12s\n", "chain", "1 wave/SIMD", "8 waves/SIMD");
  const char* names[4] = {"dep v_pk_min_i16 + s_nop 0", "indep v_pk_min_i16", "dep v_pk_minimum3_f16", "indep v_pk_minimum3_f16"};
  double r[4][2];
  r[0][0] = run<0>(d_out, cus, 1); r[0][1] = run<0>(d_out, cus, 8);
  r[1][0] = run<1>(d_out, cus, 1); r[1][1] = run<1>(d_out, cus, 8);
  r[2][0] = run<2>(d_out, cus, 1); r[2][1] = run<2>(d_out, cus, 8);
  r[3][0] = run<3>(d_out, cus, 1); r[3][1] = run<3>(d_out, cus, 8);
  for (int i = 0; i < 4; ++i) std::printf("%-28s %12.2f %12.2f\n", names[i], r[i][0], r[i][1]);
  std::printf("three-input over two-input, independent, 8 waves/SIMD: %.2f x (break-even 2.0, stop above about 1.6)\n", r[3][1] / r[1][1]);
  CK(hipFree(d_out));
  return 0;
}
