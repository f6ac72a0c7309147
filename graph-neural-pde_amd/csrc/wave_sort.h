// Single-wave bitonic sort of 64-bit keys in LDS, shared by the selection kernels (knn.hip, gdc.hip).
#pragma once
#include "common.h"

namespace gnpde {
namespace {

typedef unsigned long long u64;

// LDS traffic of ONE wave on rows no other wave touches: program order is enough for the hardware, the fence keeps the
// compiler (and the LDS counter) in line
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ascending bitonic sort of b[0 .. P) (P a power of two >= 2) by one wave
__device__ __forceinline__ void wave_sort(u64* b, int P, int lane) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = lane; p < (P >> 1); p += kWave) {
        const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));
        const int j = i | stride;
        const bool up = (i & size) == 0;
        const u64 a = b[i], c = b[j];
        if ((a > c) == up) {
          b[i] = c;
          b[j] = a;
        }
      }
      wave_lds_sync();
    }
  }
}

}  // namespace
}  // namespace gnpde
