// What the walk-staged training steps share (deepwalk.hip: skip-gram + SparseAdam; hyperbolic.hip: Poincare RSGD): the window
// geometry of include/gnpde.h, the workspace of a step (slot keys, their sorted copy = the inverted index, one contribution row per
// walk position, one partial loss per walk, the sort's temporary storage) and the fixed-order loss reduction.
#pragma once
#include "common.h"
#include "select.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace gnpde {
namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// Windows: J = L + 2 - C per walk, the position pairs (a, b) with 0 <= a < J and a < b <= a + C - 1; pair (a, b) has the index
// a (C - 1) + (b - a - 1).  Position p meets the positions q != p with |p - q| <= C - 1 and min(p, q) < J.
__host__ __device__ __forceinline__ int window_pair_index(int a, int b, int C) { return a * (C - 1) + (b - a - 1); }

// the number of pair ends at position p: it depends on (p, L, C) alone
__host__ __device__ __forceinline__ int window_pair_ends(int p, int L, int C) {
  const int J = L + 2 - C;
  const int above = p < J ? C - 1 : 0;                                       // pairs (p, b)
  const int lo = p - (C - 1) > 0 ? p - (C - 1) : 0, hi = (p - 1 < J - 1 ? p - 1 : J - 1);
  return above + (hi >= lo ? hi - lo + 1 : 0);                               // pairs (a, p)
}

struct StepLayout {
  size_t keys, sorted, contrib, partial, temp, temp_bytes, total;   // total == 0: the temp-size query failed
};

// row_floats: the floats of one contribution row
inline StepLayout step_layout(long long r_tot, int L, int row_floats) {
  StepLayout Y{};
  const size_t S = static_cast<size_t>(r_tot) * (L + 1);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  Y.keys = take(S * 8);
  Y.sorted = take(S * 8);
  Y.contrib = take(S * row_floats * 4);
  Y.partial = take(static_cast<size_t>(r_tot) * 8);
  size_t t = 0;
  u64* p = nullptr;
  if (rocprim::radix_sort_keys(nullptr, t, p, p, S, 0, 64, nullptr) != hipSuccess) return Y;
  Y.temp_bytes = align_up(t + 256, 256);
  Y.temp = take(Y.temp_bytes);
  Y.total = off;
  return Y;
}

// the bits of the (node << 32 | slot) keys that the sort has to look at
inline unsigned slot_key_bits(int n) {
  unsigned bits = 1;
  while (bits < 32 && ((static_cast<u64>(n) - 1) >> bits) != 0) ++bits;
  return 32 + bits;
}

// one workgroup: thread t adds the partials t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(kBlock) void loss_kernel(const double* __restrict__ partial, long long r_pos, long long r_neg, float* __restrict__ out) {
  __shared__ double red[kBlock];
  double s = 0.0;
  for (long long i = threadIdx.x; i < r_pos + r_neg; i += kBlock) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kBlock >> 1; w >= 1; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = static_cast<float>(red[0]);
}

}  // namespace
}  // namespace gnpde
