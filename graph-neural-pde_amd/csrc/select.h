// The selection primitives of the rewiring kernels, each stated once: order-preserving float keys, the histogram bin that holds a
// rank, the column-split rule of the tile sweeps, a single-wave bitonic sort of 64-bit keys in LDS with "keep the k best" and "merge
// S sorted lists" on it, one chunk of a one-workgroup scan, ballot + popcount slots, the whole-wave sum.  The first part is plain
// C++ -- no HIP header -- so that a host compiler builds it into tests/select_probe.cpp; the second exists under hipcc only.
#pragma once

#if defined(__HIPCC__)
#define GNPDE_HD __host__ __device__
#else
#define GNPDE_HD
#endif

namespace gnpde {

typedef unsigned long long u64;

// monotone on the floats without NaNs: a < b  <=>  ordered_key(a) < ordered_key(b), with -0 < +0; ordered_value inverts it
GNPDE_HD inline unsigned ordered_key(float f) {
  unsigned u;
  __builtin_memcpy(&u, &f, sizeof(u));
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
GNPDE_HD inline float ordered_value(unsigned k) {
  const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  __builtin_memcpy(&f, &u, sizeof(f));
  return f;
}

// the first bin of hist[begin .. end) at which the counts summed from `begin` exceed *rank; *rank becomes the rank inside that bin.
// Counts that never exceed the rank (a rank past the total) give the last bin and the rank less every count.
GNPDE_HD inline int rank_bin(const u64* hist, int begin, int end, u64* rank) {
  u64 r = *rank;
  int b = begin;
  while (b < end && r >= hist[b]) r -= hist[b++];
  *rank = r;
  return b < end ? b : end - 1;
}

// the smallest power of two >= max(c, 2): the length a bitonic sort of c keys is padded to
GNPDE_HD inline int sort_length(int c) {
  int P = 2;
  while (P < c) P <<= 1;
  return P;
}

constexpr int kKeyTile = 64;         // rows and columns of a key tile (knn_tile.h)

// Column splits of a tile sweep over n x n keys: one when the row tiles alone give every CU per_cu workgroups, otherwise enough to
// reach that; forced > 0 (gnpde_tune(19, S)) replaces the rule.  Never more than max_splits, than max_by_keys (what the merge of
// the partial lists holds) or than there are column tiles; splits that would get no column tile are dropped.
GNPDE_HD inline int column_splits(long long n, int per_cu, int max_splits, int max_by_keys, int cus, int forced) {
  const long long tiles = (n + kKeyTile - 1) / kKeyTile, want = static_cast<long long>(per_cu) * cus;
  long long s = forced;
  if (s <= 0) s = tiles >= want ? 1 : (want + tiles - 1) / tiles;
  if (s > max_splits) s = max_splits;
  if (s > max_by_keys) s = max_by_keys;
  if (s > tiles) s = tiles;
  if (s < 1) s = 1;
  const long long per = (tiles + s - 1) / s;
  return static_cast<int>((tiles + per - 1) / per);
}

}  // namespace gnpde

#if defined(__HIPCC__)
#include "common.h"

namespace gnpde {
namespace {

constexpr u64 kPadKey = ~0ull;       // sorts after every key

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

// sort the buffer's cnt keys (the caller has put a wave_lds_sync behind other lanes' stores into it); returns min(cnt, k), the
// keys that stay: buf[k - 1] is the k-th best once k are known
__device__ __forceinline__ int wave_keep_best(u64* buf, int cnt, int k, int lane) {
  const int P = sort_length(cnt);
  for (int p = cnt + lane; p < P; p += kWave) buf[p] = kPadKey;
  wave_lds_sync();
  wave_sort(buf, P, lane);
  return cnt < k ? cnt : k;
}

// buf[0 .. P) = the keys of S lists of k keys each (list s starts at lists + s * stride), padded and sorted; P = sort_length(S * k)
__device__ __forceinline__ void wave_merge_lists(u64* buf, int P, const u64* __restrict__ lists, long long stride, int S, int k,
                                                 int lane) {
  const int total = S * k;
  for (int p = lane; p < P; p += kWave) {
    u64 key = kPadKey;
    if (p < total) {
      const int s = p / k;
      key = lists[s * stride + (p - s * k)];
    }
    buf[p] = key;
  }
  wave_lds_sync();
  wave_sort(buf, P, lane);
}

// One chunk of a one-workgroup scan (all kBlock threads call it): returns *carry + the sum of v over the lower threads and advances
// *carry by the chunk's total.  buf: kBlock values of LDS.  *carry is the thread's own copy or one LDS word: every thread reads it
// before the last barrier and writes one value behind it; the next chunk's first barrier orders that write before the next read.
template <class T, class C>
__device__ __forceinline__ C block_scan_exclusive(T v, T* buf, C* carry) {
  const int tid = threadIdx.x;
  buf[tid] = v;
  __syncthreads();
  for (int off = 1; off < kBlock; off <<= 1) {   // Hillis-Steele inclusive scan
    const T add = tid >= off ? buf[tid - off] : 0;
    __syncthreads();
    buf[tid] += add;
    __syncthreads();
  }
  const C base = *carry;
  const C before = base + buf[tid] - v;
  const C next = base + buf[kBlock - 1];
  __syncthreads();
  *carry = next;
  return before;
}

// the slot of a kept entry among its wave's kept entries (every lane calls): the number of lower lanes with ok; *count = all of them
__device__ __forceinline__ int wave_rank(bool ok, int lane, int* count) {
  const u64 m = __ballot(ok);
  *count = __popcll(m);
  return __popcll(m & ((1ull << lane) - 1ull));
}

// the same among the 16 lanes 16 q + r (r = 0 .. 15) that hold one row of a 16 x 16 matrix-core tile
__device__ __forceinline__ int group16_rank(bool ok, int q, int r, int* count) {
  const unsigned g = static_cast<unsigned>(__ballot(ok) >> (16 * q)) & 0xffffu;
  *count = __popc(g);
  return __popc(g & ((1u << r) - 1u));
}

// the sum over the wave's 64 lanes in a fixed order (offsets 32 down to 1), the same value in every lane
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

}  // namespace
}  // namespace gnpde
#endif
