// Edge-sampling rewiring of BLEND's fully-adjacent layer (reference src/graph_rewiring.py:150-241, src/GNN_KNN.py:65-83), once per
// forward, training included:
//   add_edges      M random pairs (both endpoints uniform, or the anchor drawn from softmax(node importance)) joined to the edge set
//                  in both directions, then torch.unique(dim=1);
//   edge_sampling  keep the columns whose mean attention is >= a quantile (the quantile itself is gnpde_quantile, rewire.hip).
// Pieces here:
//   Philox4x32-10  counter-based generator written out in philox.h (Random123; Salmon et al., SC'11): no state, word i of a stream is a
//                  pure function of (seed, stream, call, i), so a draw does not depend on the launch shape
//   gnpde_random_nodes     j = (word * n) >> 32
//   gnpde_node_importance  mean of att_mean over a node's incoming edges: one wave per column of the graph's CSC view, lane l sums the
//                          entries l, l + 64, ... in CSC order, then a fixed butterfly: no atomics
//   gnpde_sample_nodes     multinomial with replacement in FIXED POINT: w_j = (uint64)(expf(s_j - max s) 2^32), inclusive integer prefix
//                          sums (integer addition is associative: any scan order gives the same bits), draw = first j with
//                          C_j > mulhi64(r, C_n) by binary search
//   gnpde_edge_union       64-bit keys row * n + col, radix sort, unique, decode
//   gnpde_full_adjacency   all n^2 pairs, row-major
// (gnpde_select_edges, the >= compaction, shares the compaction kernels of rewire.hip and lives there.)
// Error conditions that depend on device data set bits of a device flag word (integer atomic OR) that the caller reads.
#include "common.h"
#include "philox.h"
#include "select.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

namespace gnpde {
namespace {

// Philox4x32-10 and stream_block (block `b` of stream (seed, stream, call)) are in philox.h

__global__ __launch_bounds__(kBlock) void philox_words_kernel(u64 seed, unsigned stream, unsigned call, u64 first_block, long long n_words,
                                                             unsigned* __restrict__ out) {
  const long long b = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (4 * b >= n_words) return;
  const Words4 x = stream_block(seed, stream, call, first_block + static_cast<u64>(b));
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (4 * b + w < n_words) out[4 * b + w] = x.w[w];
}

__global__ __launch_bounds__(kBlock) void random_nodes_kernel(unsigned n, long long count, u64 seed, unsigned stream, unsigned call,
                                                             long long* __restrict__ out) {
  const long long b = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (4 * b >= count) return;
  const Words4 x = stream_block(seed, stream, call, static_cast<u64>(b));
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (4 * b + w < count) out[4 * b + w] = static_cast<long long>((static_cast<u64>(x.w[w]) * n) >> 32);
}

// one wave per column: att_mean is in the caller's edge order, the CSC view lists CSR positions, perm turns those into edge ids
__global__ __launch_bounds__(kBlock) void node_importance_kernel(const int* __restrict__ cscptr, const int* __restrict__ cscpos,
                                                                const int* __restrict__ perm, const float* __restrict__ att_mean, int n,
                                                                float* __restrict__ out, int* __restrict__ flag) {
  const long long j = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (j >= n) return;
  const int lane = threadIdx.x & 63;
  const int b = cscptr[j], e = cscptr[j + 1];
  float sum = 0.0f;
  for (int p = b + lane; p < e; p += kWave) sum += att_mean[perm[cscpos[p]]];
  sum = wave_sum(sum);
  if (lane == 0) {
    if (e == b) {
      atomicOr(flag, GNPDE_SAMPLING_EMPTY_COLUMN);
      out[j] = 0.0f;
    } else {
      out[j] = sum / static_cast<float>(e - b);
    }
  }
}

// maximum of the logits as an integer maximum of their order-preserving images (order of arrival does not matter); *maxkey starts at 0
__global__ __launch_bounds__(kBlock) void logit_max_kernel(const float* __restrict__ s, int n, unsigned* __restrict__ maxkey,
                                                          int* __restrict__ flag) {
  __shared__ unsigned red[kWavesPerBlock];
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  unsigned best = 0;
  bool bad = false;
  for (long long j = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; j < n; j += stride) {
    const float v = s[j];
    if (!isfinite(v)) bad = true;
    else best = max(best, ordered_key(v));
  }
  if (bad) atomicOr(flag, GNPDE_SAMPLING_NONFINITE);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) best = max(best, static_cast<unsigned>(__shfl_xor(best, off, kWave)));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(maxkey, max(max(red[0], red[1]), max(red[2], red[3])));
}

// t = expf(s - max) is in [0, 1]; t * 2^32 is exact in fp32 (a power-of-two scaling) and an integer after the truncation
__global__ __launch_bounds__(kBlock) void logit_weights_kernel(const float* __restrict__ s, int n, const unsigned* __restrict__ maxkey,
                                                              u64* __restrict__ w) {
  const long long j = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  const unsigned mk = *maxkey;
  const float v = s[j];
  u64 q = 0;
  if (mk != 0 && isfinite(v)) {
    const float t = expf(v - ordered_value(mk));
    q = static_cast<u64>(fminf(t, 1.0f) * 4294967296.0f);
  }
  w[j] = q;
}

// draws 2 b and 2 b + 1 from block b: r = (word 0 << 32 | word 1), (word 2 << 32 | word 3)
__global__ __launch_bounds__(kBlock) void sample_nodes_kernel(const u64* __restrict__ cum, int n, long long count, u64 seed, unsigned stream,
                                                             unsigned call, long long* __restrict__ out, int* __restrict__ flag) {
  const long long b = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (2 * b >= count) return;
  const u64 total = cum[n - 1];
  if (total == 0) {
    if (b == 0) atomicOr(flag, GNPDE_SAMPLING_ZERO_MASS);
    out[2 * b] = 0;
    if (2 * b + 1 < count) out[2 * b + 1] = 0;
    return;
  }
  const Words4 x = stream_block(seed, stream, call, static_cast<u64>(b));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (2 * b + h >= count) break;
    const u64 r = (static_cast<u64>(x.w[2 * h]) << 32) | x.w[2 * h + 1];
    const u64 target = __umul64hi(r, total);      // < total = cum[n - 1]: the search below always ends inside [0, n)
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cum[mid] > target) hi = mid;
      else lo = mid + 1;
    }
    out[2 * b + h] = lo;
  }
}

__global__ __launch_bounds__(kBlock) void union_keys_kernel(const long long* __restrict__ a, long long ea, const long long* __restrict__ b,
                                                           long long eb, long long n, u64* __restrict__ keys, int* __restrict__ flag) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= ea + eb) return;
  long long r, c;
  if (i < ea) {
    r = a[i]; c = a[ea + i];
  } else {
    r = b[i - ea]; c = b[eb + (i - ea)];
  }
  u64 key = 0;
  if (r < 0 || r >= n || c < 0 || c >= n) atomicOr(flag, GNPDE_SAMPLING_INDEX_RANGE);
  else key = static_cast<u64>(r) * static_cast<u64>(n) + static_cast<u64>(c);
  keys[i] = key;
}

__global__ __launch_bounds__(kBlock) void union_decode_kernel(const u64* __restrict__ keys, const long long* __restrict__ count, long long cap,
                                                             u64 n, long long* __restrict__ out) {
  long long m = *count;
  if (m > cap) m = cap;
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += stride) {
    const u64 key = keys[i];
    const u64 r = key / n;
    out[i] = static_cast<long long>(r);
    out[cap + i] = static_cast<long long>(key - r * n);
  }
}

__global__ __launch_bounds__(kBlock) void full_adjacency_kernel(long long n, long long* __restrict__ out) {
  const long long total = n * n;
  const long long stride = static_cast<long long>(gridDim.x) * kBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += stride) {
    const long long r = i / n;
    out[i] = r;
    out[total + i] = i - r * n;
  }
}

inline dim3 grid_of(long long items, long long cap = 0) {
  long long b = (items + kBlock - 1) / kBlock;
  if (cap > 0 && b > cap) b = cap;
  if (b < 1) b = 1;
  return dim3(static_cast<unsigned>(b));
}

struct SampleLayout {
  size_t maxkey, w, cum, temp, temp_bytes, total;   // total == 0: the temp-size query failed
};

SampleLayout sample_layout(int n) {
  SampleLayout L{};
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  L.maxkey = take(4);
  L.w = take(nn * 8);
  L.cum = take(nn * 8);
  size_t t = 0;
  u64* p = nullptr;
  if (rocprim::inclusive_scan(nullptr, t, p, p, nn, rocprim::plus<u64>(), nullptr) != hipSuccess) return L;
  L.temp_bytes = align_up(t + 256, 256);
  L.temp = take(L.temp_bytes);
  L.total = off;
  return L;
}

struct UnionLayout {
  size_t keys, sorted, uniq, temp, temp_bytes, total;   // total == 0: a temp-size query failed
};

UnionLayout union_layout(long long e) {
  UnionLayout L{};
  const size_t ee = static_cast<size_t>(e > 0 ? e : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  L.keys = take(ee * 8);
  L.sorted = take(ee * 8);
  L.uniq = take(ee * 8);
  size_t t1 = 0, t2 = 0;
  u64* p = nullptr;
  size_t* c = nullptr;
  if (rocprim::radix_sort_keys(nullptr, t1, p, p, ee, 0, 64, nullptr) != hipSuccess) return L;
  if (rocprim::unique(nullptr, t2, p, p, c, ee, rocprim::equal_to<u64>(), nullptr) != hipSuccess) return L;
  L.temp_bytes = align_up((t1 > t2 ? t1 : t2) + 256, 256);
  L.temp = take(L.temp_bytes);
  L.total = off;
  return L;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" int gnpde_philox_words(uint64_t seed, uint32_t stream_id, uint32_t call, uint64_t first_block, int64_t n_words, uint32_t* out,
                                  void* stream) {
  GNPDE_CHECK_ARG(n_words >= 0 && (n_words == 0 || out), GNPDE_EINVAL, "philox_words: bad arguments");
  if (n_words == 0) return 0;
  hipLaunchKernelGGL(philox_words_kernel, grid_of((n_words + 3) / 4), dim3(kBlock), 0, static_cast<hipStream_t>(stream), seed, stream_id, call,
                     first_block, static_cast<long long>(n_words), out);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_random_nodes(int32_t n, int64_t count, uint64_t seed, uint32_t stream_id, uint32_t call, int64_t* out, void* stream) {
  GNPDE_CHECK_ARG(n >= 1 && count >= 0 && (count == 0 || out), GNPDE_EINVAL, "random_nodes: bad arguments (1 <= n <= INT32_MAX, count >= 0)");
  if (count == 0) return 0;
  hipLaunchKernelGGL(random_nodes_kernel, grid_of((count + 3) / 4), dim3(kBlock), 0, static_cast<hipStream_t>(stream), static_cast<unsigned>(n),
                     static_cast<long long>(count), seed, stream_id, call, reinterpret_cast<long long*>(out));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_node_importance(const gnpde_graph_t* g, const float* att_mean, float* out, int32_t* flag, void* stream) {
  GNPDE_CHECK_ARG(g && out && flag && g->n >= 1 && g->e >= 0 && g->cscptr && (g->e == 0 || (att_mean && g->cscpos && g->perm)), GNPDE_EINVAL,
                  "node_importance: bad arguments (the graph needs its CSC view)");
  hipLaunchKernelGGL(node_importance_kernel, grid_of(static_cast<long long>(g->n) * kWave), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     g->cscptr, g->cscpos, g->perm, att_mean, g->n, out, flag);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnpde_sample_nodes_workspace_bytes(int32_t n) {
  if (n < 1) return 0;
  return sample_layout(n).total;
}

extern "C" int gnpde_sample_nodes(const float* logits, int32_t n, int64_t count, uint64_t seed, uint32_t stream_id, uint32_t call, int64_t* out,
                                  int32_t* flag, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(logits && n >= 1 && count >= 0 && flag && (count == 0 || out), GNPDE_EINVAL, "sample_nodes: bad arguments");
  if (count == 0) return 0;
  const SampleLayout L = sample_layout(n);
  GNPDE_CHECK_ARG(L.total != 0, GNPDE_ESTATE, "sample_nodes: the scan's temporary-storage query failed");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= L.total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "sample_nodes: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, L.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  unsigned* maxkey = reinterpret_cast<unsigned*>(ws + L.maxkey);
  u64* w = reinterpret_cast<u64*>(ws + L.w);
  u64* cum = reinterpret_cast<u64*>(ws + L.cum);
  GNPDE_HIP(hipMemsetAsync(maxkey, 0, 4, s));
  hipLaunchKernelGGL(logit_max_kernel, grid_of(n, 1024), dim3(kBlock), 0, s, logits, n, maxkey, flag);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(logit_weights_kernel, grid_of(n), dim3(kBlock), 0, s, logits, n, maxkey, w);
  GNPDE_LAUNCH_CHECK();
  size_t tb = L.temp_bytes;
  GNPDE_HIP(rocprim::inclusive_scan(ws + L.temp, tb, w, cum, static_cast<size_t>(n), rocprim::plus<u64>(), s));
  hipLaunchKernelGGL(sample_nodes_kernel, grid_of((count + 1) / 2), dim3(kBlock), 0, s, cum, n, static_cast<long long>(count), seed, stream_id,
                     call, reinterpret_cast<long long*>(out), flag);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnpde_edge_union_workspace_bytes(int64_t n_a, int64_t n_b) {
  if (n_a < 0 || n_b < 0) return 0;
  return union_layout(n_a + n_b).total;
}

extern "C" int gnpde_edge_union(const int64_t* a, int64_t n_a, const int64_t* b, int64_t n_b, int32_t n_nodes, int64_t* out_edge_index,
                                int64_t* out_count, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(n_a >= 0 && n_b >= 0 && n_nodes >= 1 && out_count && flag && (n_a == 0 || a) && (n_b == 0 || b), GNPDE_EINVAL,
                  "edge_union: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long e = n_a + n_b;
  if (e == 0) {
    GNPDE_HIP(hipMemsetAsync(out_count, 0, sizeof(int64_t), s));
    return 0;
  }
  GNPDE_CHECK_ARG(out_edge_index, GNPDE_EINVAL, "edge_union: no output");
  const UnionLayout L = union_layout(e);
  GNPDE_CHECK_ARG(L.total != 0, GNPDE_ESTATE, "edge_union: the sort's temporary-storage query failed");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= L.total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "edge_union: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, L.total);
  char* ws = static_cast<char*>(workspace);
  u64* keys = reinterpret_cast<u64*>(ws + L.keys);
  u64* sorted = reinterpret_cast<u64*>(ws + L.sorted);
  u64* uniq = reinterpret_cast<u64*>(ws + L.uniq);
  hipLaunchKernelGGL(union_keys_kernel, grid_of(e), dim3(kBlock), 0, s, reinterpret_cast<const long long*>(a), static_cast<long long>(n_a),
                     reinterpret_cast<const long long*>(b), static_cast<long long>(n_b), static_cast<long long>(n_nodes), keys, flag);
  GNPDE_LAUNCH_CHECK();
  unsigned bits = 1;                                             // keys are < n^2 < 2^62
  const u64 top = static_cast<u64>(n_nodes) * static_cast<u64>(n_nodes) - 1;
  while (bits < 64 && (top >> bits) != 0) ++bits;
  size_t tb = L.temp_bytes;
  GNPDE_HIP(rocprim::radix_sort_keys(ws + L.temp, tb, keys, sorted, static_cast<size_t>(e), 0, bits, s));
  tb = L.temp_bytes;
  static_assert(sizeof(size_t) == sizeof(int64_t), "the unique count is written as a 64-bit word");
  GNPDE_HIP(rocprim::unique(ws + L.temp, tb, sorted, uniq, reinterpret_cast<size_t*>(out_count), static_cast<size_t>(e),
                            rocprim::equal_to<u64>(), s));
  hipLaunchKernelGGL(union_decode_kernel, grid_of(e, 4096), dim3(kBlock), 0, s, uniq, reinterpret_cast<const long long*>(out_count), e,
                     static_cast<u64>(n_nodes), reinterpret_cast<long long*>(out_edge_index));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_full_adjacency(int32_t n, int64_t* out_edge_index, void* stream) {
  GNPDE_CHECK_ARG(n >= 1 && out_edge_index, GNPDE_EINVAL, "full_adjacency: bad arguments");
  hipLaunchKernelGGL(full_adjacency_kernel, grid_of(static_cast<long long>(n) * n, 4096), dim3(kBlock), 0, static_cast<hipStream_t>(stream),
                     static_cast<long long>(n), reinterpret_cast<long long*>(out_edge_index));
  GNPDE_LAUNCH_CHECK();
  return 0;
}
