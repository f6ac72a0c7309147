// Edge-set bookkeeping of the hard-attention and rewiring blocks, once per TRAINING forward:
//   threshold = torch.quantile(score, q); mask = score > threshold; edge_index[:, mask]; renormalise the kept scores by
//   their sum per endpoint   (reference src/block_transformer_hard_attention.py:48-66,
//                             src/block_transformer_rewiring.py:40-50,154-183).
// The reference (and round 1 of this package) does this with a full sort (torch.quantile), boolean indexing (two
// compactions through nonzero) and a scatter-add.  Here:
//   gnpde_quantile        two order statistics by a 4-pass 8-bit radix SELECT on the order-preserving integer image of the
//                         floats (histograms by integer atomics: order-independent, hence exact and deterministic), then
//                         torch's linear interpolation IN FLOAT32 as torch.quantile computes it (rank = fl32(q) * fl32(n-1)),
//                         so that the kept edge set equals the reference's bit for bit;
//   gnpde_select_edges    the same stable compaction with score >= threshold and nothing else (edge_sampling of the fully-adjacent
//                         layer, reference src/graph_rewiring.py:157-169): no weights, no renormalisation;
//   gnpde_threshold_edges one stable stream compaction of (row, col, score) -- block counts, one-block scan, scatter -- and
//                         the per-endpoint renormalisation (sums by float atomics, as the reference's scatter-add on a GPU).
// 10 passes over [E] floats instead of a sort: ~40 us at the ogbn-arxiv shape.
#include "common.h"
#include "select.h"

namespace gnpde {
namespace {

// select state in device memory: two ranks searched at once
struct SelectState {
  unsigned prefix[2];        // bits found so far (high to low)
  unsigned long long k[2];   // rank among the elements that share the prefix
  unsigned long long hist[2][256];   // 64-bit: the values fed piece by piece (gnpde_rank_select_hist) can pass 2^32 in all
};

__global__ __launch_bounds__(kBlock) void select_init_kernel(SelectState* st, unsigned long long k0, unsigned long long k1) {
  if (threadIdx.x == 0) {
    st->prefix[0] = st->prefix[1] = 0;
    st->k[0] = k0;
    st->k[1] = k1;
  }
  for (int i = threadIdx.x; i < 512; i += blockDim.x) (&st->hist[0][0])[i] = 0;
}

// histogram of the digit at `shift` over the elements whose higher bits equal the prefix (per searched rank)
__global__ __launch_bounds__(kBlock) void select_hist_kernel(const float* __restrict__ v, long long n, SelectState* st, int shift) {
  __shared__ unsigned h[2][256];
  for (int i = threadIdx.x; i < 512; i += blockDim.x) (&h[0][0])[i] = 0;
  __syncthreads();
  const unsigned hi_mask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
  const unsigned p0 = st->prefix[0], p1 = st->prefix[1];
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned key = ordered_key(v[i]);
    const unsigned digit = (key >> shift) & 255u;
    if ((key & hi_mask) == p0) atomicAdd(&h[0][digit], 1u);
    if ((key & hi_mask) == p1) atomicAdd(&h[1][digit], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += blockDim.x) {
    const unsigned c = (&h[0][0])[i];
    if (c) atomicAdd(&(&st->hist[0][0])[i], static_cast<unsigned long long>(c));
  }
}

// pick the digit that contains the searched rank, extend the prefix, clear the histogram for the next pass
__global__ __launch_bounds__(64) void select_pick_kernel(SelectState* st, int shift) {
  const int r = threadIdx.x;
  if (r < 2) {
    const unsigned digit = rank_bin(st->hist[r], 0, 256, &st->k[r]);
    st->prefix[r] |= digit << shift;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += blockDim.x) (&st->hist[0][0])[i] = 0;
}

// torch's lerp of the two order statistics (aten lerp: the branch keeps it monotone and exact at both ends)
__global__ void select_finish_kernel(const SelectState* st, float w, float* out) {
  const float lo = ordered_value(st->prefix[0]), hi = ordered_value(st->prefix[1]);
  const float diff = hi - lo;
  *out = w < 0.5f ? lo + w * diff : hi - diff * (1.0f - w);
}

constexpr int kItems = 16;                   // elements per thread of the compaction
constexpr int kTile = kBlock * kItems;       // per block

// kInclusive: keep score >= threshold (gnpde_select_edges) instead of score > threshold (gnpde_threshold_edges)
template <bool kInclusive>
__device__ __forceinline__ bool kept(float score, float t) { return kInclusive ? score >= t : score > t; }

template <bool kInclusive>
__global__ __launch_bounds__(kBlock) void keep_count_kernel(const float* __restrict__ score, long long n,
                                                           const float* __restrict__ thr, unsigned* __restrict__ counts) {
  __shared__ unsigned red[kWavesPerBlock];
  const float t = *thr;
  const long long base = static_cast<long long>(blockIdx.x) * kTile;
  unsigned c = 0;
  for (int j = 0; j < kItems; ++j) {
    const long long i = base + static_cast<long long>(j) * kBlock + threadIdx.x;
    if (i < n && kept<kInclusive>(score[i], t)) ++c;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// exclusive scan of the block counts (one block; sequential over chunks of 256 blocks), total -> *out_count
__global__ __launch_bounds__(kBlock) void keep_scan_kernel(unsigned* __restrict__ counts, int n_blocks, long long* out_count) {
  __shared__ unsigned buf[kBlock];
  __shared__ unsigned long long carry;
  if (threadIdx.x == 0) carry = 0;    // (read behind the scan's first barrier)
  for (int b0 = 0; b0 < n_blocks; b0 += kBlock) {
    const int i = b0 + threadIdx.x;
    const unsigned c = i < n_blocks ? counts[i] : 0;
    const unsigned long long before = block_scan_exclusive(c, buf, &carry);
    if (i < n_blocks) counts[i] = static_cast<unsigned>(before);
  }
  if (threadIdx.x == 0) *out_count = static_cast<long long>(carry);
}

// stable scatter of the kept entries: order inside a block = (item j, thread) = ascending original index; out_w may be NULL
template <bool kInclusive>
__global__ __launch_bounds__(kBlock) void keep_scatter_kernel(const long long* __restrict__ ei, const float* __restrict__ score,
                                                             long long n, const float* __restrict__ thr,
                                                             const unsigned* __restrict__ offsets, long long* __restrict__ out_ei,
                                                             long long out_stride, float* __restrict__ out_w) {
  __shared__ unsigned wave_cnt[kWavesPerBlock];
  __shared__ unsigned running;
  const float t = *thr;
  const long long base = static_cast<long long>(blockIdx.x) * kTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) running = offsets[blockIdx.x];
  __syncthreads();
  for (int j = 0; j < kItems; ++j) {
    const long long i = base + static_cast<long long>(j) * kBlock + threadIdx.x;
    const bool keep = i < n && kept<kInclusive>(score[i], t);
    int wave_kept;
    const unsigned before = wave_rank(keep, lane, &wave_kept);
    if (lane == 0) wave_cnt[wave] = wave_kept;
    __syncthreads();
    unsigned wave_off = 0;
    for (int w = 0; w < wave; ++w) wave_off += wave_cnt[w];
    const unsigned pos = running + wave_off + before;
    if (keep) {
      out_ei[pos] = ei[i];
      out_ei[out_stride + pos] = ei[n + i];
      if (out_w) out_w[pos] = score[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) running += (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void endpoint_sum_kernel(const long long* __restrict__ endpoint, const float* __restrict__ w,
                                                             const long long* __restrict__ count, float* __restrict__ sums) {
  const long long n = *count;
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    atomicAdd(&sums[endpoint[i]], w[i]);
}

__global__ __launch_bounds__(kBlock) void endpoint_div_kernel(const long long* __restrict__ endpoint, float* __restrict__ w,
                                                             const long long* __restrict__ count, const float* __restrict__ sums) {
  const long long n = *count;
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    w[i] = w[i] / (sums[endpoint[i]] + 1e-16f);
}

inline unsigned grid_for(long long n) {
  long long b = (n + kBlock - 1) / kBlock;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return static_cast<unsigned>(b);
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_quantile_workspace_bytes(void) { return align_up(sizeof(SelectState), 256); }

extern "C" int gnpde_quantile(const float* v, int64_t n, double q, float* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  GNPDE_CHECK_ARG(v && out && n >= 1 && q >= 0.0 && q <= 1.0, GNPDE_EINVAL, "quantile: bad arguments");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= sizeof(SelectState), GNPDE_EWS, "quantile: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  SelectState* st = static_cast<SelectState*>(workspace);
  // torch.quantile (aten Sorting.cpp quantile_compute): rank = q * (n - 1) evaluated in the input's dtype, float32
  const float rank = static_cast<float>(q) * static_cast<float>(n - 1);
  const float lo = floorf(rank), hi = ceilf(rank);
  long long k0 = static_cast<long long>(lo), k1 = static_cast<long long>(hi);
  if (k0 > n - 1) k0 = n - 1;
  if (k1 > n - 1) k1 = n - 1;
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(kBlock), 0, s, st, static_cast<unsigned long long>(k0),
                     static_cast<unsigned long long>(k1));
  GNPDE_LAUNCH_CHECK();
  for (int shift = 24; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, v, static_cast<long long>(n), st, shift);
    GNPDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(64), 0, s, st, shift);
    GNPDE_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(1), 0, s, st, rank - lo, out);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

// the select of gnpde_quantile with the caller's two ascending ranks, fed piece by piece (the histogram kernel ADDS to the state):
// begin, then for pass 0 .. 3: hist over every piece, pick; then values.  Graph diffusion rewiring's threshold by avg_degree.
__global__ void select_values_kernel(const SelectState* st, float* out) {
  out[0] = ordered_value(st->prefix[0]);
  out[1] = ordered_value(st->prefix[1]);
}

extern "C" int gnpde_rank_select_begin(int64_t k0, int64_t k1, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(k0 >= 0 && k1 >= 0, GNPDE_EINVAL, "rank_select_begin: negative rank");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= sizeof(SelectState), GNPDE_EWS, "rank_select_begin: workspace too small");
  hipLaunchKernelGGL(select_init_kernel, dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream), static_cast<SelectState*>(workspace),
                     static_cast<unsigned long long>(k0), static_cast<unsigned long long>(k1));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_rank_select_hist(const float* v, int64_t n, int32_t pass, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(v && n >= 1 && pass >= 0 && pass <= 3, GNPDE_EINVAL, "rank_select_hist: bad arguments");
  // a workgroup counts its share of ONE piece in 32 bits (LDS); the state's totals over all pieces are 64-bit
  GNPDE_CHECK_ARG(n <= (1ll << 32), GNPDE_ESHAPE, "rank_select_hist: a piece of %lld values exceeds 2^32 (feed smaller pieces)", static_cast<long long>(n));
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= sizeof(SelectState), GNPDE_EWS, "rank_select_hist: workspace too small");
  hipLaunchKernelGGL(select_hist_kernel, dim3(grid_for(n)), dim3(kBlock), 0, static_cast<hipStream_t>(stream), v, static_cast<long long>(n),
                     static_cast<SelectState*>(workspace), 24 - 8 * pass);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_rank_select_pick(int32_t pass, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(pass >= 0 && pass <= 3, GNPDE_EINVAL, "rank_select_pick: pass = %d outside 0 .. 3", pass);
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= sizeof(SelectState), GNPDE_EWS, "rank_select_pick: workspace too small");
  hipLaunchKernelGGL(select_pick_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<SelectState*>(workspace),
                     24 - 8 * pass);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_rank_select_values(float* out, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(out != nullptr, GNPDE_EINVAL, "rank_select_values: null output");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= sizeof(SelectState), GNPDE_EWS, "rank_select_values: workspace too small");
  hipLaunchKernelGGL(select_values_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), static_cast<const SelectState*>(workspace), out);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnpde_threshold_edges_workspace_bytes(int64_t n_edges, int32_t n_nodes) {
  const long long blocks = (n_edges + kTile - 1) / kTile;
  return align_up(static_cast<size_t>(blocks > 0 ? blocks : 1) * 4, 256) + align_up(static_cast<size_t>(n_nodes > 0 ? n_nodes : 1) * 4, 256);
}

extern "C" int gnpde_threshold_edges(const int64_t* edge_index, const float* score, int64_t n_edges, const float* threshold,
                                     int32_t norm_idx, int32_t n_nodes, int64_t* out_edge_index, float* out_weight,
                                     int64_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(edge_index && score && threshold && out_edge_index && out_weight && out_count && n_edges >= 0 && n_nodes >= 1 &&
                  (norm_idx == 0 || norm_idx == 1), GNPDE_EINVAL, "threshold_edges: bad arguments");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= gnpde_threshold_edges_workspace_bytes(n_edges, n_nodes), GNPDE_EWS,
                  "threshold_edges: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long blocks = (n_edges + kTile - 1) / kTile;
  unsigned* counts = static_cast<unsigned*>(workspace);
  float* sums = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_up(static_cast<size_t>(blocks > 0 ? blocks : 1) * 4, 256));
  if (n_edges == 0) {
    GNPDE_HIP(hipMemsetAsync(out_count, 0, sizeof(int64_t), s));
    return 0;
  }
  const long long* ei = reinterpret_cast<const long long*>(edge_index);
  long long* oe = reinterpret_cast<long long*>(out_edge_index);
  hipLaunchKernelGGL(keep_count_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, score, static_cast<long long>(n_edges),
                     threshold, counts);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(kBlock), 0, s, counts, static_cast<int>(blocks), reinterpret_cast<long long*>(out_count));
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(keep_scatter_kernel<false>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, ei, score,
                     static_cast<long long>(n_edges), threshold, counts, oe, static_cast<long long>(n_edges), out_weight);
  GNPDE_LAUNCH_CHECK();
  GNPDE_HIP(hipMemsetAsync(sums, 0, static_cast<size_t>(n_nodes) * 4, s));
  const long long* endpoint = oe + (norm_idx == 0 ? 0 : n_edges);
  hipLaunchKernelGGL(endpoint_sum_kernel, dim3(grid_for(n_edges)), dim3(kBlock), 0, s, endpoint, out_weight,
                     reinterpret_cast<const long long*>(out_count), sums);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(endpoint_div_kernel, dim3(grid_for(n_edges)), dim3(kBlock), 0, s, endpoint, out_weight,
                     reinterpret_cast<const long long*>(out_count), sums);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnpde_select_edges_workspace_bytes(int64_t n_edges) {
  const long long blocks = (n_edges + kTile - 1) / kTile;
  return align_up(static_cast<size_t>(blocks > 0 ? blocks : 1) * 4, 256);
}

extern "C" int gnpde_select_edges(const int64_t* edge_index, const float* score, int64_t n_edges, const float* threshold,
                                  int64_t* out_edge_index, int64_t* out_count, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(out_count && n_edges >= 0 && (n_edges == 0 || (edge_index && score && threshold && out_edge_index)), GNPDE_EINVAL,
                  "select_edges: bad arguments");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_edges == 0) {
    GNPDE_HIP(hipMemsetAsync(out_count, 0, sizeof(int64_t), s));
    return 0;
  }
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= gnpde_select_edges_workspace_bytes(n_edges), GNPDE_EWS, "select_edges: workspace too small");
  const long long blocks = (n_edges + kTile - 1) / kTile;
  GNPDE_CHECK_ARG(blocks <= 0x7fffffffLL, GNPDE_ESHAPE, "select_edges: too many edges");
  unsigned* counts = static_cast<unsigned*>(workspace);
  hipLaunchKernelGGL(keep_count_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s, score, static_cast<long long>(n_edges),
                     threshold, counts);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(keep_scan_kernel, dim3(1), dim3(kBlock), 0, s, counts, static_cast<int>(blocks), reinterpret_cast<long long*>(out_count));
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(keep_scatter_kernel<true>, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, s,
                     reinterpret_cast<const long long*>(edge_index), score, static_cast<long long>(n_edges), threshold, counts,
                     reinterpret_cast<long long*>(out_edge_index), static_cast<long long>(n_edges), static_cast<float*>(nullptr));
  GNPDE_LAUNCH_CHECK();
  return 0;
}
