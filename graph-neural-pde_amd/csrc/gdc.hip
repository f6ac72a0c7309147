// Graph diffusion convolution rewiring (reference src/graph_rewiring.py:51-90, 345-401, a subclass of torch_geometric's GDC):
// column blocks of S = sum_m theta_m T^m by a Horner recurrence of plain aggregations, and the device sparsifier that turns a
// finished [n, B] slab into per-column selections.  No [n, n] array exists outside the dense mode.
//
//   block      X = theta_M E_B (one-hot columns j0 .. j0 + B), then for m = M - 1 .. 0:  X <- T X (gnpde_spmm, ping-pong between the
//              caller's slab and the workspace), X[j0 + b, b] += theta_m.  theta is a DEVICE array: no host value enters a launch.
//   transpose  [n, B] -> [B, n] through a 64 x 64 LDS tile (row stride 65), so that every later pass streams a column of S as a
//              contiguous row: the column-strided read of the row-major slab would touch one float per 1 KiB row.
//   top-k      one wave per (column, row split): entries > 0 whose key beats the current k-th best are appended to a 256-key LDS
//              buffer (ballot compaction, no atomics); 64-bit keys (~value bits << 32 | row), so unsigned ascending order is
//              (value descending, row ascending).  A full buffer is sorted (bitonic), cut to k, and the k-th key becomes the bar.
//              The S sorted partial lists of a column are sorted once more by one wave (merge).  The result is a function of the
//              SET of keys: bit-identical from run to run and for every split count.
//   emit       one wave per column: column sum of the kept values in a fixed order (two per lane, then a butterfly), then
//              (row, col, value / sum) at the column's offset.
//   threshold  count (per column and split) -> per-column counts -> caller's exclusive scan -> fill (ballot compaction in
//              ascending row order at offsets[col] + the counts of the earlier splits).
//   segments   sums (and optional division) of contiguous segments of a weight list in a fixed order: the output normalisation of
//              the threshold mode and the degree sums of the input normalisation.
//   dense      column sums from the transposed slab, then dense[i, j0 + b] = X[i, b] / sum_b.
#include "common.h"
#include "select.h"

namespace gnpde {
namespace {

constexpr int kGdcMaxK = 128;
constexpr int kGdcMaxBlock = 256;
constexpr int kGdcMaxTerms = 4097;       // M <= 4096
constexpr int kGdcCap = 256;             // keys of a wave's candidate buffer: k + 64 <= CAP
constexpr int kGdcSplitRows = 512;       // rows of a column that one wave streams before another split is opened
constexpr int kGdcMaxSplits = 32;        // S * k <= 4096 keys in the merge (32 KiB of LDS)

__host__ __device__ __forceinline__ int gdc_splits(long long n) {
  long long s = (n + kGdcSplitRows - 1) / kGdcSplitRows;
  if (s > kGdcMaxSplits) s = kGdcMaxSplits;
  return s < 1 ? 1 : static_cast<int>(s);
}

// X[i, b] = (i == j0 + b) ? theta[m] : 0 over the whole [n, B] slab (B % 4 == 0: one 16-byte store per thread)
__global__ __launch_bounds__(kBlock) void gdc_init_kernel(float* __restrict__ x, long long n, int B, long long j0,
                                                         const float* __restrict__ theta, int m) {
  const long long q = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;   // 4-float group
  const int per_row = B >> 2;
  if (q >= n * per_row) return;
  const long long i = q / per_row;
  const int b = static_cast<int>(q - i * per_row) << 2;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const long long hit = i - j0;          // the column of this row's one
  if (hit >= b && hit < b + 4) {
    const float t = theta[m];
    if (hit == b) v.x = t;
    else if (hit == b + 1) v.y = t;
    else if (hit == b + 2) v.z = t;
    else v.w = t;
  }
  *reinterpret_cast<float4*>(x + i * B + b) = v;
}

__global__ __launch_bounds__(kBlock) void gdc_diag_add_kernel(float* __restrict__ x, int B, long long j0, int ncols,
                                                             const float* __restrict__ theta, int m) {
  const int b = threadIdx.x;
  if (b < ncols) x[(j0 + b) * B + b] += theta[m];
}

// xt[b, i] = x[i, b]
__global__ __launch_bounds__(kBlock) void gdc_transpose_kernel(const float* __restrict__ x, long long n, int B, float* __restrict__ xt) {
  __shared__ float tile[64][65];
  const long long i0 = static_cast<long long>(blockIdx.x) * 64;
  const int b0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
  for (int r = ty; r < 64; r += 4) {
    const long long i = i0 + r;
    tile[r][tx] = (i < n && b0 + tx < B) ? x[i * B + b0 + tx] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 64; r += 4) {
    const long long i = i0 + tx;
    if (i < n && b0 + r < B) xt[static_cast<long long>(b0 + r) * n + i] = tile[tx][r];
  }
}

// sort the buffer's cnt keys, keep the k best; returns the new count, *bar = the k-th key once k are known
__device__ __forceinline__ int gdc_prune(u64* buf, int cnt, int k, int lane, u64* bar) {
  wave_lds_sync();
  const int nc = wave_keep_best(buf, cnt, k, lane);
  if (nc == k) *bar = buf[k - 1];
  return nc;
}

// grid (ncols, S), one wave: the k best keys of rows [s * per, (s + 1) * per) of column b -> partial[(b * S + s) * k ..], padded
__global__ __launch_bounds__(kWave) void gdc_select_kernel(const float* __restrict__ xt, long long n, long long per, int k,
                                                          u64* __restrict__ partial) {
  __shared__ u64 buf[kGdcCap];
  const int lane = threadIdx.x;
  const int b = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  const float* xr = xt + static_cast<long long>(b) * n;
  const long long begin = s * per, end = begin + per < n ? begin + per : n;
  int cnt = 0;
  u64 bar = kPadKey;
  for (long long i = begin; i < end; i += 4 * kWave) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {          // four coalesced loads in flight
      const long long r = i + u * kWave + lane;
      v[u] = r < end ? xr[r] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (cnt > kGdcCap - kWave) cnt = gdc_prune(buf, cnt, k, lane, &bar);     // (wave-uniform)
      const long long r = i + u * kWave + lane;
      const u64 key = (static_cast<u64>(~__float_as_uint(v[u])) << 32) | static_cast<u64>(static_cast<unsigned>(r));
      const bool ok = v[u] > 0.f && key < bar;
      int kept;
      const int pos = cnt + wave_rank(ok, lane, &kept);
      if (ok) buf[pos] = key;
      cnt += kept;
    }
  }
  cnt = gdc_prune(buf, cnt, k, lane, &bar);
  u64* out = partial + (static_cast<long long>(b) * S + s) * k;
  for (int p = lane; p < k; p += kWave) out[p] = p < cnt ? buf[p] : kPadKey;
}

// one wave per column: the S sorted partial lists -> keys[(j0 + b) * k ..] (the k best, padded) and counts[j0 + b]
__global__ __launch_bounds__(kWave) void gdc_merge_kernel(const u64* __restrict__ partial, int S, int k, int P, long long j0,
                                                         u64* __restrict__ keys, long long* __restrict__ counts) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* buf = reinterpret_cast<u64*>(smem);
  const int lane = threadIdx.x, b = blockIdx.x;
  wave_merge_lists(buf, P, partial + static_cast<long long>(b) * S * k, k, S, k, lane);
  u64* out = keys + (j0 + b) * k;
  int c = 0;
  for (int p0 = 0; p0 < k; p0 += kWave) {
    const int p = p0 + lane;
    const u64 key = p < k ? buf[p] : kPadKey;
    if (p < k) out[p] = key;
    c += __popcll(__ballot(key != kPadKey));
  }
  if (lane == 0) counts[j0 + b] = c;
}

// one wave per column j of the whole result: keys[j * k .. + count) -> (row, j, value [/ column sum]) at offsets[j]
__global__ __launch_bounds__(kWave) void gdc_emit_kernel(const u64* __restrict__ keys, const long long* __restrict__ offsets, int k,
                                                        int normalise, long long* __restrict__ out_ei, long long out_ld,
                                                        float* __restrict__ out_w) {
  const int lane = threadIdx.x;
  const long long j = blockIdx.x;
  const long long off = offsets[j];
  const int c = static_cast<int>(offsets[j + 1] - off);
  const u64* in = keys + j * k;
  u64 key[2];
  float v[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int p = lane + u * kWave;
    key[u] = p < c ? in[p] : kPadKey;
    v[u] = p < c ? __uint_as_float(~static_cast<unsigned>(key[u] >> 32)) : 0.f;
  }
  const float sum = wave_sum(v[0] + v[1]);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int p = lane + u * kWave;
    if (p < c) {
      out_ei[off + p] = static_cast<long long>(key[u] & 0xffffffffull);
      out_ei[out_ld + off + p] = j;
      out_w[off + p] = normalise ? v[u] / sum : v[u];      // c > 0 here and every kept value is > 0: sum > 0
    }
  }
}

// grid (ncols, S), one wave: part[b * S + s] = number of entries >= eps among the split's rows of column b
__global__ __launch_bounds__(kWave) void gdc_count_kernel(const float* __restrict__ xt, long long n, long long per, float eps,
                                                         int* __restrict__ part) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  const float* xr = xt + static_cast<long long>(b) * n;
  const long long begin = s * per, end = begin + per < n ? begin + per : n;
  int c = 0;
  for (long long r = begin + lane; r < end; r += kWave) c += xr[r] >= eps ? 1 : 0;
  c = wave_sum(c);
  if (lane == 0) part[b * S + s] = c;
}

__global__ __launch_bounds__(kBlock) void gdc_count_fold_kernel(const int* __restrict__ part, int ncols, int S, long long* __restrict__ counts) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= ncols) return;
  long long c = 0;
  for (int s = 0; s < S; ++s) c += part[b * S + s];
  counts[b] = c;
}

// grid (ncols, S), one wave: the split's entries >= eps in ascending row order
__global__ __launch_bounds__(kWave) void gdc_fill_kernel(const float* __restrict__ xt, long long n, long long per, float eps, long long j0,
                                                        const int* __restrict__ part, const long long* __restrict__ offsets,
                                                        long long* __restrict__ out_ei, long long out_ld, float* __restrict__ out_w) {
  const int lane = threadIdx.x;
  const int b = blockIdx.x, s = blockIdx.y, S = gridDim.y;
  const float* xr = xt + static_cast<long long>(b) * n;
  const long long begin = s * per, end = begin + per < n ? begin + per : n;
  long long pos = offsets[b];
  for (int t = 0; t < s; ++t) pos += part[b * S + t];
  for (long long i = begin; i < end; i += kWave) {
    const long long r = i + lane;
    const float v = r < end ? xr[r] : 0.f;
    const bool ok = r < end && v >= eps;
    int kept;
    const long long p = pos + wave_rank(ok, lane, &kept);
    if (ok) {
      out_ei[p] = r;
      out_ei[out_ld + p] = j0 + b;
      out_w[p] = v;
    }
    pos += kept;
  }
}

// one wave per segment [offsets[g], offsets[g + 1]): its sum in a fixed order (lane l adds entries l, l + 64, ... in turn, then a
// butterfly); sums[g] (nullable) receives it, divide != 0 scales the segment by 1 / sum (0 for an empty sum)
__global__ __launch_bounds__(kWave) void gdc_segment_kernel(float* __restrict__ w, const long long* __restrict__ offsets,
                                                           float* __restrict__ sums, int divide) {
  const int lane = threadIdx.x;
  const long long g = blockIdx.x;
  const long long a = offsets[g], e = offsets[g + 1];
  float s = 0.f;
  for (long long p = a + lane; p < e; p += kWave) s += w[p];
  s = wave_sum(s);
  if (sums != nullptr && lane == 0) sums[g] = s;
  if (divide) {
    for (long long p = a + lane; p < e; p += kWave) w[p] = s != 0.f ? w[p] / s : 0.f;
  }
}

// one wave per column of the block: sums[b] = sum_i xt[b, i] in a fixed order
__global__ __launch_bounds__(kWave) void gdc_colsum_kernel(const float* __restrict__ xt, long long n, float* __restrict__ sums) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const float* xr = xt + static_cast<long long>(b) * n;
  float s = 0.f;
  for (long long r = lane; r < n; r += kWave) s += xr[r];
  s = wave_sum(s);
  if (lane == 0) sums[b] = s;
}

// dense[i, j0 + b] = x[i, b] (/ sums[b]) for b < ncols
__global__ __launch_bounds__(kBlock) void gdc_dense_kernel(const float* __restrict__ x, long long n, int B, long long j0, int ncols,
                                                          const float* __restrict__ sums, float* __restrict__ dense) {
  const long long q = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (q >= n * ncols) return;
  const long long i = q / ncols;
  const int b = static_cast<int>(q - i * ncols);
  float v = x[i * B + b];
  if (sums != nullptr) {
    const float s = sums[b];
    v = s != 0.f ? v / s : 0.f;
  }
  dense[i * n + j0 + b] = v;
}

// workspace: [spmm scratch | ping slab n B | transposed slab B n | keys / counts of the block]
struct GdcLayout {
  size_t spmm_bytes, ping, xt, part, total;
};

GdcLayout gdc_layout(const gnpde_graph_t* g, int B, int k) {
  GdcLayout L;
  const size_t n = static_cast<size_t>(g->n);
  L.spmm_bytes = align_up(gnpde_spmm_workspace_bytes(g, B), 256);
  L.ping = L.spmm_bytes;
  L.xt = L.ping + align_up(n * B * sizeof(float), 256);
  L.part = L.xt + align_up(n * B * sizeof(float), 256);
  const size_t S = static_cast<size_t>(gdc_splits(g->n));
  size_t part = static_cast<size_t>(B) * S * static_cast<size_t>(k > 1 ? k : 1) * sizeof(u64);   // partial keys; counts and sums fit too
  L.total = L.part + align_up(part, 256);
  return L;
}

int check_block_args(const char* what, const gnpde_graph_t* g, int B, long long j0, int k, const void* ws, size_t ws_bytes) {
  GNPDE_CHECK_ARG(g != nullptr && g->n >= 1, GNPDE_EINVAL, "%s: no graph / no nodes", what);
  GNPDE_CHECK_ARG(g->row_begin == 0, GNPDE_EINVAL, "%s: the graph is a row range of a partitioned graph", what);
  GNPDE_CHECK_ARG(B >= 4 && B <= kGdcMaxBlock && B % 4 == 0, GNPDE_ESHAPE, "%s: block = %d is not a multiple of 4 in 4 .. %d", what, B,
                  kGdcMaxBlock);
  GNPDE_CHECK_ARG(j0 >= 0 && j0 < g->n, GNPDE_EINVAL, "%s: first column %lld outside [0, %d)", what, j0, g->n);
  GNPDE_CHECK_ARG(k >= 0 && k <= kGdcMaxK, GNPDE_ESHAPE, "%s: k = %d outside 1 .. %d", what, k, kGdcMaxK);
  GNPDE_CHECK_ARG(ws != nullptr && ws_bytes >= gdc_layout(g, B, k).total, GNPDE_EWS, "%s: workspace too small", what);
  return 0;
}

int launch_transpose(const float* slab, long long n, int B, float* xt, hipStream_t s) {
  hipLaunchKernelGGL(gdc_transpose_kernel, dim3(static_cast<unsigned>((n + 63) / 64), static_cast<unsigned>((B + 63) / 64)), dim3(kBlock), 0, s,
                     slab, n, B, xt);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_gdc_workspace_bytes(const gnpde_graph_t* g, int32_t block, int32_t k) {
  if (g == nullptr || g->n < 1 || block < 4 || block > kGdcMaxBlock || block % 4 != 0 || k < 0 || k > kGdcMaxK) return 0;
  return gdc_layout(g, block, k).total;
}

extern "C" int gnpde_gdc_block(const gnpde_graph_t* g, const float* w_csr, const float* theta, int32_t n_terms, int64_t j0,
                               int32_t block, float* slab, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_block_args("gdc_block", g, block, j0, 0, workspace, workspace_bytes);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(theta != nullptr && slab != nullptr && (w_csr != nullptr || g->e == 0), GNPDE_EINVAL, "gdc_block: null pointer");
  GNPDE_CHECK_ARG(n_terms >= 1 && n_terms <= kGdcMaxTerms, GNPDE_ESHAPE, "gdc_block: %d terms outside 1 .. %d (M <= 4096)", n_terms,
                  kGdcMaxTerms);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GdcLayout L = gdc_layout(g, block, 0);
  char* ws = static_cast<char*>(workspace);
  float* ping = reinterpret_cast<float*>(ws + L.ping);
  const long long n = g->n;
  const int M = n_terms - 1;
  const int ncols = static_cast<int>(n - j0 < block ? n - j0 : block);
  // M aggregations from now: an even M starts in the slab and ends there
  float* cur = (M % 2 == 0) ? slab : ping;
  float* nxt = (M % 2 == 0) ? ping : slab;
  const long long groups = n * (block / 4);
  hipLaunchKernelGGL(gdc_init_kernel, dim3(static_cast<unsigned>((groups + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, cur, n, block,
                     static_cast<long long>(j0), theta, M);
  GNPDE_LAUNCH_CHECK();
  for (int m = M - 1; m >= 0; --m) {
    rc = gnpde_spmm(g, w_csr, cur, block, block, nxt, ws, L.spmm_bytes, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(gdc_diag_add_kernel, dim3(1), dim3(kBlock), 0, s, nxt, block, static_cast<long long>(j0), ncols, theta, m);
    GNPDE_LAUNCH_CHECK();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  return 0;
}

extern "C" int gnpde_gdc_topk(const gnpde_graph_t* g, const float* slab, int64_t j0, int32_t block, int32_t k, uint64_t* keys,
                              int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(k >= 1 && k <= kGdcMaxK, GNPDE_ESHAPE, "gdc_topk: k = %d outside 1 .. %d", k, kGdcMaxK);
  int rc = check_block_args("gdc_topk", g, block, j0, k, workspace, workspace_bytes);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(slab != nullptr && keys != nullptr && counts != nullptr, GNPDE_EINVAL, "gdc_topk: null pointer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GdcLayout L = gdc_layout(g, block, k);
  char* ws = static_cast<char*>(workspace);
  float* xt = reinterpret_cast<float*>(ws + L.xt);
  u64* partial = reinterpret_cast<u64*>(ws + L.part);
  const long long n = g->n;
  const int ncols = static_cast<int>(n - j0 < block ? n - j0 : block);
  const int S = gdc_splits(n);
  const long long per = (n + S - 1) / S;
  rc = launch_transpose(slab, n, block, xt, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(gdc_select_kernel, dim3(static_cast<unsigned>(ncols), static_cast<unsigned>(S)), dim3(kWave), 0, s, xt, n, per, k, partial);
  GNPDE_LAUNCH_CHECK();
  const int P = sort_length(S * k);
  hipLaunchKernelGGL(gdc_merge_kernel, dim3(static_cast<unsigned>(ncols)), dim3(kWave), static_cast<size_t>(P) * sizeof(u64), s, partial, S, k, P,
                     static_cast<long long>(j0), reinterpret_cast<u64*>(keys), reinterpret_cast<long long*>(counts));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_gdc_emit(const uint64_t* keys, const int64_t* offsets, int32_t n, int32_t k, int32_t normalise,
                              int64_t* out_edge_index, int64_t out_ld, float* out_weight, void* stream) {
  GNPDE_CHECK_ARG(keys && offsets && out_edge_index && out_weight && n >= 1 && out_ld >= 0, GNPDE_EINVAL, "gdc_emit: bad arguments");
  GNPDE_CHECK_ARG(k >= 1 && k <= kGdcMaxK, GNPDE_ESHAPE, "gdc_emit: k = %d outside 1 .. %d", k, kGdcMaxK);
  hipLaunchKernelGGL(gdc_emit_kernel, dim3(static_cast<unsigned>(n)), dim3(kWave), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const u64*>(keys), reinterpret_cast<const long long*>(offsets), k, normalise,
                     reinterpret_cast<long long*>(out_edge_index), static_cast<long long>(out_ld), out_weight);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_gdc_threshold_count(const gnpde_graph_t* g, const float* slab, int64_t j0, int32_t block, float eps,
                                         int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_block_args("gdc_threshold_count", g, block, j0, 0, workspace, workspace_bytes);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(slab != nullptr && counts != nullptr, GNPDE_EINVAL, "gdc_threshold_count: null pointer");
  GNPDE_CHECK_ARG(eps > 0.f, GNPDE_EINVAL, "gdc_threshold_count: eps = %g is not positive (zeros are never kept)", static_cast<double>(eps));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GdcLayout L = gdc_layout(g, block, 0);
  char* ws = static_cast<char*>(workspace);
  float* xt = reinterpret_cast<float*>(ws + L.xt);
  int* part = reinterpret_cast<int*>(ws + L.part);
  const long long n = g->n;
  const int ncols = static_cast<int>(n - j0 < block ? n - j0 : block);
  const int S = gdc_splits(n);
  const long long per = (n + S - 1) / S;
  rc = launch_transpose(slab, n, block, xt, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(gdc_count_kernel, dim3(static_cast<unsigned>(ncols), static_cast<unsigned>(S)), dim3(kWave), 0, s, xt, n, per, eps, part);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(gdc_count_fold_kernel, dim3(static_cast<unsigned>((ncols + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, part, ncols, S,
                     reinterpret_cast<long long*>(counts));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_gdc_threshold_fill(const gnpde_graph_t* g, int64_t j0, int32_t block, float eps, const int64_t* offsets,
                                        int64_t* out_edge_index, int64_t out_ld, float* out_weight, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  int rc = check_block_args("gdc_threshold_fill", g, block, j0, 0, workspace, workspace_bytes);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(offsets && out_edge_index && out_weight && out_ld >= 0, GNPDE_EINVAL, "gdc_threshold_fill: null pointer");
  GNPDE_CHECK_ARG(eps > 0.f, GNPDE_EINVAL, "gdc_threshold_fill: eps = %g is not positive", static_cast<double>(eps));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GdcLayout L = gdc_layout(g, block, 0);
  char* ws = static_cast<char*>(workspace);
  const long long n = g->n;
  const int ncols = static_cast<int>(n - j0 < block ? n - j0 : block);
  const int S = gdc_splits(n);
  const long long per = (n + S - 1) / S;
  hipLaunchKernelGGL(gdc_fill_kernel, dim3(static_cast<unsigned>(ncols), static_cast<unsigned>(S)), dim3(kWave), 0, s,
                     reinterpret_cast<const float*>(ws + L.xt), n, per, eps, static_cast<long long>(j0), reinterpret_cast<const int*>(ws + L.part),
                     reinterpret_cast<const long long*>(offsets), reinterpret_cast<long long*>(out_edge_index),
                     static_cast<long long>(out_ld), out_weight);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_gdc_segment_sums(float* w, const int64_t* offsets, int64_t n_segments, float* sums, int32_t divide, void* stream) {
  GNPDE_CHECK_ARG(w && offsets && n_segments >= 0 && n_segments <= INT32_MAX, GNPDE_EINVAL, "gdc_segment_sums: bad arguments");
  GNPDE_CHECK_ARG(sums != nullptr || divide != 0, GNPDE_EINVAL, "gdc_segment_sums: nothing to do");
  if (n_segments == 0) return 0;
  hipLaunchKernelGGL(gdc_segment_kernel, dim3(static_cast<unsigned>(n_segments)), dim3(kWave), 0, static_cast<hipStream_t>(stream), w,
                     reinterpret_cast<const long long*>(offsets), sums, divide);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_gdc_dense(const gnpde_graph_t* g, const float* slab, int64_t j0, int32_t block, int32_t normalise, float* dense,
                               size_t cap_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_block_args("gdc_dense", g, block, j0, 0, workspace, workspace_bytes);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(slab != nullptr && dense != nullptr, GNPDE_EINVAL, "gdc_dense: null pointer");
  const long long n = g->n;
  GNPDE_CHECK_ARG(static_cast<double>(n) * static_cast<double>(n) * 4.0 <= static_cast<double>(cap_bytes), GNPDE_ESHAPE,
                  "gdc_dense: the %lld x %lld matrix exceeds the cap of %zu bytes", n, n, cap_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const GdcLayout L = gdc_layout(g, block, 0);
  char* ws = static_cast<char*>(workspace);
  float* xt = reinterpret_cast<float*>(ws + L.xt);
  float* sums = reinterpret_cast<float*>(ws + L.part);
  const int ncols = static_cast<int>(n - j0 < block ? n - j0 : block);
  if (normalise) {
    rc = launch_transpose(slab, n, block, xt, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(gdc_colsum_kernel, dim3(static_cast<unsigned>(ncols)), dim3(kWave), 0, s, xt, n, sums);
    GNPDE_LAUNCH_CHECK();
  }
  const long long total = n * ncols;
  hipLaunchKernelGGL(gdc_dense_kernel, dim3(static_cast<unsigned>((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, slab, n, block,
                     static_cast<long long>(j0), ncols, normalise ? sums : nullptr, dense);
  GNPDE_LAUNCH_CHECK();
  return 0;
}
