// Radius graphs over pairwise keys: BLEND's positional-distance rewiring by a global quantile (reference
// src/graph_rewiring.py:285-342 with distances_kNN.apply_dist_threshold: np.quantile over a dense float64 [n, n] matrix, then
// np.where).  The definition is in include/gnpde.h.  Every pass is a sweep of the tile pipeline of knn_tile.h: the keys are formed
// on the fp32 matrix cores and consumed where they appear; no key is ever stored.
//
//   quantile   radix select of the key of rank lo among all n^2 keys: three sweeps over 11 / 11 / 10 key bits.  A workgroup counts
//              its keys (those that match the prefix found so far) in an LDS histogram of 2048 u32 bins and flushes it into the
//              global u64 histogram with integer atomics: integer sums do not depend on the order of arrival.  Between sweeps a
//              one-wave kernel finds the bin that holds the rank and writes the longer prefix and the residual rank to a device
//              record; the host reads nothing.
//   count      per (column split, row) the number of keys <= tau; a one-workgroup scan turns them into rowptr [n + 1] and the
//              (split, row) slot offsets.
//   fill       the same sweep again: a workgroup walks its rows' columns in ascending tiles and a row's kept columns take
//              consecutive slots by ballot + popcount (as the k-NN selection appends): ascending columns, no atomics.
//
// The layout is a pure function of the input and of tau: bit-identical from run to run and for every column split S.
// The 64 x 64 tile of the k-NN search is kept: with 16-float chunks and the 8 KiB histogram a workgroup holds 18 KiB of LDS, so
// several workgroups share a CU and cover each other's barriers; no other tile shape has been measured.
#include "common.h"
#include "knn_tile.h"
#include "select.h"

namespace gnpde {
namespace {

constexpr int kBins = 2048;
constexpr int kMaxRadiusSplits = 32;
// a workgroup's u32 bin counts are flushed every 2^18 column tiles (64 * 64 * 2^18 = 2^30 keys at the most in one bin)
constexpr int kFlushTiles = 1 << 18;

struct RadiusRecord {
  unsigned prefix;     // the key bits found so far (the high bits of tau)
  unsigned pad;
  u64 rank;            // rank of tau among the keys that share the prefix
};

// bits of the key that a pass counts: pass 0 bits 31..21, pass 1 bits 20..10 (under an 11-bit prefix), pass 2 bits 9..0
__device__ __forceinline__ int pass_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__device__ __forceinline__ int pass_bins(int pass) { return pass == 2 ? 1024 : 2048; }

template <int METRIC>
__global__ __launch_bounds__(kBlock) void radius_hist_kernel(const float* __restrict__ x, const float* __restrict__ norms,
                                                            const float* __restrict__ ball, int n, int d, long long ldx, int vec,
                                                            int tiles_per_split, int pass, const RadiusRecord* __restrict__ rec,
                                                            u64* __restrict__ hist) {
  __shared__ __align__(16) float stage[tile_lds_floats()];
  __shared__ unsigned h[kBins];
  const int tid = threadIdx.x;
  const TileRange tr = tile_range(tiles_per_split, n);
  const int shift = pass_shift(pass), mask = pass_bins(pass) - 1;
  const int hi = shift + (pass == 2 ? 10 : 11);                  // the bits above this pass's: the prefix
  const unsigned prefix = pass == 0 ? 0u : rec->prefix;
  u64* out = hist + static_cast<long long>(pass) * kBins;
  for (int b = tid; b < kBins; b += kBlock) h[b] = 0u;
  __syncthreads();
  auto flush = [&]() {
    __syncthreads();
    for (int b = tid; b < kBins; b += kBlock) {
      const unsigned c = h[b];
      if (c != 0u) atomicAdd(&out[b], static_cast<u64>(c));
      h[b] = 0u;
    }
    __syncthreads();
  };
  int tiles_done = 0;
  tile_sweep<METRIC>(
      x, norms, ball, n, d, ldx, vec, tr, stage,
      [&](long long) {
        if (++tiles_done == kFlushTiles) {   // (workgroup-uniform)
          flush();
          tiles_done = 0;
        }
      },
      [&](int, int, long long, long long, float key, bool valid) {
        const unsigned bits = __float_as_uint(key);
        const bool match = pass == 0 || (bits >> hi) == prefix;
        if (valid && match) atomicAdd(&h[(bits >> shift) & mask], 1u);
      });
  flush();
}

// one wave: the bin of this pass's histogram that holds the rank -> longer prefix, residual rank; after the last pass tau
__global__ __launch_bounds__(kWave) void radius_select_kernel(const u64* __restrict__ hist, int pass, u64 rank0, int metric,
                                                             RadiusRecord* __restrict__ rec, float* __restrict__ tau_out) {
  __shared__ u64 part[kWave];
  const int lane = threadIdx.x;
  const u64* h = hist + static_cast<long long>(pass) * kBins;
  const int bins = pass_bins(pass), per = bins / kWave;
  const u64 rank = pass == 0 ? rank0 : rec->rank;
  const unsigned prefix = pass == 0 ? 0u : rec->prefix;
  u64 mine = 0;
  for (int j = 0; j < per; ++j) mine += h[lane * per + j];
  part[lane] = mine;
  __syncthreads();
  u64 before = 0;
  for (int l = 0; l < lane; ++l) before += part[l];
  __syncthreads();                                   // rec is read above by every lane before the owner rewrites it
  if (rank >= before && rank < before + mine) {      // exactly one lane: the counts sum to more than the rank
    u64 inside = rank - before;
    const int bin = rank_bin(h, lane * per, (lane + 1) * per, &inside);
    const unsigned grown = (prefix << (pass == 2 ? 10 : 11)) | static_cast<unsigned>(bin);
    rec->prefix = grown;
    rec->rank = inside;
    if (pass == 2) {
      const float key = __uint_as_float(grown);
      tau_out[0] = key;
      tau_out[1] = metric == GNPDE_METRIC_POINCARE ? key_distance<GNPDE_METRIC_POINCARE>(key) : sqrtf(key);
    }
  }
}

template <int METRIC>
__global__ __launch_bounds__(kBlock) void radius_count_kernel(const float* __restrict__ x, const float* __restrict__ norms,
                                                             const float* __restrict__ ball, int n, int d, long long ldx, int vec,
                                                             int tiles_per_split, const float* __restrict__ tau_dev, float tau_key,
                                                             long long* __restrict__ counts) {
  __shared__ __align__(16) float stage[tile_lds_floats()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TileRange tr = tile_range(tiles_per_split, n);
  const unsigned tau = __float_as_uint(tau_dev != nullptr ? tau_dev[0] : tau_key);
  int cnt[4] = {0, 0, 0, 0};
  tile_sweep<METRIC>(
      x, norms, ball, n, d, ldx, vec, tr, stage, [](long long) {},
      [&](int i, int, long long, long long, float key, bool valid) { cnt[i] += (valid && __float_as_uint(key) <= tau) ? 1 : 0; });
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int c = cnt[i];
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) c += __shfl_xor(c, off, kWave);
    const long long row = tr.row0 + 16 * wave + 4 * q + i;
    if (r == 0 && row < n) counts[static_cast<long long>(blockIdx.y) * n + row] = c;
  }
}

// one workgroup: counts [S][n] -> rowptr [n + 1] (exclusive scan of the rows' totals) and, in place, the first slot of every
// (split, row): rowptr[row] + the counts of the row's earlier splits
__global__ __launch_bounds__(kBlock) void radius_scan_kernel(long long* __restrict__ counts, int n, int splits,
                                                            long long* __restrict__ rowptr) {
  __shared__ long long sc[kBlock];
  const int tid = threadIdx.x;
  long long carry = 0;
  for (long long base = 0; base < n; base += kBlock) {
    const long long row = base + tid;
    long long tot = 0;
    if (row < n)
      for (int s = 0; s < splits; ++s) tot += counts[static_cast<long long>(s) * n + row];
    long long o = block_scan_exclusive(tot, sc, &carry);
    if (row < n) {
      rowptr[row] = o;
      for (int s = 0; s < splits; ++s) {
        const long long c = counts[static_cast<long long>(s) * n + row];
        counts[static_cast<long long>(s) * n + row] = o;
        o += c;
      }
    }
  }
  if (tid == 0) rowptr[n] = carry;
}

template <int METRIC>
__global__ __launch_bounds__(kBlock) void radius_fill_kernel(const float* __restrict__ x, const float* __restrict__ norms,
                                                            const float* __restrict__ ball, int n, int d, long long ldx, int vec,
                                                            int tiles_per_split, const float* __restrict__ tau_dev, float tau_key,
                                                            const long long* __restrict__ offsets, long long* __restrict__ out,
                                                            long long out_ld) {
  __shared__ __align__(16) float stage[tile_lds_floats()];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TileRange tr = tile_range(tiles_per_split, n);
  const unsigned tau = __float_as_uint(tau_dev != nullptr ? tau_dev[0] : tau_key);
  long long slot[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long row = tr.row0 + 16 * wave + 4 * q + i;
    slot[i] = row < n ? offsets[static_cast<long long>(blockIdx.y) * n + row] : 0;
  }
  // a row's 16 lanes hold the columns col0 + 16 t + r: ascending in (t, r), the order the slots are handed out in
  tile_sweep<METRIC>(
      x, norms, ball, n, d, ldx, vec, tr, stage, [](long long) {},
      [&](int i, int, long long row, long long col, float key, bool valid) {
        const bool ok = valid && __float_as_uint(key) <= tau;
        int kept;
        const long long pos = slot[i] + group16_rank(ok, q, r, &kept);
        if (ok && pos < out_ld) {     // (pos < out_ld always holds for the tau and the split of the count; a guard, not a path)
          out[pos] = row;
          out[out_ld + pos] = col;
        }
        slot[i] += kept;
      });
}

// Column splits of the radius sweeps: enough workgroups for two per CU (they are small), at most 32 and at most one per column
// tile; gnpde_tune(19, S) forces S.
int radius_splits(long long n) {
  return column_splits(n, 2, kMaxRadiusSplits, kMaxRadiusSplits, num_cus(), g_tune[GNPDE_TUNE_KNN_SPLITS]);
}

size_t hist_bytes() { return 3 * kBins * sizeof(u64); }
size_t record_bytes() { return 256; }

// norms [n] | a [n] | histograms [3][2048] u64 | record | counts / slot offsets [S][n] int64
struct RadiusWs {
  float* norms;
  float* ball;
  u64* hist;
  RadiusRecord* rec;
  long long* counts;
};

RadiusWs carve(void* workspace, long long n) {
  char* p = static_cast<char*>(workspace);
  RadiusWs w;
  w.norms = reinterpret_cast<float*>(p);
  w.ball = reinterpret_cast<float*>(p + norms_bytes(n));
  w.hist = reinterpret_cast<u64*>(p + 2 * norms_bytes(n));
  w.rec = reinterpret_cast<RadiusRecord*>(p + 2 * norms_bytes(n) + hist_bytes());
  w.counts = reinterpret_cast<long long*>(p + 2 * norms_bytes(n) + hist_bytes() + record_bytes());
  return w;
}

bool known_metric(int metric) { return metric == GNPDE_METRIC_SQEUCLIDEAN || metric == GNPDE_METRIC_POINCARE; }

struct Grid {
  dim3 grid;
  int per;
};

Grid radius_grid(int n) {
  const long long tiles = (static_cast<long long>(n) + kTM - 1) / kTM;
  const int splits = radius_splits(n);
  return Grid{dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(splits)), static_cast<int>((tiles + splits - 1) / splits)};
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_radius_workspace_bytes(int64_t n, int32_t d) {
  (void)d;
  if (n < 1 || n > INT32_MAX) return 0;
  return 2 * norms_bytes(n) + hist_bytes() + record_bytes() +
         align_up(static_cast<size_t>(radius_splits(n)) * static_cast<size_t>(n) * sizeof(long long), 256);
}

#define GNPDE_RADIUS_ARGS(name)                                                                                                   \
  GNPDE_CHECK_ARG(x && n >= 1 && d >= 1 && ldx >= d, GNPDE_EINVAL, name ": bad arguments (n %lld, d %d, ldx %d)",                 \
                  static_cast<long long>(n), d, ldx);                                                                             \
  GNPDE_CHECK_ARG(n <= INT32_MAX, GNPDE_ESHAPE, name ": n = %lld exceeds int32 indices", static_cast<long long>(n));              \
  GNPDE_CHECK_ARG(known_metric(metric), GNPDE_ESHAPE, name ": unknown metric %d", metric);                                        \
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= gnpde_radius_workspace_bytes(n, d), GNPDE_EWS, name ": workspace too small")

extern "C" int gnpde_radius_quantile(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t metric, double q, float* tau_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_RADIUS_ARGS("radius_quantile");
  GNPDE_CHECK_ARG(tau_out != nullptr, GNPDE_EINVAL, "radius_quantile: tau_out is NULL");
  GNPDE_CHECK_ARG(q >= 0.0 && q <= 1.0, GNPDE_ESHAPE, "radius_quantile: q = %g outside [0, 1]", q);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nn = static_cast<int>(n);
  const RadiusWs w = carve(workspace, n);
  // rank lo = floor((n^2 - 1) q) in host double, as numpy forms the index of its lower neighbour
  const u64 last = static_cast<u64>(n) * static_cast<u64>(n) - 1;
  u64 rank = static_cast<u64>(static_cast<double>(last) * q);
  if (rank > last) rank = last;
  const bool poincare = metric == GNPDE_METRIC_POINCARE;
  int rc = launch_norms(x, nn, d, ldx, w.norms, poincare ? w.ball : nullptr, s);
  if (rc != 0) return rc;
  GNPDE_HIP(hipMemsetAsync(w.hist, 0, hist_bytes(), s));
  const Grid g = radius_grid(nn);
  const int vec = tile_vec(x, d, ldx);
  for (int pass = 0; pass < 3; ++pass) {
    with_metric(metric, [&](auto m) {
      hipLaunchKernelGGL(radius_hist_kernel<decltype(m)::value>, g.grid, dim3(kBlock), 0, s, x, w.norms, w.ball, nn, d,
                         static_cast<long long>(ldx), vec, g.per, pass, w.rec, w.hist);
    });
    GNPDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(radius_select_kernel, dim3(1), dim3(kWave), 0, s, w.hist, pass, rank, metric, w.rec, tau_out);
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int gnpde_radius_count(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t metric, const float* tau_dev,
                                  float tau_key, int64_t* rowptr, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_RADIUS_ARGS("radius_count");
  GNPDE_CHECK_ARG(rowptr != nullptr, GNPDE_EINVAL, "radius_count: rowptr is NULL");
  GNPDE_CHECK_ARG(tau_dev != nullptr || tau_key >= 0.f, GNPDE_EINVAL, "radius_count: tau_key = %g is no key (keys are >= 0)",
                  static_cast<double>(tau_key));
  tau_key = fabsf(tau_key);     // -0 is the key +0
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nn = static_cast<int>(n);
  const RadiusWs w = carve(workspace, n);
  const bool poincare = metric == GNPDE_METRIC_POINCARE;
  int rc = launch_norms(x, nn, d, ldx, w.norms, poincare ? w.ball : nullptr, s);
  if (rc != 0) return rc;
  const Grid g = radius_grid(nn);
  const int vec = tile_vec(x, d, ldx);
  with_metric(metric, [&](auto m) {
    hipLaunchKernelGGL(radius_count_kernel<decltype(m)::value>, g.grid, dim3(kBlock), 0, s, x, w.norms, w.ball, nn, d,
                       static_cast<long long>(ldx), vec, g.per, tau_dev, tau_key, w.counts);
  });
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(radius_scan_kernel, dim3(1), dim3(kBlock), 0, s, w.counts, nn, static_cast<int>(g.grid.y),
                     reinterpret_cast<long long*>(rowptr));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_radius_fill(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t metric, const float* tau_dev,
                                 float tau_key, int64_t* out_edge_index, int64_t out_ld, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  GNPDE_RADIUS_ARGS("radius_fill");
  GNPDE_CHECK_ARG(out_edge_index != nullptr && out_ld >= 1, GNPDE_EINVAL, "radius_fill: no output (out_ld %lld)",
                  static_cast<long long>(out_ld));
  GNPDE_CHECK_ARG(tau_dev != nullptr || tau_key >= 0.f, GNPDE_EINVAL, "radius_fill: tau_key = %g is no key (keys are >= 0)",
                  static_cast<double>(tau_key));
  tau_key = fabsf(tau_key);     // -0 is the key +0
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nn = static_cast<int>(n);
  const RadiusWs w = carve(workspace, n);
  const Grid g = radius_grid(nn);
  const int vec = tile_vec(x, d, ldx);
  with_metric(metric, [&](auto m) {
    hipLaunchKernelGGL(radius_fill_kernel<decltype(m)::value>, g.grid, dim3(kBlock), 0, s, x, w.norms, w.ball, nn, d,
                       static_cast<long long>(ldx), vec, g.per, tau_dev, tau_key, w.counts, reinterpret_cast<long long*>(out_edge_index),
                       static_cast<long long>(out_ld));
  });
  GNPDE_LAUNCH_CHECK();
  return 0;
}
