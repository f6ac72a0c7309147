// k-nearest-neighbour search in feature space: BLEND's graph rewiring (reference src/graph_rewiring.py:120-126, a pykeops
// LazyTensor.argKmin over D_ij = |x_i - x_j|^2) and, with metric 1, the Poincare-ball k-NN of the positional-distance rewiring
// (src/graph_rewiring.py:285-342).  One fused kernel: the key tile on the fp32 matrix cores (knn_tile.h: staging, prefetch, MFMA and
// the epilogue that forms the key of the chosen metric) and a streaming per-row top-k in LDS; no [n, n] or [chunk, n] array exists
// in global memory.
//
//   norms      s_i = sum_c x_ic^2 (16 lanes per row, fp32); metric 1 also a_i = max(1 - s_i, 2^-24)
//   tile       a workgroup (4 waves) owns 64 query rows and walks 64-column tiles of its column range (tile_sweep).  Selection:
//              every row keeps the key of its current k-th best as a threshold (+inf until k are known); entries UNDER it are
//              appended to the row's LDS buffer (ballot compaction, no atomics) as 64-bit keys (key bits << 32 | column: unsigned
//              order = (key, column) order).  When a row of the wave has fewer than 64 free slots the wave sorts its rows' buffers
//              (bitonic, in LDS), keeps k and tightens the thresholds.  Columns are walked in ascending order, so an entry EQUAL
//              to the threshold has a larger column than the k-th best and is rightly dropped: ties go to the smaller column.
//   merge      only when the column range is split S ways (few row tiles: Cora has 43 for 256 CUs): every split writes its
//              sorted partial keys to the workspace and one wave per row sorts the S * k keys.
//
// Every result is a function of the sorted set of (key, column) pairs and the key of a pair does not depend on the
// tiling: bit-identical from run to run and for every S.
#include "common.h"
#include "knn_tile.h"
#include "select.h"

namespace gnpde {
namespace {

constexpr int kMaxK = 128;
constexpr int kMaxMergeKeys = 4096;  // S * k of the merge kernel (32 KiB of LDS per row)
constexpr int kMaxSplits = 32;

// sort the buffers of the wave's 16 rows, keep the k best of each, tighten the thresholds.  cnt / thr of local row 4 q + i
// live in register i of the 16 lanes of group q.
template <int CAP>
__device__ __forceinline__ void wave_merge(u64* mybuf, int k, int lane, int (&cnt)[4], float (&thr)[4]) {
  const int q = lane >> 4;
  wave_lds_sync();
#pragma unroll
  for (int lr = 0; lr < 16; ++lr) {
    const int c = __shfl(cnt[lr & 3], (lr >> 2) * 16, kWave);
    u64* b = mybuf + lr * CAP;
    const int nc = wave_keep_best(b, c, k, lane);
    float t = __builtin_inff();
    if (nc == k) t = __uint_as_float(static_cast<unsigned>(b[k - 1] >> 32));
    if (q == (lr >> 2)) {
      cnt[lr & 3] = nc;
      thr[lr & 3] = t;
    }
  }
}

// CAP: keys per row buffer (k <= CAP - 64 so that a step's 64 columns always fit after a merge).  The tile product and the key of
// a pair are tile_sweep's (knn_tile.h); this kernel is the per-row streaming selection on those keys.
template <int CAP, int METRIC>
__global__ __launch_bounds__(kBlock) void knn_tile_kernel(const float* __restrict__ x, const float* __restrict__ norms,
                                                         const float* __restrict__ ball, int n, int d, long long ldx, int k, int vec,
                                                         int tiles_per_split, long long* __restrict__ idx, float* __restrict__ dist,
                                                         u64* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  float* stage = reinterpret_cast<float*>(smem);                              // tile_sweep's operand chunks
  u64* buf = reinterpret_cast<u64*>(stage + tile_lds_floats());                // [64][CAP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const TileRange tr = tile_range(tiles_per_split, n);
  u64* mybuf = buf + wave * 16 * CAP;

  float thr[4];
  int cnt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    thr[i] = __builtin_inff();
    cnt[i] = 0;
  }

  // selection.  C layout of a 16x16 tile: column = lane & 15, row = 4 * (lane >> 4) + register
  tile_sweep<METRIC>(
      x, norms, ball, n, d, ldx, vec, tr, stage,
      [&](long long) {
        const bool full = cnt[0] > CAP - kTN || cnt[1] > CAP - kTN || cnt[2] > CAP - kTN || cnt[3] > CAP - kTN;
        if (__any(full)) wave_merge<CAP>(mybuf, k, lane, cnt, thr);
      },
      [&](int i, int, long long, long long col, float D, bool valid) {
        const bool ok = valid && D < thr[i];
        int kept;
        const int pos = cnt[i] + group16_rank(ok, q, r, &kept);
        if (ok) mybuf[(4 * q + i) * CAP + pos] = (static_cast<u64>(__float_as_uint(D)) << 32) | static_cast<unsigned>(col);
        cnt[i] += kept;
      });

  wave_merge<CAP>(mybuf, k, lane, cnt, thr);
#pragma unroll
  for (int lr = 0; lr < 16; ++lr) {
    const long long row = tr.row0 + 16 * wave + lr;
    const int c = __shfl(cnt[lr & 3], (lr >> 2) * 16, kWave);
    if (row >= n) continue;
    const u64* b = mybuf + lr * CAP;
    for (int p = lane; p < k; p += kWave) {
      const u64 key = p < c ? b[p] : kPadKey;
      if (partial != nullptr) {
        partial[(static_cast<long long>(blockIdx.y) * n + row) * k + p] = key;
      } else {
        idx[row * k + p] = static_cast<long long>(key & 0xffffffffull);
        if (dist != nullptr) dist[row * k + p] = key_distance<METRIC>(__uint_as_float(static_cast<unsigned>(key >> 32)));
      }
    }
  }
}

// one wave per row: the S sorted partial lists -> the k best
__global__ __launch_bounds__(kWave) void knn_merge_kernel(const u64* __restrict__ partial, int n, int k, int splits, int P,
                                                         int metric, long long* __restrict__ idx, float* __restrict__ dist) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* b = reinterpret_cast<u64*>(smem);
  const long long row = blockIdx.x;
  const int lane = threadIdx.x;
  wave_merge_lists(b, P, partial + row * k, static_cast<long long>(n) * k, splits, k, lane);
  for (int p = lane; p < k; p += kWave) {
    const u64 key = b[p];
    idx[row * k + p] = static_cast<long long>(key & 0xffffffffull);
    if (dist != nullptr) {
      const float v = __uint_as_float(static_cast<unsigned>(key >> 32));
      dist[row * k + p] = metric == GNPDE_METRIC_POINCARE ? key_distance<GNPDE_METRIC_POINCARE>(v) : v;
    }
  }
}

// Column splits (select.h): a workgroup per CU, never more than the merge kernel sorts (S * k <= 4096, S <= 32)
int choose_splits(long long n, int k) {
  return column_splits(n, 1, kMaxSplits, kMaxMergeKeys / k, num_cus(), g_tune[GNPDE_TUNE_KNN_SPLITS]);
}

template <int CAP, int METRIC>
int launch_tiles(const float* x, const float* norms, const float* ball, int n, int d, int ldx, int k, int splits, long long* idx,
                 float* dist, u64* partial, hipStream_t s) {
  const size_t lds = static_cast<size_t>(tile_lds_floats()) * sizeof(float) + static_cast<size_t>(kTM) * CAP * sizeof(u64);
  auto kern = knn_tile_kernel<CAP, METRIC>;
  static bool attr_set = false;
  if (!attr_set) {
    GNPDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(lds)));
    attr_set = true;
  }
  const long long tiles = (static_cast<long long>(n) + kTM - 1) / kTM;
  const int per = static_cast<int>((tiles + splits - 1) / splits);
  const int vec = tile_vec(x, d, ldx);
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(splits)), dim3(kBlock), lds, s, x, norms, ball, n,
                     d, static_cast<long long>(ldx), k, vec, per, idx, dist, partial);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

// workspace: norms [n] | a [n] (metric 1; reserved for either metric, so that one size serves both) | partial lists (S > 1)
extern "C" size_t gnpde_knn_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  (void)d;
  if (n < 1 || k < 1 || k > kMaxK || k > n) return 0;
  const int s = choose_splits(n, k);
  size_t bytes = 2 * norms_bytes(n);
  if (s > 1) bytes += align_up(static_cast<size_t>(s) * static_cast<size_t>(n) * static_cast<size_t>(k) * sizeof(u64), 256);
  return bytes;
}

extern "C" int gnpde_knn_metric(const float* x, int32_t n, int32_t d, int32_t ldx, int32_t k, int32_t metric, int64_t* idx,
                                float* dist, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(x && idx && n >= 1 && d >= 1 && ldx >= d, GNPDE_EINVAL, "knn: bad arguments (n %d, d %d, ldx %d)", n, d, ldx);
  GNPDE_CHECK_ARG(k >= 1 && k <= n && k <= kMaxK, GNPDE_ESHAPE, "knn: k = %d outside 1 .. min(n = %d, %d)", k, n, kMaxK);
  GNPDE_CHECK_ARG(metric == GNPDE_METRIC_SQEUCLIDEAN || metric == GNPDE_METRIC_POINCARE, GNPDE_ESHAPE, "knn: unknown metric %d",
                  metric);
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= gnpde_knn_workspace_bytes(n, d, k), GNPDE_EWS, "knn: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int splits = choose_splits(n, k);
  const bool poincare = metric == GNPDE_METRIC_POINCARE;
  float* norms = static_cast<float*>(workspace);
  float* ball = poincare ? reinterpret_cast<float*>(static_cast<char*>(workspace) + norms_bytes(n)) : nullptr;
  u64* partial = splits > 1 ? reinterpret_cast<u64*>(static_cast<char*>(workspace) + 2 * norms_bytes(n)) : nullptr;
  long long* out = reinterpret_cast<long long*>(idx);
  int rc = launch_norms(x, n, d, ldx, norms, ball, s);
  if (rc != 0) return rc;
  // k <= 32: 128-key row buffers, 74 KiB of LDS: two workgroups per CU.  Above: 256-key buffers fill the CU (138 KiB);
  // gnpde_tune(20, 2) takes them for every k (A/B: faster at the Cora shape, slower at ogbn-arxiv, profiles/knn_ab.jsonl)
  const bool small = k <= 32 && g_tune[GNPDE_TUNE_KNN_VARIANT] != 2;
  with_metric(metric, [&](auto m) {
    if (small) rc = launch_tiles<128, decltype(m)::value>(x, norms, ball, n, d, ldx, k, splits, out, dist, partial, s);
    else rc = launch_tiles<256, decltype(m)::value>(x, norms, ball, n, d, ldx, k, splits, out, dist, partial, s);
  });
  if (rc != 0) return rc;
  if (splits > 1) {
    const int P = sort_length(splits * k);
    const size_t lds = static_cast<size_t>(P) * sizeof(u64);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(static_cast<unsigned>(n)), dim3(kWave), lds, s, partial, n, k, splits, P, metric, out,
                       dist);
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int gnpde_knn(const float* x, int32_t n, int32_t d, int32_t ldx, int32_t k, int64_t* idx, float* dist, void* workspace,
                         size_t workspace_bytes, void* stream) {
  return gnpde_knn_metric(x, n, d, ldx, k, GNPDE_METRIC_SQEUCLIDEAN, idx, dist, workspace, workspace_bytes, stream);
}
