// k-nearest-neighbour search in feature space: BLEND's graph rewiring (reference src/graph_rewiring.py:120-126, a pykeops
// LazyTensor.argKmin over D_ij = |x_i - x_j|^2).  One fused kernel: the distance tile on the fp32 matrix cores and a streaming
// per-row top-k in LDS; no [n, n] or [chunk, n] array exists in global memory.
//
//   norms      s_i = sum_c x_ic^2 (16 lanes per row, fp32)
//   tile       a workgroup (4 waves) owns 64 query rows and walks 64-column tiles of its column range.  Per tile: K chunks of
//              16 or 32 floats of both operands staged in LDS (rows padded by 4 floats: ds_read_b128 conflict free), wave w forms rows
//              16w..16w+15 x 64 columns with v_mfma_f32_16x16x4_f32 (4 accumulators), D = (s_i + s_j) - 2 x_i.x_j clamped at 0,
//              D_ii = 0 exactly.  Selection: every row keeps the distance of its current k-th best as a threshold (+inf until k
//              are known); entries UNDER it are appended to the row's LDS buffer (ballot compaction, no atomics) as 64-bit keys
//              (distance bits << 32 | column: unsigned order = (distance, column) order).  When a row of the wave has fewer than
//              64 free slots the wave sorts its rows' buffers (bitonic, in LDS), keeps k and tightens the thresholds.  Columns
//              are walked in ascending order, so an entry EQUAL to the threshold distance has a larger column than the k-th best
//              and is rightly dropped: ties go to the smaller column.
//   merge      only when the column range is split S ways (few row tiles: Cora has 43 for 256 CUs): every split writes its
//              sorted partial keys to the workspace and one wave per row sorts the S * k keys.
//
// Every result is a function of the sorted set of (distance, column) keys and the distance of a pair does not depend on the
// tiling: bit-identical from run to run and for every S.
#include "common.h"
#include "wave_sort.h"

namespace gnpde {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTM = 64;              // query rows per workgroup (16 per wave)
constexpr int kTN = 64;              // columns per step
// K chunk staged per barrier pair: KC = 16 or 32 floats of every row, LDS row stride KC + 4 floats (5 or 9 16-byte slots: odd, so
// the 16 rows a ds_read_b128 touches fall on 16 different slots)
constexpr int kMaxK = 128;
constexpr int kMaxMergeKeys = 4096;  // S * k of the merge kernel (32 KiB of LDS per row)
constexpr int kMaxSplits = 32;
constexpr u64 kPadKey = ~0ull;

__global__ __launch_bounds__(kBlock) void knn_norms_kernel(const float* __restrict__ x, int n, int d, long long ldx,
                                                          float* __restrict__ norms) {
  const long long row = (static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x) >> 4;
  const int part = threadIdx.x & 15;
  float s = 0.f;
  if (row < n) {
    const float* xr = x + row * ldx;
    for (int c = part; c < d; c += 16) s = fmaf(xr[c], xr[c], s);
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
  if (row < n && part == 0) norms[row] = s;
}

// x[row][c .. c+3] as loaded, every address clamped into the matrix: no branch and no select sits between the load and its use
// at the next LDS store, so a chunk's loads stay in flight under the matrix work (a branch around a load, or a select on its
// result, makes the compiler wait for it on the spot).  Rows past n repeat row n - 1: their results are never selected or
// written.  Elements past d repeat element d - 1 and are zeroed by mask_group when the chunk is stored.
// VEC: one 16-byte load; the caller guarantees c + 4 <= d and 16-byte alignment.
template <bool VEC>
__device__ __forceinline__ float4 load_group(const float* __restrict__ x, long long row, int n, int c, int d, long long ldx) {
  const float* xr = x + (row < n ? row : static_cast<long long>(n) - 1) * ldx;
  if (VEC) return *reinterpret_cast<const float4*>(xr + c);
  const int last = d - 1;
  float4 v;
  v.x = xr[c < last ? c : last];
  v.y = xr[c + 1 < last ? c + 1 : last];
  v.z = xr[c + 2 < last ? c + 2 : last];
  v.w = xr[c + 3 < last ? c + 3 : last];
  return v;
}

// the K padding: elements c + e >= d are zeros (nv = d - c valid elements)
__device__ __forceinline__ float4 mask_group(float4 v, int nv) {
  v.x = nv > 0 ? v.x : 0.f;
  v.y = nv > 1 ? v.y : 0.f;
  v.z = nv > 2 ? v.z : 0.f;
  v.w = nv > 3 ? v.w : 0.f;
  return v;
}

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
    int P = 2;
    while (P < c) P <<= 1;
    for (int p = c + lane; p < P; p += kWave) b[p] = kPadKey;
    wave_lds_sync();
    wave_sort(b, P, lane);
    const int nc = c < k ? c : k;
    float t = __builtin_inff();
    if (nc == k) t = __uint_as_float(static_cast<unsigned>(b[k - 1] >> 32));
    if (q == (lr >> 2)) {
      cnt[lr & 3] = nc;
      thr[lr & 3] = t;
    }
  }
}

// CAP: keys per row buffer (k <= CAP - 64 so that a step's 64 columns always fit after a merge)
template <int CAP, int KC>
__global__ __launch_bounds__(kBlock) void knn_tile_kernel(const float* __restrict__ x, const float* __restrict__ norms, int n, int d,
                                                         long long ldx, int k, int vec, int tiles_per_split,
                                                         long long* __restrict__ idx, float* __restrict__ dist,
                                                         u64* __restrict__ partial) {
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int LD = KC + 4;
  constexpr int NP = KC / 16;          // staging passes: 256 threads cover 64 / NP rows of KC floats with one 16-byte group each
  float* As = reinterpret_cast<float*>(smem);                     // [64][LD]
  float* Bs = As + kTM * LD;                                      // [64][LD]
  u64* buf = reinterpret_cast<u64*>(Bs + kTN * LD);               // [64][CAP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const long long row0 = static_cast<long long>(blockIdx.x) * kTM;
  const long long col_begin = static_cast<long long>(blockIdx.y) * tiles_per_split * kTN;
  long long col_end = col_begin + static_cast<long long>(tiles_per_split) * kTN;
  if (col_end > n) col_end = n;
  u64* mybuf = buf + wave * 16 * CAP;
  const bool v16 = vec != 0;

  float thr[4], nrow[4];
  int cnt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long row = row0 + 16 * wave + 4 * q + i;
    thr[i] = __builtin_inff();
    cnt[i] = 0;
    nrow[i] = row < n ? norms[row] : 0.f;
  }
  const int srow = tid / (KC / 4), sc = 4 * (tid % (KC / 4));   // staging: thread -> (tile row, 4-float group of the chunk)
  constexpr int SR = 64 / NP;                                   // rows per staging pass

  float4 pa[NP], pb[NP];
  // global loads of chunk kc_ of column tile col0_ (workgroup-uniform choice: 16-byte loads while the whole chunk lies inside the rows)
  auto stage_loads = [&](long long col0_, int kc_) {
    if (v16 && kc_ + KC <= d) {
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        pa[u] = load_group<true>(x, row0 + srow + u * SR, n, kc_ + sc, d, ldx);
        pb[u] = load_group<true>(x, col0_ + srow + u * SR, n, kc_ + sc, d, ldx);
      }
    } else {
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        pa[u] = load_group<false>(x, row0 + srow + u * SR, n, kc_ + sc, d, ldx);
        pb[u] = load_group<false>(x, col0_ + srow + u * SR, n, kc_ + sc, d, ldx);
      }
    }
  };
  if (col_begin < col_end) stage_loads(col_begin, 0);

  for (long long col0 = col_begin; col0 < col_end; col0 += kTN) {
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < d; kc += KC) {
      __syncthreads();   // the previous chunk's fragment reads are done
      if (!(v16 && kc + KC <= d)) {   // (workgroup-uniform) a chunk that reaches past d
#pragma unroll
        for (int u = 0; u < NP; ++u) {
          pa[u] = mask_group(pa[u], d - kc - sc);
          pb[u] = mask_group(pb[u], d - kc - sc);
        }
      }
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        *reinterpret_cast<float4*>(&As[(srow + u * SR) * LD + sc]) = pa[u];
        *reinterpret_cast<float4*>(&Bs[(srow + u * SR) * LD + sc]) = pb[u];
      }
      __syncthreads();
      // the next chunk's global loads fly under this chunk's matrix work -- the first chunk of the next column tile under
      // the last chunk and the selection of this one
      if (kc + KC < d) stage_loads(col0, kc + KC);
      else if (col0 + kTN < col_end) stage_loads(col0 + kTN, 0);
#pragma unroll
      for (int h = 0; h < NP; ++h) {
        const float4 a = *reinterpret_cast<const float4*>(&As[(16 * wave + r) * LD + 16 * h + 4 * q]);
        float4 b[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) b[t] = *reinterpret_cast<const float4*>(&Bs[(16 * t + r) * LD + 16 * h + 4 * q]);
        // the four accumulators take turns: a dependent f32 MFMA issues 8 cycles later than an independent one
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[t].y, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[t].z, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[t].w, acc[t], 0, 0, 0);
      }
    }

    // selection.  C layout of a 16x16 tile: column = lane & 15, row = 4 * (lane >> 4) + register
    const bool full = cnt[0] > CAP - kTN || cnt[1] > CAP - kTN || cnt[2] > CAP - kTN || cnt[3] > CAP - kTN;
    if (__any(full)) wave_merge<CAP>(mybuf, k, lane, cnt, thr);
    float ncol[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long col = col0 + 16 * t + r;
      ncol[t] = col < col_end ? norms[col] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long row = row0 + 16 * wave + 4 * q + i;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const long long col = col0 + 16 * t + r;
        float D = (nrow[i] + ncol[t]) - 2.f * acc[t][i];
        D = D > 0.f ? D : 0.f;
        if (col == row) D = 0.f;
        const bool ok = row < n && col < col_end && D < thr[i];
        const u64 m = __ballot(ok);
        const unsigned g = static_cast<unsigned>(m >> (16 * q)) & 0xffffu;
        const int pos = cnt[i] + __popc(g & ((1u << r) - 1u));
        if (ok) mybuf[(4 * q + i) * CAP + pos] = (static_cast<u64>(__float_as_uint(D)) << 32) | static_cast<unsigned>(col);
        cnt[i] += __popc(g);
      }
    }
  }

  wave_merge<CAP>(mybuf, k, lane, cnt, thr);
#pragma unroll
  for (int lr = 0; lr < 16; ++lr) {
    const long long row = row0 + 16 * wave + lr;
    const int c = __shfl(cnt[lr & 3], (lr >> 2) * 16, kWave);
    if (row >= n) continue;
    const u64* b = mybuf + lr * CAP;
    for (int p = lane; p < k; p += kWave) {
      const u64 key = p < c ? b[p] : kPadKey;
      if (partial != nullptr) {
        partial[(static_cast<long long>(blockIdx.y) * n + row) * k + p] = key;
      } else {
        idx[row * k + p] = static_cast<long long>(key & 0xffffffffull);
        if (dist != nullptr) dist[row * k + p] = __uint_as_float(static_cast<unsigned>(key >> 32));
      }
    }
  }
}

// one wave per row: the S sorted partial lists -> the k best
__global__ __launch_bounds__(kWave) void knn_merge_kernel(const u64* __restrict__ partial, int n, int k, int splits, int P,
                                                         long long* __restrict__ idx, float* __restrict__ dist) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64* b = reinterpret_cast<u64*>(smem);
  const long long row = blockIdx.x;
  const int lane = threadIdx.x;
  const int total = splits * k;
  for (int p = lane; p < P; p += kWave) {
    u64 key = kPadKey;
    if (p < total) {
      const int s = p / k, j = p - s * k;
      key = partial[(static_cast<long long>(s) * n + row) * k + j];
    }
    b[p] = key;
  }
  wave_lds_sync();
  wave_sort(b, P, lane);
  for (int p = lane; p < k; p += kWave) {
    const u64 key = b[p];
    idx[row * k + p] = static_cast<long long>(key & 0xffffffffull);
    if (dist != nullptr) dist[row * k + p] = __uint_as_float(static_cast<unsigned>(key >> 32));
  }
}

int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

// Column splits: one when the row tiles alone give every CU a workgroup, otherwise enough to reach the CU count; never more
// than the merge kernel sorts (S * k <= 4096, S <= 32) or than there are column tiles.  gnpde_tune(19, S) forces S (same caps).
int choose_splits(long long n, int k) {
  const long long tiles = (n + kTM - 1) / kTM;
  long long s = g_tune[GNPDE_TUNE_KNN_SPLITS];
  if (s <= 0) s = tiles >= num_cus() ? 1 : (num_cus() + tiles - 1) / tiles;
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > kMaxMergeKeys / k) s = kMaxMergeKeys / k;
  if (s > tiles) s = tiles;
  if (s < 1) s = 1;
  // splits that would get no column tile are dropped
  const long long per = (tiles + s - 1) / s;
  s = (tiles + per - 1) / per;
  return static_cast<int>(s);
}

size_t norms_bytes(long long n) { return align_up(static_cast<size_t>(n) * sizeof(float), 256); }

template <int CAP, int KC>
int launch_tiles(const float* x, const float* norms, int n, int d, int ldx, int k, int splits, long long* idx, float* dist,
                 u64* partial, hipStream_t s) {
  const size_t lds = static_cast<size_t>(kTM + kTN) * (KC + 4) * sizeof(float) + static_cast<size_t>(kTM) * CAP * sizeof(u64);
  auto kern = knn_tile_kernel<CAP, KC>;
  static bool attr_set = false;
  if (!attr_set) {
    GNPDE_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(lds)));
    attr_set = true;
  }
  const long long tiles = (static_cast<long long>(n) + kTM - 1) / kTM;
  const int per = static_cast<int>((tiles + splits - 1) / splits);
  const int vec = (ldx % 4 == 0 && d >= 4 && reinterpret_cast<uintptr_t>(x) % 16 == 0) ? 1 : 0;
  hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(splits)), dim3(kBlock), lds, s, x, norms, n, d,
                     static_cast<long long>(ldx), k, vec, per, idx, dist, partial);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_knn_workspace_bytes(int64_t n, int32_t d, int32_t k) {
  (void)d;
  if (n < 1 || k < 1 || k > kMaxK || k > n) return 0;
  const int s = choose_splits(n, k);
  size_t bytes = norms_bytes(n);
  if (s > 1) bytes += align_up(static_cast<size_t>(s) * static_cast<size_t>(n) * static_cast<size_t>(k) * sizeof(u64), 256);
  return bytes;
}

extern "C" int gnpde_knn(const float* x, int32_t n, int32_t d, int32_t ldx, int32_t k, int64_t* idx, float* dist, void* workspace,
                         size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(x && idx && n >= 1 && d >= 1 && ldx >= d, GNPDE_EINVAL, "knn: bad arguments (n %d, d %d, ldx %d)", n, d, ldx);
  GNPDE_CHECK_ARG(k >= 1 && k <= n && k <= kMaxK, GNPDE_ESHAPE, "knn: k = %d outside 1 .. min(n = %d, %d)", k, n, kMaxK);
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= gnpde_knn_workspace_bytes(n, d, k), GNPDE_EWS, "knn: workspace too small");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int splits = choose_splits(n, k);
  float* norms = static_cast<float*>(workspace);
  u64* partial = splits > 1 ? reinterpret_cast<u64*>(static_cast<char*>(workspace) + norms_bytes(n)) : nullptr;
  long long* out = reinterpret_cast<long long*>(idx);
  const long long norm_blocks = (static_cast<long long>(n) * 16 + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(knn_norms_kernel, dim3(static_cast<unsigned>(norm_blocks)), dim3(kBlock), 0, s, x, n, d,
                     static_cast<long long>(ldx), norms);
  GNPDE_LAUNCH_CHECK();
  // k <= 32: 128-key row buffers, 74 KiB of LDS with the 16-float chunks: two workgroups per CU.  Above: 256-key buffers fill the
  // CU (138 KiB).  32-float chunks (twice the matrix work per barrier pair) measured SLOWER at the ogbn-arxiv shape and stay
  // behind gnpde_tune(20, 1) for A/B
  const int variant = g_tune[GNPDE_TUNE_KNN_VARIANT];
  int rc;
  if (k <= 32 && variant != 2) rc = launch_tiles<128, 16>(x, norms, n, d, ldx, k, splits, out, dist, partial, s);
  else if (variant == 1) rc = launch_tiles<256, 32>(x, norms, n, d, ldx, k, splits, out, dist, partial, s);
  else rc = launch_tiles<256, 16>(x, norms, n, d, ldx, k, splits, out, dist, partial, s);
  if (rc != 0) return rc;
  if (splits > 1) {
    int P = 2;
    while (P < splits * k) P <<= 1;
    const size_t lds = static_cast<size_t>(P) * sizeof(u64);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(static_cast<unsigned>(n)), dim3(kWave), lds, s, partial, n, k, splits, P, out, dist);
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}
