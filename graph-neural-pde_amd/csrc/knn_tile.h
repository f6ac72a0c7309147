// The all-pairs tile pipeline shared by the selection back-ends over pairwise keys (knn.hip: streaming per-row top-k; posdist.hip:
// radix select over all n^2 keys, radius count and fill).  A workgroup (4 waves) owns 64 rows and walks 64-column tiles of a column
// range: K chunks of both operands staged in LDS (rows padded by 4 floats: ds_read_b128 conflict free), the next chunk's global
// loads in flight under the matrix work, wave w forms rows 16w..16w+15 x 64 columns with v_mfma_f32_16x16x4_f32 (4 accumulators),
// and the epilogue turns a product into the pair's KEY:
//   metric 0 (GNPDE_METRIC_SQEUCLIDEAN)  D_ij = (s_i + s_j) - 2 x_i.x_j clamped at 0, D_ii = 0 exactly
//   metric 1 (GNPDE_METRIC_POINCARE)     r_ij = D_ij / (a_i a_j), a_i = max(1 - s_i, 2^-24): ONE IEEE division (no fast-math in
//                                        this build; hipcc's fp32 division is correctly rounded by default), r_ii = +0
// Nothing of a key depends on the tiling, and key(i, j) is bit-identical to key(j, i): the products are the same, the k order is
// the same and the additions commute.  Keys are non-negative floats: their bit patterns order as unsigned integers.
#pragma once
#include "common.h"
#include "select.h"
#include <type_traits>

namespace gnpde {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTM = kKeyTile;        // rows per workgroup (16 per wave)
constexpr int kTN = kKeyTile;        // columns per step
// K chunk staged per barrier pair: 16 floats of every row, LDS row stride 20 floats (5 16-byte slots: odd, so the 16 rows a
// ds_read_b128 touches fall on 16 different slots).  32-float chunks measured slower at both shapes (profiles/knn_ab.jsonl).
constexpr int kKC = 16;

// s_i = sum_c x_ic^2 (16 lanes per row, fp32); ball != nullptr: also a_i = max(1 - s_i, 2^-24), the Poincare denominator
__global__ __launch_bounds__(kBlock) void knn_norms_kernel(const float* __restrict__ x, int n, int d, long long ldx,
                                                          float* __restrict__ norms, float* __restrict__ ball) {
  const long long row = (static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x) >> 4;
  const int part = threadIdx.x & 15;
  float s = 0.f;
  if (row < n) {
    const float* xr = x + row * ldx;
    for (int c = part; c < d; c += 16) s = fmaf(xr[c], xr[c], s);
  }
#pragma unroll
  for (int off = 8; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
  if (row < n && part == 0) {
    norms[row] = s;
    if (ball != nullptr) ball[row] = fmaxf(1.f - s, 0x1p-24f);
  }
}

inline int launch_norms(const float* x, int n, int d, int ldx, float* norms, float* ball, hipStream_t s) {
  const long long norm_blocks = (static_cast<long long>(n) * 16 + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(knn_norms_kernel, dim3(static_cast<unsigned>(norm_blocks)), dim3(kBlock), 0, s, x, n, d,
                     static_cast<long long>(ldx), norms, ball);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

inline size_t norms_bytes(long long n) { return align_up(static_cast<size_t>(n) * sizeof(float), 256); }

// 16-byte staging loads need rows that start on 16-byte boundaries
inline int tile_vec(const float* x, int d, int ldx) { return (ldx % 4 == 0 && d >= 4 && reinterpret_cast<uintptr_t>(x) % 16 == 0) ? 1 : 0; }

inline int num_cus() {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
    if (cus <= 0) cus = 256;
  }
  return cus;
}

// the distance a key stands for, where one is returned: metric 0 keeps the key (the squared distance); metric 1
// arccosh(1 + 2 r) evaluated as log1p(2 r + 2 sqrt(r (r + 1))) (no cancellation at small r)
template <int METRIC>
__device__ __forceinline__ float key_distance(float key) {
  if (METRIC == GNPDE_METRIC_POINCARE) return log1pf(2.f * key + 2.f * sqrtf(key * (key + 1.f)));
  return key;
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

constexpr int tile_lds_floats() { return (kTM + kTN) * (kKC + 4); }

// the rows and the column range of workgroup (blockIdx.x, blockIdx.y) of a sweep whose splits take tiles_per_split column tiles each
struct TileRange { long long row0, col_begin, col_end; };
__device__ __forceinline__ TileRange tile_range(int tiles_per_split, int n) {
  const long long begin = static_cast<long long>(blockIdx.y) * tiles_per_split * kTN;
  const long long end = begin + static_cast<long long>(tiles_per_split) * kTN;
  return TileRange{static_cast<long long>(blockIdx.x) * kTM, begin, end < n ? end : n};
}

// f(the metric as a compile-time constant): the launch sites instantiate their kernel for it
template <class F>
inline void with_metric(int metric, F&& f) {
  if (metric == GNPDE_METRIC_POINCARE) f(std::integral_constant<int, GNPDE_METRIC_POINCARE>());
  else f(std::integral_constant<int, GNPDE_METRIC_SQEUCLIDEAN>());
}

// The sweep of one workgroup (all kBlock threads call it together): rows row0 .. row0 + 64 against the 64-column tiles of
// [col_begin, col_end), ascending.  Per tile, after the products: begin_tile(col0) once, then visit(i, t, row, col, key, valid)
// for the lane's 16 entries -- C layout of a 16x16 tile: col = col0 + 16 t + (lane & 15), row = row0 + 16 wave + 4 (lane >> 4) + i;
// valid = row < n && col < col_end.  Both are called by every lane (ballots inside them are whole).  stage: tile_lds_floats()
// floats of LDS.  ball (metric 1): the a_i of knn_norms_kernel.
template <int METRIC, class BeginTile, class Visit>
__device__ __forceinline__ void tile_sweep(const float* __restrict__ x, const float* __restrict__ norms,
                                           const float* __restrict__ ball, int n, int d, long long ldx, int vec, const TileRange& tr,
                                           float* stage, BeginTile&& begin_tile, Visit&& visit) {
  constexpr int KC = kKC, LD = KC + 4;
  const long long row0 = tr.row0, col_begin = tr.col_begin, col_end = tr.col_end;
  // staging passes: 256 threads cover 64 / NP rows of KC floats with one 16-byte group each.  NP is 1, and the loops over it stay:
  // with pa / pb as plain float4s the compiler folds the two load forms of stage_loads into one and waits on them earlier
  // (318 against 229 ms at the ogbn-arxiv shape)
  constexpr int NP = KC / 16;
  float* As = stage;                   // [64][LD]
  float* Bs = As + kTM * LD;           // [64][LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const bool v16 = vec != 0;

  float nrow[4], arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long row = row0 + 16 * wave + 4 * q + i;
    nrow[i] = row < n ? norms[row] : 0.f;
    if (METRIC == GNPDE_METRIC_POINCARE) arow[i] = row < n ? ball[row] : 1.f;
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

    begin_tile(col0);
    float ncol[4], acol[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const long long col = col0 + 16 * t + r;
      ncol[t] = col < col_end ? norms[col] : 0.f;
      if (METRIC == GNPDE_METRIC_POINCARE) acol[t] = col < col_end ? ball[col] : 1.f;
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
        if (METRIC == GNPDE_METRIC_POINCARE) D = D / (arow[i] * acol[t]);
        visit(i, t, row, col, D, row < n && col < col_end);
      }
    }
  }
}

}  // namespace
}  // namespace gnpde
