// DeepWalk positional encodings (reference src/deepwalk_embeddings.py: torch_geometric's Node2Vec with p = q = 1, SparseAdam): uniform
// random walks, the skip-gram-with-negative-sampling step and the sparse Adam update.  include/gnpde.h has the definitions.
//   walks_kernel        one lane per walk; word t of walk w is word (t & 3) of block w ceil(L / 4) + (t >> 2) of the Philox stream
//                       (philox.h), so a walk does not depend on the launch shape.  Positive walks follow the CSR graph, negative
//                       walks draw every column uniformly from [0, n).
//   permutation         keys (word_i << 32 | i), radix sort, low words
//   pair_kernel         one wave per walk: stages the walk's L + 1 embedding rows in LDS, forms the J (C - 1) window dot products in
//                       lane groups of G = the power of two >= d / 4 (a fixed butterfly inside the group), keeps their coefficients
//                       scale * dl/dx in LDS, and reduces INSIDE the walk: position p gets ONE contribution row
//                       sum_q coef(min(p, q), max(p, q)) e[rw[q]].  Plain stores of [R, L + 1, d] rows, one partial loss per walk,
//                       and the (node << 32 | slot) key of every slot.
//   radix sort          of the keys: the inverted index (per node, its slots ascending)
//   adam_kernel         one lane group per sorted entry; the head of a run adds the run's contribution rows in slot order and
//                       updates m, v and e of that row.  No float atomics anywhere: bit-identical from run to run.
//   loss_kernel         the partial losses (float64) summed in a fixed order by one workgroup
// walk_step.h holds what the step shares with hyperbolic.hip: the step's workspace layout, the sort's key bits and loss_kernel.
#include "common.h"
#include "philox.h"
#include "select.h"
#include "walk_step.h"

#include <cmath>

namespace gnpde {
namespace {

constexpr int kMaxWalkLength = 127;
constexpr int kMaxDim = 256;
constexpr int kLdsFloats = 16384;       // 64 KiB: a walk's rows and coefficients

inline dim3 grid_of(long long items) {
  long long b = (items + kBlock - 1) / kBlock;
  if (b < 1) b = 1;
  return dim3(static_cast<unsigned>(b));
}

__global__ __launch_bounds__(kBlock) void walks_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, long long n_edges,
                                                      unsigned n, const long long* __restrict__ starts, long long n_starts, long long R, int L,
                                                      u64 seed, unsigned stream, unsigned call, u64 first_walk, int negative,
                                                      int* __restrict__ out, int* __restrict__ flag) {
  const long long r = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (r >= R) return;
  long long s = starts[r % n_starts];
  if (s < 0 || s >= static_cast<long long>(n)) {
    atomicOr(flag, GNPDE_DEEPWALK_BAD_START);
    s = 0;
  }
  int cur = static_cast<int>(s);
  int* o = out + r * (L + 1);
  o[0] = cur;
  const int nb = (L + 3) >> 2;
  const u64 base = (first_walk + static_cast<u64>(r)) * static_cast<u64>(nb);
  for (int q = 0; q < nb; ++q) {
    const Words4 x = stream_block(seed, stream, call, base + static_cast<u64>(q));
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int t = 4 * q + w;
      if (t >= L) break;
      if (negative) {
        cur = static_cast<int>((static_cast<u64>(x.w[w]) * n) >> 32);
      } else {
        const long long b = rowptr[cur], e = rowptr[cur + 1];
        if (b < 0 || e > n_edges || e < b) {
          atomicOr(flag, GNPDE_DEEPWALK_BAD_GRAPH);
        } else if (e > b) {                                     // out-degree 0: the walk stays
          const int nxt = col[b + static_cast<long long>((static_cast<u64>(x.w[w]) * static_cast<u64>(e - b)) >> 32)];
          if (static_cast<unsigned>(nxt) >= n) atomicOr(flag, GNPDE_DEEPWALK_BAD_GRAPH);
          else cur = nxt;
        }
      }
      o[t + 1] = cur;
    }
  }
}

__global__ __launch_bounds__(kBlock) void perm_keys_kernel(long long n, u64 seed, unsigned stream, unsigned call, u64* __restrict__ keys) {
  const long long b = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (4 * b >= n) return;
  const Words4 x = stream_block(seed, stream, call, static_cast<u64>(b));
#pragma unroll
  for (int w = 0; w < 4; ++w)
    if (4 * b + w < n) keys[4 * b + w] = (static_cast<u64>(x.w[w]) << 32) | static_cast<u64>(4 * b + w);
}

__global__ __launch_bounds__(kBlock) void perm_decode_kernel(const u64* __restrict__ keys, long long n, long long* __restrict__ out) {
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) out[i] = static_cast<long long>(keys[i] & 0xffffffffull);
}

struct StepShape {
  int L, C, J, P, d, d4, G, waves;     // P = J (C - 1) pairs per walk; G lanes per pair / position; waves per workgroup
  int lds_floats;                      // per wave: rows (L + 1) d, then the P coefficients (rounded up to a multiple of 4)
};

// one wave per walk; every wave of a workgroup runs the same trip counts (the barriers below are workgroup barriers), a wave past the
// last walk recomputes the last walk and stores nothing
__global__ __launch_bounds__(kBlock) void pair_kernel(const float* __restrict__ emb, int ld, unsigned n, const int* __restrict__ pos_rw,
                                                     long long r_pos, const int* __restrict__ neg_rw, long long r_neg, StepShape sh,
                                                     float scale_pos, float scale_neg, double mean_pos, double mean_neg,
                                                     float* __restrict__ contrib, u64* __restrict__ keys,
                                                     double* __restrict__ partial, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r_tot = r_pos + r_neg;
  long long walk = static_cast<long long>(blockIdx.x) * sh.waves + wave;
  const bool live = walk < r_tot;
  if (!live) walk = r_tot - 1;
  const bool positive = walk < r_pos;
  const int L = sh.L, C = sh.C, d = sh.d, d4 = sh.d4, G = sh.G;
  const int* rw = positive ? pos_rw + walk * (L + 1) : neg_rw + (walk - r_pos) * (L + 1);
  float* rows = lds + static_cast<size_t>(wave) * sh.lds_floats;
  float* coef = rows + (L + 1) * d;

  // node ids: position p in lane p (id0) or lane p - 64 (id1); an id outside [0, n) raises the flag and counts as node 0
  int id0 = 0, id1 = 0;
  bool bad = false;
  if (lane <= L) {
    id0 = rw[lane];
    if (static_cast<unsigned>(id0) >= n) { bad = true; id0 = 0; }
  }
  if (lane + 64 <= L) {
    id1 = rw[lane + 64];
    if (static_cast<unsigned>(id1) >= n) { bad = true; id1 = 0; }
  }
  if (bad) atomicOr(flag, GNPDE_DEEPWALK_BAD_WALK);
  if (live) {
    const u64 slot = static_cast<u64>(walk) * (L + 1);
    if (lane <= L) keys[slot + lane] = (static_cast<u64>(id0) << 32) | (slot + lane);
    if (lane + 64 <= L) keys[slot + lane + 64] = (static_cast<u64>(id1) << 32) | (slot + lane + 64);
  }

  // stage the L + 1 rows: item i = (position i / d4, 16-byte column i % d4)
  const int items = (L + 1) * d4;
  for (int i0 = 0; i0 < items; i0 += kWave) {
    const int i = i0 + lane;
    const int p = min(i / d4, L), c = i % d4;
    const int a = __shfl(id0, p & 63, kWave), b = __shfl(id1, p & 63, kWave);
    const int id = p < 64 ? a : b;
    if (i < items) st4(rows + p * d + 4 * c, ld4(emb + static_cast<size_t>(id) * ld + 4 * c));
  }
  __syncthreads();

  // dot products, coefficients and the loss: pair q = (a, a + 1 + j), a = q / (C - 1), j = q % (C - 1)
  const int g = lane / G, li = lane % G, per = kWave / G;
  const float scale = positive ? scale_pos : scale_neg;
  double loss = 0.0;
  for (int q0 = 0; q0 < sh.P; q0 += per) {
    const int q = q0 + g;
    float s = 0.0f;
    if (q < sh.P && li < d4) {
      const int a = q / (C - 1), b = a + 1 + q % (C - 1);
      const float4 x = ld4(rows + a * d + 4 * li), y = ld4(rows + b * d + 4 * li);
      s = x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
    }
    for (int off = G >> 1; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
    if (q < sh.P && li == 0) {
      // sigma(x) and sigma(-x) without cancellation: u = exp(-|x|), big = 1 / (1 + u), small = u / (1 + u)
      const float u = expf(-fabsf(s));
      const float big = 1.0f / (1.0f + u), small = u * big;
      const float sp = s >= 0.0f ? big : small, sm = s >= 0.0f ? small : big;      // sigma(x), sigma(-x)
      const float target = positive ? sp : sm;                                      // the loss is -log(target + EPS)
      const float denom = target + 1e-15f;
      loss += static_cast<double>(-logf(denom));
      const float dldx = sp * sm / denom;                                           // |d loss / d x|
      coef[q] = positive ? -scale * dldx : scale * dldx;
    }
  }
  __syncthreads();

  // contribution row of position p: sum over q != p with |p - q| <= C - 1 and min(p, q) < J of coef(min, max) * row q, ascending q
  for (int p0 = 0; p0 <= L; p0 += per) {
    const int p = p0 + g;
    if (p <= L && li < d4) {
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const int lo = max(0, p - (C - 1)), hi = min(L, p + (C - 1));
      for (int q = lo; q <= hi; ++q) {
        if (q == p) continue;
        const int a = min(p, q), b = max(p, q);
        if (a >= sh.J) continue;
        const float c = coef[a * (C - 1) + (b - a - 1)];
        const float4 y = ld4(rows + q * d + 4 * li);
        acc.x += c * y.x; acc.y += c * y.y; acc.z += c * y.z; acc.w += c * y.w;
      }
      if (live) st4(contrib + (static_cast<size_t>(walk) * (L + 1) + p) * d + 4 * li, acc);
    }
  }
  loss = wave_sum(loss);
  if (live && lane == 0) partial[walk] = loss * (positive ? mean_pos : mean_neg);
}

// G lanes per sorted entry; the head of a node's run sums the run's contribution rows in slot order and applies SparseAdam to the row
__global__ __launch_bounds__(kBlock) void adam_kernel(const u64* __restrict__ sorted, long long S, const float* __restrict__ contrib, int d,
                                                     int d4, int G, float* __restrict__ emb, int ld, float* __restrict__ m, float* __restrict__ v,
                                                     int ld_mv, float step_size, float beta1, float beta2, float eps) {
  const int per = kBlock / G;
  const long long i = static_cast<long long>(blockIdx.x) * per + threadIdx.x / G;
  const int li = threadIdx.x % G;
  if (i >= S || li >= d4) return;
  const u64 node = sorted[i] >> 32;
  if (i > 0 && (sorted[i - 1] >> 32) == node) return;
  float4 gsum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (long long j = i; j < S; ++j) {
    const u64 k = sorted[j];
    if ((k >> 32) != node) break;
    const float4 c = ld4(contrib + static_cast<size_t>(k & 0xffffffffull) * d + 4 * li);
    gsum.x += c.x; gsum.y += c.y; gsum.z += c.z; gsum.w += c.w;
  }
  float* pe = emb + static_cast<size_t>(node) * ld + 4 * li;
  float* pm = m + static_cast<size_t>(node) * ld_mv + 4 * li;
  float* pv = v + static_cast<size_t>(node) * ld_mv + 4 * li;
  float4 e4 = ld4(pe), m4 = ld4(pm), v4 = ld4(pv);
  const float gg[4] = {gsum.x, gsum.y, gsum.z, gsum.w};
  float ee[4] = {e4.x, e4.y, e4.z, e4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    mm[c] = mm[c] + (gg[c] - mm[c]) * (1.0f - beta1);
    vv[c] = vv[c] + (gg[c] * gg[c] - vv[c]) * (1.0f - beta2);
    ee[c] = ee[c] - step_size * (mm[c] / (sqrtf(vv[c]) + eps));
  }
  st4(pe, make_float4(ee[0], ee[1], ee[2], ee[3]));
  st4(pm, make_float4(mm[0], mm[1], mm[2], mm[3]));
  st4(pv, make_float4(vv[0], vv[1], vv[2], vv[3]));
}

// the limits of the step; returns nullptr when the shape is supported, else the message
const char* step_shape(int L, int C, int d, StepShape* sh) {
  if (L < 1 || L > kMaxWalkLength) return "walk_length outside 1 .. 127";
  if (C < 2 || C > L) return "context_size outside 2 .. walk_length";
  if (d < 4 || d > kMaxDim || d % 4 != 0) return "the embedding width must be a multiple of 4 in 4 .. 256";
  sh->L = L; sh->C = C; sh->d = d; sh->d4 = d / 4;
  sh->J = L + 2 - C;
  sh->P = sh->J * (C - 1);
  int G = 1;
  while (G < sh->d4) G <<= 1;
  sh->G = G;
  sh->lds_floats = (L + 1) * d + (sh->P + 3) / 4 * 4;
  if ((L + 1) * d > kLdsFloats) return "(walk_length + 1) * width exceeds 16384 floats (64 KiB of LDS)";
  if (sh->lds_floats > kLdsFloats) return "(walk_length + 1) * width + windows * (context_size - 1) exceeds 16384 floats (64 KiB of LDS)";
  sh->waves = kLdsFloats / sh->lds_floats;
  if (sh->waves > kWavesPerBlock) sh->waves = kWavesPerBlock;
  return nullptr;
}

struct PermLayout {
  size_t keys, sorted, temp, temp_bytes, total;
};

PermLayout perm_layout(long long n) {
  PermLayout Y{};
  const size_t nn = static_cast<size_t>(n > 0 ? n : 1);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  Y.keys = take(nn * 8);
  Y.sorted = take(nn * 8);
  size_t t = 0;
  u64* p = nullptr;
  if (rocprim::radix_sort_keys(nullptr, t, p, p, nn, 0, 64, nullptr) != hipSuccess) return Y;
  Y.temp_bytes = align_up(t + 256, 256);
  Y.temp = take(Y.temp_bytes);
  Y.total = off;
  return Y;
}

int launch_walks(const int* rowptr, const int* col, long long n_edges, int n, const int64_t* starts, int64_t n_starts, int64_t R, int L,
                 uint64_t seed, uint32_t stream_id, uint32_t call, uint64_t first_walk, int negative, int32_t* out, int32_t* flag, void* stream) {
  if (R == 0) return 0;
  hipLaunchKernelGGL(walks_kernel, grid_of(R), dim3(kBlock), 0, static_cast<hipStream_t>(stream), rowptr, col, n_edges,
                     static_cast<unsigned>(n), reinterpret_cast<const long long*>(starts), static_cast<long long>(n_starts),
                     static_cast<long long>(R), L, seed, stream_id, call, first_walk, negative, out, flag);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

#define WALK_ARGS_OK(who)                                                                                                          \
  GNPDE_CHECK_ARG(n >= 1 && n_walks >= 0 && n_starts >= 0 && flag, GNPDE_EINVAL, who ": bad arguments (1 <= n <= INT32_MAX)");       \
  GNPDE_CHECK_ARG(walk_length >= 1 && walk_length <= kMaxWalkLength, GNPDE_ESHAPE, who ": walk_length %d outside 1 .. %d",         \
                  walk_length, kMaxWalkLength);                                                                                     \
  GNPDE_CHECK_ARG(n_walks == 0 || (starts && out && n_starts >= 1), GNPDE_EINVAL, who ": walks without start nodes or output");     \
  GNPDE_CHECK_ARG(n_walks <= INT32_MAX, GNPDE_ESHAPE, who ": more than INT32_MAX walks in one call")

extern "C" int gnpde_random_walks(const int32_t* rowptr, const int32_t* col, int64_t n_edges, int32_t n, const int64_t* starts,
                                  int64_t n_starts, int64_t n_walks, int32_t walk_length, uint64_t seed, uint32_t stream_id, uint32_t call,
                                  uint64_t first_walk, int32_t* out, int32_t* flag, void* stream) {
  WALK_ARGS_OK("random_walks");
  GNPDE_CHECK_ARG(rowptr && n_edges >= 0 && n_edges <= INT32_MAX && (n_edges == 0 || col), GNPDE_EINVAL,
                  "random_walks: bad graph (rowptr [n + 1] and col [n_edges] int32, n_edges <= INT32_MAX)");
  return launch_walks(rowptr, col, n_edges, n, starts, n_starts, n_walks, walk_length, seed, stream_id, call, first_walk, 0, out, flag, stream);
}

extern "C" int gnpde_negative_walks(int32_t n, const int64_t* starts, int64_t n_starts, int64_t n_walks, int32_t walk_length, uint64_t seed,
                                    uint32_t stream_id, uint32_t call, uint64_t first_walk, int32_t* out, int32_t* flag, void* stream) {
  WALK_ARGS_OK("negative_walks");
  return launch_walks(nullptr, nullptr, 0, n, starts, n_starts, n_walks, walk_length, seed, stream_id, call, first_walk, 1, out, flag, stream);
}

extern "C" size_t gnpde_random_permutation_workspace_bytes(int64_t n) {
  if (n < 1 || n > INT32_MAX) return 0;
  return perm_layout(n).total;
}

extern "C" int gnpde_random_permutation(int64_t n, uint64_t seed, uint32_t stream_id, uint32_t call, int64_t* out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(n >= 1 && n <= INT32_MAX && out, GNPDE_EINVAL, "random_permutation: bad arguments (1 <= n <= INT32_MAX)");
  const PermLayout Y = perm_layout(n);
  GNPDE_CHECK_ARG(Y.total != 0, GNPDE_ESTATE, "random_permutation: the sort's temporary-storage query failed");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= Y.total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "random_permutation: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, Y.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  u64* keys = reinterpret_cast<u64*>(ws + Y.keys);
  u64* sorted = reinterpret_cast<u64*>(ws + Y.sorted);
  hipLaunchKernelGGL(perm_keys_kernel, grid_of((n + 3) / 4), dim3(kBlock), 0, s, static_cast<long long>(n), seed, stream_id, call, keys);
  GNPDE_LAUNCH_CHECK();
  size_t tb = Y.temp_bytes;
  GNPDE_HIP(rocprim::radix_sort_keys(ws + Y.temp, tb, keys, sorted, static_cast<size_t>(n), 0, 64, s));
  hipLaunchKernelGGL(perm_decode_kernel, grid_of(n), dim3(kBlock), 0, s, sorted, static_cast<long long>(n), reinterpret_cast<long long*>(out));
  GNPDE_LAUNCH_CHECK();
  return 0;
}

static int step_args(const char* who, int64_t r_pos, int64_t r_neg, int32_t L, int32_t C, int32_t d, StepShape* sh) {
  const char* why = step_shape(L, C, d, sh);
  GNPDE_CHECK_ARG(why == nullptr, GNPDE_ESHAPE, "%s: %s (walk_length %d, context_size %d, width %d)", who, why, L, C, d);
  GNPDE_CHECK_ARG(r_pos >= 1 && r_neg >= 1, GNPDE_EINVAL, "%s: at least one positive and one negative walk are needed", who);
  GNPDE_CHECK_ARG((r_pos + r_neg) * static_cast<int64_t>(L + 1) <= INT32_MAX, GNPDE_ESHAPE, "%s: more than INT32_MAX walk positions in one step", who);
  return 0;
}

extern "C" size_t gnpde_deepwalk_step_workspace_bytes(int64_t r_pos, int64_t r_neg, int32_t walk_length, int32_t context_size, int32_t d) {
  StepShape sh;
  if (step_args("deepwalk_step_workspace_bytes", r_pos, r_neg, walk_length, context_size, d, &sh) != 0) return 0;
  return step_layout(r_pos + r_neg, walk_length, d).total;
}

extern "C" int gnpde_deepwalk_step(float* emb, int32_t ld, float* m, float* v, int32_t ld_mv, int32_t n, int32_t d, int32_t t,
                                   const int32_t* pos_rw, int64_t r_pos, const int32_t* neg_rw, int64_t r_neg, int32_t walk_length,
                                   int32_t context_size, float lr, float beta1, float beta2, float eps, float* loss_out, int32_t* flag,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  StepShape sh;
  const int rc = step_args("deepwalk_step", r_pos, r_neg, walk_length, context_size, d, &sh);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(emb && m && v && pos_rw && neg_rw && loss_out && flag && n >= 1, GNPDE_EINVAL, "deepwalk_step: bad arguments (null pointer or n < 1)");
  GNPDE_CHECK_ARG(ld >= d && ld_mv >= d && ld % 4 == 0 && ld_mv % 4 == 0, GNPDE_EINVAL,
                  "deepwalk_step: row strides %d / %d must be multiples of 4 and at least the width %d", ld, ld_mv, d);
  GNPDE_CHECK_ARG((reinterpret_cast<uintptr_t>(emb) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) % 16 == 0, GNPDE_EINVAL,
                  "deepwalk_step: emb, m and v must be 16-byte aligned");
  GNPDE_CHECK_ARG(t >= 1, GNPDE_EINVAL, "deepwalk_step: the step count t = %d starts at 1", t);
  GNPDE_CHECK_ARG(lr >= 0.0f && beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f && eps >= 0.0f, GNPDE_EINVAL,
                  "deepwalk_step: lr >= 0, 0 <= beta < 1 and eps >= 0 are required");
  const long long r_tot = r_pos + r_neg;
  const StepLayout Y = step_layout(r_tot, walk_length, d);
  GNPDE_CHECK_ARG(Y.total != 0, GNPDE_ESTATE, "deepwalk_step: the sort's temporary-storage query failed");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= Y.total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "deepwalk_step: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, Y.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  u64* keys = reinterpret_cast<u64*>(ws + Y.keys);
  u64* sorted = reinterpret_cast<u64*>(ws + Y.sorted);
  float* contrib = reinterpret_cast<float*>(ws + Y.contrib);
  double* partial = reinterpret_cast<double*>(ws + Y.partial);
  const long long S = r_tot * (walk_length + 1);
  const double mean_pos = 1.0 / (static_cast<double>(r_pos) * sh.P), mean_neg = 1.0 / (static_cast<double>(r_neg) * sh.P);
  const float scale_pos = static_cast<float>(mean_pos), scale_neg = static_cast<float>(mean_neg);
  const unsigned blocks = static_cast<unsigned>((r_tot + sh.waves - 1) / sh.waves);
  hipLaunchKernelGGL(pair_kernel, dim3(blocks), dim3(sh.waves * kWave), static_cast<size_t>(sh.waves) * sh.lds_floats * sizeof(float), s, emb, ld,
                     static_cast<unsigned>(n), pos_rw, static_cast<long long>(r_pos), neg_rw, static_cast<long long>(r_neg), sh, scale_pos,
                     scale_neg, mean_pos, mean_neg, contrib, keys, partial, flag);
  GNPDE_LAUNCH_CHECK();
  size_t tb = Y.temp_bytes;
  GNPDE_HIP(rocprim::radix_sort_keys(ws + Y.temp, tb, keys, sorted, static_cast<size_t>(S), 0, slot_key_bits(n), s));
  const double bc1 = 1.0 - std::pow(static_cast<double>(beta1), t), bc2 = 1.0 - std::pow(static_cast<double>(beta2), t);
  const float step_size = static_cast<float>(static_cast<double>(lr) * std::sqrt(bc2) / bc1);
  const int per = kBlock / sh.G;
  hipLaunchKernelGGL(adam_kernel, dim3(static_cast<unsigned>((S + per - 1) / per)), dim3(kBlock), 0, s, sorted, S, contrib, d, sh.d4, sh.G, emb, ld,
                     m, v, ld_mv, step_size, beta1, beta2, eps);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(kBlock), 0, s, partial, static_cast<long long>(r_pos), static_cast<long long>(r_neg), loss_out);
  GNPDE_LAUNCH_CHECK();
  return 0;
}
