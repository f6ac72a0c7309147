// Hyperbolic positional encodings (BLEND's `--pos_enc_type HYPS<dd>`): one row-normalised Riemannian SGD step on the Poincare ball
// over DeepWalk's walks and windows.  include/gnpde.h has the definitions; the walks and the epoch order are deepwalk.hip's entry
// points on stream ids of their own.
//   pair_kernel         one wave per walk: stages the walk's L + 1 embedding rows in LDS (a width of 2 is padded to 4 with zeros),
//                       forms |e|^2 per position and q = |e_a - e_b|^2 per window pair in lane groups of G = the power of two
//                       >= d / 4 (a fixed butterfly inside the group), keeps per pair w = dl/ddist * 1/sqrt(r (1 + r)) * 2 / (alpha beta)
//                       and q in LDS, and reduces INSIDE the walk: position p gets ONE contribution row
//                       sum_q w(p, q) [(1 + q(p, q) / alpha_p) e_p - e_q].  Plain stores of [R, L + 1, max(d, 4)] rows, one partial loss
//                       per walk, and the (node << 32 | slot) key of every slot.
//   radix sort          of the keys: the inverted index (per node, its slots ascending)
//   update_kernel       one lane group per sorted entry; the head of a run adds the run's contribution rows in slot order, counts the
//                       run's pair ends (a function of the slot's position alone), rescales, updates and projects that row.  No float
//                       atomics anywhere: bit-identical from run to run.
//   loss_kernel         the partial losses (float64) summed in a fixed order by one workgroup (walk_step.h)
#include "common.h"
#include "select.h"
#include "walk_step.h"

#include <cmath>

namespace gnpde {
namespace {

constexpr int kMaxWalkLength = 127;
constexpr int kMaxDim = 128;
constexpr int kLdsFloats = 16384;       // 64 KiB: a walk's rows, squared norms and pair coefficients
constexpr float kBallEdge = 1.0f - 1e-5f;

struct StepShape {
  int L, C, J, P, d, dp, d4, G, waves;  // P = J (C - 1) pairs per walk; dp = max(d, 4) floats per staged row; G lanes per pair / position
  int pairs_at;                         // per wave: rows (L + 1) dp, then L + 1 squared norms (rounded up to a multiple of 4), then
  int lds_floats;                       // the P coefficients w and the P squared distances q (each rounded up to a multiple of 4)
};

__device__ __forceinline__ float group_sum(float s, int G) {
  for (int off = G >> 1; off >= 1; off >>= 1) s += __shfl_xor(s, off, kWave);
  return s;
}

// row `id` of emb as the 16-byte column c of the staged row; a width of 2 has one column whose upper half is zero
__device__ __forceinline__ float4 load_row4(const float* __restrict__ emb, int ld, int d, int id, int c) {
  const float* p = emb + static_cast<size_t>(id) * ld;
  if (d == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    return make_float4(v.x, v.y, 0.0f, 0.0f);
  }
  return ld4(p + 4 * c);
}

// one wave per walk; every wave of a workgroup runs the same trip counts (the barriers below are workgroup barriers), a wave past the
// last walk recomputes the last walk and stores nothing
__global__ __launch_bounds__(kBlock) void pair_kernel(const float* __restrict__ emb, int ld, unsigned n, const int* __restrict__ pos_rw,
                                                     long long r_pos, const int* __restrict__ neg_rw, long long r_neg, StepShape sh,
                                                     float radius, float temperature, double mean_pos, double mean_neg,
                                                     float* __restrict__ contrib, u64* __restrict__ keys,
                                                     double* __restrict__ partial, int* __restrict__ flag) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long r_tot = r_pos + r_neg;
  long long walk = static_cast<long long>(blockIdx.x) * sh.waves + wave;
  const bool live = walk < r_tot;
  if (!live) walk = r_tot - 1;
  const bool positive = walk < r_pos;
  const int L = sh.L, C = sh.C, dp = sh.dp, d4 = sh.d4, G = sh.G;
  const int* rw = positive ? pos_rw + walk * (L + 1) : neg_rw + (walk - r_pos) * (L + 1);
  float* rows = lds + static_cast<size_t>(wave) * sh.lds_floats;
  float* sq = rows + (L + 1) * dp;
  float* coef = rows + sh.pairs_at;
  float* dist2 = coef + (sh.P + 3) / 4 * 4;

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
    if (i < items) st4(rows + p * dp + 4 * c, load_row4(emb, ld, sh.d, id, c));
  }
  __syncthreads();

  // s_p = |e_p|^2
  const int g = lane / G, li = lane % G, per = kWave / G;
  for (int p0 = 0; p0 <= L; p0 += per) {
    const int p = p0 + g;
    float s = 0.0f;
    if (p <= L && li < d4) {
      const float4 x = ld4(rows + p * dp + 4 * li);
      s = x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
    }
    s = group_sum(s, G);
    if (p <= L && li == 0) sq[p] = s;
  }
  __syncthreads();

  // squared distances, coefficients and the loss: pair q = (a, a + 1 + j), a = q / (C - 1), j = q % (C - 1)
  double loss = 0.0;
  for (int q0 = 0; q0 < sh.P; q0 += per) {
    const int q = q0 + g;
    const int a = min(q, sh.P - 1) / (C - 1), b = a + 1 + min(q, sh.P - 1) % (C - 1);
    float s = 0.0f;
    if (q < sh.P && li < d4) {
      const float4 x = ld4(rows + a * dp + 4 * li), y = ld4(rows + b * dp + 4 * li);
      const float4 t = make_float4(x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w);
      s = t.x * t.x + t.y * t.y + t.z * t.z + t.w * t.w;
    }
    s = group_sum(s, G);
    if (q < sh.P && li == 0) {
      const float ab = (1.0f - sq[a]) * (1.0f - sq[b]);
      const float r = s / ab;
      const bool apart = r > 0.0f;                                                  // r == 0: the same point, dist = 0 and no gradient
      const float dist = apart ? 2.0f * logf(sqrtf(r) + sqrtf(1.0f + r)) : 0.0f;
      const float x = (radius - dist) / temperature;
      // sigma(x) and sigma(-x) without cancellation: u = exp(-|x|), big = 1 / (1 + u), small = u / (1 + u)
      const float u = expf(-fabsf(x));
      const float big = 1.0f / (1.0f + u), small = u * big;
      const float sp = x >= 0.0f ? big : small, sm = x >= 0.0f ? small : big;      // sigma(x), sigma(-x)
      const float target = positive ? sp : sm;                                      // the loss term is -log(target + EPS)
      const float denom = target + 1e-15f;
      loss += static_cast<double>(-logf(denom));
      const float dldx = sp * sm / denom;                                           // |d loss / d x|; d x / d dist = -1 / T
      const float dldd = (positive ? dldx : -dldx) / temperature;
      coef[q] = apart ? dldd * (1.0f / sqrtf(r * (1.0f + r))) * (2.0f / ab) : 0.0f;
      dist2[q] = s;
    }
  }
  __syncthreads();

  // contribution row of position p: over q != p with |p - q| <= C - 1 and min(p, q) < J, ascending q,
  //   sum of w [(1 + dist2 / alpha_p) e_p - e_q]  =  (sum of w (1 + dist2 / alpha_p)) e_p - sum of w e_q
  for (int p0 = 0; p0 <= L; p0 += per) {
    const int p = p0 + g;
    if (p <= L && li < d4) {
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      float own = 0.0f;
      const float alpha = 1.0f - sq[p];
      const int lo = max(0, p - (C - 1)), hi = min(L, p + (C - 1));
      for (int q = lo; q <= hi; ++q) {
        if (q == p) continue;
        const int a = min(p, q), b = max(p, q);
        if (a >= sh.J) continue;
        const int k = window_pair_index(a, b, C);
        const float w = coef[k];
        own += w * (1.0f + dist2[k] / alpha);
        const float4 y = ld4(rows + q * dp + 4 * li);
        acc.x -= w * y.x; acc.y -= w * y.y; acc.z -= w * y.z; acc.w -= w * y.w;
      }
      const float4 e = ld4(rows + p * dp + 4 * li);
      acc.x += own * e.x; acc.y += own * e.y; acc.z += own * e.z; acc.w += own * e.w;
      if (live) st4(contrib + (static_cast<size_t>(walk) * (L + 1) + p) * dp + 4 * li, acc);
    }
  }
  loss = wave_sum(loss);
  if (live && lane == 0) partial[walk] = loss * (positive ? mean_pos : mean_neg);
}

// G lanes per sorted entry; the head of a node's run sums the run's contribution rows in slot order, divides by the run's pair ends
// and moves the row:  e <- proj(e - lr (alpha^2 / 4) g / c).  A whole group leaves together, so the butterflies see every lane.
__global__ __launch_bounds__(kBlock) void update_kernel(const u64* __restrict__ sorted, long long S, const float* __restrict__ contrib, int L,
                                                       int C, int d, int dp, int d4, int G, float* __restrict__ emb, int ld, float lr) {
  const int per = kBlock / G;
  const long long i = static_cast<long long>(blockIdx.x) * per + threadIdx.x / G;
  const int li = threadIdx.x % G;
  if (i >= S) return;
  const u64 node = sorted[i] >> 32;
  if (i > 0 && (sorted[i - 1] >> 32) == node) return;
  const bool mine = li < d4;
  float4 gsum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  long long ends = 0;
  for (long long j = i; j < S; ++j) {
    const u64 k = sorted[j];
    if ((k >> 32) != node) break;
    const u64 slot = k & 0xffffffffull;
    ends += window_pair_ends(static_cast<int>(slot % static_cast<u64>(L + 1)), L, C);
    if (mine) {
      const float4 c = ld4(contrib + static_cast<size_t>(slot) * dp + 4 * li);
      gsum.x += c.x; gsum.y += c.y; gsum.z += c.z; gsum.w += c.w;
    }
  }
  float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (mine) e = load_row4(emb, ld, d, static_cast<int>(node), li);
  const float alpha = 1.0f - group_sum(e.x * e.x + e.y * e.y + e.z * e.z + e.w * e.w, G);
  const float step = lr * (alpha * alpha * 0.25f) / static_cast<float>(ends);
  float4 y = make_float4(e.x - step * gsum.x, e.y - step * gsum.y, e.z - step * gsum.z, e.w - step * gsum.w);
  const float norm = sqrtf(group_sum(y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w, G));
  if (!(norm < kBallEdge)) {
    const float back = kBallEdge / norm;
    y = make_float4(y.x * back, y.y * back, y.z * back, y.w * back);
  }
  if (!mine) return;
  float* pe = emb + static_cast<size_t>(node) * ld;
  if (d == 2) *reinterpret_cast<float2*>(pe) = make_float2(y.x, y.y);
  else st4(pe + 4 * li, y);
}

// the limits of the step; returns nullptr when the shape is supported, else the message
const char* step_shape(int L, int C, int d, StepShape* sh) {
  if (L < 1 || L > kMaxWalkLength) return "walk_length outside 1 .. 127";
  if (C < 2 || C > L) return "context_size outside 2 .. walk_length";
  if (d != 2 && (d < 4 || d > kMaxDim || d % 4 != 0)) return "the embedding width must be 2 or a multiple of 4 in 4 .. 128";
  sh->L = L; sh->C = C; sh->d = d;
  sh->dp = d < 4 ? 4 : d;
  sh->d4 = sh->dp / 4;
  sh->J = L + 2 - C;
  sh->P = sh->J * (C - 1);
  int G = 1;
  while (G < sh->d4) G <<= 1;
  sh->G = G;
  sh->pairs_at = (L + 1) * sh->dp + (L + 1 + 3) / 4 * 4;
  sh->lds_floats = sh->pairs_at + 2 * ((sh->P + 3) / 4 * 4);
  if (sh->lds_floats > kLdsFloats)
    return "(walk_length + 1) * width + the walk_length + 1 norms + 2 * windows * (context_size - 1) exceeds 16384 floats (64 KiB of LDS)";
  sh->waves = kLdsFloats / sh->lds_floats;
  if (sh->waves > kWavesPerBlock) sh->waves = kWavesPerBlock;
  return nullptr;
}

int step_args(const char* who, int64_t r_pos, int64_t r_neg, int32_t L, int32_t C, int32_t d, StepShape* sh) {
  const char* why = step_shape(L, C, d, sh);
  GNPDE_CHECK_ARG(why == nullptr, GNPDE_ESHAPE, "%s: %s (walk_length %d, context_size %d, width %d)", who, why, L, C, d);
  GNPDE_CHECK_ARG(r_pos >= 1 && r_neg >= 1, GNPDE_EINVAL, "%s: at least one positive and one negative walk are needed", who);
  GNPDE_CHECK_ARG((r_pos + r_neg) * static_cast<int64_t>(L + 1) <= INT32_MAX, GNPDE_ESHAPE, "%s: more than INT32_MAX walk positions in one step", who);
  return 0;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_poincare_step_workspace_bytes(int64_t r_pos, int64_t r_neg, int32_t walk_length, int32_t context_size, int32_t d) {
  StepShape sh;
  if (step_args("poincare_step_workspace_bytes", r_pos, r_neg, walk_length, context_size, d, &sh) != 0) return 0;
  return step_layout(r_pos + r_neg, walk_length, sh.dp).total;
}

extern "C" int gnpde_poincare_step(float* emb, int32_t ld, int32_t n, int32_t d, const int32_t* pos_rw, int64_t r_pos, const int32_t* neg_rw,
                                   int64_t r_neg, int32_t walk_length, int32_t context_size, float lr, float radius, float temperature,
                                   float* loss_out, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream) {
  StepShape sh;
  const int rc = step_args("poincare_step", r_pos, r_neg, walk_length, context_size, d, &sh);
  if (rc != 0) return rc;
  GNPDE_CHECK_ARG(emb && pos_rw && neg_rw && loss_out && flag && n >= 1, GNPDE_EINVAL, "poincare_step: bad arguments (null pointer or n < 1)");
  const int quantum = d == 2 ? 2 : 4;                                    // floats per vector access of a row
  GNPDE_CHECK_ARG(ld >= d && ld % quantum == 0 && reinterpret_cast<uintptr_t>(emb) % (4 * quantum) == 0, GNPDE_EINVAL,
                  "poincare_step: the row stride %d must be a multiple of %d and at least the width %d, and emb %d-byte aligned", ld, quantum, d,
                  4 * quantum);
  GNPDE_CHECK_ARG(lr >= 0.0f && temperature > 0.0f && std::isfinite(lr) && std::isfinite(radius) && std::isfinite(temperature), GNPDE_EINVAL,
                  "poincare_step: finite lr >= 0, radius and temperature > 0 are required");
  const long long r_tot = r_pos + r_neg;
  const StepLayout Y = step_layout(r_tot, walk_length, sh.dp);
  GNPDE_CHECK_ARG(Y.total != 0, GNPDE_ESTATE, "poincare_step: the sort's temporary-storage query failed");
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= Y.total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "poincare_step: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, Y.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  u64* keys = reinterpret_cast<u64*>(ws + Y.keys);
  u64* sorted = reinterpret_cast<u64*>(ws + Y.sorted);
  float* contrib = reinterpret_cast<float*>(ws + Y.contrib);
  double* partial = reinterpret_cast<double*>(ws + Y.partial);
  const long long S = r_tot * (walk_length + 1);
  const double mean_pos = 1.0 / (static_cast<double>(r_pos) * sh.P), mean_neg = 1.0 / (static_cast<double>(r_neg) * sh.P);
  const unsigned blocks = static_cast<unsigned>((r_tot + sh.waves - 1) / sh.waves);
  hipLaunchKernelGGL(pair_kernel, dim3(blocks), dim3(sh.waves * kWave), static_cast<size_t>(sh.waves) * sh.lds_floats * sizeof(float), s, emb, ld,
                     static_cast<unsigned>(n), pos_rw, static_cast<long long>(r_pos), neg_rw, static_cast<long long>(r_neg), sh, radius,
                     temperature, mean_pos, mean_neg, contrib, keys, partial, flag);
  GNPDE_LAUNCH_CHECK();
  size_t tb = Y.temp_bytes;
  GNPDE_HIP(rocprim::radix_sort_keys(ws + Y.temp, tb, keys, sorted, static_cast<size_t>(S), 0, slot_key_bits(n), s));
  const int per = kBlock / sh.G;
  hipLaunchKernelGGL(update_kernel, dim3(static_cast<unsigned>((S + per - 1) / per)), dim3(kBlock), 0, s, sorted, S, contrib, walk_length,
                     context_size, d, sh.dp, sh.d4, sh.G, emb, ld, lr);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(kBlock), 0, s, partial, static_cast<long long>(r_pos), static_cast<long long>(r_neg), loss_out);
  GNPDE_LAUNCH_CHECK();
  return 0;
}
