// Edge attention: per-edge multi-head scores -> per-node (row or column) softmax / squareplus ->
// head-mean weights in CSR order (+ the reference's [E,h] outputs in the caller's edge order).
//
// Replaces SpGraphTransAttentionLayer.forward (reference src/function_transformer_attention.py:
// 190-213), SpGraphAttentionLayer.forward (src/function_GAT_attention.py:111-114),
// torch_geometric.utils.softmax [3P] and utils.squareplus (src/utils.py:179-208).  The reference
// materialises q[edge[0]] and k[edge[1]] as two [E,d_k,h] tensors, their product, and runs
// scatter_max / scatter_add (atomics) per head; here a lane owns one (edge, head) pair, gathers its
// d_k-slice of q and k straight from the [N,A] projections (16-byte loads), and the segment
// statistics are wave reductions over the CSR (norm_idx=0) or CSC (norm_idx=1) segment -- no atomics
// except one order-independent max per block for squareplus' global maximum.
//
// General path (any attention_norm_idx, squareplus, [E,h] outputs):
//   Pass 1  scores[p,h]   (CSR order)            edge-parallel, balanced regardless of degree skew
//   Pass 2  seg stats     m[seg,h], den[seg,h]   one wavefront per segment, one block per long segment
//   Pass 3  normalise     w[p] = mean_h att      edge-parallel; optional scatter to edge order
// Fused path (the solver's hot case: softmax over the ROW, only the head-mean weights wanted):
//   one launch; a 16-lane group (rows with <= 16 entries, 4 rows per wavefront) or a whole wavefront
//   (<= GNPDE_LONG_ROW entries) owns a row, lanes own edges, the h scores of up to 8 passes stay in
//   registers, max / sum are DPP-style xor reductions inside the group, w is written once.  Long
//   rows run the general passes restricted to their chunks.
#include <cmath>
#include <type_traits>
#include "common.h"
#include "rhs.h"

namespace gnpde {
namespace {

constexpr int kGmaxSlots = 64;
constexpr int kGmaxPartCap = 8192;      // waves of a "small" squareplus maximum sweep (AttArgs::gmax_part)

struct AttArgs {
  int n, e, h, dk, type, norm_idx, square_plus;
  float inv_sqrt_dk_den;  // sqrt(d_k), divisor of the scaled dot product
  float scale_mul;        // fl32(1 / sqrt(d_k)): the row kernels multiply (exactly the quotient when sqrt(d_k) is a power of two: d_k = 4, 16, 64; within 1 ulp of it otherwise)
  float leaky_slope;
  const int* __restrict__ rowidx;
  const int* __restrict__ colidx;
  const int* __restrict__ perm;
  const int* __restrict__ segptr;   // rowptr or cscptr
  const int* __restrict__ segpos;   // nullptr (rows: positions are contiguous) or cscpos
  const float* __restrict__ q;
  const float* __restrict__ k;
  int ldqk;
  const float* __restrict__ gat_terms;  // [n, 2h]: src terms then dst terms
  const float* __restrict__ output_var;
  const float* __restrict__ lengthscale;
  const float* __restrict__ edge_w;
  float* scores;      // [e,h]
  float* seg_m;       // [n,h]
  float* seg_den;     // [n,h]
  unsigned* gmax;     // ordered-uint encoding of the global max score
  unsigned* gmax_slots;   // squareplus maximum sweep of the fused path: kGmaxSlots partial maxima, 128 bytes apart (a block updates slot
                          // blockIdx % kGmaxSlots; gmax_fold_kernel folds them into *gmax).  A small graph's whole grid is resident at once,
                          // so every wave sees the initial value and issues its atomic: on ONE address they serialise at ~10 ns each --
                          // 24-36 us of a 48-us Cora evaluation (profiles/r05_c2_as_run_sequence_before.txt).  nullptr: straight into *gmax.
  float* w_mean;      // [e] or null
  float* att_edge;    // [E,h] or null
  float* prods_edge;  // [E,h] or null
  // when non-null the edge-parallel passes work on these CSR ranges only (one block per chunk)
  const int* __restrict__ chunk_begin;
  const int* __restrict__ chunk_end;
  // long segments handled by seg_stats_long_kernel (segment ids); others by the wave-per-segment kernel
  const int* __restrict__ long_segs;
  const int* __restrict__ rowptr;
  const int* __restrict__ bin_rows;
  int hub_fold_lds;   // default on; gnpde_tune(11, 2) folds straight from memory: see hub_normalise_body
  // fused scaled-dot segment kernels beyond the plain row softmax (row_attention_sd_kernel and its hub phases):
  const int* __restrict__ out_pos;   // nullptr, or position e of the walked graph -> position of the weight in w_mean (the walked graph
                                     // is the TRANSPOSED one when the normalisation runs over columns)
  int sp_mode;                       // 0 softmax; 1 squareplus with the global maximum in *gmax; 2 only form that maximum
  // squareplus on a SMALL grid (at most kGmaxPartCap waves in the maximum sweep, no hub rows): every wave of the sweep stores its
  // maximum in gmax_part[gmax_base + wave] (no atomic, nothing to clear beforehand) and every block of the second sweep folds the
  // gmax_count entries itself (block 0 also publishes *gmax for the kernels behind) -- no memset node and no fold launch, two of
  // the eight launches of such an evaluation (Cora as run_GNN.py runs it: ~4.5 us each)
  unsigned* gmax_part;
  int gmax_base, gmax_count;
};

__device__ __forceinline__ unsigned f2ord(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o) {
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

// the partial maxima of the squareplus sweep (AttArgs::gmax_slots) -> *gmax; one wavefront
__global__ __launch_bounds__(kWave) void gmax_fold_kernel(const unsigned* __restrict__ slots, unsigned* __restrict__ gmax) {
  unsigned v = slots[32 * static_cast<int>(threadIdx.x)];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned w = static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, kWave));
    v = w > v ? w : v;
  }
  if (threadIdx.x == 0 && v > *gmax) *gmax = v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// ---- pass 0 (GAT): per-node terms  src[i,h] = sum_c a[c] h_i[c,head],  dst[i,h] = sum_c a[d_k+c] h_i[c,head]
// `table` (optional, [n, 8h]): the same terms as 4-wide query / key vectors for the scaled-dot row kernels --
//   q_i[head] = (2 src, 2, 0, 0),  k_j[head] = (1, dst, 0, 0):  q . k / sqrt(4) = src_i + dst_j  (bit for bit: 2 src and 2 dst are
//   exact, their sum is rounded once, halving is exact), so GAT's row softmax rides row_attention_sd_kernel (MODE 3: leaky ReLU on the
//   score) instead of the generic row kernel + separate hub launches: 103 -> 47 us of attention per evaluation at the ogbn-arxiv shape
__global__ __launch_bounds__(kBlock) void gat_terms_kernel(const float* __restrict__ wx, int ld, const float* __restrict__ a,
                                                          int n, int h, int dk, float* __restrict__ terms, float* __restrict__ table) {
  const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<long long>(n) * h) return;
  const int i = static_cast<int>(idx / h), head = static_cast<int>(idx % h);
  const float* row = wx + static_cast<size_t>(i) * ld + head * dk;
  float s = 0.f, t = 0.f;
  for (int c = 0; c < dk; ++c) {
    const float v = row[c];
    s = fmaf(a[c], v, s);
    t = fmaf(a[dk + c], v, t);
  }
  terms[static_cast<size_t>(i) * 2 * h + head] = s;
  terms[static_cast<size_t>(i) * 2 * h + h + head] = t;
  if (table != nullptr) {
    float* row = table + static_cast<size_t>(i) * 8 * h;
    *reinterpret_cast<float4*>(row + 4 * head) = make_float4(2.0f * s, 2.0f, 0.f, 0.f);
    *reinterpret_cast<float4*>(row + 4 * h + 4 * head) = make_float4(1.0f, t, 0.f, 0.f);
  }
}

// score of one (edge, head): q-slice of the row node against k-slice of the column node
template <int TYPE, bool VEC4>
__device__ __forceinline__ float edge_score(const AttArgs& a, int p, int r, int c, int head) {
  float s;
  if constexpr (TYPE == GNPDE_ATT_GAT) {
    const float v = a.gat_terms[static_cast<size_t>(r) * 2 * a.h + head] +
                    a.gat_terms[static_cast<size_t>(c) * 2 * a.h + a.h + head];
    s = v > 0.f ? v : v * a.leaky_slope;
  } else {
    const float* qp = a.q + static_cast<size_t>(r) * a.ldqk + head * a.dk;
    const float* kp = a.k + static_cast<size_t>(c) * a.ldqk + head * a.dk;
    float mq = 0.f, mk = 0.f;
    if constexpr (TYPE == GNPDE_ATT_PEARSON) {
      for (int j = 0; j < a.dk; ++j) { mq += qp[j]; mk += kp[j]; }
      mq = mq / static_cast<float>(a.dk);
      mk = mk / static_cast<float>(a.dk);
    }
    float dot = 0.f, nq = 0.f, nk = 0.f;
    auto term = [&](float qv, float kv) {
      if constexpr (TYPE == GNPDE_ATT_SCALED_DOT) {
        dot = fmaf(qv, kv, dot);
      } else if constexpr (TYPE == GNPDE_ATT_EXP_KERNEL) {
        const float df = qv - kv;
        dot = fmaf(df, df, dot);
      } else {
        qv -= mq; kv -= mk;
        dot = fmaf(qv, kv, dot);
        nq = fmaf(qv, qv, nq);
        nk = fmaf(kv, kv, nk);
      }
    };
    if constexpr (VEC4) {
      for (int j = 0; j < a.dk; j += 4) {
        const float4 qv = *reinterpret_cast<const float4*>(qp + j);
        const float4 kv = *reinterpret_cast<const float4*>(kp + j);
        term(qv.x, kv.x); term(qv.y, kv.y); term(qv.z, kv.z); term(qv.w, kv.w);
      }
    } else {
      for (int j = 0; j < a.dk; ++j) term(qp[j], kp[j]);
    }
    if constexpr (TYPE == GNPDE_ATT_SCALED_DOT) {
      s = dot * a.scale_mul;      // fl32(1 / sqrt(d_k)): exactly the quotient for d_k = 4, 16, 64, within 1 ulp otherwise
    } else if constexpr (TYPE == GNPDE_ATT_EXP_KERNEL) {
      const float ov = *a.output_var, ls = *a.lengthscale;
      s = (ov * ov) * expf(-(dot / (2.0f * (ls * ls))));
    } else {
      // cosine / pearson: x1.x2 / (max(|x1|, eps) max(|x2|, eps)), eps = 1e-5 -- EACH norm clamped, torch >= 1.12's cosine_similarity (the
      // torch the golden vectors were recorded with) and what the per-vector normalisation of the fused path expresses (misc.hip
      // normalise_heads_kernel), so that the layer's [E,h] attention and ODEFunc.forward agree for degenerate rows too.  torch 1.8 (the
      // reference's pin) clamps the PRODUCT at eps instead: the two differ only when |x1| |x2| < 1e-5 or one norm alone is below 1e-5
      // (tests/test_properties_cpu.py::test_cosine_clamp_against_torch_1_8_product_clamp).  Until round 5 this kernel
      // used the product clamp and disagreed with the fused path by up to 1e-3 on such rows.
      s = dot / (fmaxf(sqrtf(nq), 1e-5f) * fmaxf(sqrtf(nk), 1e-5f));
    }
  }
  if (a.edge_w != nullptr) s = s * a.edge_w[p];
  return s;
}

// ---- pass 1: one lane per (CSR position, head); over all edges (grid-stride) or one block per chunk
template <int TYPE, bool VEC4>
__global__ __launch_bounds__(kBlock) void scores_kernel(const AttArgs a) {
  long long first, total, stride;
  if (a.chunk_begin != nullptr) {
    first = static_cast<long long>(a.chunk_begin[blockIdx.x]) * a.h + threadIdx.x;
    total = static_cast<long long>(a.chunk_end[blockIdx.x]) * a.h;
    stride = blockDim.x;
  } else {
    first = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    total = static_cast<long long>(a.e) * a.h;
    stride = static_cast<long long>(gridDim.x) * blockDim.x;
  }
  float lmax = -INFINITY;
  for (long long idx = first; idx < total; idx += stride) {
    const int p = static_cast<int>(idx / a.h);
    const int head = static_cast<int>(idx - static_cast<long long>(p) * a.h);
    const float s = edge_score<TYPE, VEC4>(a, p, a.rowidx[p], a.colidx[p], head);
    a.scores[idx] = s;
    lmax = fmaxf(lmax, s);
  }
  if (a.square_plus) {  // block max -> one order-independent atomic
    __shared__ float smax[kWavesPerBlock];
    lmax = wave_max(lmax);
    if ((threadIdx.x & (kWave - 1)) == 0) smax[threadIdx.x >> 6] = lmax;
    __syncthreads();
    if (threadIdx.x == 0) {
      float m = smax[0];
      for (int i = 1; i < kWavesPerBlock; ++i) m = fmaxf(m, smax[i]);
      atomicMax(a.gmax, f2ord(m));
    }
  }
}

__device__ __forceinline__ float squareplus_num(float s, float gmax) {
  const float z = s - gmax;
  return (z + sqrtf(z * z + 4.0f)) / 2.0f;
}
// the same with v_sqrt_f32 (1 ulp) and an exact halving: the fused row kernel is bound by VALU issue, and the IEEE square root is a
// dozen instructions per (entry, head)
__device__ __forceinline__ float squareplus_num_fast(float s, float gmax) {
  const float z = s - gmax;
  return (z + __builtin_amdgcn_sqrtf(fmaf(z, z, 4.0f))) * 0.5f;
}

// ---- pass 2: one wavefront per segment (heads in an outer loop); segments longer than GNPDE_LONG_ROW
// are left to seg_stats_long_kernel so that a hub does not serialise on one wave
__device__ __forceinline__ float stat_term(const AttArgs& a, int t, int head, float gmax, float m) {
  const int p = a.segpos ? a.segpos[t] : t;
  const float s = a.scores[static_cast<size_t>(p) * a.h + head];
  if (a.square_plus) return squareplus_num(s, gmax);
  return expf(s - m);
}

__global__ __launch_bounds__(kBlock) void seg_stats_kernel(const AttArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int seg = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6));
  if (seg >= a.n) return;
  const int b = a.segptr[seg], e = a.segptr[seg + 1];
  if (e - b > GNPDE_LONG_ROW && a.long_segs != nullptr) return;
  const float gmax = a.square_plus ? ord2f(*a.gmax) : 0.f;
  for (int head = 0; head < a.h; ++head) {
    float m = 0.f;
    if (!a.square_plus) {
      float mx = -INFINITY;
      for (int t = b + lane; t < e; t += kWave) {
        const int p = a.segpos ? a.segpos[t] : t;
        mx = fmaxf(mx, a.scores[static_cast<size_t>(p) * a.h + head]);
      }
      mx = wave_max(mx);
      m = (e > b) ? mx : 0.f;
    }
    float sum = 0.f;
    for (int t = b + lane; t < e; t += kWave) sum += stat_term(a, t, head, gmax, m);
    const float den = wave_sum(sum) + 1e-16f;
    if (lane == 0) {
      a.seg_m[static_cast<size_t>(seg) * a.h + head] = m;
      a.seg_den[static_cast<size_t>(seg) * a.h + head] = den;
    }
  }
}

// Head-parallel variant for h in {1,2,4,8}: lane = (entry slot, head) with the head fastest, so the h scores of
// an entry are one contiguous 4h-byte read (instead of h strided passes over the segment) and both sweeps
// cover all heads at once.  Reductions over the entry slots are xor butterflies with stride H.
template <int H>
__global__ __launch_bounds__(kBlock) void seg_stats_heads_kernel(const AttArgs a) {
  constexpr int ES = kWave / H;  // entries per wave pass
  const int lane = threadIdx.x & (kWave - 1);
  const int seg = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6));
  if (seg >= a.n) return;
  const int b = a.segptr[seg], e = a.segptr[seg + 1];
  if (e - b > GNPDE_LONG_ROW && a.long_segs != nullptr) return;
  const int es = lane / H, head = lane % H;
  const float gmax = a.square_plus ? ord2f(*a.gmax) : 0.f;
  float m = 0.f;
  if (!a.square_plus) {
    float mx = -INFINITY;
    for (int t = b + es; t < e; t += ES) {
      const int p = a.segpos ? a.segpos[t] : t;
      mx = fmaxf(mx, a.scores[static_cast<size_t>(p) * H + head]);
    }
#pragma unroll
    for (int off = H; off < kWave; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
    m = (e > b) ? mx : 0.f;
  }
  float sum = 0.f;
  for (int t = b + es; t < e; t += ES) {
    const int p = a.segpos ? a.segpos[t] : t;
    const float sv = a.scores[static_cast<size_t>(p) * H + head];
    sum += a.square_plus ? squareplus_num(sv, gmax) : expf(sv - m);
  }
#pragma unroll
  for (int off = H; off < kWave; off <<= 1) sum += __shfl_xor(sum, off, kWave);
  if (es == 0) {
    a.seg_m[static_cast<size_t>(seg) * H + head] = m;
    a.seg_den[static_cast<size_t>(seg) * H + head] = sum + 1e-16f;
  }
}

// Long segments: blockIdx.x = long segment, blockIdx.y = 512-entry chunk of it.  Every chunk leaves an
// online-softmax partial (m_c, l_c) per head (squareplus: just the partial sum); seg_stats_long_combine
// folds them:  m = max_c m_c,  den = sum_c l_c exp(m_c - m) + 1e-16.
__global__ __launch_bounds__(kBlock) void seg_stats_long_partial_kernel(const AttArgs a, float* __restrict__ part, int max_chunks) {
  __shared__ float red[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int seg = a.long_segs[blockIdx.x];
  const int b = a.segptr[seg] + static_cast<int>(blockIdx.y) * GNPDE_LONG_ROW;
  const int e = min(a.segptr[seg + 1], b + GNPDE_LONG_ROW);
  if (b >= a.segptr[seg + 1]) return;
  const float gmax = a.square_plus ? ord2f(*a.gmax) : 0.f;
  float* out = part + (static_cast<size_t>(blockIdx.x) * max_chunks + blockIdx.y) * 2 * a.h;
  for (int head = 0; head < a.h; ++head) {
    float m = 0.f;
    if (!a.square_plus) {
      float mx = -INFINITY;
      for (int t = b + threadIdx.x; t < e; t += kBlock) {
        const int p = a.segpos ? a.segpos[t] : t;
        mx = fmaxf(mx, a.scores[static_cast<size_t>(p) * a.h + head]);
      }
      mx = wave_max(mx);
      if (lane == 0) red[wave] = mx;
      __syncthreads();
      m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
      __syncthreads();
    }
    float sum = 0.f;
    for (int t = b + threadIdx.x; t < e; t += kBlock) sum += stat_term(a, t, head, gmax, m);
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      out[head] = m;
      out[a.h + head] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kWave) void seg_stats_long_combine_kernel(const AttArgs a, const float* __restrict__ part,
                                                                      int max_chunks) {
  const int seg = a.long_segs[blockIdx.x];
  const int len = a.segptr[seg + 1] - a.segptr[seg];
  const int nch = (len + GNPDE_LONG_ROW - 1) / GNPDE_LONG_ROW;
  const float* base = part + static_cast<size_t>(blockIdx.x) * max_chunks * 2 * a.h;
  for (int head = threadIdx.x; head < a.h; head += blockDim.x) {
    float m = -INFINITY;
    if (a.square_plus) m = 0.f;
    else
      for (int c = 0; c < nch; ++c) m = fmaxf(m, base[static_cast<size_t>(c) * 2 * a.h + head]);
    float l = 0.f;
    for (int c = 0; c < nch; ++c) {
      const float lc = base[static_cast<size_t>(c) * 2 * a.h + a.h + head];
      l += a.square_plus ? lc : lc * expf(base[static_cast<size_t>(c) * 2 * a.h + head] - m);
    }
    a.seg_m[static_cast<size_t>(seg) * a.h + head] = m;
    a.seg_den[static_cast<size_t>(seg) * a.h + head] = l + 1e-16f;
  }
}

// ---- pass 3: one lane per CSR position, heads serial (same order as attention.mean(dim=1))
__global__ __launch_bounds__(kBlock) void normalise_kernel(const AttArgs a) {
  long long first, last, stride;
  if (a.chunk_begin != nullptr) {
    first = static_cast<long long>(a.chunk_begin[blockIdx.x]) + threadIdx.x;
    last = a.chunk_end[blockIdx.x];
    stride = blockDim.x;
  } else {
    first = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    last = a.e;
    stride = static_cast<long long>(gridDim.x) * blockDim.x;
  }
  const float gmax = a.square_plus ? ord2f(*a.gmax) : 0.f;
  for (long long p = first; p < last; p += stride) {
    const int seg = a.norm_idx == 0 ? a.rowidx[p] : a.colidx[p];
    const long long dst = (a.att_edge || a.prods_edge) ? static_cast<long long>(a.perm[p]) * a.h : 0;
    float acc = 0.f;
    for (int head = 0; head < a.h; ++head) {
      const float s = a.scores[p * a.h + head];
      const float den = a.seg_den[static_cast<size_t>(seg) * a.h + head];
      float v;
      if (a.square_plus) v = squareplus_num(s, gmax) / den;
      else v = expf(s - a.seg_m[static_cast<size_t>(seg) * a.h + head]) / den;
      acc += v;
      if (a.att_edge) a.att_edge[dst + head] = v;
      if (a.prods_edge) a.prods_edge[dst + head] = s;
    }
    if (a.w_mean) a.w_mean[p] = acc / static_cast<float>(a.h);
  }
}

// ---- hub rows of the fused path (softmax over the row, head-mean weights only), two launches:
// (a) one block per 512-entry chunk: scores -> scratch, chunk maximum and sum of exponentials per head
// (b) one block per chunk: fold the row's chunk partials (<= max_chunks of them) and write the weights
template <int TYPE, bool VEC4>
__device__ __forceinline__ void hub_scores_partial_body(const AttArgs& a, float* __restrict__ part, int chunk) {
  __shared__ float red[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int b = a.chunk_begin[chunk], e = a.chunk_end[chunk];
  const int row = a.rowidx[b];
  float* out = part + static_cast<size_t>(chunk) * 2 * a.h;
  for (int head = 0; head < a.h; ++head) {
    float sv[GNPDE_LONG_ROW / kBlock];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < GNPDE_LONG_ROW / kBlock; ++i) {
      const int p = b + i * kBlock + threadIdx.x;
      sv[i] = -INFINITY;
      if (p < e) {
        sv[i] = edge_score<TYPE, VEC4>(a, p, row, a.colidx[p], head);
        a.scores[static_cast<size_t>(p) * a.h + head] = sv[i];
        mx = fmaxf(mx, sv[i]);
      }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < GNPDE_LONG_ROW / kBlock; ++i) sum += expf(sv[i] - m);
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      out[head] = m;
      out[a.h + head] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    __syncthreads();
  }
}

// Head-parallel form for H in {1,2,4,8} (the hot case): lane = (entry, head) with the head fastest, so the H lanes of an entry
// read ONE contiguous A-float row of k (round 1 looped over the heads and gathered every k row H times, 64 B at a time: 6.9 ms
// for the 99.5 k hub chunks of the R-MAT graph); the scores of the PER passes stay in registers, the per-head maximum / sum
// are xor butterflies over the lanes with equal head and a fold over the four waves in LDS.
template <int TYPE, bool VEC4, int H, int MODE = 0>
__device__ __forceinline__ void hub_scores_partial_heads(const AttArgs& a, float* __restrict__ part, int chunk) {
  constexpr int EPB = kBlock / H;                 // entries per block pass
  constexpr int PER = GNPDE_LONG_ROW / EPB;       // passes
  __shared__ float red[kWavesPerBlock][H];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int head = threadIdx.x % H, slot = threadIdx.x / H;
  const int b = a.chunk_begin[chunk], e = a.chunk_end[chunk];
  const int row = a.rowidx[b];
  float* out = part + static_cast<size_t>(chunk) * 2 * H;
  int cols[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {                 // all column ids first, then all k gathers
    const int p = b + i * EPB + slot;
    cols[i] = p < e ? a.colidx[p] : -1;
  }
  float sv[PER];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int p = b + i * EPB + slot;
    sv[i] = -INFINITY;
    if (cols[i] >= 0) {
      sv[i] = edge_score<TYPE, VEC4>(a, p, row, cols[i], head);
      if constexpr (MODE == 3) sv[i] = sv[i] > 0.f ? sv[i] : sv[i] * a.leaky_slope;
      a.scores[static_cast<size_t>(p) * H + head] = sv[i];
      mx = fmaxf(mx, sv[i]);
    }
  }
#pragma unroll
  for (int off = H; off < kWave; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, kWave));
  if (lane < H) red[wave][lane] = mx;
  __syncthreads();
  const float m = fmaxf(fmaxf(red[0][head], red[1][head]), fmaxf(red[2][head], red[3][head]));
  __syncthreads();
  if constexpr (MODE == 2) {     // squareplus, first sweep: only the global maximum of the scores (utils.py:196 `src.max()`)
    if (threadIdx.x < H && m > -INFINITY) {
      const unsigned mine = f2ord(m);
      unsigned* tgt = a.gmax_slots != nullptr ? a.gmax_slots + 32 * (blockIdx.x % kGmaxSlots) : a.gmax;
      if (mine > __hip_atomic_load(tgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(tgt, mine);
    }
    return;
  }
  float sum = 0.f;
  if constexpr (MODE == 1) {     // squareplus: the chunk's share of the segment sum of u = (z + sqrt(z^2 + 4)) / 2, z = s - max
    const float gm = ord2f(*a.gmax);
#pragma unroll
    for (int i = 0; i < PER; ++i) sum += cols[i] >= 0 ? squareplus_num(sv[i], gm) : 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < PER; ++i) sum += __builtin_amdgcn_exp2f((sv[i] - m) * 1.44269504088896341f);   // v_exp_f32; exp(-inf) = 0 for the absent entries
  }
#pragma unroll
  for (int off = H; off < kWave; off <<= 1) sum += __shfl_xor(sum, off, kWave);
  if (lane < H) red[wave][lane] = sum;
  __syncthreads();
  if (threadIdx.x < H) {
    out[threadIdx.x] = m;
    out[H + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
  }
}

template <int TYPE, bool VEC4>
__global__ __launch_bounds__(kBlock) void hub_scores_partial_kernel(const AttArgs a, float* __restrict__ part) {
  hub_scores_partial_body<TYPE, VEC4>(a, part, blockIdx.x);
}

template <int MODE = 0, bool SCATTER = false>
__device__ __forceinline__ void hub_normalise_body(const AttArgs& a, const float* __restrict__ part,
                                                   const int* __restrict__ long_chunk_row_first, int c) {
  // long_chunk_row_first[c] = index of the first chunk of the row chunk c belongs to
  __shared__ float st[2 * 64];  // [2h]: row maximum and denominator per head
  constexpr int kStage = 2048;  // floats of chunk partials staged through LDS (a row of up to 2048 / 2h chunks)
  __shared__ float sp_[kStage];
  const int b = a.chunk_begin[c], e = a.chunk_end[c];
  const int row = a.rowidx[b];
  const int c0 = long_chunk_row_first[c];
  const int nch = (a.rowptr[row + 1] - a.rowptr[row] + GNPDE_LONG_ROW - 1) / GNPDE_LONG_ROW;
  // The fold below is a chain of 2 nch DEPENDENT-latency loads issued by h threads (the compiler keeps two in flight): 22
  // chunks of the largest hub of the ogbn-arxiv shape = ~20 round trips before any of the block's 512 weights can be written,
  // repeated by every chunk block of the row.  Staged form (the default; measured round 3, profiles/r03_v0_blind_changes_measured.txt: equal at the ogbn-arxiv shape,
  // 4.85 -> 4.68 ms per attention at the R-MAT shape; gnpde_tune(11, 2) selects the fold from memory): the whole
  // block fetches the row's partials in ONE round trip into LDS and the h folding threads read them from there -- the same
  // values combined in the same order, so the weights are bit-identical.
  const int nval = nch * 2 * a.h;                   // block-uniform
  const bool staged = a.hub_fold_lds != 0 && nval <= kStage;
  if (staged) {
    const float* src = part + static_cast<size_t>(c0) * 2 * a.h;
    for (int t = threadIdx.x; t < nval; t += kBlock) sp_[t] = src[t];
    __syncthreads();
  }
  constexpr bool sp = MODE == 1;
  if (threadIdx.x < a.h && sp) {       // squareplus: the statistics are plain sums of the chunks' shares
    const int head = threadIdx.x;
    float l = 0.f;
    for (int i = 0; i < nch; ++i) l += staged ? sp_[i * 2 * a.h + a.h + head] : part[static_cast<size_t>(c0 + i) * 2 * a.h + a.h + head];
    st[head] = ord2f(*a.gmax);
    st[a.h + head] = __builtin_amdgcn_rcpf(l + 1e-16f);
  } else if (threadIdx.x < a.h) {
    const int head = threadIdx.x;
    float m = -INFINITY;
    float l = 0.f;
    if (staged) {
      for (int i = 0; i < nch; ++i) m = fmaxf(m, sp_[i * 2 * a.h + head]);
      for (int i = 0; i < nch; ++i) {
        const float* q = sp_ + i * 2 * a.h;
        l += q[a.h + head] * expf(q[head] - m);
      }
    } else {
      for (int i = 0; i < nch; ++i) m = fmaxf(m, part[static_cast<size_t>(c0 + i) * 2 * a.h + head]);
      for (int i = 0; i < nch; ++i) {
        const float* q = part + static_cast<size_t>(c0 + i) * 2 * a.h;
        l += q[a.h + head] * expf(q[head] - m);
      }
    }
    st[head] = m;
    st[a.h + head] = __builtin_amdgcn_rcpf(l + 1e-16f);     // one reciprocal per (row, head), a multiplication per entry
  }
  __syncthreads();
  for (int p = b + threadIdx.x; p < e; p += kBlock) {
    float acc = 0.f;
    if (sp) {
      for (int head = 0; head < a.h; ++head) acc += squareplus_num(a.scores[static_cast<size_t>(p) * a.h + head], st[head]) * st[a.h + head];
    } else {
      for (int head = 0; head < a.h; ++head)
        acc += __builtin_amdgcn_exp2f((a.scores[static_cast<size_t>(p) * a.h + head] - st[head]) * 1.44269504088896341f) * st[a.h + head];
    }
    if constexpr (SCATTER) a.w_mean[a.out_pos[p]] = acc / static_cast<float>(a.h);
    else a.w_mean[p] = acc / static_cast<float>(a.h);
  }
}

__global__ __launch_bounds__(kBlock) void hub_normalise_kernel(const AttArgs a, const float* __restrict__ part,
                                                              const int* __restrict__ long_chunk_row_first) {
  hub_normalise_body<0, false>(a, part, long_chunk_row_first, blockIdx.x);
}

// ---- fused path: softmax over the row, head-mean weights only.
// GL lanes own one row; inside a group lane = (edge slot, head) with the head fastest, so the H lanes
// of an edge read one contiguous A-float row of k (one 16-byte load each when d_k = 4) and a pass covers
// GE = GL / H edges.  Scores of up to P passes stay in registers (one float per pass per lane).
template <int TYPE, int H, int GL, int P, bool VEC4>
__global__ __launch_bounds__(kBlock) void row_attention_kernel(const AttArgs a, int first_row, int n_rows) {
  constexpr int RPW = kWave / GL;  // rows per wavefront
  constexpr int GE = GL / H;       // edges per pass
  const int lane = threadIdx.x & (kWave - 1);
  const int gi = lane % GL;
  const int slot = gi / H, head = gi % H;
  const long long ridx = (static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6)) * RPW + lane / GL;
  const bool live = ridx < n_rows;
  int4 info = make_int4(0, 0, 0, 0);  // {row, first CSR position, length, -}
  if (live) info = reinterpret_cast<const int4*>(a.bin_rows)[first_row + ridx];
  int row = info.x, e0 = info.y, e1 = info.y + info.z;
  if constexpr (GL == kWave) {
    row = __builtin_amdgcn_readfirstlane(row);
    e0 = __builtin_amdgcn_readfirstlane(e0);
    e1 = __builtin_amdgcn_readfirstlane(e1);
  }
  int npass = P;  // passes that hold any edge (wave-uniform when a wavefront owns one row)
  if constexpr (GL == kWave) npass = (e1 - e0 + GE - 1) / GE;

  float s[P];
  float m = -INFINITY;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    s[p] = -INFINITY;
    if (p < npass) {
      const int e = e0 + p * GE + slot;
      if (e < e1) {
        s[p] = edge_score<TYPE, VEC4>(a, e, row, a.colidx[e], head);
        m = fmaxf(m, s[p]);
      }
    }
  }
#pragma unroll
  for (int off = H; off < GL; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
  float l = 0.f;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (p < npass) {
      s[p] = expf(s[p] - m);  // empty slots: exp(-inf) = 0
      l += s[p];
    }
  }
#pragma unroll
  for (int off = H; off < GL; off <<= 1) l += __shfl_xor(l, off, kWave);
  const float den = l + 1e-16f;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (p < npass) {
      float v = s[p] / den;
#pragma unroll
      for (int off = 1; off < H; off <<= 1) v += __shfl_xor(v, off, kWave);
      const int e = e0 + p * GE + slot;
      if (head == 0 && e < e1) a.w_mean[e] = v / static_cast<float>(H);
    }
  }
}

// ---- scaled-dot specialisation of the fused row kernel with batched gathers.
// The generic kernel above issues, per pass, colidx -> k -> use, i.e. two dependent memory round trips
// that the scheduler cannot overlap across passes (or rows).  Here all index loads of a batch (RI rows x
// PB passes) are issued first, then all k gathers, then the arithmetic -- 2 round trips per BATCH.
// Out-of-range slots read a clamped (valid, cached) position and are masked to -inf afterwards, so the
// batch is branch-free.  d_k = 4 * DK4.
// The first `n_hub` blocks of the launch do the hub-row work instead (phase 0: chunk scores + partial
// statistics, phase 1: fold partials + normalise), so the long rows ride along with the row kernels rather
// than costing two extra serialised launches.
// MODE 0: softmax over the segment.  MODE 1: squareplus with the global maximum already in *a.gmax (utils.py:179-208: u = (z +
// sqrt(z^2 + 4)) / 2 with z = s - max over ALL scores, normalised by the segment sum).  MODE 2: the sweep that forms that maximum
// (scores recomputed, nothing stored).  The segments are the rows of whatever graph a.bin_rows / a.colidx describe -- the
// transposed graph, with a.q / a.k exchanged and a.out_pos mapping its positions to the CSR positions of the weights, when the
// reference normalises over edge[1] (attention_norm_idx = 1, function_transformer_attention.py:210-213).
// The rows of one class (bin_rows[first_row .. first_row + n_rows)); the class's workgroups follow the first `n_hub` of the launch.  The body of
// row_attention_sd_kernel, and of both row classes of row_attention_sd_one_kernel (same code and lane mapping per row: the weights
// are the same bits whichever launch runs it).
template <int H, int DK4, int GL, int RI, int PB, int NB, int MODE, bool SCATTER>
__device__ __forceinline__ void row_attention_sd_rows(const AttArgs& a, int first_row, int n_rows, int n_hub) {
  constexpr int RPW = kWave / GL;
  constexpr int GE = GL / H;
  const int lane = threadIdx.x & (kWave - 1);
  const int gi = lane % GL;
  const int slot = gi / H, head = gi % H;
  const long long rbase = ((static_cast<long long>(blockIdx.x - n_hub) * kWavesPerBlock + (threadIdx.x >> 6)) * RPW + lane / GL) * RI;

  int row[RI], e0[RI], e1[RI];
  bool live[RI];
  // all RI records are requested before the first one is used (round 3: with the load, its wait and the readfirstlane inside
  // one loop body the four record fetches of a wave were four dependent round trips); a slot past the end re-reads the
  // class's last record -- valid addresses, nothing written (live[r])
  int4 info[RI];
#pragma unroll
  for (int r = 0; r < RI; ++r) {
    live[r] = rbase + r < n_rows;
    const long long idx = live[r] ? rbase + r : static_cast<long long>(n_rows) - 1;
    info[r] = reinterpret_cast<const int4*>(a.bin_rows)[first_row + (idx < 0 ? 0 : idx)];
  }
#pragma unroll
  for (int r = 0; r < RI; ++r) {
    row[r] = info[r].x; e0[r] = info[r].y; e1[r] = info[r].y + info[r].z;
    if constexpr (GL == kWave) {
      row[r] = __builtin_amdgcn_readfirstlane(row[r]);
      e0[r] = __builtin_amdgcn_readfirstlane(e0[r]);
      e1[r] = __builtin_amdgcn_readfirstlane(e1[r]);
    }
  }
  float s[RI][NB * PB];
  float m[RI];
#pragma unroll
  for (int r = 0; r < RI; ++r) m[r] = -INFINITY;
  int nbatch = NB;
  if constexpr (GL == kWave && RI == 1) nbatch = (e1[0] - e0[0] + PB * GE - 1) / (PB * GE);  // wave-uniform
  if constexpr (MODE == 1) {
    // squareplus, second sweep: the scores were stored by the maximum sweep (MODE 2) -- one coalesced 4 H-byte read per entry
    // instead of the k-row gather
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i) {
          const int e = e0[r] + (nb * PB + i) * GE + slot;
          s[r][nb * PB + i] = (nb < nbatch && e < e1[r]) ? a.scores[static_cast<size_t>(e) * H + head] : -INFINITY;
        }
  } else {
  float4 qv[RI][DK4];
#pragma unroll
  for (int r = 0; r < RI; ++r)
#pragma unroll
    for (int j = 0; j < DK4; ++j)
      qv[r][j] = *reinterpret_cast<const float4*>(a.q + static_cast<size_t>(row[r]) * a.ldqk + head * a.dk + 4 * j);
  float exp_ov2 = 0.f, exp_den = 1.f;
  if constexpr (MODE == 4) {
    const float ov = *a.output_var, ls = *a.lengthscale;
    exp_ov2 = ov * ov;
    exp_den = 2.0f * (ls * ls);
  }

  // column ids of the batch AFTER the current one are requested before the current batch's k rows are used, so that a row of
  // several batches pays one dependent round trip per batch (k rows), not two (ids -> k rows)
  int cn[RI][PB];
  auto load_ids = [&](int nb) {
#pragma unroll
    for (int r = 0; r < RI; ++r)
#pragma unroll
      for (int i = 0; i < PB; ++i) {
        const int e = e0[r] + (nb * PB + i) * GE + slot;
        cn[r][i] = a.colidx[e < e1[r] ? e : e1[r] - 1];
      }
  };
  load_ids(0);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    if (nb < nbatch) {
      int c[RI][PB];
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i) c[r][i] = cn[r][i];
      if (NB > 1 && nb + 1 < nbatch) load_ids(nb + 1);
      float4 kv[RI][PB][DK4];
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i)
#pragma unroll
          for (int j = 0; j < DK4; ++j)
            kv[r][i][j] = *reinterpret_cast<const float4*>(a.k + static_cast<size_t>(c[r][i]) * a.ldqk + head * a.dk + 4 * j);
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i) {
          float dot = 0.f;
#pragma unroll
          for (int j = 0; j < DK4; ++j) {
            if constexpr (MODE == 4) {   // exp kernel: |q - k|^2, the same chain as edge_score<GNPDE_ATT_EXP_KERNEL>
              float t;
              t = qv[r][j].x - kv[r][i][j].x; dot = fmaf(t, t, dot);
              t = qv[r][j].y - kv[r][i][j].y; dot = fmaf(t, t, dot);
              t = qv[r][j].z - kv[r][i][j].z; dot = fmaf(t, t, dot);
              t = qv[r][j].w - kv[r][i][j].w; dot = fmaf(t, t, dot);
            } else {
              dot = fmaf(qv[r][j].x, kv[r][i][j].x, dot);
              dot = fmaf(qv[r][j].y, kv[r][i][j].y, dot);
              dot = fmaf(qv[r][j].z, kv[r][i][j].z, dot);
              dot = fmaf(qv[r][j].w, kv[r][i][j].w, dot);
            }
          }
          const int e = e0[r] + (nb * PB + i) * GE + slot;
          // (this kernel is bound by VALU issue, not by memory: ~580 wave instructions per 4 rows, a fifth of them the IEEE
          //  division sequences and the full-range expf -- round 3: exact power-of-two scale, one reciprocal per row, v_exp)
          float sv = dot * a.scale_mul;
          if constexpr (MODE == 3) sv = sv > 0.f ? sv : sv * a.leaky_slope;      // GAT: the vectors are gat_terms_kernel's table
          if constexpr (MODE == 4) sv = exp_ov2 * expf(-(dot / exp_den));        // ov^2 exp(-|q - k|^2 / 2 l^2) (reference :193-196)
          if (a.edge_w != nullptr) sv = sv * a.edge_w[e < e1[r] ? e : e1[r] - 1];
          if constexpr (MODE == 2) {
            if (live[r] && e < e1[r]) a.scores[static_cast<size_t>(e) * H + head] = sv;     // kept for the second sweep
          }
          sv = e < e1[r] ? sv : -INFINITY;
          s[r][nb * PB + i] = sv;
          m[r] = fmaxf(m[r], sv);
        }
    } else {
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i) s[r][nb * PB + i] = -INFINITY;
    }
  }
  }   // MODE != 1
  // The reductions run LEVEL by level over all RI rows of the wave, not row by row: every xor step is a dependent LDS round
  // trip (ds_bpermute + wait), and written row by row the 10 steps of a row x RI rows formed one chain of 40 (round 3, from the
  // ISA); level-synchronous there are RI independent exchanges in flight per step.  Same operations per row, same order.
  if constexpr (MODE == 2) {     // only the maximum over every score (slots past the end hold -inf, rows past the end repeat a listed row)
    float mw = m[0];
#pragma unroll
    for (int r = 1; r < RI; ++r) mw = fmaxf(mw, m[r]);
    mw = wave_max(mw);
    // one atomic per wave at most, and only while the wave's maximum beats the value it can see (a stale read only costs an atomic:
    // tens of thousands of waves hammering ONE address serialise -- 0.7 ms per sweep at the ogbn-arxiv shape when every wave did)
    if (a.gmax_part != nullptr) {      // small grid: one plain store per wave (0 = below every encoded float)
      if (lane == 0)
        a.gmax_part[a.gmax_base + (static_cast<int>(blockIdx.x) - n_hub) * kWavesPerBlock + static_cast<int>(threadIdx.x >> 6)] =
            mw > -INFINITY ? f2ord(mw) : 0u;
      return;
    }
    if (lane == 0 && mw > -INFINITY) {
      const unsigned mine = f2ord(mw);
      unsigned* tgt = a.gmax_slots != nullptr ? a.gmax_slots + 32 * (blockIdx.x % kGmaxSlots) : a.gmax;
      if (mine > __hip_atomic_load(tgt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(tgt, mine);
    }
    return;
  }
  float l[RI];
  if constexpr (MODE == 1) {
    float gm;
    if (a.gmax_part != nullptr) {      // (block-uniform) fold the sweep's per-wave maxima: gmax_count / 256 coalesced loads per thread
      __shared__ unsigned s_gmax[kWavesPerBlock];
      unsigned v = 0u;
      for (int i = threadIdx.x; i < a.gmax_count; i += kBlock) {
        const unsigned w = a.gmax_part[i];
        v = w > v ? w : v;
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        const unsigned w = static_cast<unsigned>(__shfl_xor(static_cast<int>(v), o, kWave));
        v = w > v ? w : v;
      }
      if (lane == 0) s_gmax[threadIdx.x >> 6] = v;
      __syncthreads();
      v = s_gmax[0];
#pragma unroll
      for (int w = 1; w < kWavesPerBlock; ++w) v = s_gmax[w] > v ? s_gmax[w] : v;
      if (blockIdx.x == 0 && threadIdx.x == 0 && first_row == 0) *a.gmax = v;     // (for the kernels behind this launch: the backward passes)
      gm = ord2f(v);
    } else {
      gm = ord2f(*a.gmax);
    }
#pragma unroll
    for (int r = 0; r < RI; ++r) {
      l[r] = 0.f;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (nb < nbatch) {
#pragma unroll
          for (int i = 0; i < PB; ++i) {
            const float sv = s[r][nb * PB + i];
            s[r][nb * PB + i] = sv > -INFINITY ? squareplus_num_fast(sv, gm) : 0.f;
            l[r] += s[r][nb * PB + i];
          }
        }
    }
  } else {
#pragma unroll
    for (int off = H; off < GL; off <<= 1)
#pragma unroll
      for (int r = 0; r < RI; ++r) m[r] = fmaxf(m[r], __shfl_xor(m[r], off, kWave));
#pragma unroll
    for (int r = 0; r < RI; ++r) {
      l[r] = 0.f;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        if (nb < nbatch) {
#pragma unroll
          for (int i = 0; i < PB; ++i) {
            s[r][nb * PB + i] = __builtin_amdgcn_exp2f((s[r][nb * PB + i] - m[r]) * 1.44269504088896341f);   // v_exp_f32: arguments are <= 0, -inf -> 0
            l[r] += s[r][nb * PB + i];
          }
        }
    }
  }
#pragma unroll
  for (int off = H; off < GL; off <<= 1)
#pragma unroll
    for (int r = 0; r < RI; ++r) l[r] += __shfl_xor(l[r], off, kWave);
  float rden[RI];
#pragma unroll
  for (int r = 0; r < RI; ++r) rden[r] = __builtin_amdgcn_rcpf(l[r] + 1e-16f);   // v_rcp_f32 (1 ulp), one per (row, head); a multiplication per entry
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
    if (nb < nbatch) {
      float v[RI][PB];
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i) v[r][i] = s[r][nb * PB + i] * rden[r];
#pragma unroll
      for (int off = 1; off < H; off <<= 1)
#pragma unroll
        for (int r = 0; r < RI; ++r)
#pragma unroll
          for (int i = 0; i < PB; ++i) v[r][i] += __shfl_xor(v[r][i], off, kWave);
#pragma unroll
      for (int r = 0; r < RI; ++r)
#pragma unroll
        for (int i = 0; i < PB; ++i) {
          const int e = e0[r] + (nb * PB + i) * GE + slot;
          if (head == 0 && live[r] && e < e1[r]) {
            if constexpr (SCATTER) a.w_mean[a.out_pos[e]] = v[r][i] / static_cast<float>(H);     // (a template switch: the plain row softmax keeps its store as it was)
            else a.w_mean[e] = v[r][i] / static_cast<float>(H);
          }
        }
    }
}

template <int H, int DK4, int GL, int RI, int PB, int NB, int MODE, bool SCATTER>
__global__ __launch_bounds__(kBlock) void row_attention_sd_kernel(const AttArgs a, int first_row, int n_rows, int n_hub,
                                                                 int hub_phase, float* __restrict__ part,
                                                                 const int* __restrict__ chunk_first) {
  if (static_cast<int>(blockIdx.x) < n_hub) {
    if (hub_phase == 0) hub_scores_partial_heads<(MODE == 4 ? GNPDE_ATT_EXP_KERNEL : GNPDE_ATT_SCALED_DOT), true, H, MODE>(a, part, blockIdx.x);
    else hub_normalise_body<MODE, SCATTER>(a, part, chunk_first, blockIdx.x);
    return;
  }
  row_attention_sd_rows<H, DK4, GL, RI, PB, NB, MODE, SCATTER>(a, first_row, n_rows, n_hub);
}

// Row softmax of a whole graph in ONE launch, for an evaluation whose aggregation follows on the same stream: workgroups
// [0, n_hub) score the 512-entry chunks of the hub rows and store their statistics (phase 0, as above), the next blocks64 take the
// rows of 17..512 entries (a wave per row, longest first: bin_rows' order) and the rest the rows of <= 16 entries, which fill the
// tail.  There is no phase 1: the grid-wide dependency between the chunk statistics and the hub entries' weights is carried by
// the kernel boundary in front of the aggregation, whose hub-chunk items fold the statistics and form (and store) those weights
// themselves (spmm.hip, HubDefer).  Two launches of < 20 us each paid two ramps, two tails and a boundary.
template <int H, int DK4, int GL16, int RI16, int P16, int PB64, int NB64>
__global__ __launch_bounds__(kBlock) void row_attention_sd_one_kernel(const AttArgs a, int n16, int n64, int n_hub,
                                                                     float* __restrict__ part) {
  const int b = static_cast<int>(blockIdx.x);
  const int blocks64 = (n64 + kWavesPerBlock - 1) / kWavesPerBlock;
  if (b < n_hub) {
    hub_scores_partial_heads<GNPDE_ATT_SCALED_DOT, true, H, 0>(a, part, b);
    return;
  }
  if (b < n_hub + blocks64) {
    row_attention_sd_rows<H, DK4, kWave, 1, PB64, NB64, 0, false>(a, n16, n64, n_hub);
    return;
  }
  row_attention_sd_rows<H, DK4, GL16, RI16, P16, 1, 0, false>(a, 0, n16, n_hub + blocks64);
}

__global__ __launch_bounds__(kBlock) void edge_to_csr_mean_kernel(const int* __restrict__ perm, const float* __restrict__ src,
                                                                 int h, int e, float* __restrict__ w) {
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long p = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; p < e; p += stride) {
    const float* s = src + static_cast<size_t>(perm[p]) * h;
    if (h == 1) {
      w[p] = s[0];
    } else {
      float acc = 0.f;
      for (int j = 0; j < h; ++j) acc += s[j];
      w[p] = acc / static_cast<float>(h);
    }
  }
}

inline unsigned stream_grid(long long work_items) {
  long long blocks = (work_items + kBlock - 1) / kBlock;
  const long long cap = 256LL * 8;  // 256 CUs x 8 blocks, grid-stride beyond
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return static_cast<unsigned>(blocks);
}

inline size_t long_slots_of(const gnpde_graph_t* g) {
  const size_t rc = static_cast<size_t>(g->n_long_rows) * ((g->max_row_len + GNPDE_LONG_ROW - 1) / GNPDE_LONG_ROW);
  const size_t cc = static_cast<size_t>(g->n_long_cols) * ((g->max_col_len + GNPDE_LONG_ROW - 1) / GNPDE_LONG_ROW);
  const size_t lc = static_cast<size_t>(g->n_long_chunks);
  const size_t m = rc > cc ? rc : cc;
  return m > lc ? m : lc;
}

struct AttLayout {
  size_t scores, seg_m, seg_den, gmax, gat, gat_table, part, total;
};
// `long_slots` = (number of long segments) x (max chunks of one segment), an upper bound is fine
AttLayout att_layout(int n, int e, int h, bool gat, size_t long_slots, int key_rows = 0) {
  AttLayout L{};
  size_t off = 0;
  L.scores = off; off += align_up(static_cast<size_t>(e) * h * 4, 256);
  L.seg_m = off;  off += align_up(static_cast<size_t>(n) * h * 4, 256);
  L.seg_den = off; off += align_up(static_cast<size_t>(n) * h * 4, 256);
  L.gmax = off; off += 256 + (kGmaxSlots * 128 > kGmaxPartCap * 4 ? kGmaxSlots * 128 : kGmaxPartCap * 4);   // the maximum, then its partial slots
                                                                                                             // (AttArgs::gmax_slots / gmax_part)
  L.gat = off; if (gat) off += align_up(static_cast<size_t>(key_rows > n ? key_rows : n) * 2 * h * 4, 256);   // (halo rows of a partitioned graph)
  L.gat_table = off; if (gat) off += align_up(static_cast<size_t>(key_rows > n ? key_rows : n) * 8 * h * 4, 256);
  L.part = off; off += align_up(long_slots * 2 * h * 4, 256);
  L.total = off;
  return L;
}

template <int H>
__global__ __launch_bounds__(kBlock) void hub_scores_partial_sd_kernel(const AttArgs a, float* __restrict__ part) {
  hub_scores_partial_heads<GNPDE_ATT_SCALED_DOT, true, H>(a, part, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Host side.  ONE decision per call -- validation, route, template line of the row kernels, sweeps, grids, hub handling -- taken in
// plan_attention, exported as it is taken by gnpde_attention_plan (gnpde.h documents the table) and carried out by launch_planned.
// ------------------------------------------------------------------------------------------------

// What a call asks of the attention; default-constructed: nothing.
struct AttRequest {
  float* w_mean = nullptr;       // outputs wanted: [e] head-mean weights in CSR order,
  float* att_edge = nullptr;     //   [E,h] attention and
  float* prods_edge = nullptr;   //   [E,h] scores in the caller's edge order
  const Fork* fork = nullptr;    // the hub rows' own launches as a branch on the second stream
  HubDefer* defer = nullptr;     // the caller's aggregation follows on this stream and can normalise the hub rows
  bool hubs_only = false;        // the weights of the hub rows' entries only (the short rows are attended elsewhere)
  bool stats_only = false;       // the general passes 1-2 only (scores + segment statistics stay in the workspace) ...
  AttArgs* args_out = nullptr;   // ... and the kernel arguments handed back: the backward pass continues from there
  int pass = 0;                  // 1..3: that pass of the general path alone; 0: all
};

// THE (heads, d_k) dispatcher and THE score-type dispatcher: every template line of this file's launches is reached through them.
// visit_value calls f(Int<v>) for the v of its list that equals x (false: none does), so a call site instantiates its kernel for the
// values it lists and for no other.
template <int V> using Int = std::integral_constant<int, V>;
template <int... V, class F>
bool visit_value(int x, F&& f) { return ((x == V && (f(Int<V>{}), true)) || ...); }
// heads 1, 2, 4 and, unless MAXH says 4, 8 ...
template <int MAXH = 8, class F>
bool visit_heads(int h, F&& f) {
  if constexpr (MAXH >= 8) return visit_value<1, 2, 4, 8>(h, f);
  else return visit_value<1, 2, 4>(h, f);
}
// ... x d_k / 4 in {1, 2, 4}
template <int MAXH = 8, class F>
bool visit_line(int h, int dk4, F&& f) {
  return visit_heads<MAXH>(h, [&](auto H) { visit_value<1, 2, 4>(dk4, [&](auto D) { f(H, D); }); });
}
// (a type outside the list is GAT's: plan_attention has refused every other)
template <class F>
void visit_type(int type, F&& f) {
  if (!visit_value<GNPDE_ATT_SCALED_DOT, GNPDE_ATT_COSINE, GNPDE_ATT_PEARSON, GNPDE_ATT_EXP_KERNEL>(type, f)) f(Int<GNPDE_ATT_GAT>{});
}

// THE lane mapping of the two row classes.  dk4 = d_k / 4 for the scaled-dot row kernels (row_attention_sd_kernel and its one-launch
// form), 0 for row_attention_kernel, which interleaves no rows.
// Rows of <= 16 entries.  4 heads, d_k 4 or 16 (round 6): a QUARTER of a wave per row -- 16 lanes = 4 entries x 4 heads per pass, four
// passes, two rows interleaved per group: 8 rows per wave instead of 4 on whole waves, where a median row of 8 entries left half of the
// lanes without an entry.  Measured at the ogbn-arxiv shape: row attention 41.2 -> 37.3 us per evaluation (1074 -> 1089 steps/s at
// T = 100), R-MAT (d_k = 16) 4.48 -> 3.98 ms; the other packings tried on the row softmax (half a wave x 2 passes with 8 / 4 rows per
// wave: 38.2; a quarter with 16 rows per wave: 40.4, with 4: 37.3; half with 16 rows: 43.0; an eighth x 8 passes with 16 / 8 rows:
// 40.4 / 37.2) are in DESIGN.md, the whole-wave form (quarter_rows = false: four or two rows interleaved) stays behind
// gnpde_tune(17, 9) for the row softmax (A/B).  Other head counts: 16 H lanes (at most a wave) per row.
struct RowShape {
  bool quarter;
  int gl16, p16, ri16;   // <= 16 entries: lanes per row, passes to cover 16 entries x H heads, rows interleaved per group,
  int rows16;            //   rows per workgroup
  int p64, pb64;         // 17..GNPDE_LONG_ROW entries, a wave per row: passes to cover GNPDE_LONG_ROW entries, passes per batch
};
constexpr RowShape row_shape(int h, int dk4, bool quarter_rows = true) {
  RowShape s{};
  s.quarter = quarter_rows && h == 4 && (dk4 == 1 || dk4 == 4);
  s.gl16 = s.quarter ? 16 : ((16 * h < kWave) ? 16 * h : kWave);
  s.p16 = (16 * h + s.gl16 - 1) / s.gl16;
  s.ri16 = dk4 == 0 ? 1 : s.quarter ? 2 : ((dk4 == 1 && s.p16 == 1) ? 4 : (s.p16 == 1 ? 2 : 1));
  s.rows16 = (kWave / s.gl16) * s.ri16 * kWavesPerBlock;
  s.p64 = GNPDE_LONG_ROW / (kWave / h);
  s.pb64 = (dk4 == 1) ? 4 : 2;
  return s;
}

struct AttPlan {
  gnpde_attention_launch_t l;     // what gnpde_attention_plan reports
  const gnpde_graph_t* g;         // the call
  const gnpde_attention_t* at;
  AttRequest rq;
  const gnpde_graph_t* rows;      // the graph whose rows the row and hub kernels walk: g, or its transpose (normalisation over columns)
  char* ws;                       // the workspace and its regions
  AttLayout L;
  int row_hubs;                   // hub blocks in front of the row launches (l.n_hub or 0)
  const int* long_list;           // general path: the long segments that have passes of their own (nullptr: none)
  unsigned scores_grid, stats_grid, norm_grid;
};

inline unsigned ceil_blocks(long long items, long long per_block) { return static_cast<unsigned>((items + per_block - 1) / per_block); }

// The plan of a call.  Operand pointers are read for their alignment and for being null, never through; ws_bytes is compared and nothing
// else.  g_tune is read here and nowhere else on the attention's host side.
int plan_attention(const gnpde_graph_t* g, const gnpde_attention_t* at, const AttRequest& rq, void* ws, size_t ws_bytes, AttPlan* p) {
  *p = AttPlan{};
  gnpde_attention_launch_t& l = p->l;
  GNPDE_CHECK_ARG(g && at, GNPDE_EINVAL, "edge_attention: null descriptor");
  GNPDE_CHECK_ARG(rq.stats_only || rq.pass == 1 || rq.pass == 2 || rq.w_mean || rq.att_edge || rq.prods_edge, GNPDE_EINVAL,
                  "edge_attention: no output requested");
  GNPDE_CHECK_ARG(at->heads >= 1 && at->att_dim >= at->heads && at->att_dim % at->heads == 0, GNPDE_EINVAL,
                  "edge_attention: heads (%d) must be a factor of the attention dimension (%d)", at->heads, at->att_dim);
  GNPDE_CHECK_ARG(at->type >= GNPDE_ATT_SCALED_DOT && at->type <= GNPDE_ATT_GAT, GNPDE_EINVAL, "edge_attention: bad type %d", at->type);
  GNPDE_CHECK_ARG(at->norm_idx == 0 || at->norm_idx == 1, GNPDE_EINVAL, "edge_attention: attention_norm_idx must be 0 or 1");
  GNPDE_CHECK_ARG(at->q && at->k && at->ldqk >= at->att_dim, GNPDE_EINVAL, "edge_attention: bad q/k");
  GNPDE_CHECK_ARG(at->type != GNPDE_ATT_GAT || at->gat_a, GNPDE_EINVAL, "edge_attention: GAT needs the vector a");
  GNPDE_CHECK_ARG(at->type != GNPDE_ATT_EXP_KERNEL || (at->output_var && at->lengthscale), GNPDE_EINVAL,
                  "edge_attention: exp_kernel needs output_var and lengthscale");
  GNPDE_CHECK_ARG(at->norm_idx == 0 || (g->cscptr && g->cscpos), GNPDE_EINVAL, "edge_attention: norm_idx=1 needs the CSC view");
  GNPDE_CHECK_ARG(g->rowidx && g->perm, GNPDE_EINVAL, "edge_attention: graph lacks rowidx/perm");
  if (g->e == 0 || g->n == 0) return 0;     // (GNPDE_ATT_ROUTE_NONE: nothing to launch)
  const bool gat = at->type == GNPDE_ATT_GAT;
  p->L = att_layout(g->n, g->e, at->heads, gat, long_slots_of(g), at->n_key_rows);
  GNPDE_CHECK_ARG(ws && ws_bytes >= p->L.total, GNPDE_EWS, "edge_attention: workspace %zu < %zu bytes", ws_bytes, p->L.total);
  GNPDE_CHECK_ARG(reinterpret_cast<uintptr_t>(ws) % 16 == 0, GNPDE_EINVAL, "edge_attention: workspace must be 16-byte aligned");
  p->g = g; p->at = at; p->rq = rq; p->ws = static_cast<char*>(ws);

  const int h = at->heads, dk = at->att_dim / h;
  const bool heads_ok = h == 1 || h == 2 || h == 4 || h == 8;       // the row kernels' head counts
  const bool dk_ok = dk == 4 || dk == 8 || dk == 16;                // the scaled-dot row kernels' head widths
  const bool generic = g_tune[GNPDE_TUNE_ATT_GENERIC_ROWS] != 0;    // A/B: no scaled-dot row kernels
  const bool one_stream = rq.fork == nullptr || rq.fork->aux == nullptr;
  const bool sq = at->square_plus != 0;
  // the scaled-dot row kernels carry a graph's hub chunks in their first blocks, given its chunk -> first-chunk table
  auto hubs_ride = [&](const gnpde_graph_t* x) { return one_stream && (x->n_long_rows == 0 || x->long_chunk_first != nullptr); };
  const bool w_alone = !rq.stats_only && rq.pass == 0 && rq.att_edge == nullptr && rq.prods_edge == nullptr;
  l.h = h;
  l.hub_fold = g_tune[GNPDE_TUNE_HUB_FOLD] == 2 ? 2 : 0;   // (0, staged through LDS: default since round 3, bit-identical; -3.4 % on the R-MAT launch)
  l.vec4 = (dk % 4 == 0) && (at->ldqk % 4 == 0) && (reinterpret_cast<uintptr_t>(at->q) % 16 == 0) && (reinterpret_cast<uintptr_t>(at->k) % 16 == 0);
  if (gat) l.gat_terms = 1;

  // the row softmax with the head-mean weights alone: fused row kernels exist for these (type, heads, alignment) combinations
  const bool fused = w_alone && at->norm_idx == 0 && !sq && g->bin_rows != nullptr && heads_ok && (gat || l.vec4);
  GNPDE_CHECK_ARG(g->row_begin == 0 || fused, GNPDE_EINVAL, "edge_attention: a row sub-range needs the fused row path");
  // ... and the scaled-dot scores with the OTHER normalisers in fused segment passes (the three general passes round-trip an [E,h]
  // score array and walk the segments twice: 2 - 2.5 x the time of the row softmax at the ogbn-arxiv shape).  squareplus: one sweep for
  // the global maximum (MODE 2), then the fused kernel with it (MODE 1); normalisation over the columns: the same kernels over the rows
  // of the transposed graph with q and k exchanged, the weights scattered to their CSR positions.
  const gnpde_graph_t* sg = at->norm_idx == 0 ? g : at->graph_t;
  const bool sd_fast = !fused && w_alone && !rq.hubs_only && at->type == GNPDE_ATT_SCALED_DOT && l.vec4 && rq.w_mean != nullptr && heads_ok &&
                       dk_ok && !generic && g->row_begin == 0 && sg != nullptr && sg->bin_rows != nullptr && sg->rowidx != nullptr &&
                       sg->n == g->n && sg->e == g->e && sg->row_begin == 0 && one_stream &&
                       (sg->n_long_rows == 0 || (sg->long_chunk_first != nullptr && sg->long_chunk_begin != nullptr)) &&
                       (at->norm_idx == 0 || (at->t_from_csr != nullptr && at->edge_w_csr == nullptr));
  p->rows = sd_fast ? sg : g;
  l.n_hub = p->rows->n_long_rows > 0 ? p->rows->n_long_chunks : 0;
  const int n16 = p->rows->n_bin16, n64 = p->rows->n_bin64;

  // a route whose row launches are row_attention_sd_kernel's (or its one-launch form): template line (l.h, dk4, MODE per sweep, l.scatter)
  auto sd = [&l](int route, int dk4, int mode0, int mode1 = -1) {
    l.route = route; l.dk4 = dk4; l.n_sweeps = mode1 < 0 ? 1 : 2; l.mode[0] = mode0; l.mode[1] = mode1 < 0 ? 0 : mode1;
  };
  if (fused && rq.hubs_only) {
    l.route = GNPDE_ATT_ROUTE_HUBS_ONLY;
    l.hubs = l.n_hub > 0 ? GNPDE_ATT_HUBS_OWN : GNPDE_ATT_HUBS_NONE;
  } else if (fused && gat && rq.w_mean != nullptr && at->edge_w_csr == nullptr && hubs_ride(g) && !generic) {
    // GAT's row softmax on the scaled-dot row kernels (gat_terms_kernel's table, MODE 3: leaky ReLU on the score)
    sd(GNPDE_ATT_ROUTE_SD_ROWS, 1, 3);
    l.gat_terms = 2;
  } else if (fused && rq.defer != nullptr && at->type == GNPDE_ATT_SCALED_DOT && rq.fork == nullptr && at->edge_w_csr == nullptr &&
             rq.w_mean != nullptr && g->row_begin == 0 && at->n_key_rows == 0 && dk_ok && h <= 4 &&
             (g->n_long_rows == 0 || (g->long_chunk_first != nullptr && g->long_chunk_begin != nullptr && g->long_chunk_end != nullptr)) &&
             g_tune[GNPDE_TUNE_ATT_ONE_LAUNCH] == 0 && !generic && g_tune[GNPDE_TUNE_ATT_ROWS16] == 0) {
    // THE one-launch condition: the caller's aggregation takes the hub rows' normalisation (HubDefer).  8 heads keep the two launches:
    // their long-row body needs 96 - 123 VGPRs, and one kernel would run the <= 16-entry rows -- 54 - 56 VGPRs, 8 waves per SIMD in a
    // launch of their own -- at 4 - 5.
    sd(GNPDE_ATT_ROUTE_SD_ONE, dk / 4, 0);
  } else if (fused && (at->type == GNPDE_ATT_SCALED_DOT || at->type == GNPDE_ATT_EXP_KERNEL) && dk_ok && hubs_ride(g) && !generic) {
    // (the exp kernel through the same row kernels, MODE 4: squared distance instead of the dot product, per-entry formula as
    //  edge_score<GNPDE_ATT_EXP_KERNEL>: 815 -> ~1000 steps/s at the ogbn-arxiv shape)
    sd(GNPDE_ATT_ROUTE_SD_ROWS, dk / 4, at->type == GNPDE_ATT_EXP_KERNEL ? 4 : 0);
  } else if (fused) {
    // a row kernel per class; the hub rows in two launches of their own, as a parallel branch when a second stream is given.  The
    // scaled-dot scores keep their specialised row kernels here (a forked stream, or a graph without the chunk table)
    sd(GNPDE_ATT_ROUTE_ROWS, at->type == GNPDE_ATT_SCALED_DOT && dk_ok && !generic ? dk / 4 : 0, 0);
    l.hubs = l.n_hub == 0 ? GNPDE_ATT_HUBS_NONE : one_stream ? GNPDE_ATT_HUBS_OWN : GNPDE_ATT_HUBS_OWN_FORKED;
  } else if (sd_fast) {
    sd(GNPDE_ATT_ROUTE_SD_ROWS, dk / 4, sq ? 2 : 0, sq ? 1 : -1);
    l.swapped = l.scatter = at->norm_idx == 1;
  } else {
    l.route = GNPDE_ATT_ROUTE_GENERAL;
    l.passes = (rq.pass == 0 ? 7 : 1 << (rq.pass - 1)) & (rq.stats_only ? 3 : 7);
    if (sq && rq.pass <= 1) l.gmax = GNPDE_ATT_GMAX_ATOMIC;      // (scores_kernel: atomic maxima, behind a memset)
    l.seg_stats_heads = heads_ok;
    l.n_long = at->norm_idx == 0 ? g->n_long_rows : g->n_long_cols;
    p->long_list = l.n_long > 0 ? (at->norm_idx == 0 ? g->long_rows : g->long_cols) : nullptr;
    l.max_chunks = ((at->norm_idx == 0 ? g->max_row_len : g->max_col_len) + GNPDE_LONG_ROW - 1) / GNPDE_LONG_ROW;
    const bool long_passes = p->long_list != nullptr && (l.passes & 2);
    if (long_passes) l.hubs = GNPDE_ATT_HUBS_LONG_STATS;
    p->scores_grid = stream_grid(static_cast<long long>(g->e) * h);
    p->stats_grid = ceil_blocks(g->n, kWavesPerBlock);
    p->norm_grid = stream_grid(g->e);
    l.launches = (l.passes & 1) + ((l.passes >> 1) & 1) * (long_passes ? 3 : 1) + ((l.passes >> 2) & 1);
  }

  if (l.route == GNPDE_ATT_ROUTE_SD_ROWS) p->row_hubs = l.n_hub;
  if (p->row_hubs > 0) l.hubs = GNPDE_ATT_HUBS_IN_ROWS;
  // the grids of the row launches: [sweep][0] rows of <= 16 entries, [sweep][1] rows of 17..GNPDE_LONG_ROW entries (0: no launch)
  if (l.route == GNPDE_ATT_ROUTE_SD_ONE) {
    // ONE launch: hub phase 0, the rows of 17..512 entries, the rows of <= 16 entries.  The hub entries' weights are NOT written.
    const RowShape s = row_shape(h, l.dk4);
    l.hubs = l.n_hub > 0 ? GNPDE_ATT_HUBS_DEFERRED : GNPDE_ATT_HUBS_NONE;
    l.rows16 = s.quarter ? GNPDE_ATT_ROWS16_QUARTER : GNPDE_ATT_ROWS16_LANES;
    l.grid[0][0] = static_cast<unsigned>(l.n_hub) + ceil_blocks(n64, kWavesPerBlock) + ceil_blocks(n16, s.rows16);
  } else {
    for (int sw = 0; sw < l.n_sweeps; ++sw) {
      // first launch: hub phase 0 + rows of <= 16 entries; second: hub phase 1 + rows of 17..512 entries (the maximum sweep of
      // squareplus, MODE 2, has no hub phase 1)
      const bool whole_wave = l.dk4 != 0 && l.mode[sw] == 0 && !l.scatter && g_tune[GNPDE_TUNE_ATT_ROWS16] == 9 && row_shape(h, l.dk4).quarter;
      const RowShape s = row_shape(h, l.dk4, !whole_wave);
      if (sw == 0) l.rows16 = whole_wave ? GNPDE_ATT_ROWS16_WHOLE_WAVE : s.quarter ? GNPDE_ATT_ROWS16_QUARTER : GNPDE_ATT_ROWS16_LANES;
      const int hubs2 = l.mode[sw] == 2 ? 0 : p->row_hubs;
      if (n16 > 0 || p->row_hubs > 0) l.grid[sw][0] = ceil_blocks(n16, s.rows16) + p->row_hubs;
      if (n64 > 0 || hubs2 > 0) l.grid[sw][1] = ceil_blocks(n64, kWavesPerBlock) + hubs2;
    }
    if (l.n_sweeps == 2) {
      // the maximum sweep of a small grid without hub blocks: per-wave maxima, folded by the blocks of the second sweep
      // (AttArgs::gmax_part) -- nothing to clear, no fold launch; else slot atomics behind a memset, folded by gmax_fold_kernel
      const long long waves = (static_cast<long long>(l.grid[0][0]) + l.grid[0][1]) * kWavesPerBlock;
      const bool per_wave = l.n_hub == 0 && waves <= kGmaxPartCap && g_tune[GNPDE_TUNE_GMAX_SMALL] == 0;
      l.gmax = per_wave ? GNPDE_ATT_GMAX_PER_WAVE : GNPDE_ATT_GMAX_SLOTS_FOLD;
      if (per_wave) l.gmax_count = static_cast<int>(waves);
    }
  }
  if (l.route != GNPDE_ATT_ROUTE_GENERAL) {
    for (int sw = 0; sw < 2; ++sw) l.launches += (l.grid[sw][0] > 0) + (l.grid[sw][1] > 0);
    l.launches += (l.gmax == GNPDE_ATT_GMAX_SLOTS_FOLD) + (l.hubs == GNPDE_ATT_HUBS_OWN || l.hubs == GNPDE_ATT_HUBS_OWN_FORKED ? 2 : 0);
  }
  l.launches += l.gat_terms != 0;
  return 0;
}

// AttArgs of a plan: filled once, here.
AttArgs fill_args(const AttPlan& p) {
  const gnpde_graph_t* g = p.g;
  const gnpde_attention_t* at = p.at;
  const gnpde_attention_launch_t& l = p.l;
  AttArgs a{};
  a.n = g->n; a.e = g->e; a.h = at->heads; a.dk = at->att_dim / at->heads;
  a.type = at->type; a.norm_idx = at->norm_idx; a.square_plus = at->square_plus ? 1 : 0;
  a.inv_sqrt_dk_den = static_cast<float>(std::sqrt(static_cast<double>(a.dk)));
  a.scale_mul = static_cast<float>(1.0 / std::sqrt(static_cast<double>(a.dk)));
  a.leaky_slope = at->leaky_slope;
  a.rowidx = g->rowidx; a.colidx = g->colidx; a.perm = g->perm;
  a.rowptr = g->rowptr; a.bin_rows = g->bin_rows;
  a.segptr = at->norm_idx == 0 ? g->rowptr : g->cscptr;
  a.segpos = at->norm_idx == 0 ? nullptr : g->cscpos;
  a.q = at->q; a.k = at->k; a.ldqk = at->ldqk;
  a.output_var = at->output_var; a.lengthscale = at->lengthscale; a.edge_w = at->edge_w_csr;
  a.scores = reinterpret_cast<float*>(p.ws + p.L.scores);
  a.seg_m = reinterpret_cast<float*>(p.ws + p.L.seg_m);
  a.seg_den = reinterpret_cast<float*>(p.ws + p.L.seg_den);
  a.gmax = reinterpret_cast<unsigned*>(p.ws + p.L.gmax);
  a.gat_terms = reinterpret_cast<float*>(p.ws + p.L.gat);
  a.w_mean = p.rq.w_mean; a.att_edge = p.rq.att_edge; a.prods_edge = p.rq.prods_edge;
  a.hub_fold_lds = l.hub_fold == 2 ? 0 : 1;
  if (l.route == GNPDE_ATT_ROUTE_GENERAL) {
    a.long_segs = p.long_list;
    return a;
  }
  // the row and hub kernels: the walked graph and its hub chunks
  const gnpde_graph_t* r = p.rows;
  a.rowidx = r->rowidx; a.colidx = r->colidx; a.rowptr = r->rowptr; a.bin_rows = r->bin_rows;
  a.chunk_begin = r->long_chunk_begin; a.chunk_end = r->long_chunk_end; a.long_segs = r->long_rows;
  if (l.swapped) {
    a.q = at->k; a.k = at->q;            // the segment's own vector is k_j, the gathered one q_i
    a.out_pos = at->t_from_csr;
  }
  if (l.gat_terms == 2) {                // gat_terms_kernel's table, read as 4-wide scaled-dot vectors
    a.type = GNPDE_ATT_SCALED_DOT;
    a.q = reinterpret_cast<const float*>(p.ws + p.L.gat_table);
    a.k = a.q + 4 * a.h;
    a.ldqk = 8 * a.h;
    a.dk = 4;
    a.scale_mul = 0.5f;
    a.inv_sqrt_dk_den = 2.0f;
  }
  a.sp_mode = l.mode[0];
  if (l.gmax == GNPDE_ATT_GMAX_PER_WAVE) {
    a.gmax_part = a.gmax + 64;           // (256 bytes behind the maximum itself, as the slots)
    a.gmax_count = l.gmax_count;
  }
  return a;
}

// ---- launch_planned and its parts: they carry a plan out and decide nothing
float* hub_part(const AttPlan& p) { return reinterpret_cast<float*>(p.ws + p.L.part); }

// one sweep of the scaled-dot row kernels over both row classes, the plan's hub blocks in front of each launch
template <int H, int DK4, int MODE, bool SCATTER>
void launch_sd_sweep(const AttPlan& p, AttArgs a, int sw, hipStream_t s) {
  const gnpde_attention_launch_t& l = p.l;
  const int n16 = p.rows->n_bin16, n64 = p.rows->n_bin64;
  float* part = p.row_hubs > 0 ? hub_part(p) : nullptr;
  const int* chunk_first = p.row_hubs > 0 ? p.rows->long_chunk_first : nullptr;
  constexpr RowShape S = row_shape(H, DK4);
  a.sp_mode = MODE;
  if (l.grid[sw][0] > 0) {
    bool whole_wave = false;
    if constexpr (S.quarter && MODE == 0 && !SCATTER) {
      if (l.rows16 == GNPDE_ATT_ROWS16_WHOLE_WAVE) {      // A/B: a whole wave per row, four (d_k 4) or two rows interleaved (until round 6)
        constexpr RowShape W = row_shape(H, DK4, false);
        hipLaunchKernelGGL((row_attention_sd_kernel<H, DK4, W.gl16, W.ri16, W.p16, 1, MODE, SCATTER>), dim3(l.grid[sw][0]), dim3(kBlock), 0, s,
                           a, 0, n16, p.row_hubs, 0, part, chunk_first);
        whole_wave = true;
      }
    }
    if (!whole_wave)
      hipLaunchKernelGGL((row_attention_sd_kernel<H, DK4, S.gl16, S.ri16, S.p16, 1, MODE, SCATTER>), dim3(l.grid[sw][0]), dim3(kBlock), 0, s,
                         a, 0, n16, p.row_hubs, 0, part, chunk_first);
    if (MODE == 2 && l.gmax == GNPDE_ATT_GMAX_PER_WAVE) a.gmax_base = static_cast<int>(l.grid[sw][0]) * kWavesPerBlock;   // the second launch's waves follow
  }
  if (l.grid[sw][1] > 0)
    hipLaunchKernelGGL((row_attention_sd_kernel<H, DK4, kWave, 1, S.pb64, S.p64 / S.pb64, MODE, SCATTER>), dim3(l.grid[sw][1]), dim3(kBlock), 0, s,
                       a, n16, n64, MODE == 2 ? 0 : p.row_hubs, 1, part, chunk_first);
}

// THE (MODE, SCATTER) switch of the scaled-dot row kernels: MODE 3 at d_k = 4 only, SCATTER at MODE 0 and 1
void launch_sd_rows(const AttPlan& p, const AttArgs& a, int sw, hipStream_t s) {
  const int mode = p.l.mode[sw];
  const bool sc = p.l.scatter != 0;
  visit_line(p.l.h, p.l.dk4, [&](auto H_, auto D_) {
    constexpr int H = decltype(H_)::value, DK4 = decltype(D_)::value;
    if (mode == 4) launch_sd_sweep<H, DK4, 4, false>(p, a, sw, s);             // exp kernel scores
    else if (mode == 3) {                                                       // GAT scores (4-wide vectors only)
      if constexpr (DK4 == 1) launch_sd_sweep<H, DK4, 3, false>(p, a, sw, s);
    }
    else if (mode == 2) launch_sd_sweep<H, DK4, 2, false>(p, a, sw, s);        // (the maximum sweep: writes no weights)
    else if (mode == 1 && sc) launch_sd_sweep<H, DK4, 1, true>(p, a, sw, s);
    else if (mode == 1) launch_sd_sweep<H, DK4, 1, false>(p, a, sw, s);
    else if (sc) launch_sd_sweep<H, DK4, 0, true>(p, a, sw, s);
    else launch_sd_sweep<H, DK4, 0, false>(p, a, sw, s);
  });
}

// the row launches of GNPDE_ATT_ROUTE_ROWS: row_attention_kernel per class, or the scaled-dot row kernels without hub blocks
void launch_rows(const AttPlan& p, const AttArgs& a, hipStream_t s) {
  if (p.l.dk4 != 0) return launch_sd_rows(p, a, 0, s);
  const int n16 = p.rows->n_bin16, n64 = p.rows->n_bin64;
  visit_type(a.type, [&](auto T_) {
    visit_heads(p.l.h, [&](auto H_) {
      constexpr int TYPE = decltype(T_)::value, H = decltype(H_)::value;
      constexpr bool VEC4 = TYPE != GNPDE_ATT_GAT;
      constexpr RowShape S = row_shape(H, 0);
      if (p.l.grid[0][0] > 0)
        hipLaunchKernelGGL((row_attention_kernel<TYPE, H, S.gl16, S.p16, VEC4>), dim3(p.l.grid[0][0]), dim3(kBlock), 0, s, a, 0, n16);
      if (p.l.grid[0][1] > 0)
        hipLaunchKernelGGL((row_attention_kernel<TYPE, H, kWave, S.p64, VEC4>), dim3(p.l.grid[0][1]), dim3(kBlock), 0, s, a, n16, n64);
    });
  });
}

// the hub rows in two launches of their own: chunk statistics, then the weights of the chunks' entries
int launch_hubs(const AttPlan& p, const AttArgs& a, hipStream_t s) {
  float* part = hub_part(p);
  const dim3 grid(p.l.n_hub);
  visit_type(a.type, [&](auto T_) {
    constexpr int TYPE = decltype(T_)::value;
    const bool v = p.l.vec4 && TYPE != GNPDE_ATT_GAT;
    if constexpr (TYPE == GNPDE_ATT_SCALED_DOT) {
      if (v && visit_heads(p.l.h, [&](auto H_) {
            hipLaunchKernelGGL(hub_scores_partial_sd_kernel<decltype(H_)::value>, grid, dim3(kBlock), 0, s, a, part);
          })) return;
    }
    if (v) hipLaunchKernelGGL((hub_scores_partial_kernel<TYPE, true>), grid, dim3(kBlock), 0, s, a, part);
    else hipLaunchKernelGGL((hub_scores_partial_kernel<TYPE, false>), grid, dim3(kBlock), 0, s, a, part);
  });
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(hub_normalise_kernel, grid, dim3(kBlock), 0, s, a, part, p.rows->long_chunk_first);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

int launch_planned(const AttPlan& p, hipStream_t stream) {
  const gnpde_attention_launch_t& l = p.l;
  if (l.route == GNPDE_ATT_ROUTE_NONE) return 0;
  AttArgs a = fill_args(p);
  if (l.gat_terms != 0) {
    const int term_rows = p.at->n_key_rows > p.g->n ? p.at->n_key_rows : p.g->n;      // every row a column may address
    hipLaunchKernelGGL(gat_terms_kernel, dim3(ceil_blocks(static_cast<long long>(term_rows) * l.h, kBlock)), dim3(kBlock), 0, stream,
                       p.at->q, p.at->ldqk, p.at->gat_a, term_rows, l.h, p.at->att_dim / l.h, reinterpret_cast<float*>(p.ws + p.L.gat),
                       l.gat_terms == 2 ? reinterpret_cast<float*>(p.ws + p.L.gat_table) : nullptr);
    GNPDE_LAUNCH_CHECK();
  }
  switch (l.route) {
    case GNPDE_ATT_ROUTE_HUBS_ONLY:
      return l.hubs == GNPDE_ATT_HUBS_OWN ? launch_hubs(p, a, stream) : 0;
    case GNPDE_ATT_ROUTE_SD_ONE: {
      if (l.grid[0][0] > 0)
        visit_line<4>(l.h, l.dk4, [&](auto H_, auto D_) {
          constexpr RowShape S = row_shape(decltype(H_)::value, decltype(D_)::value);
          hipLaunchKernelGGL((row_attention_sd_one_kernel<decltype(H_)::value, decltype(D_)::value, S.gl16, S.ri16, S.p16, S.pb64, S.p64 / S.pb64>),
                             dim3(l.grid[0][0]), dim3(kBlock), 0, stream, a, p.g->n_bin16, p.g->n_bin64, l.n_hub, hub_part(p));
        });
      GNPDE_LAUNCH_CHECK();
      *p.rq.defer = HubDefer{hub_part(p), a.scores, p.g->long_chunk_first, p.rq.w_mean, l.h, 1};     // (taken)
      return 0;
    }
    case GNPDE_ATT_ROUTE_SD_ROWS:
      for (int sw = 0; sw < l.n_sweeps; ++sw) {
        const bool slots = sw == 0 && l.gmax == GNPDE_ATT_GMAX_SLOTS_FOLD;
        if (slots) {
          GNPDE_HIP(hipMemsetAsync(a.gmax, 0, 256 + kGmaxSlots * 128, stream));
          a.gmax_slots = a.gmax + 64;          // (256 bytes behind the maximum itself)
        }
        launch_sd_rows(p, a, sw, stream);
        GNPDE_LAUNCH_CHECK();
        if (slots) {
          hipLaunchKernelGGL(gmax_fold_kernel, dim3(1), dim3(kWave), 0, stream, a.gmax_slots, a.gmax);
          GNPDE_LAUNCH_CHECK();
          a.gmax_slots = nullptr;
        }
      }
      return 0;
    case GNPDE_ATT_ROUTE_ROWS: {
      hipStream_t br = stream;
      if (l.hubs != GNPDE_ATT_HUBS_NONE) {  // hubs: chunk passes, as a parallel branch when a fork stream is given
        if (const int rc = fork_begin(p.rq.fork, stream, &br)) return rc;
        if (const int rc = launch_hubs(p, a, br)) return rc;
      }
      launch_rows(p, a, stream);      // (a carries the hub chunk tables too: the row kernels read them in hub blocks only, and here they have none)
      GNPDE_LAUNCH_CHECK();
      return l.hubs != GNPDE_ATT_HUBS_NONE ? fork_end(p.rq.fork, stream, br) : 0;
    }
    default: break;
  }
  // the three general passes
  if (l.gmax == GNPDE_ATT_GMAX_ATOMIC) GNPDE_HIP(hipMemsetAsync(a.gmax, 0, 256 + kGmaxSlots * 128, stream));
  if (l.passes & 1) {
    visit_type(a.type, [&](auto T_) {
      constexpr int TYPE = decltype(T_)::value;
      if (l.vec4 && TYPE != GNPDE_ATT_GAT) hipLaunchKernelGGL((scores_kernel<TYPE, true>), dim3(p.scores_grid), dim3(kBlock), 0, stream, a);
      else hipLaunchKernelGGL((scores_kernel<TYPE, false>), dim3(p.scores_grid), dim3(kBlock), 0, stream, a);
    });
    GNPDE_LAUNCH_CHECK();
  }
  if (l.passes & 2) {
    if (l.seg_stats_heads)
      visit_heads(l.h, [&](auto H_) { hipLaunchKernelGGL(seg_stats_heads_kernel<decltype(H_)::value>, dim3(p.stats_grid), dim3(kBlock), 0, stream, a); });
    else
      hipLaunchKernelGGL(seg_stats_kernel, dim3(p.stats_grid), dim3(kBlock), 0, stream, a);
    GNPDE_LAUNCH_CHECK();
  }
  if (l.hubs == GNPDE_ATT_HUBS_LONG_STATS) {
    hipLaunchKernelGGL(seg_stats_long_partial_kernel, dim3(l.n_long, l.max_chunks), dim3(kBlock), 0, stream, a, hub_part(p), l.max_chunks);
    GNPDE_LAUNCH_CHECK();
    hipLaunchKernelGGL(seg_stats_long_combine_kernel, dim3(l.n_long), dim3(kWave), 0, stream, a, hub_part(p), l.max_chunks);
    GNPDE_LAUNCH_CHECK();
  }
  if (p.rq.args_out != nullptr) *p.rq.args_out = a;
  if (l.passes & 4) {
    hipLaunchKernelGGL(normalise_kernel, dim3(p.norm_grid), dim3(kBlock), 0, stream, a);
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}

int edge_attention_impl(const gnpde_graph_t* g, const gnpde_attention_t* at, const AttRequest& rq, void* ws, size_t ws_bytes, hipStream_t stream) {
  AttPlan plan;
  if (const int rc = plan_attention(g, at, rq, ws, ws_bytes, &plan)) return rc;
  return launch_planned(plan, stream);
}

}  // namespace

size_t attention_workspace_bytes(const gnpde_graph_t* g, int h, bool gat);

// One pass of the general path at a time (the row-partitioned solver exchanges between them: the global maximum of squareplus
// after pass 1, the per-column partial statistics of attention_norm_idx = 1 after pass 2)
int launch_edge_attention_pass(const gnpde_graph_t* g, const gnpde_attention_t* at, int pass, float* w_mean_csr, void* ws,
                               size_t ws_bytes, hipStream_t stream) {
  GNPDE_CHECK_ARG(pass >= 1 && pass <= 3, GNPDE_EINVAL, "edge_attention_pass: pass must be 1 (scores), 2 (segment statistics) or 3 (normalise)");
  GNPDE_CHECK_ARG(pass != 3 || w_mean_csr != nullptr, GNPDE_EINVAL, "edge_attention_pass: pass 3 writes w_mean_csr");
  AttRequest rq;
  rq.pass = pass;
  rq.w_mean = pass == 3 ? w_mean_csr : nullptr;      // (passes 1 and 2 write no output)
  return edge_attention_impl(g, at, rq, ws, ws_bytes, stream);
}

int launch_edge_attention(const gnpde_graph_t* g, const gnpde_attention_t* at, float* w_mean_csr, float* att_edge,
                          float* prods_edge, void* ws, size_t ws_bytes, hipStream_t stream, const Fork* fork) {
  AttRequest rq;
  rq.w_mean = w_mean_csr; rq.att_edge = att_edge; rq.prods_edge = prods_edge;
  rq.fork = fork;
  return edge_attention_impl(g, at, rq, ws, ws_bytes, stream);
}

// The attention of an evaluation whose aggregation (launch_spmm_rhs with `defer`, same stream) follows.  Where the plain scaled-dot
// row softmax runs (whole graph, no re-weighting, a specialised (heads, d_k)) it takes ONE launch, leaves the weights of the hub
// rows' entries unwritten and sets defer->taken: the aggregation's hub-chunk items form and store them.  Everything else runs
// launch_edge_attention's launches and leaves defer->taken == 0 (the weights are complete): one plan either way.
int launch_edge_attention_deferred(const gnpde_graph_t* g, const gnpde_attention_t* at, float* w_mean_csr, void* ws, size_t ws_bytes,
                                   hipStream_t stream, HubDefer* defer) {
  *defer = HubDefer{};
  AttRequest rq;
  rq.w_mean = w_mean_csr;
  rq.defer = defer;
  return edge_attention_impl(g, at, rq, ws, ws_bytes, stream);
}

// w_mean_csr[p] for the entries of the rows longer than GNPDE_LONG_ROW only (row softmax path); the caller attends the
// other rows itself (attn_spmm_kernel)
int launch_hub_attention(const gnpde_graph_t* g, const gnpde_attention_t* at, float* w_mean_csr, void* ws, size_t ws_bytes,
                         hipStream_t stream) {
  AttRequest rq;
  rq.w_mean = w_mean_csr;
  rq.hubs_only = true;
  return edge_attention_impl(g, at, rq, ws, ws_bytes, stream);
}

// merge of segment statistics (m, den) <- (m, den) (+) (m_in, den_in) for the rows listed: the online-softmax combination,
// or the plain sum for squareplus (its statistics carry no maximum)
__global__ __launch_bounds__(kBlock) void stats_merge_kernel(float* __restrict__ m, float* __restrict__ den, const int* __restrict__ rows,
                                                            int n_rows, int h, const float* __restrict__ m_in,
                                                            const float* __restrict__ den_in, int square_plus) {
  const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<long long>(n_rows) * h) return;
  const int i = static_cast<int>(idx / h), head = static_cast<int>(idx % h);
  const size_t o = static_cast<size_t>(rows != nullptr ? rows[i] : i) * h + head;
  if (square_plus) {
    den[o] = den[o] + den_in[idx];
    return;
  }
  const float ma = m[o], mb = m_in[idx];
  const float mm = fmaxf(ma, mb);
  // (both maxima -inf = a segment without entries on either side: exp(-inf - -inf) would be NaN; its statistics stay (-inf, sum))
  den[o] = mm == -INFINITY ? den[o] + den_in[idx] : den[o] * expf(ma - mm) + den_in[idx] * expf(mb - mm);
  m[o] = mm;
}


// ------------------------------------------------------------------------------------------------
// Backward of the normalisation + head mean for EVERY normaliser (softmax or squareplus, over rows or columns):
//   given dw[p] = dL/d(mean_h att[p,h]) / scale  (CSR order; the aggregation's SDDMM r = g_row . x_col)
//   returns ds[p,h] = dL/d(prods[p,h])  -- the scores BEFORE the optional edge re-weighting.
// softmax    a = e^{s-m}/den :  ds = c a (dw - t),            t[seg,h] = sum_{seg} a dw,   c = scale / H
// squareplus a = u/den, u = (z + sqrt(z^2+4))/2, z = s - M :   dz = c (dw - t)/den * u / sqrt(z^2+4),  ds = dz, and the
//            global maximum M (reference src/utils.py:196, `src.max()`) takes -sum(dz), which autograd hands EVENLY to the
//            entries equal to M (evenly_distribute_backward): ds -= [s == M] sum(dz) / #{s == M}.
// Passes: scores + segment statistics (the forward's passes 1-2, recomputed), t by one wavefront per segment (a block per
// long segment), one edge-parallel pass for ds with block partials of (sum dz, #max) summed in a fixed order, and for
// squareplus a second edge-parallel pass that applies the maximum's share.  No atomics.
// ------------------------------------------------------------------------------------------------
namespace {

struct BwdArgs {
  const float* __restrict__ dw;      // [e] CSR order: gradient of the HEAD MEAN (shared by the heads), or
  const float* __restrict__ datt;    // [E,h] caller's edge order: gradient of every head's attention (then dw == nullptr)
  const int* __restrict__ perm;      // CSR position -> edge id (for datt)
  int post;                          // 0: ds w.r.t. the raw scores (times edge_w); 1: (ds w.r.t. the score) * score  -- the
                                     //    common factor of every derivative of an exp kernel; 2: ds * leaky'(score) (GAT)
  float leaky_slope;
  float* t;                          // [n,h]
  float* ds;                         // [e,h]
  float* partial;                    // [grid,2]: sum dz, count of maxima
  const float* __restrict__ scale_ptr;
  int scale_sigmoid;
};

__device__ __forceinline__ float grad_in(const BwdArgs& b, long long p, int head, int h) {
  return b.dw != nullptr ? b.dw[p] : b.datt[static_cast<long long>(b.perm[p]) * h + head];
}

__device__ __forceinline__ float att_value(const AttArgs& a, float s, int seg, int head, float gmax) {
  const float den = a.seg_den[static_cast<size_t>(seg) * a.h + head];
  if (a.square_plus) return squareplus_num(s, gmax) / den;
  return expf(s - a.seg_m[static_cast<size_t>(seg) * a.h + head]) / den;
}

// t[seg,h] = sum over the segment of att * dw; BLOCK = false: a wavefront per segment (long ones skipped),
// BLOCK = true: a block per long segment
template <bool BLOCK>
__global__ __launch_bounds__(kBlock) void seg_dot_kernel(const AttArgs a, const BwdArgs b) {
  __shared__ float red[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  int seg;
  if (BLOCK) {
    seg = a.long_segs[blockIdx.x];
  } else {
    seg = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kWavesPerBlock + wave);
    if (seg >= a.n) return;
  }
  const int s0 = a.segptr[seg], s1 = a.segptr[seg + 1];
  if (!BLOCK && s1 - s0 > GNPDE_LONG_ROW && a.long_segs != nullptr) return;
  const float gmax = a.square_plus ? ord2f(*a.gmax) : 0.f;
  const int first = BLOCK ? static_cast<int>(threadIdx.x) : lane;
  const int step = BLOCK ? kBlock : kWave;
  for (int head = 0; head < a.h; ++head) {
    float sum = 0.f;
    for (int t = s0 + first; t < s1; t += step) {
      const int p = a.segpos ? a.segpos[t] : t;
      sum += att_value(a, a.scores[static_cast<size_t>(p) * a.h + head], seg, head, gmax) * grad_in(b, p, head, a.h);
    }
    sum = wave_sum(sum);
    if (BLOCK) {
      if (lane == 0) red[wave] = sum;
      __syncthreads();
      if (threadIdx.x == 0) b.t[static_cast<size_t>(seg) * a.h + head] = (red[0] + red[1]) + (red[2] + red[3]);
      __syncthreads();
    } else if (lane == 0) {
      b.t[static_cast<size_t>(seg) * a.h + head] = sum;
    }
  }
}

// what multiplies d L / d score: edge_w (raw-score gradient), the score itself (exp kernels), or LeakyReLU' (GAT)
__device__ __forceinline__ float post_factor(const BwdArgs& b, float s, float ew) {
  if (b.post == 1) return s;
  if (b.post == 2) return s > 0.f ? 1.0f : b.leaky_slope;
  return ew;
}

__global__ __launch_bounds__(kBlock) void att_bwd_edge_kernel(const AttArgs a, const BwdArgs b) {
  __shared__ float rs[kWavesPerBlock], rc[kWavesPerBlock];
  float scale = 1.0f;
  if (b.scale_ptr != nullptr) {
    scale = *b.scale_ptr;
    if (b.scale_sigmoid) scale = 1.0f / (1.0f + expf(-scale));
  }
  const float c = b.dw != nullptr ? scale / static_cast<float>(a.h) : scale;   // the head mean's 1/H only for a shared dw
  const float gmax = a.square_plus ? ord2f(*a.gmax) : 0.f;
  float lsum = 0.f, lcnt = 0.f;
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long p = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; p < a.e; p += stride) {
    const int seg = a.norm_idx == 0 ? a.rowidx[p] : a.colidx[p];
    const float ew = a.edge_w != nullptr ? a.edge_w[p] : 1.0f;
    for (int head = 0; head < a.h; ++head) {
      const float s = a.scores[p * a.h + head];
      const float v = grad_in(b, p, head, a.h) - b.t[static_cast<size_t>(seg) * a.h + head];
      float out;
      if (a.square_plus) {
        const float z = s - gmax;
        const float den = a.seg_den[static_cast<size_t>(seg) * a.h + head];
        const float root = sqrtf(z * z + 4.0f);
        out = c * v / den * (0.5f * (z + root)) / root;    // du/dz = u / sqrt(z^2 + 4)
        lsum += out;
        lcnt += (s == gmax) ? 1.0f : 0.0f;
      } else {
        out = c * att_value(a, s, seg, head, gmax) * v;
      }
      b.ds[p * a.h + head] = out * post_factor(b, s, ew);
    }
  }
  if (a.square_plus) {   // block partials, folded in block order by att_bwd_max_share_kernel
    lsum = wave_sum(lsum);
    lcnt = wave_sum(lcnt);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (lane == 0) { rs[wave] = lsum; rc[wave] = lcnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
      b.partial[2 * blockIdx.x] = (rs[0] + rs[1]) + (rs[2] + rs[3]);
      b.partial[2 * blockIdx.x + 1] = (rc[0] + rc[1]) + (rc[2] + rc[3]);
    }
  }
}

// squareplus: ds -= [s == M] sum(dz) / #{s == M}   (every block folds the partials in the same order)
__global__ __launch_bounds__(kBlock) void att_bwd_max_share_kernel(const AttArgs a, const BwdArgs b, int n_partials) {
  __shared__ float share;
  if (threadIdx.x == 0) {
    float tot = 0.f, cnt = 0.f;
    for (int i = 0; i < n_partials; ++i) { tot += b.partial[2 * i]; cnt += b.partial[2 * i + 1]; }
    share = cnt > 0.f ? tot / cnt : 0.f;
  }
  __syncthreads();
  const float gmax = ord2f(*a.gmax);
  const long long total = static_cast<long long>(a.e) * a.h;
  const long long stride = static_cast<long long>(gridDim.x) * blockDim.x;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += stride) {
    if (a.scores[i] == gmax) {
      const float ew = a.edge_w != nullptr ? a.edge_w[i / a.h] : 1.0f;
      b.ds[i] -= share * post_factor(b, a.scores[i], ew);
    }
  }
}

constexpr int kBwdPartials = 2048;

}  // namespace

size_t attention_bwd_workspace_bytes(const gnpde_graph_t* g, int h, bool gat) {
  return align_up(attention_workspace_bytes(g, h, gat), 256) + align_up(static_cast<size_t>(g->n) * h * 4, 256) + kBwdPartials * 2 * 4;
}

int launch_edge_attention_bwd(const gnpde_graph_t* g, const gnpde_attention_t* at, const float* dw_csr, const float* datt_edge,
                              int post, const float* scale, int scale_sigmoid, float* ds_csr, void* ws, size_t ws_bytes,
                              hipStream_t stream) {
  GNPDE_CHECK_ARG(g && at && ds_csr && ((dw_csr != nullptr) != (datt_edge != nullptr)) && post >= 0 && post <= 2, GNPDE_EINVAL,
                  "edge_attention_bwd: need exactly one of dw_csr / datt_edge, post in 0..2");
  if (g->e == 0 || g->n == 0) return 0;
  const bool gat = at->type == GNPDE_ATT_GAT;
  const size_t fwd = align_up(attention_workspace_bytes(g, at->heads, gat), 256);
  const size_t need = attention_bwd_workspace_bytes(g, at->heads, gat);
  GNPDE_CHECK_ARG(ws && ws_bytes >= need, GNPDE_EWS, "edge_attention_bwd: workspace %zu < %zu bytes", ws_bytes, need);
  AttArgs a{};
  AttRequest rq;     // the forward's general passes 1-2, recomputed, and their arguments
  rq.stats_only = true;
  rq.args_out = &a;
  int rc = edge_attention_impl(g, at, rq, ws, fwd, stream);
  if (rc) return rc;
  BwdArgs b{};
  b.dw = dw_csr;
  b.datt = datt_edge;
  b.perm = g->perm;
  b.post = post;
  b.leaky_slope = at->leaky_slope;
  b.ds = ds_csr;
  b.t = reinterpret_cast<float*>(static_cast<char*>(ws) + fwd);
  b.partial = reinterpret_cast<float*>(static_cast<char*>(ws) + fwd + align_up(static_cast<size_t>(g->n) * at->heads * 4, 256));
  b.scale_ptr = scale;
  b.scale_sigmoid = scale_sigmoid;
  hipLaunchKernelGGL(seg_dot_kernel<false>, dim3((g->n + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, stream, a, b);
  GNPDE_LAUNCH_CHECK();
  if (a.long_segs != nullptr) {
    const int n_long = at->norm_idx == 0 ? g->n_long_rows : g->n_long_cols;
    hipLaunchKernelGGL(seg_dot_kernel<true>, dim3(n_long), dim3(kBlock), 0, stream, a, b);
    GNPDE_LAUNCH_CHECK();
  }
  unsigned grid = stream_grid(a.e);
  if (grid > kBwdPartials) grid = kBwdPartials;
  hipLaunchKernelGGL(att_bwd_edge_kernel, dim3(grid), dim3(kBlock), 0, stream, a, b);
  GNPDE_LAUNCH_CHECK();
  if (a.square_plus) {
    hipLaunchKernelGGL(att_bwd_max_share_kernel, dim3(stream_grid(static_cast<long long>(a.e) * a.h)), dim3(kBlock), 0, stream,
                       a, b, static_cast<int>(grid));
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}

size_t attention_workspace_bytes_rows(const gnpde_graph_t* g, int h, bool gat, int key_rows) {
  return att_layout(g->n, g->e, h, gat, long_slots_of(g), key_rows).total;
}

size_t attention_workspace_bytes(const gnpde_graph_t* g, int h, bool gat) {
  return att_layout(g->n, g->e, h, gat, long_slots_of(g)).total;
}

}  // namespace gnpde

extern "C" size_t gnpde_attention_workspace_bytes(const gnpde_graph_t* g, const gnpde_attention_t* a) {
  if (!g || !a || a->heads < 1) return 0;
  return gnpde::attention_workspace_bytes_rows(g, a->heads, a->type == GNPDE_ATT_GAT, a->n_key_rows);
}

extern "C" int gnpde_edge_attention_pass(const gnpde_graph_t* g, const gnpde_attention_t* a, int32_t pass, float* w_mean_csr,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return gnpde::launch_edge_attention_pass(g, a, pass, w_mean_csr, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

namespace gnpde {
AttLayoutView att_layout_view(const gnpde_graph_t* g, const gnpde_attention_t* a) {
  const AttLayout L = att_layout(g->n, g->e, a->heads, a->type == GNPDE_ATT_GAT, long_slots_of(g), a->n_key_rows);
  return AttLayoutView{L.seg_m, L.seg_den, L.gmax, L.total};
}
}  // namespace gnpde

extern "C" int gnpde_attention_workspace_regions(const gnpde_graph_t* g, const gnpde_attention_t* a, size_t* offsets) {
  GNPDE_CHECK_ARG(g && a && offsets && a->heads >= 1, GNPDE_EINVAL, "attention_workspace_regions: bad arguments");
  const gnpde::AttLayout L = gnpde::att_layout(g->n, g->e, a->heads, a->type == GNPDE_ATT_GAT, gnpde::long_slots_of(g), a->n_key_rows);
  offsets[0] = L.scores; offsets[1] = L.seg_m; offsets[2] = L.seg_den; offsets[3] = L.gmax;
  return 0;
}

extern "C" int gnpde_segment_stats_merge(float* seg_m, float* seg_den, const int32_t* rows, int32_t n_rows, int32_t heads,
                                         const float* m_in, const float* den_in, int32_t square_plus, void* stream) {
  GNPDE_CHECK_ARG(n_rows >= 0 && heads >= 1, GNPDE_EINVAL, "segment_stats_merge: bad shape");
  if (n_rows == 0) return 0;
  GNPDE_CHECK_ARG(seg_den && den_in && (square_plus || (seg_m && m_in)), GNPDE_EINVAL, "segment_stats_merge: null pointer");
  const long long items = static_cast<long long>(n_rows) * heads;
  hipLaunchKernelGGL(gnpde::stats_merge_kernel, dim3(static_cast<unsigned>((items + gnpde::kBlock - 1) / gnpde::kBlock)),
                     dim3(gnpde::kBlock), 0, static_cast<hipStream_t>(stream), seg_m, seg_den, rows, n_rows, heads, m_in, den_in, square_plus);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

extern "C" int gnpde_edge_attention(const gnpde_graph_t* g, const gnpde_attention_t* a, float* w_mean_csr, float* att_edge,
                                    float* prods_edge, void* workspace, size_t workspace_bytes, void* stream) {
  return gnpde::launch_edge_attention(g, a, w_mean_csr, att_edge, prods_edge, workspace, workspace_bytes,
                                      static_cast<hipStream_t>(stream), nullptr);
}

extern "C" int gnpde_attention_plan(const gnpde_graph_t* g, const gnpde_attention_t* a, uint32_t request_flags, int32_t pass,
                                    uint64_t workspace_addr, gnpde_attention_launch_t* plan) {
  GNPDE_CHECK_ARG(plan != nullptr && pass >= 0 && pass <= 3, GNPDE_EINVAL, "attention_plan: plan is null or pass outside 0..3");
  // stand-ins for what the flags say is given: the planner reads that they are there
  float* const given = reinterpret_cast<float*>(uintptr_t{16});
  gnpde::Fork fork;
  fork.aux = reinterpret_cast<hipStream_t>(uintptr_t{16});
  gnpde::HubDefer defer;
  gnpde::AttRequest rq;
  if (request_flags & GNPDE_ATT_PLAN_W_MEAN) rq.w_mean = given;
  if (request_flags & GNPDE_ATT_PLAN_ATT_EDGE) rq.att_edge = given;
  if (request_flags & GNPDE_ATT_PLAN_PRODS_EDGE) rq.prods_edge = given;
  if (request_flags & GNPDE_ATT_PLAN_FORK) rq.fork = &fork;
  if (request_flags & GNPDE_ATT_PLAN_DEFER) rq.defer = &defer;
  rq.hubs_only = (request_flags & GNPDE_ATT_PLAN_HUBS_ONLY) != 0;
  rq.stats_only = (request_flags & GNPDE_ATT_PLAN_STATS_ONLY) != 0;
  rq.pass = pass;
  gnpde::AttPlan p;
  const int rc = gnpde::plan_attention(g, a, rq, reinterpret_cast<void*>(static_cast<uintptr_t>(workspace_addr)), SIZE_MAX, &p);
  *plan = p.l;
  return rc;
}

extern "C" size_t gnpde_attention_bwd_workspace_bytes(const gnpde_graph_t* g, const gnpde_attention_t* a) {
  if (!g || !a || a->heads < 1) return 0;
  return gnpde::attention_bwd_workspace_bytes(g, a->heads, a->type == GNPDE_ATT_GAT);
}

extern "C" int gnpde_edge_attention_bwd(const gnpde_graph_t* g, const gnpde_attention_t* a, const float* dw_csr, const float* scale,
                                        int32_t scale_sigmoid, float* ds_csr, void* workspace, size_t workspace_bytes, void* stream) {
  return gnpde::launch_edge_attention_bwd(g, a, dw_csr, nullptr, 0, scale, scale_sigmoid, ds_csr, workspace, workspace_bytes,
                                          static_cast<hipStream_t>(stream));
}

extern "C" int gnpde_edge_attention_bwd_heads(const gnpde_graph_t* g, const gnpde_attention_t* a, const float* datt_edge,
                                              int32_t post, float* ds_csr, void* workspace, size_t workspace_bytes, void* stream) {
  return gnpde::launch_edge_attention_bwd(g, a, nullptr, datt_edge, post, nullptr, 0, ds_csr, workspace, workspace_bytes,
                                          static_cast<hipStream_t>(stream));
}

extern "C" int gnpde_edge_to_csr_mean(const gnpde_graph_t* g, const float* src_edge, int32_t h, float* w_csr, void* stream) {
  GNPDE_CHECK_ARG(g && g->perm && src_edge && w_csr && h >= 1, GNPDE_EINVAL, "edge_to_csr_mean: bad arguments");
  if (g->e == 0) return 0;
  hipLaunchKernelGGL(gnpde::edge_to_csr_mean_kernel, dim3(gnpde::stream_grid(g->e)), dim3(gnpde::kBlock), 0,
                     static_cast<hipStream_t>(stream), g->perm, src_edge, h, g->e, w_csr);
  GNPDE_LAUNCH_CHECK();
  return 0;
}
