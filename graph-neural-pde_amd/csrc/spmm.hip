// Row-parallel CSR aggregation  ax[i] = sum_e w[e] * u[col_e]  fused with the diffusion epilogue
// f = alpha' (ax - u_i) + beta x0_i  and the fixed-step solver's stage algebra (gnpde.h).
//
// Replaces torch_sparse.spmm (index_select -> mul -> scatter_add_ with an [E,d] temporary) plus
// the elementwise tail of ODEFunc.forward (reference src/function_laplacian_diffusion.py:31-51,
// src/function_transformer_attention.py:35,46-53) and torchdiffeq's per-stage AXPY chain.
//
// Mapping (HBM/L2-gather bound, no MFMA): one 64-lane wavefront per row.  L = lanes that cover one
// neighbour's feature row (VEC floats each, K column tiles), G = 64/L neighbours are gathered by one
// wave instruction, U independent gathers are issued before the first FMA so that >= 8 x 16 B loads
// are in flight per lane.  The G partial sums are combined with an xor butterfly (deterministic, no
// atomics).  Rows longer than GNPDE_LONG_ROW are processed as independent chunks into a partial
// buffer and summed by a second small kernel, so a 13k-degree hub does not serialise on one wave.
#include <atomic>
#include "common.h"
#include "epilogue.h"

namespace gnpde {
namespace {

struct SpmmArgs {
  // work of one launch: long-row chunks [chunk_begin, chunk_end) and rows [row_begin, row_end)
  int chunk_begin, chunk_end, row_begin, row_end;
  int n, n_long_chunks;
  const int* __restrict__ rowptr;
  const int* __restrict__ colidx;
  const int* __restrict__ lc_row;
  const int* __restrict__ lc_begin;
  const int* __restrict__ lc_end;
  const float* __restrict__ w;
  const float* __restrict__ u;
  int d, ld;
  float* plain_out;      // != nullptr: write ax only (no epilogue)
  float* partial;        // [n_long_chunks, ldp]
  int ldp;
  int short_rows;        // host-side hint: at least half of the rows have <= 16 entries (-> row pairs for d = 68..128)
  int row_shift;         // rows are dealt to the XCDs in blocks of 2^row_shift rows (xcd_row); < 0: contiguous eighths
  gnpde_epilogue_t ep;
  // optional bf16 gather operand (kernels instantiated with LO): the neighbour rows come from u_lo [n, ld] instead of u (the row's
  // own term still reads u), and the epilogue stores the bf16 rounding of out_y to out_y_lo (nullable) as well
  const uint16_t* __restrict__ u_lo;
  uint16_t* out_y_lo;
  // hub rows whose softmax the attention launch left un-normalised (HubDefer, common.h; kernels instantiated with DEFER): the
  // hub-chunk items form the weights of their entries themselves and store them to w_out (the buffer `w` points to)
  const float* __restrict__ hub_part;
  const float* __restrict__ hub_scores;
  const int* __restrict__ hub_chunk_first;
  float* w_out;
  int hub_h;
  // in-kernel fold of the hub rows (row-pair kernel, epilogue launches; fold_ticket below): one arrival counter per long row, in
  // long_rows order, and the chunk list the counter's index is found in.  null: spmm_long_reduce4_kernel folds in a launch of its own.
  unsigned* tickets;
  const int* __restrict__ long_chunk_ptr;
  int n_long_rows;
};


// The per-row streaming operands of every aggregation kernel's epilogue (x0, y, k1 in; k, y out) are read and written once per
// launch: nontemporal, so that they do not evict the gathered table from L2 (cached form measured slower, profiles/r02_ab_*.log).
constexpr bool kNT = true;

// Work item of wave `lw` (index local to the XCD) of a block that runs on XCD x = blockIdx % 8.  Every XCD gets every
// 8th long-row chunk FIRST (512 entries each = the longest-running waves: they start at time 0 and overlap with
// everything else instead of forming the kernel's tail) and then its share of the rows.  (Handing the chunks out
// contiguously put all of them -- 58 % of the entries of the R-MAT graph, 10 % at the ogbn-arxiv shape -- on XCD 0: 42 ms
// instead of 18.)
//
// Rows -> XCDs (gnpde_graph_t.xcd_deal).  CONTIGUOUS: every XCD takes a contiguous eighth of the rows, so that rows that are
// neighbours in a locality-ordered graph share that XCD's 4 MiB L2.  That is only balanced when the row length does not
// depend on the row id: in an R-MAT graph the expected degree falls by a factor 0.32 with every set bit of the id, so
// the eighth with the top bits 000 holds 7.5x the entries of the eighth with 111 (8.9 M vs 1.2 M non-hub entries at the 2^21
// shape) and the launch lasts as long as XCD 0 needs: 1.46x the balanced time by the work model (entries + 3 per row, hub
// chunks included; tools/xcd_balance.py).  Real graphs have the same trait (ids in order of publication, crawl or degree).
// HASHED (chosen by the graph builder when the contiguous deal is more than 3 % out of balance): the rows are dealt in BLOCKS
// of B = 2^row_shift consecutive rows (16 .. 128: the rows of a pair, and a stretch of neighbouring rows, stay on one XCD),
// eight consecutive blocks form a group, and the eight XCDs take the blocks of group j in an order rotated by a hash of j:
// block(x, j) = 8 j + ((x + hash(j)) mod 8).  A fixed rotation (plain round robin) would keep the R-MAT skew -- it only
// selects three OTHER id bits -- the hashed one leaves 0.1 - 0.5 % (same tool).  A bijection for any hash, so every row is
// still taken exactly once; which XCD takes it does not enter the arithmetic (bit-identical results, tools/xcd_check.py).
struct Item { int row, e0, e1, chunk; bool valid; };

__device__ __forceinline__ int chunks_of_xcd(const SpmmArgs& a, int x) {
  return (a.chunk_end - a.chunk_begin + kXcds - 1 - x) / kXcds;
}
__device__ __forceinline__ int rows_per_xcd(const SpmmArgs& a) { return xcd_rows_per(a.row_end - a.row_begin, a.row_shift); }
__device__ __forceinline__ int xcd_row(const SpmmArgs& a, int x, int r) { return xcd_row_of(a.row_begin, a.row_end, a.row_shift, x, r); }

__device__ __forceinline__ Item item_of(const SpmmArgs& a, int x, int lw) {
  Item it;
  it.valid = false;
  it.chunk = -1;
  it.row = it.e0 = it.e1 = 0;
  const int cx = chunks_of_xcd(a, x);
  if (lw < cx) {
    it.chunk = a.chunk_begin + lw * kXcds + x;
    it.row = __builtin_amdgcn_readfirstlane(a.lc_row[it.chunk]);
    it.e0 = __builtin_amdgcn_readfirstlane(a.lc_begin[it.chunk]);
    it.e1 = __builtin_amdgcn_readfirstlane(a.lc_end[it.chunk]);
    it.valid = true;
    return it;
  }
  const int row = xcd_row(a, x, lw - cx);
  if (row < 0) return it;
  it.row = row;
  it.e0 = __builtin_amdgcn_readfirstlane(a.rowptr[it.row]);
  it.e1 = __builtin_amdgcn_readfirstlane(a.rowptr[it.row + 1]);
  it.valid = it.e1 - it.e0 <= GNPDE_LONG_ROW;   // longer rows are processed as chunks
  return it;
}

template <int VEC, int L, int K, int U, bool LO = false>
__global__ __launch_bounds__(kBlock) void spmm_rows_kernel(const SpmmArgs a) {
  constexpr int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int xcd = static_cast<int>(blockIdx.x % kXcds);
  const int lw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x / kXcds) * kWavesPerBlock + wave);
  const Item it = item_of(a, xcd, lw);
  if (!it.valid) return;
  const int sub = lane / L;   // neighbour slot
  const int cl = lane % L;    // column lane
  const int row = it.row, e0 = it.e0, e1 = it.e1, chunk = it.chunk;

  float acc[K][VEC];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[k][v] = 0.0f;

  for (int j = e0; j < e1; j += G * U) {
    float vals[U][K][VEC];
    float ww[U];
#pragma unroll
    for (int t = 0; t < U; ++t) {
      const int e = j + t * G + sub;
      ww[t] = 0.0f;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) vals[t][k][v] = 0.0f;
      if (e < e1) {  // masked lanes issue no memory request
        const int c = a.colidx[e];
        ww[t] = a.w[e];
        if constexpr (LO) {
          const uint16_t* src = a.u_lo + static_cast<size_t>(c) * a.ld;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const int col = (k * L + cl) * VEC;
            if (col < a.d) load_lo4(src + col, vals[t][k]);
          }
        } else {
          const float* src = a.u + static_cast<size_t>(c) * a.ld;
#pragma unroll
          for (int k = 0; k < K; ++k) {
            const int col = (k * L + cl) * VEC;
            if (col < a.d) load_vec<VEC>(src + col, vals[t][k]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < U; ++t)
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[k][v] = fmaf(ww[t], vals[t][k][v], acc[k][v]);
  }

  // combine the G neighbour slots (lanes with equal column lane)
#pragma unroll
  for (int off = L; off < kWave; off <<= 1)
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[k][v] += __shfl_xor(acc[k][v], off, kWave);

  if (sub != 0) return;

  if (chunk >= 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int col = (k * L + cl) * VEC;
      if (col < a.d) store_vec<VEC>(a.partial + static_cast<size_t>(chunk) * a.ldp + col, acc[k]);
    }
    return;  // spmm_long_reduce_kernel folds the chunks of a row in chunk order
  }
  if (a.plain_out != nullptr) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int col = (k * L + cl) * VEC;
      if (col < a.d) store_vec<VEC>(a.plain_out + static_cast<size_t>(row) * a.ld + col, acc[k]);
    }
    return;
  }
  const float alpha = alpha_of(a.ep);
  const float beta = a.ep.x0 != nullptr ? *a.ep.beta : 0.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int col = (k * L + cl) * VEC;
    if (col < a.d) {
      const size_t off = static_cast<size_t>(row) * a.ld + col;
      float ui[VEC];
      load_vec<VEC>(a.u + off, ui);
      epilogue<VEC, kNT, LO>(a.ep, alpha, beta, off, acc[k], ui, a.out_y_lo);
    }
  }
}

// One block per long row: sum its chunk partials in chunk order, then the epilogue.
__global__ __launch_bounds__(kBlock) void spmm_long_reduce_kernel(const SpmmArgs a, const int* __restrict__ long_rows,
                                                                 const int* __restrict__ long_chunk_ptr) {
  const int lr = blockIdx.x;
  const int row = long_rows[lr];
  const int c0 = long_chunk_ptr[lr], c1 = long_chunk_ptr[lr + 1];
  if (row < a.row_begin) return;   // a launch over rows [row_begin, n) writes no other row
  const bool plain = a.plain_out != nullptr;
  const float alpha = plain ? 0.0f : alpha_of(a.ep);
  const float beta = (!plain && a.ep.x0 != nullptr) ? *a.ep.beta : 0.0f;
  for (int col = threadIdx.x; col < a.d; col += blockDim.x) {
    float s = 0.0f;
    for (int c = c0; c < c1; ++c) s += a.partial[static_cast<size_t>(c) * a.ldp + col];
    const size_t off = static_cast<size_t>(row) * a.ld + col;
    if (plain) {
      a.plain_out[off] = s;
    } else {
      const float ax[1] = {s};
      const float ui[1] = {a.u[off]};
      epilogue<1, false>(a.ep, alpha, beta, off, ax, ui);
    }
  }
}


// ------------------------------------------------------------------------------------------------
// Wide-row variant (state widths whose row fits ONE wave instruction: d <= 64 VEC).  Differences from
// spmm_rows_kernel, all aimed at the HBM-bound shapes (RMAT, d = 256: 1-KB rows, table >> Infinity Cache):
//  * the column ids and weights of up to 64 entries are fetched by ONE coalesced load per wave (lane = entry)
//    and handed to the gather loop by v_readlane (G == 1: the neighbour is wave-uniform, so the row base
//    address lives in SGPRs and the gather is `global_load_dwordx4 v, v_off, s[base]`) or by ds_bpermute
//    (G > 1), instead of every lane group re-loading them: the dependent chain per 64 entries is
//    index load -> U gathers, not (index load -> gather) x 64/(G U);
//  * the per-row streaming operands of the epilogue (u_i, x0_i, y_i, k1_i) are requested BEFORE the gather
//    loop, so their latency overlaps the gathers instead of extending the wave's life;
//  * one wavefront per workgroup, so a finished wave frees its slot at once (rows of a power-law graph differ
//    by 100x in length; with 4 waves per workgroup the slots of the short ones idle until the longest is done).
// Same work items, same summation order inside a row (entries in CSR order, G slots combined by the xor
// butterfly), same epilogue arithmetic.
// ------------------------------------------------------------------------------------------------
template <int VEC, bool NT>
struct Pre {   // epilogue operands requested ahead of the gather loop
  float ui[VEC], x0[VEC], y[VEC], k1[VEC];
};

// THE list of stages whose operands are requested ahead of the gather loop (epilogue_pre) and that fold_stage states float by float:
// the kernels, both folds and the launch plan (which lets the row-pair kernel fold a hub row only for these) ask here
constexpr __host__ __device__ bool stage_prefetchable(int stage) {
  return stage == GNPDE_STAGE_RHS || stage == GNPDE_STAGE_EULER || (stage >= GNPDE_STAGE_RK1C && stage <= GNPDE_STAGE_RK4C);
}

// k = alpha (ax - u_i) + beta x0_i and the compact / euler / plain stages from operands already in registers
template <int VEC, bool NT, bool LO = false>
__device__ __forceinline__ void epilogue_pre(const gnpde_epilogue_t& ep, float alpha, float beta, size_t off,
                                             const float (&ax)[VEC], const Pre<VEC, NT>& p, uint16_t* lo = nullptr) {
  auto st = [](float* q, const float (&v)[VEC]) { if constexpr (NT) store_vec_nt<VEC>(q, v); else store_vec<VEC>(q, v); };
  constexpr float kThird = 1.0f / 3.0f;
  float k[VEC], o[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) k[v] = alpha * (ax[v] - p.ui[v]);
  if (ep.x0 != nullptr) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) k[v] = k[v] + beta * p.x0[v];
  }
  const float dt = ep.dt;
  switch (ep.stage) {
    case GNPDE_STAGE_RHS:
      st(ep.out_k + off, k);
      break;
    case GNPDE_STAGE_EULER:
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = p.y[v] + dt * k[v];
      st(ep.out_y + off, o);
      if constexpr (LO) store_lo<VEC>(lo, off, o);
      break;
    case GNPDE_STAGE_RK1C:
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = p.ui[v] + (dt * k[v]) * kThird;
      st(ep.out_y + off, o);
      if constexpr (LO) store_lo<VEC>(lo, off, o);
      break;
    case GNPDE_STAGE_RK2C:
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = (2.0f * p.y[v] - p.ui[v]) + dt * k[v];
      st(ep.out_y + off, o);
      if constexpr (LO) store_lo<VEC>(lo, off, o);
      break;
    case GNPDE_STAGE_RK3C:
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = (2.0f * p.k1[v] - p.ui[v]) + dt * k[v];
      st(ep.out_y + off, o);
      if constexpr (LO) store_lo<VEC>(lo, off, o);
      break;
    case GNPDE_STAGE_RK4C:
#pragma unroll
      for (int v = 0; v < VEC; ++v) o[v] = (((6.0f * p.k1[v] + 3.0f * p.ui[v]) - p.y[v]) + dt * k[v]) * 0.125f;
      st(ep.out_y + off, o);
      if constexpr (LO) store_lo<VEC>(lo, off, o);
      break;
    default:
      break;
  }
}


// The long-row fold on 16-byte lanes: one wavefront per long row, the epilogue operands requested before the chunk loop and the
// chunk partials fetched eight at a time (the scalar kernel above walks a chain of dependent-latency loads: 8.4 us for the 204
// hub rows of the ogbn-arxiv shape, 99 us for the 27 896 of the R-MAT shape).  Same summation: the chunks of a row in chunk order.
//
// One body (fold_long_row) for the fold launch and for the last-arriving chunk item of the row-pair kernel (fold_ticket): the same loads in
// the same order, the same float sequence (fold_stage), the same bits.  HANDOFF: the partials were published by other waves of the SAME
// launch -- they are read past this CU's L1 (agent-scope relaxed 8-byte loads: global_load_dwordx2 sc1), never by a plain load.
template <bool HANDOFF>
__device__ __forceinline__ void load_partial4(const float* p, float (&v)[4]) {
  if constexpr (HANDOFF) {
    const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
    const unsigned long long lo = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v[0] = __uint_as_float(static_cast<unsigned>(lo));
    v[1] = __uint_as_float(static_cast<unsigned>(lo >> 32));
    v[2] = __uint_as_float(static_cast<unsigned>(hi));
    v[3] = __uint_as_float(static_cast<unsigned>(hi >> 32));
  } else {
    load_vec<4>(p, v);
  }
}

// The prefetchable stages on a folded hub row with every rounding written out.  epilogue_pre leaves the contraction of a x + b y to the
// compiler, whose choice depends on the code around it -- the same source inlined in the fold launch and in the row-pair kernel gave sums
// one ulp apart -- and what it chose for the fold launch was not even uniform across the four floats of a lane.  A body that is inlined
// in two places must not depend on where it is inlined, and the stored results hold the fold launch's sequence, so that sequence is
// stated here float by float (v = position in the lane's 16 bytes).  Compared once with the launch as it was before this body existed,
// bit for bit on every hub row: RHS, EULER and RK1C..RK4C, each with and without x0, at d = 128 and d = 96, on the whole-graph route and
// behind the wide-row kernel (d = 256); the stages outside this list (classic rk4) still take epilogue<> and were compared the same way:
//   k      = fma(beta, x0, rn(alpha (ax - u)))                        (no x0: the rounded product)
//   EULER  = fma(dt, k, y)            RK1C = fma(rn(dt k), 1/3, u)
//   RK2C   = (2 y - u) + dt k         fused but for v = 0: rn(2 y - u) + rn(dt k)
//   RK3C   = (2 k1 - u) + dt k        fused for v = 1, 2; v = 0, 3: rn(2 k1 - u) + rn(dt k)
//   RK4C   = (fma(dt, k, t - y)) / 8  t = rn(3 u) + rn(6 k1) for v = 0, 3; fma(3, u, rn(6 k1)) for v = 1; fma(6, k1, rn(3 u)) for v = 2
__device__ __forceinline__ void fold_stage(const gnpde_epilogue_t& ep, float alpha, float beta, size_t off, const float (&ax)[4],
                                           const Pre<4, false>& p) {
  const float dt = ep.dt;
  float o[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    float k = __fmul_rn(alpha, __fsub_rn(ax[v], p.ui[v]));
    if (ep.x0 != nullptr) k = fmaf(beta, p.x0[v], k);
    float t;
    switch (ep.stage) {
      case GNPDE_STAGE_EULER:
        o[v] = fmaf(dt, k, p.y[v]);
        break;
      case GNPDE_STAGE_RK1C:
        o[v] = fmaf(__fmul_rn(dt, k), 1.0f / 3.0f, p.ui[v]);
        break;
      case GNPDE_STAGE_RK2C:
        t = __fsub_rn(__fmul_rn(2.0f, p.y[v]), p.ui[v]);
        o[v] = v == 0 ? __fadd_rn(t, __fmul_rn(dt, k)) : fmaf(dt, k, t);
        break;
      case GNPDE_STAGE_RK3C:
        t = __fsub_rn(__fmul_rn(2.0f, p.k1[v]), p.ui[v]);
        o[v] = (v == 0 || v == 3) ? __fadd_rn(t, __fmul_rn(dt, k)) : fmaf(dt, k, t);
        break;
      case GNPDE_STAGE_RK4C:
        if (v == 1) t = fmaf(3.0f, p.ui[v], __fmul_rn(6.0f, p.k1[v]));
        else if (v == 2) t = fmaf(6.0f, p.k1[v], __fmul_rn(3.0f, p.ui[v]));
        else t = __fadd_rn(__fmul_rn(3.0f, p.ui[v]), __fmul_rn(6.0f, p.k1[v]));
        o[v] = __fmul_rn(fmaf(dt, k, __fsub_rn(t, p.y[v])), 0.125f);
        break;
      default:      // GNPDE_STAGE_RHS
        o[v] = k;
        break;
    }
  }
  store_vec<4>((ep.stage == GNPDE_STAGE_RHS ? ep.out_k : ep.out_y) + off, o);
}

// fp32 table.  HANDOFF (the row-pair kernel's last arriver): prefetchable stages only -- the launch plan keeps the fold launch otherwise
template <bool HANDOFF>
__device__ __forceinline__ void fold_long_row(const SpmmArgs& a, int row, int c0, int c1, int lane) {
  constexpr int VEC = 4;
  const bool plain = a.plain_out != nullptr;
  const float alpha = plain ? 0.0f : alpha_of(a.ep);
  const float beta = (!plain && a.ep.x0 != nullptr) ? *a.ep.beta : 0.0f;
  const bool pre_ok = !plain && stage_prefetchable(a.ep.stage);
  for (int col = lane * VEC; col < a.d; col += kWave * VEC) {
    const size_t off = static_cast<size_t>(row) * a.ld + col;
    Pre<VEC, false> pre;
    if (pre_ok) {
      load_vec<VEC>(a.u + off, pre.ui);
      if (a.ep.x0 != nullptr) load_vec<VEC>(a.ep.x0 + off, pre.x0);
      const int st = a.ep.stage;
      if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) load_vec<VEC>(a.ep.y + off, pre.y);
      if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) load_vec<VEC>(a.ep.k1 + off, pre.k1);
    }
    float acc[VEC] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* p = a.partial + static_cast<size_t>(c0) * a.ldp + col;
    int c = c0;
    for (; c + 8 <= c1; c += 8, p += 8 * static_cast<size_t>(a.ldp)) {
      float v[8][VEC];
#pragma unroll
      for (int t = 0; t < 8; ++t) load_partial4<HANDOFF>(p + t * static_cast<size_t>(a.ldp), v[t]);
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] += v[t][q];
    }
    for (; c < c1; ++c, p += a.ldp) {
      float v[VEC];
      load_partial4<HANDOFF>(p, v);
#pragma unroll
      for (int q = 0; q < VEC; ++q) acc[q] += v[q];
    }
    if (pre_ok) {
      fold_stage(a.ep, alpha, beta, off, acc, pre);
      continue;
    }
    if constexpr (!HANDOFF) {
      if (plain) {
        store_vec<VEC>(a.plain_out + off, acc);
      } else {
        float ui[VEC];
        load_vec<VEC>(a.u + off, ui);
        epilogue<VEC, false, false>(a.ep, alpha, beta, off, acc, ui, nullptr);
      }
    }
  }
}

// fp32 table: fold_long_row.  bf16 gather operand (never folded inside the aggregation launch): the fold as this launch always had it, in
// its own text, so that its compiled float sequence stays what it was.
template <bool LO>
__global__ __launch_bounds__(kWave) void spmm_long_reduce4_kernel(const SpmmArgs a, const int* __restrict__ long_rows,
                                                                 const int* __restrict__ long_chunk_ptr) {
  constexpr int VEC = 4;
  const int lr = blockIdx.x;
  const int row = long_rows[lr];
  const int c0 = long_chunk_ptr[lr], c1 = long_chunk_ptr[lr + 1];
  if (row < a.row_begin) return;   // a launch over rows [row_begin, n) writes no other row
  if constexpr (!LO) {
    fold_long_row<false>(a, row, c0, c1, static_cast<int>(threadIdx.x));
  } else {
    const bool plain = a.plain_out != nullptr;
    const float alpha = plain ? 0.0f : alpha_of(a.ep);
    const float beta = (!plain && a.ep.x0 != nullptr) ? *a.ep.beta : 0.0f;
    const bool pre_ok = !plain && stage_prefetchable(a.ep.stage);
    for (int col = static_cast<int>(threadIdx.x) * VEC; col < a.d; col += kWave * VEC) {
      const size_t off = static_cast<size_t>(row) * a.ld + col;
      Pre<VEC, false> pre;
      if (pre_ok) {
        load_vec<VEC>(a.u + off, pre.ui);
        if (a.ep.x0 != nullptr) load_vec<VEC>(a.ep.x0 + off, pre.x0);
        const int st = a.ep.stage;
        if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) load_vec<VEC>(a.ep.y + off, pre.y);
        if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) load_vec<VEC>(a.ep.k1 + off, pre.k1);
      }
      float acc[VEC] = {0.0f, 0.0f, 0.0f, 0.0f};
      const float* p = a.partial + static_cast<size_t>(c0) * a.ldp + col;
      int c = c0;
      for (; c + 8 <= c1; c += 8, p += 8 * static_cast<size_t>(a.ldp)) {
        float v[8][VEC];
#pragma unroll
        for (int t = 0; t < 8; ++t) load_vec<VEC>(p + t * static_cast<size_t>(a.ldp), v[t]);
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
          for (int q = 0; q < VEC; ++q) acc[q] += v[t][q];
      }
      for (; c < c1; ++c, p += a.ldp) {
        float v[VEC];
        load_vec<VEC>(p, v);
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] += v[q];
      }
      if (plain) {
        store_vec<VEC>(a.plain_out + off, acc);
      } else if (pre_ok) {
        epilogue_pre<VEC, false, true>(a.ep, alpha, beta, off, acc, pre, a.out_y_lo);
      } else {
        float ui[VEC];
        load_vec<VEC>(a.u + off, ui);
        epilogue<VEC, false, true>(a.ep, alpha, beta, off, acc, ui, a.out_y_lo);
      }
    }
  }
}

// The fold without a launch of its own (row-pair kernel, epilogue launches with SpmmArgs::tickets).  A hub-chunk item publishes its partial
// so that it leaves the XCD (agent-scope relaxed 8-byte stores: write-through, sc1), drains its stores, and adds one to the ticket of its
// row: one unsharded counter per row, so the wave whose add returns n_chunks - 1 knows that every other chunk of the row was published
// before its own add was -- it is the row's consumer and folds.  Every other wave ends: nothing polls, spins or waits for another wave.
// The consumer loads the partials only after its add has returned, behind an agent-scope acquire (twelve one-wave workgroups share a CU
// here, so its L1 is not known to be free of these lines), with loads that pass L1 (load_partial4<true>); it puts its ticket back to 0,
// so the next launch -- a replay of a captured solve, or the next evaluation -- needs no memset in between.  No release fence anywhere:
// a fence per chunk wave writes back the XCD's dirty L2 lines (the gathered state's epilogue outputs) and cost 1.7x on the whole launch.
// Index of the row in long_rows order: the chunk lists are in that order, so it is the position of the row's first chunk c0 in
// long_chunk_ptr -- halved by scalar loads until 64 candidates are left, which one load per lane and a ballot settle.
__device__ __forceinline__ int long_row_index(const SpmmArgs& a, int c0, int lane) {
  int lo = 0, hi = a.n_long_rows;     // long_chunk_ptr[lo] <= c0 < long_chunk_ptr[hi]
  while (hi - lo > kWave) {
    const int mid = (lo + hi) >> 1;
    if (__builtin_amdgcn_readfirstlane(a.long_chunk_ptr[mid]) <= c0) lo = mid; else hi = mid;
  }
  const int i = lo + lane;
  const bool le = i < hi && a.long_chunk_ptr[i] <= c0;
  return lo + static_cast<int>(__popcll(__ballot(le))) - 1;
}

// returns true for the wave that goes on to fold the row [c0, c0 + nch)
__device__ __forceinline__ bool fold_ticket(const SpmmArgs& a, int c0, int nch, int lane) {
  const int lr = long_row_index(a, c0, lane);
  // the stores of every lane of this wave have left for memory before the one add that signals for them (written as inline assembly:
  // a wait the compiler can prove redundant from its own scoreboard is dropped)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(a.tickets + lr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  old = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(old)));
  if (old != static_cast<unsigned>(nch - 1)) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (lane == 0) __hip_atomic_store(a.tickets + lr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

__device__ __forceinline__ void store_partial4(float* p, const float (&v)[4]) {
  unsigned long long* q = reinterpret_cast<unsigned long long*>(p);
  __hip_atomic_store(q, static_cast<unsigned long long>(__float_as_uint(v[0])) | (static_cast<unsigned long long>(__float_as_uint(v[1])) << 32),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(q + 1, static_cast<unsigned long long>(__float_as_uint(v[2])) | (static_cast<unsigned long long>(__float_as_uint(v[3])) << 32),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// DEFER: the weights of a hub chunk's entries from the stored scores and the chunk statistics of the chunk's row -- the float sequence of
// hub_normalise_body (attention.hip), so the same bits: per head the maximum over the row's chunks, l += sum_c * expf(max_c - m) in
// chunk order, rcp(l + 1e-16f); per entry the sum over the heads of exp2((s - m) log2 e) * rcp in head order, then / h -- both sums as
// the fused multiply-adds the compiler contracts them to there (written out here: left to the compiler, the four-head form below
// became packed multiplications and separate additions, one ulp away on some entries).  Every lane
// folds the statistics of head lane % h (h <= 8: the same addresses across the wave, one dependent chain per wave, before the first
// gather of a 512-entry item); an entry's lane fetches them by head.  No cross-block dependency: the attention launch has ended.
struct HubStat { float m, rinv; };
__device__ __forceinline__ HubStat hub_row_stat(const SpmmArgs& a, int chunk, int row, int lane) {
  const int h = a.hub_h, head = lane % h;
  const int c0 = __builtin_amdgcn_readfirstlane(a.hub_chunk_first[chunk]);
  const int nch = (__builtin_amdgcn_readfirstlane(a.rowptr[row + 1]) - __builtin_amdgcn_readfirstlane(a.rowptr[row]) + GNPDE_LONG_ROW - 1) /
                  GNPDE_LONG_ROW;
  const float* q0 = a.hub_part + static_cast<size_t>(c0) * 2 * h;
  // four chunks per trip, their loads issued together (a slot past the end re-reads the row's last chunk: a maximum taken twice changes
  // nothing, its share of the sum is skipped): written chunk by chunk every statistic was a dependent round trip of its own, up to
  // 2 x 26 of them in front of the first gather of the largest hub's items
  constexpr int B = 4;
  float m = -INFINITY;
  for (int i0 = 0; i0 < nch; i0 += B) {
    float v[B];
#pragma unroll
    for (int j = 0; j < B; ++j) v[j] = q0[(i0 + j < nch ? i0 + j : nch - 1) * 2 * h + head];
#pragma unroll
    for (int j = 0; j < B; ++j) m = fmaxf(m, v[j]);
  }
  float l = 0.f;
  for (int i0 = 0; i0 < nch; i0 += B) {
    float mx[B], sm[B];
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const float* q = q0 + (i0 + j < nch ? i0 + j : nch - 1) * 2 * h;
      mx[j] = q[head];
      sm[j] = q[h + head];
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const float t = fmaf(sm[j], expf(mx[j] - m), l);
      l = i0 + j < nch ? t : l;
    }
  }
  HubStat st;
  st.m = m;
  st.rinv = __builtin_amdgcn_rcpf(l + 1e-16f);
  return st;
}
// weight of entry p (a valid position for EVERY lane: the statistics travel by cross-lane reads)
__device__ __forceinline__ float hub_entry_weight(const SpmmArgs& a, const HubStat& st, int p) {
  const int h = a.hub_h;
  float acc = 0.f;
  if (h == 4) {    // (wave-uniform) the headline head count: one 16-byte load of the entry's scores
    const float4 sc = *reinterpret_cast<const float4*>(a.hub_scores + static_cast<size_t>(p) * 4);
    acc = fmaf(__builtin_amdgcn_exp2f((sc.x - __shfl(st.m, 0, kWave)) * 1.44269504088896341f), __shfl(st.rinv, 0, kWave), acc);
    acc = fmaf(__builtin_amdgcn_exp2f((sc.y - __shfl(st.m, 1, kWave)) * 1.44269504088896341f), __shfl(st.rinv, 1, kWave), acc);
    acc = fmaf(__builtin_amdgcn_exp2f((sc.z - __shfl(st.m, 2, kWave)) * 1.44269504088896341f), __shfl(st.rinv, 2, kWave), acc);
    acc = fmaf(__builtin_amdgcn_exp2f((sc.w - __shfl(st.m, 3, kWave)) * 1.44269504088896341f), __shfl(st.rinv, 3, kWave), acc);
  } else {
    for (int head = 0; head < h; ++head)
      acc = fmaf(__builtin_amdgcn_exp2f((a.hub_scores[static_cast<size_t>(p) * h + head] - __shfl(st.m, head, kWave)) * 1.44269504088896341f),
                 __shfl(st.rinv, head, kWave), acc);
  }
  return acc / static_cast<float>(h);
}
// ids and weights of the 64 entries at `base` of an item: the weights from memory, or formed (and stored) here for a hub chunk
template <bool DEFER>
__device__ __forceinline__ float item_weight(const SpmmArgs& a, const HubStat& hs, int chunk, int me, bool in, int e1) {
  if constexpr (DEFER) {
    if (chunk >= 0) {    // wave-uniform
      const float w = hub_entry_weight(a, hs, in ? me : e1 - 1);
      if (in) a.w_out[me] = w;
      return in ? w : 0.0f;
    }
  }
  return in ? a.w[me] : 0.0f;
}

// U gathers of one wave (G neighbours each) from the 64 (column id, weight) pairs held one per lane in cv / wv.
// G == 1: the entry is wave-uniform -> v_readlane, row base address in SGPRs.  TAIL: entries >= cnt are skipped.
template <int VEC, int L, int U, bool TAIL, bool FULL, bool LO = false>
__device__ __forceinline__ void gather_batch(const SpmmArgs& a, int cv, float wv, int t0, int cnt, int sub, int col,
                                             bool col_ok_rt, float (&acc)[VEC]) {
  const bool col_ok = FULL ? true : col_ok_rt;   // FULL: d == L * VEC, no column predicate
  constexpr int G = kWave / L;
  float vals[U][VEC];
  float ww[U];
  int cs[U];
  bool oks[U];
  // ids / weights of the whole batch first, then the row loads (one loop made the predicated tail a chain of LDS round trips)
#pragma unroll
  for (int t = 0; t < U; ++t) {
    bool ok = col_ok;
    if constexpr (G == 1) {
      const int idx = t0 + t;
      cs[t] = __builtin_amdgcn_readlane(cv, idx & (kWave - 1));
      ww[t] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wv), idx & (kWave - 1)));   // bit pattern, not a numeric conversion
      if constexpr (TAIL) ok = ok && idx < cnt;
    } else {
      const int idx = t0 + t * G + sub;
      cs[t] = __shfl(cv, idx & (kWave - 1), kWave);
      ww[t] = __shfl(wv, idx & (kWave - 1), kWave);
      if constexpr (TAIL) ok = ok && idx < cnt;
    }
    if constexpr (TAIL) ww[t] = ok ? ww[t] : 0.0f;
    oks[t] = ok;
  }
#pragma unroll
  for (int t = 0; t < U; ++t) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) vals[t][v] = 0.0f;
    if constexpr (LO) {
      const uint16_t* rowp = a.u_lo + static_cast<size_t>(cs[t]) * a.ld;
      if (oks[t]) load_lo4(rowp + col, vals[t]);
    } else {
      const float* rowp = a.u + static_cast<size_t>(cs[t]) * a.ld;
      if (oks[t]) load_vec<VEC>(rowp + col, vals[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < U; ++t)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = fmaf(ww[t], vals[t][v], acc[v]);
}

template <int VEC, int L, int U, bool FULL, bool LO = false>
__global__ __launch_bounds__(kWave) void spmm_wide_kernel(const SpmmArgs a) {
  constexpr int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane / L;   // neighbour slot
  const int cl = lane % L;    // column lane
  const int col = cl * VEC;
  const bool col_ok = FULL ? true : col < a.d;
  const int xcd = static_cast<int>(blockIdx.x % kXcds);
  int lw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x / kXcds) + static_cast<int>(threadIdx.x >> 6));
  const int stride = static_cast<int>(gridDim.x / kXcds);   // waves per XCD of this launch
  const int lw_end = chunks_of_xcd(a, xcd) + rows_per_xcd(a);
  const bool pre_ok = a.plain_out == nullptr && stage_prefetchable(a.ep.stage);
  const float alpha = a.plain_out == nullptr ? alpha_of(a.ep) : 0.0f;
  const float beta = (a.plain_out == nullptr && a.ep.x0 != nullptr) ? *a.ep.beta : 0.0f;

  // One item per wave: the grid has a wave for every item (agg_grid), so stride >= lw_end and the loop body runs once.  It stays
  // written as the loop it was when a resident grid strode over the items: as straight-line code (and as a call of shared_row_item
  // with L as a parameter) the compiler emits a different instruction stream for all eight instantiations, and this kernel is only
  // changed together with a measurement.
  for (; lw < lw_end; lw += stride) {
    const Item it = item_of(a, xcd, lw);
    if (!it.valid) break;
    const int row = it.row, e0 = it.e0, e1 = it.e1, chunk = it.chunk;
    const size_t off = static_cast<size_t>(row) * a.ld + col;

    // epilogue operands: in flight while the neighbours are gathered
    Pre<VEC, kNT> pre;
    const bool do_pre = pre_ok && chunk < 0 && sub == 0 && col_ok;
    if (do_pre) {
      auto ldp = [](const float* q, float (&v)[VEC]) { load_vec_nt<VEC>(q, v); };
      load_vec<VEC>(a.u + off, pre.ui);
      if (a.ep.x0 != nullptr) ldp(a.ep.x0 + off, pre.x0);
      const int st = a.ep.stage;
      if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) ldp(a.ep.y + off, pre.y);
      if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) ldp(a.ep.k1 + off, pre.k1);
    }

    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;

    for (int base = e0; base < e1; base += kWave) {
      const int me = base + lane;
      const bool in = me < e1;
      const int cv = in ? a.colidx[me] : 0;     // ONE coalesced load of 64 column ids ...
      const float wv = in ? a.w[me] : 0.0f;     // ... and weights per wave
      const int cnt = (e1 - base) < kWave ? (e1 - base) : kWave;   // wave-uniform
      // full batches of G*U entries without predicates (all U gathers issue back to back), then one predicated tail
      int t0 = 0;
      for (; t0 + G * U <= cnt; t0 += G * U) gather_batch<VEC, L, U, false, FULL, LO>(a, cv, wv, t0, cnt, sub, col, col_ok, acc);
      if (t0 < cnt) gather_batch<VEC, L, U, true, FULL, LO>(a, cv, wv, t0, cnt, sub, col, col_ok, acc);
    }

    // combine the G neighbour slots (lanes with equal column lane)
#pragma unroll
    for (int o = L; o < kWave; o <<= 1)
#pragma unroll
      for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o, kWave);

    if (sub != 0 || !col_ok) continue;
    if (chunk >= 0) {
      store_vec<VEC>(a.partial + static_cast<size_t>(chunk) * a.ldp + col, acc);
      continue;  // spmm_long_reduce_kernel folds the chunks of a row in chunk order
    }
    if (a.plain_out != nullptr) {
      store_vec<VEC>(a.plain_out + off, acc);
      continue;
    }
    if (pre_ok) {
      epilogue_pre<VEC, kNT, LO>(a.ep, alpha, beta, off, acc, pre, a.out_y_lo);
    } else {
      float ui[VEC];
      load_vec<VEC>(a.u + off, ui);
      epilogue<VEC, kNT, LO>(a.ep, alpha, beta, off, acc, ui, a.out_y_lo);
    }
    break;
  }
}


// ------------------------------------------------------------------------------------------------
// Row-PAIR variant of the wide-row kernel for rows of 17..32 16-byte lanes (d = 68..128, the ogbn-arxiv shape).
// There a row occupies half a wavefront, and the wide kernel lets the two halves share ONE row (two neighbour slots):
// with a median of 8 entries per row a wave then has 4 KB of neighbour rows in flight and runs its epilogue on 32 of its 64
// lanes.  Here the two halves of a wave take two CONSECUTIVE rows when both have <= 32 entries (one coalesced 32-entry index
// load each): twice the bytes in flight per wave for the same registers, half the waves, every lane busy in the epilogue.
// Each half keeps the wide kernel's summation order -- even entries into one accumulator, odd entries into a second, in
// CSR order, then even + odd -- so the result is bit-identical to the shared-row mode whatever row a row is paired with.
// A pair with a longer row falls back to the shared-row mode for its two rows in turn; hub chunks are shared-row items.
template <int VEC, int U, bool FULL, bool LO = false, bool DEFER = false>
__device__ __forceinline__ void shared_row_item(const SpmmArgs& a, int row, int e0, int e1, int chunk, int lane, int sub, int col,
                                                bool col_ok, bool pre_ok, float alpha, float beta) {
  constexpr int L = 32, G = 2;
  const size_t off = static_cast<size_t>(row) * a.ld + col;
  Pre<VEC, kNT> pre;   // epilogue operands: in flight while the neighbours are gathered
  const bool do_pre = pre_ok && chunk < 0 && sub == 0 && col_ok;
  if (do_pre) {
    auto ldp = [](const float* q, float (&v)[VEC]) { load_vec_nt<VEC>(q, v); };
    load_vec<VEC>(a.u + off, pre.ui);
    if (a.ep.x0 != nullptr) ldp(a.ep.x0 + off, pre.x0);
    const int st = a.ep.stage;
    if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) ldp(a.ep.y + off, pre.y);
    if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) ldp(a.ep.k1 + off, pre.k1);
  }
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
  HubStat hs{};
  if constexpr (DEFER) {
    if (chunk >= 0) hs = hub_row_stat(a, chunk, row, lane);
  }
  for (int base = e0; base < e1; base += kWave) {
    const int me = base + lane;
    const bool in = me < e1;
    const int cv = in ? a.colidx[me] : 0;     // ONE coalesced load of 64 column ids ...
    const float wv = item_weight<DEFER>(a, hs, chunk, me, in, e1);     // ... and weights per wave
    const int cnt = (e1 - base) < kWave ? (e1 - base) : kWave;   // wave-uniform
    // full batches of G*U entries without predicates (all U gathers issue back to back), then one predicated tail
    int t0 = 0;
    for (; t0 + G * U <= cnt; t0 += G * U) gather_batch<VEC, L, U, false, FULL, LO>(a, cv, wv, t0, cnt, sub, col, col_ok, acc);
    if (t0 < cnt) gather_batch<VEC, L, U, true, FULL, LO>(a, cv, wv, t0, cnt, sub, col, col_ok, acc);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], L, kWave);
  if constexpr (VEC == 4 && !LO) {
    if (chunk >= 0 && a.tickets != nullptr) {   // (wave-uniform) the last chunk item of a row to arrive folds the row: fold_ticket
      if (sub == 0 && col_ok) store_partial4(a.partial + static_cast<size_t>(chunk) * a.ldp + col, acc);
      const int rs = __builtin_amdgcn_readfirstlane(a.rowptr[row]), re = __builtin_amdgcn_readfirstlane(a.rowptr[row + 1]);
      const int nch = (re - rs + GNPDE_LONG_ROW - 1) / GNPDE_LONG_ROW;
      const int c0 = chunk - (e0 - rs) / GNPDE_LONG_ROW;
      if (fold_ticket(a, c0, nch, lane)) fold_long_row<true>(a, row, c0, c0 + nch, lane);
      return;
    }
  }
  if (sub != 0 || !col_ok) return;
  if (chunk >= 0) {
    store_vec<VEC>(a.partial + static_cast<size_t>(chunk) * a.ldp + col, acc);
    return;  // spmm_long_reduce_kernel folds the chunks of a row in chunk order
  }
  if (a.plain_out != nullptr) {
    store_vec<VEC>(a.plain_out + off, acc);
    return;
  }
  if (pre_ok) {
    epilogue_pre<VEC, kNT, LO>(a.ep, alpha, beta, off, acc, pre, a.out_y_lo);
  } else {
    float ui[VEC];
    load_vec<VEC>(a.u + off, ui);
    epilogue<VEC, kNT, LO>(a.ep, alpha, beta, off, acc, ui, a.out_y_lo);
  }
}

template <int VEC, bool FULL, bool LO = false, bool DEFER = false>
__global__ __launch_bounds__(kWave) void spmm_pair_kernel(const SpmmArgs a) {
  constexpr int L = 32, U = 16;   // 16 gathers in flight per half
  const int lane = threadIdx.x & (kWave - 1);
  const int half = lane >> 5;
  const int cl = lane & (L - 1);
  const int col = cl * VEC;
  const bool col_ok = FULL ? true : col < a.d;
  const int xcd = static_cast<int>(blockIdx.x % kXcds);
  const int lw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x / kXcds) + static_cast<int>(threadIdx.x >> 6));
  const bool pre_ok = a.plain_out == nullptr && stage_prefetchable(a.ep.stage);
  const float alpha = a.plain_out == nullptr ? alpha_of(a.ep) : 0.0f;
  const float beta = (a.plain_out == nullptr && a.ep.x0 != nullptr) ? *a.ep.beta : 0.0f;

  const int cx = chunks_of_xcd(a, xcd);
  if (lw < cx) {   // hub chunk first (as item_of)
    const int chunk = a.chunk_begin + lw * kXcds + xcd;
    const int row = __builtin_amdgcn_readfirstlane(a.lc_row[chunk]);
    const int e0 = __builtin_amdgcn_readfirstlane(a.lc_begin[chunk]);
    const int e1 = __builtin_amdgcn_readfirstlane(a.lc_end[chunk]);
    shared_row_item<VEC, U, FULL, LO, DEFER>(a, row, e0, e1, chunk, lane, half, col, col_ok, pre_ok, alpha, beta);
    return;
  }
  const int per = rows_per_xcd(a);
  const int r0 = 2 * (lw - cx);
  if (r0 >= per) return;
  int row = xcd_row(a, xcd, r0 + half);         // r0 is even and the blocks have an even size: both rows of a pair are consecutive
  bool have = row >= 0;
  if (!have) row = 0;
  int e0 = 0, e1 = 0;
  if (have) {
    e0 = a.rowptr[row];
    e1 = a.rowptr[row + 1];
  }
  if (e1 - e0 > GNPDE_LONG_ROW) have = false;   // processed as chunks
  const int len = have ? e1 - e0 : 0;
  const int len_a = __builtin_amdgcn_readlane(len, 0), len_b = __builtin_amdgcn_readlane(len, L);
  if (len_a > L || len_b > L) {                 // a longer row in the pair: both halves share each row in turn
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int hv = __builtin_amdgcn_readlane(static_cast<int>(have), h * L);
      if (!hv) continue;
      const int hr = __builtin_amdgcn_readlane(row, h * L);
      const int h0 = __builtin_amdgcn_readlane(e0, h * L), h1 = __builtin_amdgcn_readlane(e1, h * L);
      shared_row_item<VEC, U, FULL, LO>(a, hr, h0, h1, -1, lane, half, col, col_ok, pre_ok, alpha, beta);
    }
    return;
  }

  const size_t off = static_cast<size_t>(row) * a.ld + col;
  Pre<VEC, kNT> pre;
  const bool mine = have && col_ok;
  if (pre_ok && mine) {
    auto ldp = [](const float* q, float (&v)[VEC]) { load_vec_nt<VEC>(q, v); };
    load_vec<VEC>(a.u + off, pre.ui);
    if (a.ep.x0 != nullptr) ldp(a.ep.x0 + off, pre.x0);
    const int st = a.ep.stage;
    if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) ldp(a.ep.y + off, pre.y);
    if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) ldp(a.ep.k1 + off, pre.k1);
  }
  const bool in = cl < len;
  const int cv = in ? a.colidx[e0 + cl] : 0;     // the whole row: one coalesced load per half
  const float wv = in ? a.w[e0 + cl] : 0.0f;
  const int cmax = len_a > len_b ? len_a : len_b;
  float acc0[VEC], acc1[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc0[v] = acc1[v] = 0.0f;
  for (int t0 = 0; t0 < cmax; t0 += U) {
    float vals[U][VEC];
    float ww[U];
    // (round 3) all ids / weights of the batch are handed out FIRST, then the row loads: written as one loop, the compiler
    // emitted bpermute, bpermute, wait, predicated load per entry -- sixteen LDS round trips between the first and the last
    // gather of a wave
    int cs[U];
#pragma unroll
    for (int t = 0; t < U; ++t) {
      const int idx = t0 + t;                    // < 32 (cmax <= 32, U divides 32)
      cs[t] = __shfl(cv, (half << 5) + idx, kWave);
      const float w = __shfl(wv, (half << 5) + idx, kWave);
      ww[t] = (col_ok && idx < len) ? w : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < U; ++t) {
      const bool ok = col_ok && t0 + t < len;
#pragma unroll
      for (int v = 0; v < VEC; ++v) vals[t][v] = 0.0f;
      if constexpr (LO) {
        if (ok) load_lo4(a.u_lo + static_cast<size_t>(cs[t]) * a.ld + col, vals[t]);
      } else {
        if (ok) load_vec<VEC>(a.u + static_cast<size_t>(cs[t]) * a.ld + col, vals[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < U; ++t) {
      if (t % 2 == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc0[v] = fmaf(ww[t], vals[t][v], acc0[v]);
      } else {
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc1[v] = fmaf(ww[t], vals[t][v], acc1[v]);
      }
    }
  }
  if (!mine) return;
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = acc0[v] + acc1[v];
  if (a.plain_out != nullptr) {
    store_vec<VEC>(a.plain_out + off, acc);
    return;
  }
  if (pre_ok) {
    epilogue_pre<VEC, kNT, LO>(a.ep, alpha, beta, off, acc, pre, a.out_y_lo);
  } else {
    float ui[VEC];
    load_vec<VEC>(a.u + off, ui);
    epilogue<VEC, kNT, LO>(a.ep, alpha, beta, off, acc, ui, a.out_y_lo);
  }
}

// ------------------------------------------------------------------------------------------------
// Row attention + aggregation in ONE kernel (scaled-dot scores, softmax over the row, head mean): what
// row_attention_sd_kernel (two launches) + spmm_wide_kernel did, per row and per wave, without the [E] weight round trip,
// the second read of the column ids and the two launch boundaries -- the attention's dependent gathers (ids -> k rows)
// now overlap with the neighbouring waves' x-row gathers instead of running as a latency-bound kernel of their own.
//   scores : lane = (entry slot, head), head fastest: the H lanes of an entry read ONE contiguous A-float row of k
//            (DK4 16-byte loads each), 64 / H entries per pass; max / sum over the slots by xor butterflies with stride H
//   weights: w_e = (1/H) sum_h exp(s_eh - m_h) / (l_h + 1e-16), summed over the H lanes of the entry, then redistributed
//            so that lane e of the wave holds the weight of entry e of the 64-entry chunk (what gather_batch expects)
//   rows with <= 64 entries keep their scores in registers; longer rows (<= 512) take an online-softmax pass over their
//   chunks (running max / sum per lane) and RECOMPUTE the scores chunk by chunk in the aggregation pass (the k rows are
//   64 B against 512 B of x per entry); hub chunks (rows > 512) take their weights from memory, written by the two small
//   hub launches of attention.hip (launch_hub_attention) before this kernel.
// ------------------------------------------------------------------------------------------------
struct AttnSpmmArgs {
  SpmmArgs s;
  const float* __restrict__ q;       // [n, ldqk] row-side projection
  const float* __restrict__ k;       // [n_cols, ldqk] column-side projection
  int ldqk;
  float inv_sqrt_dk;
  const float* __restrict__ edge_w;  // CSR order or null (reweight_attention)
};

// scores of the 64-entry chunk starting at `base` for this lane's (slot, head): PASSES = H registers, entry = p * (64/H) + slot
template <int H, int DK4>
__device__ __forceinline__ void chunk_scores(const AttnSpmmArgs& fa, int cv, int base, int cnt, int slot, int head,
                                             const float (&qv)[DK4 * 4], float (&sc)[H]) {
  constexpr int ES = kWave / H;
#pragma unroll
  for (int p = 0; p < H; ++p) {
    const int idx = p * ES + slot;
    const int c = __shfl(cv, idx, kWave);
    sc[p] = -INFINITY;
    if (idx < cnt) {
      const float* kp = fa.k + static_cast<size_t>(c) * fa.ldqk + head * (DK4 * 4);
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < DK4; ++j) {
        const float4 kv = *reinterpret_cast<const float4*>(kp + 4 * j);
        dot = fmaf(qv[4 * j + 0], kv.x, dot);
        dot = fmaf(qv[4 * j + 1], kv.y, dot);
        dot = fmaf(qv[4 * j + 2], kv.z, dot);
        dot = fmaf(qv[4 * j + 3], kv.w, dot);
      }
      float sv = dot * fa.inv_sqrt_dk;
      if (fa.edge_w != nullptr) sv *= fa.edge_w[base + idx];
      sc[p] = sv;
    }
  }
}

template <int H>
__device__ __forceinline__ float slots_max(float v) {
#pragma unroll
  for (int off = H; off < kWave; off <<= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  return v;
}
template <int H>
__device__ __forceinline__ float slots_sum(float v) {
#pragma unroll
  for (int off = H; off < kWave; off <<= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// head-mean weights from the scores and the row statistics of this lane's head; returns the weight of entry `lane`
template <int H>
__device__ __forceinline__ float chunk_weights(const float (&sc)[H], float m, float inv_l, int lane) {
  constexpr int ES = kWave / H;
  float wv = 0.f;
#pragma unroll
  for (int p = 0; p < H; ++p) {
    float a = expf(sc[p] - m) * inv_l;                 // exp(-inf) = 0 for the absent entries
#pragma unroll
    for (int off = 1; off < H; off <<= 1) a += __shfl_xor(a, off, kWave);   // sum over the H lanes of the entry
    a *= (1.0f / static_cast<float>(H));
    // entry p * ES + slot lives in the lanes slot * H ..: lane e of the wave wants entry e
    const float got = __shfl(a, (lane % ES) * H, kWave);
    if (lane / ES == p) wv = got;
  }
  return wv;
}

template <int VEC, int L, int U, int H, int DK4, bool FULL>
__global__ __launch_bounds__(kWave) void attn_spmm_kernel(const AttnSpmmArgs fa) {
  const SpmmArgs& a = fa.s;
  constexpr int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane / L, cl = lane % L;
  const int col = cl * VEC;
  const bool col_ok = FULL ? true : col < a.d;
  const int head = lane % H, slot = lane / H;
  const int xcd = static_cast<int>(blockIdx.x % kXcds);
  const int lw = static_cast<int>(blockIdx.x / kXcds);
  const Item it = item_of(a, xcd, lw);
  if (!it.valid) return;
  const int row = it.row, e0 = it.e0, e1 = it.e1, chunk = it.chunk;
  const size_t off = static_cast<size_t>(row) * a.ld + col;
  const bool pre_ok = stage_prefetchable(a.ep.stage);

  Pre<VEC, kNT> pre;
  const bool do_pre = pre_ok && chunk < 0 && sub == 0 && col_ok;
  if (do_pre) {
    auto ldp = [](const float* q, float (&v)[VEC]) { load_vec_nt<VEC>(q, v); };
    load_vec<VEC>(a.u + off, pre.ui);
    if (a.ep.x0 != nullptr) ldp(a.ep.x0 + off, pre.x0);
    const int st = a.ep.stage;
    if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) ldp(a.ep.y + off, pre.y);
    if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) ldp(a.ep.k1 + off, pre.k1);
  }

  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;

  auto aggregate = [&](int cv, float wv, int cnt) {
    int t0 = 0;
    for (; t0 + G * U <= cnt; t0 += G * U) gather_batch<VEC, L, U, false, FULL>(a, cv, wv, t0, cnt, sub, col, col_ok, acc);
    if (t0 < cnt) gather_batch<VEC, L, U, true, FULL>(a, cv, wv, t0, cnt, sub, col, col_ok, acc);
  };

  if (chunk >= 0) {                               // hub chunk: weights were written by the hub launches
    for (int base = e0; base < e1; base += kWave) {
      const int me = base + lane;
      const bool in = me < e1;
      aggregate(in ? a.colidx[me] : 0, in ? a.w[me] : 0.0f, (e1 - base) < kWave ? (e1 - base) : kWave);
    }
  } else if (e1 > e0) {
    float qv[DK4 * 4];
    {
      const float* qp = fa.q + static_cast<size_t>(row) * fa.ldqk + head * (DK4 * 4);
#pragma unroll
      for (int j = 0; j < DK4; ++j) {
        const float4 t = *reinterpret_cast<const float4*>(qp + 4 * j);
        qv[4 * j] = t.x; qv[4 * j + 1] = t.y; qv[4 * j + 2] = t.z; qv[4 * j + 3] = t.w;
      }
    }
    float sc[H];
    if (e1 - e0 <= kWave) {                       // one chunk: scores stay in registers
      const int cnt = e1 - e0;
      const int cv = lane < cnt ? a.colidx[e0 + lane] : 0;
      chunk_scores<H, DK4>(fa, cv, e0, cnt, slot, head, qv, sc);
      float m = sc[0];
#pragma unroll
      for (int p = 1; p < H; ++p) m = fmaxf(m, sc[p]);
      m = slots_max<H>(m);
      float l = 0.f;
#pragma unroll
      for (int p = 0; p < H; ++p) l += expf(sc[p] - m);
      l = slots_sum<H>(l) + 1e-16f;
      aggregate(cv, chunk_weights<H>(sc, m, 1.0f / l, lane), cnt);
    } else {                                      // 65 .. 512 entries: online statistics, then recompute per chunk
      float m = -INFINITY, l = 0.f;
      for (int base = e0; base < e1; base += kWave) {
        const int cnt = (e1 - base) < kWave ? (e1 - base) : kWave;
        const int cv = lane < cnt ? a.colidx[base + lane] : 0;
        chunk_scores<H, DK4>(fa, cv, base, cnt, slot, head, qv, sc);
        float mc = sc[0];
#pragma unroll
        for (int p = 1; p < H; ++p) mc = fmaxf(mc, sc[p]);
        if (mc > m) {                             // (mc == -inf only for lanes without entries in this chunk)
          l *= expf(m - mc);
          m = mc;
        }
        if (m > -INFINITY) {
#pragma unroll
          for (int p = 0; p < H; ++p) l += expf(sc[p] - m);
        }
      }
      const float mrow = slots_max<H>(m);
      l = slots_sum<H>(m > -INFINITY ? l * expf(m - mrow) : 0.f) + 1e-16f;
      const float inv_l = 1.0f / l;
      for (int base = e0; base < e1; base += kWave) {
        const int cnt = (e1 - base) < kWave ? (e1 - base) : kWave;
        const int cv = lane < cnt ? a.colidx[base + lane] : 0;
        chunk_scores<H, DK4>(fa, cv, base, cnt, slot, head, qv, sc);
        aggregate(cv, chunk_weights<H>(sc, mrow, inv_l, lane), cnt);
      }
    }
  }

#pragma unroll
  for (int o = L; o < kWave; o <<= 1)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o, kWave);

  if (sub != 0 || !col_ok) return;
  if (chunk >= 0) {
    store_vec<VEC>(a.partial + static_cast<size_t>(chunk) * a.ldp + col, acc);
    return;
  }
  const float alpha = alpha_of(a.ep);
  const float beta = a.ep.x0 != nullptr ? *a.ep.beta : 0.0f;
  if (pre_ok) {
    epilogue_pre<VEC, kNT>(a.ep, alpha, beta, off, acc, pre);
  } else {
    float ui[VEC];
    load_vec<VEC>(a.u + off, ui);
    epilogue<VEC, kNT>(a.ep, alpha, beta, off, acc, ui);
  }
}

template <int H, int DK4>
bool launch_attn_spmm_hd(const AttnSpmmArgs& fa, hipStream_t st) {
  const SpmmArgs& a = fa.s;
  const int slots = (a.d + 3) / 4;
  const unsigned grid = agg_grid(a.chunk_end - a.chunk_begin, a.row_end - a.row_begin, a.row_shift, 1, 1);
#define GNPDE_AS(LL)                                                                                                     \
  if (a.d == LL * 4) hipLaunchKernelGGL((attn_spmm_kernel<4, LL, 8, H, DK4, true>), dim3(grid), dim3(kWave), 0, st, fa); \
  else hipLaunchKernelGGL((attn_spmm_kernel<4, LL, 8, H, DK4, false>), dim3(grid), dim3(kWave), 0, st, fa);
  if (slots <= 16) return false;
  if (slots <= 32) { GNPDE_AS(32) return true; }
  if (slots <= 64) { GNPDE_AS(64) return true; }
#undef GNPDE_AS
  return false;
}

// Row-QUAD form of the row-pair kernel for the bf16 gather operand: a bf16 row of d <= 128 columns is 256 bytes, so with the pair
// kernel's mapping (32 lanes x 4 elements) a lane gathers 8 bytes per neighbour.  Here 16 lanes x 8 elements cover a row -- 16-byte
// gathers again -- and the four quarters of a wave take four consecutive rows of <= 32 entries (ids and weights: two coalesced
// 16-entry loads per quarter).  Per row the summation is the pair kernel's (even entries into one accumulator, odd entries into a
// second, CSR order, then even + odd), so the results are bit-identical to it.  A quad with a longer row falls back to the
// shared-row mode (32 x 4) for its rows in turn; hub chunks are shared-row items.  Needs d % 8 == 0, ld % 8 == 0, 16-byte aligned shadows.
template <int U>
__global__ __launch_bounds__(kWave) void spmm_quad_lo_kernel(const SpmmArgs a) {
  constexpr int VEC = 4, L = 16, E = 8;
  const int lane = threadIdx.x & (kWave - 1);
  const int quarter = lane >> 4;
  const int cl = lane & (L - 1);
  const int col = cl * E;
  const bool col_ok = col < a.d;
  const int xcd = static_cast<int>(blockIdx.x % kXcds);
  const int lw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x / kXcds));
  const bool pre_ok = a.plain_out == nullptr && stage_prefetchable(a.ep.stage);
  const float alpha = a.plain_out == nullptr ? alpha_of(a.ep) : 0.0f;
  const float beta = (a.plain_out == nullptr && a.ep.x0 != nullptr) ? *a.ep.beta : 0.0f;
  // the shared-row mode keeps the 32 x 4 mapping
  const int half = lane >> 5, col4 = (lane & 31) * VEC;
  const bool col4_ok = col4 < a.d;

  const int cx = chunks_of_xcd(a, xcd);
  if (lw < cx) {   // hub chunk first (as item_of)
    const int chunk = a.chunk_begin + lw * kXcds + xcd;
    const int row = __builtin_amdgcn_readfirstlane(a.lc_row[chunk]);
    const int e0 = __builtin_amdgcn_readfirstlane(a.lc_begin[chunk]);
    const int e1 = __builtin_amdgcn_readfirstlane(a.lc_end[chunk]);
    shared_row_item<VEC, 16, false, true>(a, row, e0, e1, chunk, lane, half, col4, col4_ok, pre_ok, alpha, beta);
    return;
  }
  const int per = rows_per_xcd(a);
  const int r0 = 4 * (lw - cx);
  if (r0 >= per) return;
  int row = xcd_row(a, xcd, r0 + quarter);
  bool have = row >= 0;
  if (!have) row = 0;
  int e0 = 0, e1 = 0;
  if (have) {
    e0 = a.rowptr[row];
    e1 = a.rowptr[row + 1];
  }
  if (e1 - e0 > GNPDE_LONG_ROW) have = false;   // processed as chunks
  const int len = have ? e1 - e0 : 0;
  int cmax = 0;
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int lh = __builtin_amdgcn_readlane(len, h * L);
    cmax = lh > cmax ? lh : cmax;
  }
  if (cmax > 2 * L) {                           // a longer row in the quad: the whole wave shares each row in turn
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int hv = __builtin_amdgcn_readlane(static_cast<int>(have), h * L);
      if (!hv) continue;
      const int hr = __builtin_amdgcn_readlane(row, h * L);
      const int h0 = __builtin_amdgcn_readlane(e0, h * L), h1 = __builtin_amdgcn_readlane(e1, h * L);
      shared_row_item<VEC, 16, false, true>(a, hr, h0, h1, -1, lane, half, col4, col4_ok, pre_ok, alpha, beta);
    }
    return;
  }

  const size_t off = static_cast<size_t>(row) * a.ld + col;
  Pre<VEC, kNT> pre[2];
  const bool mine = have && col_ok;
  if (pre_ok && mine) {
    auto ldp = [](const float* q, float (&v)[VEC]) { load_vec_nt<VEC>(q, v); };
    const int st = a.ep.stage;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const size_t o = off + h * VEC;
      load_vec<VEC>(a.u + o, pre[h].ui);
      if (a.ep.x0 != nullptr) ldp(a.ep.x0 + o, pre[h].x0);
      if (st == GNPDE_STAGE_EULER || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C) ldp(a.ep.y + o, pre[h].y);
      if (st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C) ldp(a.ep.k1 + o, pre[h].k1);
    }
  }
  // the whole row: two coalesced 16-entry loads per quarter
  const bool in0 = cl < len, in1 = L + cl < len;
  const int cv0 = in0 ? a.colidx[e0 + cl] : 0, cv1 = in1 ? a.colidx[e0 + L + cl] : 0;
  const float wv0 = in0 ? a.w[e0 + cl] : 0.0f, wv1 = in1 ? a.w[e0 + L + cl] : 0.0f;
  float acc0[E], acc1[E];
#pragma unroll
  for (int v = 0; v < E; ++v) acc0[v] = acc1[v] = 0.0f;
  static_assert(U == L, "one batch per 16-entry id register");
  for (int t0 = 0; t0 < cmax; t0 += U) {
    const int cv = t0 == 0 ? cv0 : cv1;
    const float wv = t0 == 0 ? wv0 : wv1;
    uint4 raw[U];
    float ww[U];
    int cs[U];
#pragma unroll
    for (int t = 0; t < U; ++t) {
      cs[t] = __shfl(cv, (quarter << 4) + t, kWave);
      const float w = __shfl(wv, (quarter << 4) + t, kWave);
      ww[t] = (col_ok && t0 + t < len) ? w : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < U; ++t) {
      raw[t] = make_uint4(0u, 0u, 0u, 0u);
      if (col_ok && t0 + t < len) raw[t] = *reinterpret_cast<const uint4*>(a.u_lo + static_cast<size_t>(cs[t]) * a.ld + col);
    }
#pragma unroll
    for (int t = 0; t < U; ++t) {
      const float vals[E] = {__uint_as_float(raw[t].x << 16), __uint_as_float(raw[t].x & 0xffff0000u),
                             __uint_as_float(raw[t].y << 16), __uint_as_float(raw[t].y & 0xffff0000u),
                             __uint_as_float(raw[t].z << 16), __uint_as_float(raw[t].z & 0xffff0000u),
                             __uint_as_float(raw[t].w << 16), __uint_as_float(raw[t].w & 0xffff0000u)};
      if (t % 2 == 0) {
#pragma unroll
        for (int v = 0; v < E; ++v) acc0[v] = fmaf(ww[t], vals[v], acc0[v]);
      } else {
#pragma unroll
        for (int v = 0; v < E; ++v) acc1[v] = fmaf(ww[t], vals[v], acc1[v]);
      }
    }
  }
  if (!mine) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const size_t o = off + h * VEC;
    float acc[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = acc0[h * VEC + v] + acc1[h * VEC + v];
    if (a.plain_out != nullptr) {
      store_vec<VEC>(a.plain_out + o, acc);
    } else if (pre_ok) {
      epilogue_pre<VEC, kNT, true>(a.ep, alpha, beta, o, acc, pre[h], a.out_y_lo);
    } else {
      float ui[VEC];
      load_vec<VEC>(a.u + o, ui);
      epilogue<VEC, kNT, true>(a.ep, alpha, beta, o, acc, ui, a.out_y_lo);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Host side.  What the three launchers of this file share (the graph part of SpmmArgs, the epilogue rules, the lane test), then the launch
// plan of launch_spmm_rhs: ONE decision -- lanes, kernel and template line, grid, fork, hub-row fold -- taken in plan_spmm, exported as it
// is taken by gnpde_spmm_plan (gnpde.h documents the table) and carried out by launch_planned.
// ------------------------------------------------------------------------------------------------

// The graph, state and work ranges of a launch over rows [g->row_begin, n) and all hub chunks; the chunk partials must fit the workspace.
int fill_args(SpmmArgs& a, const gnpde_graph_t* g, const float* w, const float* u, int d, int ld, void* ws, size_t ws_bytes, const char* who) {
  a.n = g->n; a.n_long_chunks = g->n_long_chunks;
  a.rowptr = g->rowptr; a.colidx = g->colidx;
  a.lc_row = g->long_chunk_row; a.lc_begin = g->long_chunk_begin; a.lc_end = g->long_chunk_end;
  a.w = w; a.u = u; a.d = d; a.ld = ld;
  a.ldp = static_cast<int>(align_up(static_cast<size_t>(d), 4));
  a.partial = static_cast<float*>(ws);
  a.chunk_begin = 0; a.chunk_end = g->n_long_chunks; a.row_begin = g->row_begin; a.row_end = g->n;
  a.row_shift = choose_row_shift(static_cast<long long>(a.row_end) - a.row_begin, g->xcd_deal);
  a.short_rows = 2LL * g->n_bin16 >= g->n ? 1 : 0;
  if (g->n_long_chunks > 0) {
    const size_t need = static_cast<size_t>(g->n_long_chunks) * a.ldp * sizeof(float);
    GNPDE_CHECK_ARG(ws != nullptr && ws_bytes >= need, GNPDE_EWS, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
  }
  return 0;
}

// An epilogue against the stages a launcher accepts (bit s: stage s) and the operands each stage reads and writes.
constexpr unsigned kStagesAll = kEpilogueStagesAll;
constexpr unsigned kStagesAdjoint = 1u << GNPDE_STAGE_LINCOMB | 1u << GNPDE_STAGE_EULER | 0xFu << GNPDE_STAGE_RK1C;
}  // namespace
// (check_epilogue and on_lanes are shared with out_proj.hip: common.h)
int check_epilogue(const char* who, const gnpde_epilogue_t& e, const void* u, unsigned accepted) {
  const int st = e.stage;
  GNPDE_CHECK_ARG(st >= GNPDE_STAGE_RHS && st <= GNPDE_STAGE_LINCOMB && (accepted >> st & 1u), GNPDE_EINVAL, "%s: bad stage %d", who, st);
  GNPDE_CHECK_ARG(e.alpha != nullptr, GNPDE_EINVAL, "%s: alpha pointer is null", who);
  GNPDE_CHECK_ARG(e.x0 == nullptr || e.beta != nullptr, GNPDE_EINVAL, "%s: x0 given without beta", who);
  if (st == GNPDE_STAGE_LINCOMB) {
    GNPDE_CHECK_ARG(e.n_prev >= 0 && e.n_prev <= GNPDE_MAX_PREV, GNPDE_EINVAL, "%s: bad n_prev %d", who, e.n_prev);
    GNPDE_CHECK_ARG(e.out_y == nullptr || e.y != nullptr, GNPDE_EINVAL, "%s: LINCOMB needs y", who);
    for (int j = 0; j < e.n_prev; ++j) GNPDE_CHECK_ARG(e.prev[j] != nullptr, GNPDE_EINVAL, "%s: LINCOMB prev[%d] is null", who, j);
  }
  const bool needs_k = st == GNPDE_STAGE_RHS || (st >= GNPDE_STAGE_RK1 && st <= GNPDE_STAGE_RK3);
  const bool needs_y = st == GNPDE_STAGE_EULER || (st >= GNPDE_STAGE_RK1 && st <= GNPDE_STAGE_RK4) || st == GNPDE_STAGE_RK2C || st == GNPDE_STAGE_RK4C;
  const bool needs_k1 = (st >= GNPDE_STAGE_RK2 && st <= GNPDE_STAGE_RK4) || st == GNPDE_STAGE_RK3C || st == GNPDE_STAGE_RK4C;
  GNPDE_CHECK_ARG(!needs_k || e.out_k != nullptr, GNPDE_EINVAL, "%s: out_k is null", who);
  GNPDE_CHECK_ARG(st == GNPDE_STAGE_RHS || st == GNPDE_STAGE_LINCOMB || e.out_y != nullptr, GNPDE_EINVAL, "%s: out_y is null", who);
  GNPDE_CHECK_ARG(!needs_y || e.y != nullptr, GNPDE_EINVAL, "%s: y is null", who);
  GNPDE_CHECK_ARG(!needs_k1 || e.k1 != nullptr, GNPDE_EINVAL, "%s: k1 is null", who);
  GNPDE_CHECK_ARG(!(st == GNPDE_STAGE_RK3 || st == GNPDE_STAGE_RK4) || e.k2 != nullptr, GNPDE_EINVAL, "%s: k2 is null", who);
  GNPDE_CHECK_ARG(st != GNPDE_STAGE_RK4 || e.k3 != nullptr, GNPDE_EINVAL, "%s: k3 is null", who);
  // every row gathers from u while other rows run their epilogue: outputs must not alias u
  GNPDE_CHECK_ARG(e.out_k != u && e.out_y != u, GNPDE_EINVAL, "%s: output aliases the gathered operand", who);
  return 0;
}

// THE lane test: the row stride and every operand of a launch -- the state, two more tables (plain output, workspace, second state) and
// whatever the epilogue reads or writes -- on lanes of `bytes` bytes (16 or 8).  The width rule (d against padded rows) is the caller's.
bool on_lanes(size_t bytes, int ld, const void* u, const void* t1, const void* t2, const gnpde_epilogue_t* e) {
  bool ok = ld % static_cast<int>(bytes / sizeof(float)) == 0 && aligned(u, bytes) && aligned(t1, bytes) && aligned(t2, bytes);
  if (e == nullptr) return ok;
  const void* ptrs[] = {e->x0, e->y, e->k1, e->k2, e->k3, e->out_k, e->out_y};
  for (const void* p : ptrs) ok = ok && aligned(p, bytes);
  if (e->stage == GNPDE_STAGE_LINCOMB)
    for (int j = 0; j < e->n_prev && j < GNPDE_MAX_PREV; ++j) ok = ok && aligned(e->prev[j], bytes);
  return ok;
}
namespace {

struct SpmmPlan {
  gnpde_spmm_launch_t l;     // what gnpde_spmm_plan reports
  int chunk_end, row_end;    // work of the launch with grid l.grid: chunks [0, chunk_end), rows [g->row_begin, row_end)
  bool pair_only;            // the route on which the row-pair kernel may be handed work that it alone does
};

// rows per wave and waves per workgroup of a planned kernel -> its grid over `chunks` hub chunks and `rows` rows
unsigned plan_grid(const gnpde_spmm_launch_t& l, long long chunks, long long rows, int row_shift) {
  const int rows_per_wave = l.family == GNPDE_SPMM_PAIR ? 2 : l.family == GNPDE_SPMM_QUAD_LO ? 4 : 1;
  return agg_grid(chunks, rows, row_shift, rows_per_wave, static_cast<int>(l.block) / kWave);
}

// THE table: one line per width class (slots = lanes of `vec` floats that cover a row); what every class takes was measured, the
// alternatives that lost are recorded in DESIGN.md section 3 and profiles/.  The bf16 gather operand (16-byte lanes only) takes the
// same line with the gather element type switched -- same work items, lane mapping and summation order, so a plain aggregation from
// a shadow is bit-identical to gnpde_spmm on the widened table.
int width_class(int vec, int d, bool short_rows, bool quad_lo, gnpde_spmm_launch_t& l) {
  const int slots = (d + vec - 1) / vec;
  auto rows = [&l](int L, int K, int U) { l.family = GNPDE_SPMM_ROWS; l.L = L; l.K = K; l.U = U; l.block = kBlock; };
  if (slots <= 8) rows(8, 1, 4);
  else if (slots <= 16) rows(16, 1, 4);
  else if (slots <= 64 && vec == 4) {
    // 16-byte lanes, rows of 17..64 lanes (d = 68..256): the wide-row kernel, 8 gathers in flight, one wavefront per workgroup --
    // measured best at the ogbn-arxiv shape (178 vs 221 us) and within 1 % of the best at the R-MAT d = 256 shape (16.6 vs
    // 16.8 ms), profiles/r02_ab_*.log.
    // Rows of 17..32 lanes (d = 68..128) in graphs whose rows are mostly short (the ogbn-arxiv shape: median 8 entries): two rows
    // per wave, 16 gathers in flight per half (spmm_pair_kernel; bit-identical results): 171 vs 184 us at the ogbn-arxiv shape,
    // 193 vs 230 us on a uniform degree-8 graph, but 2 % slower at degree 24 -- hence the hint (profiles/r02_ab_row_pairs.txt).
    // The quad form (four rows per wave from a bf16 table, GNPDE_TUNE_LO_MAPPING 2) has no FULL instantiation.
    const bool pair = slots <= 32 && short_rows;
    l.family = !pair ? GNPDE_SPMM_WIDE : quad_lo ? GNPDE_SPMM_QUAD_LO : GNPDE_SPMM_PAIR;
    l.L = l.family == GNPDE_SPMM_QUAD_LO ? 16 : slots <= 32 ? 32 : 64;
    l.K = 1;
    l.U = pair ? 16 : 8;
    l.full = l.family != GNPDE_SPMM_QUAD_LO && d == l.L * 4;
    l.block = kWave;
  }
  else if (slots <= 32) rows(16, 2, 4);
  else if (slots <= 64) rows(32, 2, 4);
  else if (slots <= 128) rows(64, 2, 2);
  else if (slots <= 192) rows(64, 3, 1);
  else if (slots <= 256) rows(64, 4, 1);
  else {
    set_error("spmm: feature width d=%d too large for %d-byte lanes (max %d)", d, 4 * vec, 256 * vec);
    return GNPDE_ESHAPE;
  }
  return 0;
}

// The plan of launch_spmm_rhs for these operands.  Operand pointers are read for their alignment and for being null, never through; of the
// options: whether there is a second stream, tickets, a bf16 operand (and its alignment), hub weights to form.
int plan_spmm(const gnpde_graph_t* g, const void* u, int d, int ld, const gnpde_epilogue_t* e, const void* plain_out, const void* ws,
              const SpmmOptions& opt, SpmmPlan* p) {
  *p = SpmmPlan{};
  gnpde_spmm_launch_t& l = p->l;
  const LoPair* lo = opt.lo != nullptr && opt.lo->u_lo != nullptr ? opt.lo : nullptr;
  // (a plain aggregation from a shadow has no fp32 table at all)
  GNPDE_CHECK_ARG(g && (u || (lo && plain_out)), GNPDE_EINVAL, "spmm: null pointer");
  GNPDE_CHECK_ARG(d >= 1 && ld >= d, GNPDE_EINVAL, "spmm: bad d=%d ld=%d", d, ld);
  GNPDE_CHECK_ARG((e != nullptr) != (plain_out != nullptr), GNPDE_EINVAL, "spmm: need exactly one of epilogue / plain output");
  if (g->n == 0) return 0;
  GNPDE_CHECK_ARG(g->n_long_chunks <= 0 || (g->long_rows && g->long_chunk_ptr && g->long_chunk_row && g->long_chunk_begin && g->long_chunk_end),
                  GNPDE_EINVAL, "spmm: long-row arrays missing");
  if (e != nullptr) {
    if (const int rc = check_epilogue("spmm", *e, u, kStagesAll)) return rc;
    GNPDE_CHECK_ARG(e->stage != GNPDE_STAGE_LINCOMB || e->out_k != nullptr || e->out_y != nullptr, GNPDE_EINVAL, "spmm: LINCOMB without output");
  } else {
    GNPDE_CHECK_ARG(plain_out != u, GNPDE_EINVAL, "spmm: output aliases the gathered operand");
  }
  // padded_rows: the caller guarantees that columns [d, ld) of every operand are padding (GNPDE_RHS_PADDED_ROWS), so a
  // width that is not a multiple of 4 still takes 16-byte lanes (the last lane reads / writes up to 3 padding columns)
  const bool a16 = (d % 4 == 0 || opt.padded_rows) && on_lanes(16, ld, u, plain_out, ws, e);
  const bool a8 = d % 2 == 0 && on_lanes(8, ld, u, plain_out, ws, e);
  l.lane_bytes = a16 ? 16 : a8 ? 8 : 4;
  const uint16_t* out_y_lo = lo != nullptr && e != nullptr ? lo->out_y_lo : nullptr;
  if (lo != nullptr) {
    l.lo = 1;
    GNPDE_CHECK_ARG(a16 && aligned(lo->u_lo, 8) && aligned(out_y_lo, 8), GNPDE_ESHAPE,
                    "spmm: the bf16 gather operand needs 16-byte lanes (d %% 4 == 0, or padded rows with ld %% 4 == 0; 16-byte aligned "
                    "operands, 8-byte aligned shadows): d=%d ld=%d", d, ld);
    GNPDE_CHECK_ARG(out_y_lo == nullptr || out_y_lo != lo->u_lo, GNPDE_EINVAL, "spmm: a stage must not write the shadow it gathers from");
  }
  // Rows and long-row chunks in one launch, then the per-row reduction of the chunk partials; with a fork the chunks + reduction
  // run as a parallel branch.  The boundary pass of a partitioned graph covers rows [row_begin, n) only (its chunks belong to those rows).
  GNPDE_CHECK_ARG(g->row_begin >= 0 && g->row_begin <= g->n, GNPDE_EINVAL, "spmm: bad row_begin %d", g->row_begin);
  const bool forked = opt.fork != nullptr && opt.fork->aux != nullptr && g->n_long_rows > 0;
  GNPDE_CHECK_ARG(!(forked && g->row_begin > 0), GNPDE_EINVAL, "spmm: fork with row_begin");
  l.forked = forked;
  const int part = g_tune[GNPDE_TUNE_SPMM_PART];           // (timing the two kinds of work items separately)
  p->chunk_end = forked || part == 2 ? 0 : g->n_long_chunks;
  p->row_end = part == 1 ? g->row_begin : g->n;
  const bool quad_lo = lo != nullptr && g_tune[GNPDE_TUNE_LO_MAPPING] == 2 && d % 8 == 0 && ld % 8 == 0 && aligned(lo->u_lo, 16) && aligned(out_y_lo, 16);
  if (const int rc = width_class(l.lane_bytes / 4, d, 2LL * g->n_bin16 >= g->n, quad_lo, l)) return rc;
  l.grid = plan_grid(l, p->chunk_end, p->row_end - g->row_begin, choose_row_shift(static_cast<long long>(g->n) - g->row_begin, g->xcd_deal));
  // THE condition for work that spmm_pair_kernel<.., LO = false> alone does -- the weights of the hub entries (HubDefer) and the hub-row
  // fold by the last chunk item to arrive (tickets): its instantiations over the whole graph, on one stream, with every work item.  The
  // wide-row kernel is left as it is: with the deferred path its instantiations need 92 - 101 VGPRs instead of 80 - 86 (a wave per SIMD
  // less for EVERY row of the launch) and spill SGPRs, for the sake of the hub chunks alone.
  p->pair_only = l.family == GNPDE_SPMM_PAIR && l.lane_bytes == 16 && !l.lo && !forked && g->row_begin == 0 && part == 0;
  const bool defer = opt.defer != nullptr && opt.defer->taken != 0 && g->n_long_rows > 0;     // (without hub rows there is no weight left to form)
  GNPDE_CHECK_ARG(!defer || p->pair_only, GNPDE_EINVAL,
                  "spmm: deferred hub weights need the row-pair kernel (16-byte lanes, d = 68..128, mostly short rows, the whole graph; d=%d ld=%d)", d, ld);
  l.defer = defer;
  // Where the row-pair kernel runs an epilogue launch and the caller gave tickets, the last chunk item of a hub row to arrive folds the
  // row inside that launch (fold_ticket: write-through partials, a drained store queue and one counter add per chunk wave; a first form
  // with an agent-scope release fence in every chunk wave was measured 1.7x slower on the whole launch, every fence writing back the
  // XCD's dirty L2 lines) and the reduction launch is not enqueued.  gnpde_agg_fold_launch(1) keeps the launch (A/B and bit reference),
  // as does every other route and every stage that fold_stage does not state.
  if (g->n_long_rows <= 0) l.fold = GNPDE_SPMM_FOLD_NONE;
  else if (opt.tickets != nullptr && e != nullptr && p->pair_only && stage_prefetchable(e->stage) && g_agg_fold_launch == 0) l.fold = GNPDE_SPMM_FOLD_IN_KERNEL;
  else l.fold = l.lo ? GNPDE_SPMM_FOLD_REDUCE4_LO : a16 ? GNPDE_SPMM_FOLD_REDUCE4 : GNPDE_SPMM_FOLD_SCALAR;
  return 0;
}

// The launch of a planned kernel: one template per family, LO = the bf16 gather operand.  Only the lines of width_class are instantiated.
template <int VEC, bool LO>
bool launch_rows(const SpmmArgs& a, const gnpde_spmm_launch_t& l, unsigned grid, hipStream_t s) {
#define GNPDE_ROWS(LL, KK, UU)                                                                                              \
  if (l.L == LL && l.K == KK && l.U == UU) {                                                                                \
    hipLaunchKernelGGL((spmm_rows_kernel<VEC, LL, KK, UU, LO>), dim3(grid), dim3(kBlock), 0, s, a);                         \
    return true;                                                                                                            \
  }
  GNPDE_ROWS(8, 1, 4) GNPDE_ROWS(16, 1, 4)
  if constexpr (VEC != 4) { GNPDE_ROWS(16, 2, 4) GNPDE_ROWS(32, 2, 4) }
  GNPDE_ROWS(64, 2, 2) GNPDE_ROWS(64, 3, 1) GNPDE_ROWS(64, 4, 1)
#undef GNPDE_ROWS
  return false;
}

template <int L, bool LO>
void launch_wide(const SpmmArgs& a, bool full, unsigned grid, hipStream_t s) {   // 8 gathers in flight, one wavefront per workgroup
  if (full) hipLaunchKernelGGL((spmm_wide_kernel<4, L, 8, true, LO>), dim3(grid), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL((spmm_wide_kernel<4, L, 8, false, LO>), dim3(grid), dim3(kWave), 0, s, a);
}

template <bool LO>
void launch_pair(const SpmmArgs& a, const gnpde_spmm_launch_t& l, unsigned grid, hipStream_t s) {
  if constexpr (!LO) {
    if (l.defer) {    // hub-chunk items that normalise their row's softmax (the row pairs: the same code)
      if (l.full) hipLaunchKernelGGL((spmm_pair_kernel<4, true, false, true>), dim3(grid), dim3(kWave), 0, s, a);
      else hipLaunchKernelGGL((spmm_pair_kernel<4, false, false, true>), dim3(grid), dim3(kWave), 0, s, a);
      return;
    }
  }
  if (l.full) hipLaunchKernelGGL((spmm_pair_kernel<4, true, LO>), dim3(grid), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL((spmm_pair_kernel<4, false, LO>), dim3(grid), dim3(kWave), 0, s, a);
}

int launch_planned(const SpmmArgs& a, const gnpde_spmm_launch_t& l, unsigned grid, hipStream_t s) {
  if (a.chunk_end <= a.chunk_begin && a.row_end <= a.row_begin) return 0;
  bool ok = true;
  switch (l.family) {
    case GNPDE_SPMM_ROWS:
      ok = l.lo ? launch_rows<4, true>(a, l, grid, s) : l.lane_bytes == 16 ? launch_rows<4, false>(a, l, grid, s) :
           l.lane_bytes == 8 ? launch_rows<2, false>(a, l, grid, s) : launch_rows<1, false>(a, l, grid, s);
      break;
    case GNPDE_SPMM_WIDE:
      if (l.L == 32) l.lo ? launch_wide<32, true>(a, l.full, grid, s) : launch_wide<32, false>(a, l.full, grid, s);
      else l.lo ? launch_wide<64, true>(a, l.full, grid, s) : launch_wide<64, false>(a, l.full, grid, s);
      break;
    case GNPDE_SPMM_PAIR:
      l.lo ? launch_pair<true>(a, l, grid, s) : launch_pair<false>(a, l, grid, s);
      break;
    case GNPDE_SPMM_QUAD_LO:
      hipLaunchKernelGGL((spmm_quad_lo_kernel<16>), dim3(grid), dim3(kWave), 0, s, a);
      break;
    default:
      ok = false;
  }
  GNPDE_CHECK_ARG(ok, GNPDE_ESTATE, "spmm: a launch plan names no kernel (family %d, L %d K %d U %d)", l.family, l.L, l.K, l.U);
  GNPDE_LAUNCH_CHECK();
  return 0;
}


// ------------------------------------------------------------------------------------------------
// One stage of the native adjoint solve, row side (csrc/adjoint.hip): the aggregation F = alpha (A u - u) + beta x0 with its
// LINCOMB stage epilogue, the SDDMM r_e = g[row] . u[col] of the SAME gathered rows, and the two dot products the scalar
// gradients need (sum g . F, sum g . x0) -- what ran as three kernels, two of which gathered every neighbour row
// (spmm_pair_kernel 187 us + sddmm_kernel 181 us + a 53-us streaming pass at the ogbn-arxiv shape).  Work items and summation
// order of the aggregation as in spmm_wide_kernel (L lanes of 16 bytes per neighbour row, G = 64 / L neighbour slots, U gathers
// in flight, slots combined by the xor butterfly).  The dot of a gathered row with g_i needs a sum over the L lanes of its slot;
// the U partial dots of a batch are reduced TOGETHER by a transposing butterfly -- at every step a lane keeps half of its values
// and hands the other half to its partner, so U values cost U - 1 + log2(L / U) shuffles instead of U log2(L), and lane
// cl ends up with the dot of entry cl / (L / U) of the batch.  r is complete per entry, so hub chunks need no second pass for it.
// ------------------------------------------------------------------------------------------------
struct AdjRowsArgs {
  SpmmArgs s;                      // graph, w, u (the state-side stage input), LINCOMB epilogue, hub-chunk partials
  const float* __restrict__ g;     // [n, ld] adjoint-side stage input
  float* __restrict__ r;           // [e] out
  float* __restrict__ dots;        // [gridDim.x + n_long_rows][2] out: per-wave sums of g . F and g . x0
  int r_accumulate;                // != 0: r[e] += (every entry belongs to exactly one lane of one launch: no race); the recorded
                                   // dopri5 backward sums the edge products of all its evaluations this way
  float r_scale;                   // weight of this launch's products in the sum (the recorded fixed-grid backward: the stage's b_j h)
  const int* __restrict__ wpos;    // or null: the weight of entry p is w[wpos[p]] (weights stored in ANOTHER graph's order: the cotangent-side
                                   // sweep runs on the transposed graph with the weights as the attention wrote them, no permutation pass)
};

template <int N, int MASK>
struct TransposeReduce {   // N values per lane -> 1, over the lane pairs (cl ^ MASK), then recursively MASK / 2
  static __device__ __forceinline__ void run(float* p, int cl) {
    constexpr int H = N / 2;
    const bool upper = (cl & MASK) != 0;
#pragma unroll
    for (int j = 0; j < H; ++j) {
      const float send = upper ? p[j] : p[j + H];
      const float keep = upper ? p[j + H] : p[j];
      p[j] = keep + __shfl_xor(send, MASK, kWave);
    }
    if constexpr (H > 1) TransposeReduce<H, MASK / 2>::run(p, cl);
  }
};

// k = alpha (ax - u_i) + beta x0_i: this lane's share of g_i . k and g_i . x0_i, then the stage algebra of the shared epilogue
// (compact rk4 / euler / LINCOMB: epilogue.h; it forms k by the same expression, the source row comes from L1 the second time)
template <int VEC>
__device__ __forceinline__ void adjoint_epilogue(const gnpde_epilogue_t& ep, float alpha, float beta, size_t off, const float (&ax)[VEC],
                                                 const float (&ui)[VEC], const float (&gi)[VEC], const float (&cmask)[VEC],
                                                 float& d1, float& d2) {
  float k[VEC], s[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) { k[v] = alpha * (ax[v] - ui[v]); s[v] = 0.f; }
  if (ep.x0 != nullptr) {
    load_vec<VEC>(ep.x0 + off, s);
#pragma unroll
    for (int v = 0; v < VEC; ++v) k[v] = k[v] + beta * s[v];
  }
  // d1: with alpha' = sigmoid(alpha_train) the dot with k (d alpha_train = (1 - sigma)(sum g . k - beta sum g . x0)); with the raw
  // alpha (opt['no_alpha_sigmoid']) the dot with A u - u itself, which IS d k / d alpha_train
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    d1 = fmaf(gi[v] * cmask[v], ep.alpha_sigmoid ? k[v] : ax[v] - ui[v], d1);
    d2 = fmaf(gi[v] * cmask[v], s[v], d2);
  }
  epilogue<VEC, true>(ep, alpha, beta, off, ax, ui);
}

// one work item (a row, or a 512-entry chunk of a hub row) by a whole wavefront: G = 64 / L neighbour slots share the row
template <int L, int U>
__device__ __forceinline__ void adjoint_item(const AdjRowsArgs& fa, int row, int e0, int e1, int chunk, int lane, float& d1, float& d2) {
  constexpr int VEC = 4;
  constexpr int G = kWave / L;
  constexpr int EPB = G * U;          // entries per batch
  constexpr int LPE = L / U;          // lanes that end up with the same entry's dot
  static_assert(U <= L && (L % U) == 0, "transposing butterfly needs U <= L");
  const SpmmArgs& a = fa.s;
  const int sub = lane / L, cl = lane % L;
  const int col = cl * VEC;
  const bool col_ok = col < a.d;
  const size_t off = static_cast<size_t>(row) * a.ld + col;
  float gi[VEC], ui[VEC], cmask[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) { gi[v] = 0.f; ui[v] = 0.f; cmask[v] = col + v < a.d ? 1.0f : 0.0f; }   // padded rows: columns [d, ld) are not data
  if (col_ok) {
    load_vec<VEC>(fa.g + off, gi);
    if (chunk < 0 && sub == 0) load_vec<VEC>(a.u + off, ui);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) gi[v] *= cmask[v];
  float acc[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
  for (int base = e0; base < e1; base += kWave) {
    const int me = base + lane;
    const bool in = me < e1;
    const int cv = in ? a.colidx[me] : 0;          // one coalesced load of 64 column ids and weights per wave
    const float wv = in ? a.w[fa.wpos != nullptr ? fa.wpos[me] : me] : 0.0f;
    const int cnt = (e1 - base) < kWave ? (e1 - base) : kWave;
    for (int t0 = 0; t0 < cnt; t0 += EPB) {
      float vals[U][VEC], ww[U], p[U];
      int cs[U];
      bool oks[U];
#pragma unroll
      for (int t = 0; t < U; ++t) {
        const int idx = t0 + t * G + sub;
        cs[t] = __shfl(cv, idx & (kWave - 1), kWave);
        const float w = __shfl(wv, idx & (kWave - 1), kWave);
        oks[t] = col_ok && idx < cnt;
        ww[t] = oks[t] ? w : 0.0f;
      }
#pragma unroll
      for (int t = 0; t < U; ++t) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) vals[t][v] = 0.0f;
        if (oks[t]) load_vec<VEC>(a.u + static_cast<size_t>(cs[t]) * a.ld + col, vals[t]);
      }
#pragma unroll
      for (int t = 0; t < U; ++t) {
        float q = 0.f;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc[v] = fmaf(ww[t], vals[t][v], acc[v]);
          q = fmaf(gi[v], vals[t][v], q);
        }
        p[t] = q;
      }
      TransposeReduce<U, L / 2>::run(p, cl);
#pragma unroll
      for (int m = LPE / 2; m >= 1; m >>= 1) p[0] += __shfl_xor(p[0], m, kWave);
      const int idx = t0 + (cl / LPE) * G + sub;
      if ((cl % LPE) == 0 && idx < cnt) {
        if (fa.r_accumulate) fa.r[base + idx] = fmaf(fa.r_scale, p[0], fa.r[base + idx]);
        else fa.r[base + idx] = p[0];
      }
    }
  }
#pragma unroll
  for (int o = L; o < kWave; o <<= 1)
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] += __shfl_xor(acc[v], o, kWave);
  if (sub == 0 && col_ok) {
    if (chunk >= 0) {
      store_vec<VEC>(a.partial + static_cast<size_t>(chunk) * a.ldp + col, acc);   // adjoint_long_reduce4_kernel folds the chunks of a row
    } else {
      const float alpha = alpha_of(a.ep);
      const float beta = a.ep.x0 != nullptr ? *a.ep.beta : 0.0f;
      adjoint_epilogue<VEC>(a.ep, alpha, beta, off, acc, ui, gi, cmask, d1, d2);
    }
  }
}

__device__ __forceinline__ void write_wave_dots(const AdjRowsArgs& fa, int lane, float d1, float d2) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    d1 += __shfl_xor(d1, o, kWave);
    d2 += __shfl_xor(d2, o, kWave);
  }
  if (lane == 0) {
    fa.dots[2 * static_cast<size_t>(blockIdx.x)] = d1;
    fa.dots[2 * static_cast<size_t>(blockIdx.x) + 1] = d2;
  }
}

template <int L, int U>
__global__ __launch_bounds__(kWave) void adjoint_rows_kernel(const AdjRowsArgs fa) {
  const SpmmArgs& a = fa.s;
  const int lane = threadIdx.x;
  const int xcd = static_cast<int>(blockIdx.x % kXcds);
  const int lw = static_cast<int>(blockIdx.x / kXcds);
  const Item it = item_of(a, xcd, lw);
  float d1 = 0.f, d2 = 0.f;
  if (it.valid) adjoint_item<L, U>(fa, it.row, it.e0, it.e1, it.chunk, lane, d1, d2);
  write_wave_dots(fa, lane, d1, d2);
}

// hub rows of the adjoint stage: chunk partials in chunk order (as spmm_long_reduce4_kernel), then the same epilogue and dots
__global__ __launch_bounds__(kWave) void adjoint_long_reduce4_kernel(const AdjRowsArgs fa, const int* __restrict__ long_rows,
                                                                    const int* __restrict__ long_chunk_ptr, int dots_base) {
  constexpr int VEC = 4;
  const SpmmArgs& a = fa.s;
  const int lr = blockIdx.x;
  const int row = long_rows[lr];
  const int c0 = long_chunk_ptr[lr], c1 = long_chunk_ptr[lr + 1];
  const float alpha = alpha_of(a.ep);
  const float beta = a.ep.x0 != nullptr ? *a.ep.beta : 0.0f;
  float d1 = 0.f, d2 = 0.f;
  for (int col = static_cast<int>(threadIdx.x) * VEC; col < a.d; col += kWave * VEC) {
    const size_t off = static_cast<size_t>(row) * a.ld + col;
    float gi[VEC], ui[VEC], cmask[VEC];
    load_vec<VEC>(fa.g + off, gi);
    load_vec<VEC>(a.u + off, ui);
#pragma unroll
    for (int v = 0; v < VEC; ++v) cmask[v] = col + v < a.d ? 1.0f : 0.0f;
    float acc[VEC] = {0.0f, 0.0f, 0.0f, 0.0f};
    const float* p = a.partial + static_cast<size_t>(c0) * a.ldp + col;
    int c = c0;
    for (; c + 8 <= c1; c += 8, p += 8 * static_cast<size_t>(a.ldp)) {
      float v[8][VEC];
#pragma unroll
      for (int t = 0; t < 8; ++t) load_vec<VEC>(p + t * static_cast<size_t>(a.ldp), v[t]);
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int q = 0; q < VEC; ++q) acc[q] += v[t][q];
    }
    for (; c < c1; ++c, p += a.ldp) {
      float v[VEC];
      load_vec<VEC>(p, v);
#pragma unroll
      for (int q = 0; q < VEC; ++q) acc[q] += v[q];
    }
    adjoint_epilogue<VEC>(a.ep, alpha, beta, off, acc, ui, gi, cmask, d1, d2);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    d1 += __shfl_xor(d1, o, kWave);
    d2 += __shfl_xor(d2, o, kWave);
  }
  if (threadIdx.x == 0) {
    fa.dots[2 * (static_cast<size_t>(dots_base) + lr)] = d1;
    fa.dots[2 * (static_cast<size_t>(dots_base) + lr) + 1] = d2;
  }
}

}  // namespace

// THE grid formula (common.h): blocks of waves_per_block waves so that every XCD can reach the end of its local list
unsigned agg_grid(long long chunks, long long rows, int row_shift, int rows_per_wave, int waves_per_block) {
  const long long per = xcd_rows_per(static_cast<int>(rows), row_shift);
  const long long waves = (chunks + kXcds - 1) / kXcds + (per + rows_per_wave - 1) / rows_per_wave;
  long long blocks = (waves + waves_per_block - 1) / waves_per_block;
  if (blocks < 1) blocks = 1;
  return static_cast<unsigned>(blocks * kXcds);
}

// Grid of the adjoint row kernel: one wavefront per work item.  (A row-PAIR form as spmm_pair_kernel -- two rows of <= 32 entries per
// wave, 16 gathers in flight per half -- was built and measured SLOWER at the ogbn-arxiv shape, 263 vs 248 us: with the 16 partial
// dots and g_i next to the 16 gathered float4s it needs 140 VGPRs, three waves per SIMD against five here; profiles/r04_train_*.)
// Number of per-wave dot slots launch_adjoint_rows writes: that grid + one per long row.
int adjoint_rows_dot_slots(const gnpde_graph_t* g, int d) {
  (void)d;
  return static_cast<int>(agg_grid(g->n_long_chunks, g->n, choose_row_shift(g->n, g->xcd_deal), 1, 1)) + g->n_long_rows;
}

int launch_adjoint_rows(const gnpde_graph_t* g, const float* w_csr, const float* u, const float* gvec, int d, int ld,
                        const gnpde_epilogue_t* epi, float* r_out, float* dots, void* ws, size_t ws_bytes, hipStream_t stream,
                        bool padded_rows, bool accumulate_r, float r_scale, const int* wpos) {
  GNPDE_CHECK_ARG(g && u && gvec && epi && r_out && dots && (w_csr || g->e == 0), GNPDE_EINVAL, "adjoint_rows: null pointer");
  if (const int rc = check_epilogue("adjoint_rows", *epi, u, kStagesAdjoint)) return rc;      // LINCOMB, euler or compact rk4
  GNPDE_CHECK_ARG(g->row_begin == 0 && d >= 1 && d <= 256 && ld >= d && ld % 4 == 0 && (d % 4 == 0 || padded_rows), GNPDE_ESHAPE,
                  "adjoint_rows: whole graphs, rows of up to 256 floats in 16-byte lanes");
  if (g->n == 0) return 0;
  AdjRowsArgs fa{};
  SpmmArgs& a = fa.s;
  if (const int rc = fill_args(a, g, w_csr, u, d, ld, ws, ws_bytes, "adjoint_rows")) return rc;
  a.ep = *epi;
  GNPDE_CHECK_ARG(on_lanes(16, ld, u, gvec, ws, epi), GNPDE_EINVAL, "adjoint_rows: operands must be 16-byte aligned");
  fa.g = gvec; fa.r = r_out; fa.dots = dots; fa.r_accumulate = accumulate_r ? 1 : 0; fa.r_scale = r_scale; fa.wpos = wpos;
  const unsigned grid = agg_grid(a.chunk_end, a.row_end, a.row_shift, 1, 1);
  const int slots = (d + 3) / 4;
  if (slots <= 16) hipLaunchKernelGGL((adjoint_rows_kernel<16, 8>), dim3(grid), dim3(kWave), 0, stream, fa);
  else if (slots <= 32) hipLaunchKernelGGL((adjoint_rows_kernel<32, 8>), dim3(grid), dim3(kWave), 0, stream, fa);
  else hipLaunchKernelGGL((adjoint_rows_kernel<64, 8>), dim3(grid), dim3(kWave), 0, stream, fa);
  GNPDE_LAUNCH_CHECK();
  if (g->n_long_rows > 0) {
    hipLaunchKernelGGL(adjoint_long_reduce4_kernel, dim3(g->n_long_rows), dim3(kWave), 0, stream, fa, g->long_rows, g->long_chunk_ptr,
                       static_cast<int>(grid));
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}

// aggregation launches whose hub rows were folded inside the row-pair kernel (gnpde_in_kernel_fold_launches)
static std::atomic<long long> g_in_kernel_folds{0};

int launch_spmm_rhs(const gnpde_graph_t* g, const float* w_csr, const float* u, int d, int ld,
                    const gnpde_epilogue_t* epi, float* plain_out, void* ws, size_t ws_bytes, hipStream_t stream, const SpmmOptions& opt) {
  GNPDE_CHECK_ARG(g && (w_csr || g->e == 0), GNPDE_EINVAL, "spmm: null pointer");
  GNPDE_CHECK_ARG(opt.tickets == nullptr || (opt.ticket_bytes >= gnpde_spmm_ticket_bytes(g) && aligned(opt.tickets, 4)), GNPDE_EWS,
                  "spmm: tickets %zu < %zu bytes (one 32-bit word per long row)", opt.ticket_bytes, gnpde_spmm_ticket_bytes(g));
  SpmmPlan plan;
  if (const int rc = plan_spmm(g, u, d, ld, epi, plain_out, ws, opt, &plan)) return rc;
  if (g->n == 0) return 0;
  const gnpde_spmm_launch_t& l = plan.l;
  SpmmArgs a{};
  if (const int rc = fill_args(a, g, w_csr, u, d, ld, ws, ws_bytes, "spmm")) return rc;
  a.plain_out = plain_out;
  if (epi) a.ep = *epi;
  if (l.lo) {
    a.u_lo = opt.lo->u_lo;
    a.out_y_lo = epi ? opt.lo->out_y_lo : nullptr;
  }
  if (l.defer) {     // the hub entries' weights do not exist yet: the planned kernel's chunk items form them
    const HubDefer* defer = opt.defer;
    GNPDE_CHECK_ARG(defer->part && defer->scores && defer->chunk_first && defer->w_out == w_csr && defer->h >= 1 && defer->h <= 8 &&
                    aligned(defer->scores, 16), GNPDE_EINVAL, "spmm: incomplete deferred hub weights (h=%d)", defer->h);
    a.hub_part = defer->part;
    a.hub_scores = defer->scores;
    a.hub_chunk_first = defer->chunk_first;
    a.w_out = defer->w_out;
    a.hub_h = defer->h;
  }
  a.chunk_end = plan.chunk_end;
  a.row_end = plan.row_end;
  if (l.fold == GNPDE_SPMM_FOLD_IN_KERNEL) {
    a.tickets = static_cast<unsigned*>(opt.tickets);
    a.long_chunk_ptr = g->long_chunk_ptr;
    a.n_long_rows = g->n_long_rows;
  }
  if (const int rc = launch_planned(a, l, l.grid, stream)) return rc;
  if (l.fold == GNPDE_SPMM_FOLD_IN_KERNEL) g_in_kernel_folds.fetch_add(1, std::memory_order_relaxed);
  if (l.fold == GNPDE_SPMM_FOLD_NONE || l.fold == GNPDE_SPMM_FOLD_IN_KERNEL) return 0;
  hipStream_t br = stream;
  if (l.forked) {
    if (const int rc = fork_begin(opt.fork, stream, &br)) return rc;
    SpmmArgs c = a;
    c.chunk_end = g->n_long_chunks;
    c.row_begin = c.row_end = 0;
    if (const int rc = launch_planned(c, l, plan_grid(l, c.chunk_end, 0, c.row_shift), br)) return rc;
  }
  if (l.fold == GNPDE_SPMM_FOLD_REDUCE4_LO)
    hipLaunchKernelGGL(spmm_long_reduce4_kernel<true>, dim3(g->n_long_rows), dim3(kWave), 0, br, a, g->long_rows, g->long_chunk_ptr);
  else if (l.fold == GNPDE_SPMM_FOLD_REDUCE4)
    hipLaunchKernelGGL(spmm_long_reduce4_kernel<false>, dim3(g->n_long_rows), dim3(kWave), 0, br, a, g->long_rows, g->long_chunk_ptr);
  else
    hipLaunchKernelGGL(spmm_long_reduce_kernel, dim3(g->n_long_rows), dim3(kBlock), 0, br, a, g->long_rows, g->long_chunk_ptr);
  GNPDE_LAUNCH_CHECK();
  return l.forked ? fork_end(opt.fork, stream, br) : 0;
}

// the route test of launch_spmm_rhs for an epilogue launch, ahead of the attention that decides on the one-launch form
bool spmm_hub_defer_supported(const gnpde_graph_t* g, const float* u, int d, int ld, const gnpde_epilogue_t& e, const void* ws,
                              bool padded_rows) {
  if (g == nullptr || u == nullptr) return false;
  SpmmOptions opt;
  opt.padded_rows = padded_rows;
  SpmmPlan plan;
  return plan_spmm(g, u, d, ld, &e, nullptr, ws, opt, &plan) == 0 && plan.pair_only;
}

bool attn_spmm_supported(const gnpde_graph_t* g, const gnpde_attention_t& at, int d, int ld, const float* u,
                         const gnpde_epilogue_t& e) {
  // Row attention inside the aggregation kernel: measured SLOWER than the separate kernels where the kernels are bound by memory
  // (ogbn-arxiv and up: DESIGN.md section 4) -- opt-in there (gnpde_tune(6, 1)); where an evaluation is bound by its LAUNCHES (a
  // state that fits one XCD's L2: Cora, 0.87 MB) one launch instead of three is the point: 7.8 us vs 5.2 + 5.2 (+ boundaries),
  // profiles/r04_cora_*.  gnpde_tune(6, 2) keeps the separate kernels there too (A/B).
  const bool small = static_cast<long long>(g->n) * ld * 4 <= (4LL << 20) && g->n_long_rows == 0;
  if (!(g_tune[GNPDE_TUNE_ROW_FUSION] == 1 || (small && g_tune[GNPDE_TUNE_ROW_FUSION] != 2))) return false;
  if (at.type != GNPDE_ATT_SCALED_DOT || at.norm_idx != 0 || at.square_plus) return false;
  const int dk = at.att_dim / at.heads;
  if (!((at.heads == 4 && dk == 4) || (at.heads == 8 && dk == 16) || (at.heads == 4 && dk == 16) || (at.heads == 2 && dk == 16)))
    return false;
  const int slots = (d + 3) / 4;
  return slots > 16 && slots <= 64 && g->row_begin == 0 && on_lanes(16, ld, u, nullptr, nullptr, &e);
}

// rows: attention + aggregation in one kernel; hub chunks aggregate with the weights in w_hub_csr (written before by
// launch_hub_attention); then the per-row fold of the chunk partials
int launch_attn_spmm(const gnpde_graph_t* g, const gnpde_attention_t* at, const float* w_hub_csr, const float* u, int d, int ld,
                     const gnpde_epilogue_t* epi, void* ws, size_t ws_bytes, hipStream_t stream, bool padded_rows) {
  GNPDE_CHECK_ARG(g && at && u && epi && at->q && at->k, GNPDE_EINVAL, "attn_spmm: null argument");
  GNPDE_CHECK_ARG(d % 4 == 0 || padded_rows, GNPDE_ESHAPE, "attn_spmm: width %d needs padded rows", d);
  if (const int rc = check_epilogue("attn_spmm", *epi, u, kStagesAll)) return rc;
  if (g->n == 0) return 0;
  AttnSpmmArgs fa{};
  SpmmArgs& a = fa.s;
  GNPDE_CHECK_ARG(g->row_begin == 0 && (g->n_long_chunks == 0 || w_hub_csr != nullptr), GNPDE_EINVAL, "attn_spmm: whole graphs, hub weights given");
  if (const int rc = fill_args(a, g, w_hub_csr, u, d, ld, ws, ws_bytes, "attn_spmm")) return rc;
  a.ep = *epi;
  fa.q = at->q; fa.k = at->k; fa.ldqk = at->ldqk;
  const int dk = at->att_dim / at->heads;
  fa.inv_sqrt_dk = 1.0f / sqrtf(static_cast<float>(dk));
  fa.edge_w = at->edge_w_csr;
  GNPDE_CHECK_ARG(at->ldqk % 4 == 0 && aligned(at->q, 16) && aligned(at->k, 16), GNPDE_EINVAL, "attn_spmm: q / k must be 16-byte aligned rows");
  bool ok = false;
  if (at->heads == 4 && dk == 4) ok = launch_attn_spmm_hd<4, 1>(fa, stream);
  else if (at->heads == 8 && dk == 16) ok = launch_attn_spmm_hd<8, 4>(fa, stream);
  else if (at->heads == 4 && dk == 16) ok = launch_attn_spmm_hd<4, 4>(fa, stream);
  else if (at->heads == 2 && dk == 16) ok = launch_attn_spmm_hd<2, 4>(fa, stream);
  GNPDE_CHECK_ARG(ok, GNPDE_ESHAPE, "attn_spmm: configuration not covered");
  GNPDE_LAUNCH_CHECK();
  if (g->n_long_rows > 0) {
    hipLaunchKernelGGL(spmm_long_reduce_kernel, dim3(g->n_long_rows), dim3(kBlock), 0, stream, a, g->long_rows, g->long_chunk_ptr);
    GNPDE_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace gnpde

extern "C" int gnpde_spmm_plan(const gnpde_graph_t* g, uint64_t u_addr, int32_t d, int32_t ld, const gnpde_epilogue_t* epi, uint64_t plain_out_addr,
                               uint64_t workspace_addr, int32_t padded_rows, uint32_t flags, gnpde_spmm_launch_t* plan) {
  GNPDE_CHECK_ARG(plan != nullptr, GNPDE_EINVAL, "spmm_plan: plan is null");
  auto ptr = [](uint64_t v) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(v)); };
  // stand-ins for what the flags say is given: the planner reads that they are there, and the alignment of the two shadows (16 bytes)
  gnpde::LoPair lo;
  lo.u_lo = reinterpret_cast<const uint16_t*>(uintptr_t{16});
  lo.out_y_lo = reinterpret_cast<uint16_t*>(uintptr_t{32});
  gnpde::Fork fork;
  fork.aux = reinterpret_cast<hipStream_t>(uintptr_t{16});
  gnpde::HubDefer defer;
  defer.taken = 1;
  gnpde::SpmmOptions opt;
  opt.padded_rows = padded_rows != 0;
  if (flags & GNPDE_SPMM_PLAN_LO) opt.lo = &lo;
  if (flags & GNPDE_SPMM_PLAN_FORK) opt.fork = &fork;
  if (flags & GNPDE_SPMM_PLAN_DEFER) opt.defer = &defer;
  if (flags & GNPDE_SPMM_PLAN_TICKETS) opt.tickets = &lo;
  gnpde::SpmmPlan p;
  const int rc = gnpde::plan_spmm(g, ptr(u_addr), d, ld, epi, ptr(plain_out_addr), ptr(workspace_addr), opt, &p);
  *plan = p.l;
  return rc;
}

extern "C" int32_t gnpde_adjoint_rows_dot_slots(const gnpde_graph_t* g, int32_t d) { return g ? gnpde::adjoint_rows_dot_slots(g, d) : 0; }

extern "C" int gnpde_xcd_row_map(int32_t row_begin, int32_t row_end, int32_t deal, int32_t* row_shift, int32_t* rows_per_xcd,
                                 int32_t* map) {
  GNPDE_CHECK_ARG(row_begin >= 0 && row_end >= row_begin && row_shift && rows_per_xcd &&
                  (deal == GNPDE_XCD_CONTIGUOUS || deal == GNPDE_XCD_HASHED), GNPDE_EINVAL, "xcd_row_map: bad arguments");
  const int shift = gnpde::choose_row_shift(static_cast<long long>(row_end) - row_begin, deal);
  const int per = gnpde::xcd_rows_per(row_end - row_begin, shift);
  *row_shift = shift;
  *rows_per_xcd = per;
  if (map != nullptr)
    for (int x = 0; x < gnpde::kXcds; ++x)
      for (int r = 0; r < per; ++r) map[static_cast<size_t>(x) * per + r] = gnpde::xcd_row_of(row_begin, row_end, shift, x, r);
  return 0;
}

extern "C" size_t gnpde_spmm_workspace_bytes(const gnpde_graph_t* g, int32_t d) {
  if (!g || d < 1) return 0;
  return static_cast<size_t>(g->n_long_chunks) * gnpde::align_up(static_cast<size_t>(d), 4) * sizeof(float);
}

extern "C" size_t gnpde_spmm_ticket_bytes(const gnpde_graph_t* g) {
  if (!g || g->n_long_rows < 0) return 0;
  return static_cast<size_t>(g->n_long_rows) * sizeof(uint32_t);
}

extern "C" int64_t gnpde_in_kernel_fold_launches(void) { return gnpde::g_in_kernel_folds.load(std::memory_order_relaxed); }

extern "C" int gnpde_spmm_rhs_tickets(const gnpde_graph_t* g, const float* w_csr, const float* u, int32_t d, int32_t ld,
                                      const gnpde_epilogue_t* epi, void* workspace, size_t workspace_bytes, void* tickets,
                                      size_t ticket_bytes, void* stream) {
  GNPDE_CHECK_ARG(epi != nullptr, GNPDE_EINVAL, "spmm_rhs: epilogue is null");
  GNPDE_CHECK_ARG(tickets != nullptr || ticket_bytes == 0, GNPDE_EINVAL, "spmm_rhs: ticket bytes without tickets");
  gnpde::SpmmOptions opt;
  opt.tickets = tickets;
  opt.ticket_bytes = ticket_bytes;
  return gnpde::launch_spmm_rhs(g, w_csr, u, d, ld, epi, nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), opt);
}

extern "C" int gnpde_spmm_rhs(const gnpde_graph_t* g, const float* w_csr, const float* u, int32_t d, int32_t ld,
                              const gnpde_epilogue_t* epi, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(epi != nullptr, GNPDE_EINVAL, "spmm_rhs: epilogue is null");
  return gnpde::launch_spmm_rhs(g, w_csr, u, d, ld, epi, nullptr, workspace, workspace_bytes,
                                static_cast<hipStream_t>(stream));
}

extern "C" int gnpde_spmm(const gnpde_graph_t* g, const float* w_csr, const float* u, int32_t d, int32_t ld,
                          float* out, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(out != nullptr, GNPDE_EINVAL, "spmm: out is null");
  return gnpde::launch_spmm_rhs(g, w_csr, u, d, ld, nullptr, out, workspace, workspace_bytes,
                                static_cast<hipStream_t>(stream));
}

extern "C" int gnpde_spmm_lo(const gnpde_graph_t* g, const float* w_csr, const void* u_lo, int32_t d, int32_t ld,
                             float* out, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(out != nullptr && u_lo != nullptr, GNPDE_EINVAL, "spmm_lo: out / u_lo is null");
  gnpde::LoPair lo;
  lo.u_lo = static_cast<const uint16_t*>(u_lo);
  gnpde::SpmmOptions opt;
  opt.padded_rows = ld % 4 == 0;
  opt.lo = &lo;
  return gnpde::launch_spmm_rhs(g, w_csr, nullptr, d, ld, nullptr, out, workspace, workspace_bytes, static_cast<hipStream_t>(stream), opt);
}

extern "C" int gnpde_spmm_rhs_lo(const gnpde_graph_t* g, const float* w_csr, const float* u, const void* u_lo, int32_t d, int32_t ld,
                                 const gnpde_epilogue_t* epi, void* out_y_lo, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(epi != nullptr && u != nullptr && u_lo != nullptr, GNPDE_EINVAL, "spmm_rhs_lo: epilogue / u / u_lo is null");
  gnpde::LoPair lo;
  lo.u_lo = static_cast<const uint16_t*>(u_lo);
  lo.out_y_lo = static_cast<uint16_t*>(out_y_lo);
  gnpde::SpmmOptions opt;
  opt.padded_rows = ld % 4 == 0;
  opt.lo = &lo;
  return gnpde::launch_spmm_rhs(g, w_csr, u, d, ld, epi, nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), opt);
}
