// SDDMM: out[p] = scale * a[row_p] . b[col_p] for every stored entry -- the gradient of the aggregation
// w.r.t. the edge weights (d w_e = alpha' g_row . x_col), needed when attention_weights carry gradients.
// Same work items as the aggregation (spmm.hip: 512-entry chunks of the hub rows first, then one wavefront per row, XCD-aware
// block order), a_row slice kept in registers, L lanes per neighbour, U independent gathers in flight,
// xor-butterfly dot.  Entries are independent, so the hub chunks need no second pass.
#include "common.h"
#include "epilogue.h"

namespace gnpde {
namespace {

struct SddmmArgs {
  int n, n_long_chunks;
  const int* __restrict__ rowptr;
  const int* __restrict__ colidx;
  const int* __restrict__ lc_row;
  const int* __restrict__ lc_begin;
  const int* __restrict__ lc_end;
  const float* __restrict__ a;
  const float* __restrict__ b;
  int d, lda, ldb;
  const float* __restrict__ scale_ptr;
  int scale_sigmoid;
  float* __restrict__ out;
  int row_shift;         // rows -> XCDs as in the aggregation (xcd_row_of): < 0 contiguous eighths, else hashed blocks of 2^row_shift rows
};

template <int VEC, int L, int K, int U>
__global__ __launch_bounds__(kBlock) void sddmm_kernel(const SddmmArgs s) {
  constexpr int G = kWave / L;
  const int lane = threadIdx.x & (kWave - 1);
  // same XCD-balanced work list as the aggregation (item_of): every 8th chunk first, then this XCD's share of the rows
  const int x = static_cast<int>(blockIdx.x % kXcds);
  const int lw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x / kXcds) * kWavesPerBlock + static_cast<int>(threadIdx.x >> 6));
  const int cx = (s.n_long_chunks + kXcds - 1 - x) / kXcds;
  int row, e0, e1;
  if (lw >= cx) {
    row = xcd_row_of(0, s.n, s.row_shift, x, lw - cx);
    if (row < 0) return;
    e0 = s.rowptr[row];
    e1 = s.rowptr[row + 1];
    if (e1 - e0 > GNPDE_LONG_ROW) return;  // processed as chunks
  } else {
    const int item = lw * kXcds + x;
    row = s.lc_row[item];
    e0 = s.lc_begin[item];
    e1 = s.lc_end[item];
  }
  const int sub = lane / L, cl = lane % L;
  float scale = 1.0f;
  if (s.scale_ptr != nullptr) {
    scale = *s.scale_ptr;
    if (s.scale_sigmoid) scale = 1.0f / (1.0f + expf(-scale));
  }
  float av[K][VEC];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int col = (k * L + cl) * VEC;
#pragma unroll
    for (int v = 0; v < VEC; ++v) av[k][v] = 0.0f;
    if (col < s.d) load_vec<VEC>(s.a + static_cast<size_t>(row) * s.lda + col, av[k]);
  }
  for (int j = e0; j < e1; j += G * U) {
    float bv[U][K][VEC];
#pragma unroll
    for (int t = 0; t < U; ++t) {
      const int e = j + t * G + sub;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) bv[t][k][v] = 0.0f;
      if (e < e1) {
        const float* src = s.b + static_cast<size_t>(s.colidx[e]) * s.ldb;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int col = (k * L + cl) * VEC;
          if (col < s.d) load_vec<VEC>(src + col, bv[t][k]);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < U; ++t) {
      float p = 0.0f;
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int v = 0; v < VEC; ++v) p = fmaf(av[k][v], bv[t][k][v], p);
#pragma unroll
      for (int off = 1; off < L; off <<= 1) p += __shfl_xor(p, off, kWave);
      const int e = j + t * G + sub;
      if (cl == 0 && e < e1) s.out[e] = scale * p;
    }
  }
}

template <int VEC>
int dispatch_sddmm(const gnpde_graph_t* g, const float* a, const float* b, int d, int lda, int ldb, const float* scale,
                   int scale_sigmoid, float* out, hipStream_t st) {
  SddmmArgs s;
  s.n = g->n; s.n_long_chunks = g->n_long_chunks;
  s.rowptr = g->rowptr; s.colidx = g->colidx;
  s.lc_row = g->long_chunk_row; s.lc_begin = g->long_chunk_begin; s.lc_end = g->long_chunk_end;
  s.a = a; s.b = b; s.d = d; s.lda = lda; s.ldb = ldb; s.scale_ptr = scale; s.scale_sigmoid = scale_sigmoid; s.out = out;
  s.row_shift = choose_row_shift(g->n, g->xcd_deal);
  const unsigned grid = agg_grid(g->n_long_chunks, g->n, s.row_shift, 1, kWavesPerBlock);
  const int slots = (d + VEC - 1) / VEC;
#define GNPDE_SDDMM(LL, KK, UU) hipLaunchKernelGGL((sddmm_kernel<VEC, LL, KK, UU>), dim3(grid), dim3(kBlock), 0, st, s)
  if (slots <= 16) GNPDE_SDDMM(16, 1, 4);
  else if (slots <= 32) GNPDE_SDDMM(16, 2, 4);
  else if (slots <= 64) GNPDE_SDDMM(32, 2, 2);
  else if (slots <= 128) GNPDE_SDDMM(64, 2, 2);
  else if (slots <= 256) GNPDE_SDDMM(64, 4, 1);
  else {
    set_error("sddmm: feature width d=%d too large for VEC=%d", d, VEC);
    return GNPDE_ESHAPE;
  }
#undef GNPDE_SDDMM
  return 0;
}

}  // namespace
}  // namespace gnpde

extern "C" int gnpde_sddmm(const gnpde_graph_t* g, const float* a, int32_t lda, const float* b, int32_t ldb, int32_t d,
                           const float* scale, int32_t scale_sigmoid, float* out_csr, void* stream) {
  using namespace gnpde;
  GNPDE_CHECK_ARG(g && a && b && out_csr && d >= 1 && lda >= d && ldb >= d, GNPDE_EINVAL, "sddmm: bad arguments");
  if (g->n == 0 || g->e == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc;
  if (d % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && aligned(a, 16) && aligned(b, 16)) rc = dispatch_sddmm<4>(g, a, b, d, lda, ldb, scale, scale_sigmoid, out_csr, s);
  else if (d % 2 == 0 && lda % 2 == 0 && ldb % 2 == 0 && aligned(a, 8) && aligned(b, 8)) rc = dispatch_sddmm<2>(g, a, b, d, lda, ldb, scale, scale_sigmoid, out_csr, s);
  else rc = dispatch_sddmm<1>(g, a, b, d, lda, ldb, scale, scale_sigmoid, out_csr, s);
  if (rc) return rc;
  GNPDE_LAUNCH_CHECK();
  return 0;
}
