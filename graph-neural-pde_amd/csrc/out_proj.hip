// out = stage(alpha' (z Wout - u) + beta x0): the out-projection of the GAT function's mix_features form with the diffusion epilogue and
// the solver's stage algebra behind it.
//
// Reference src/function_GAT_attention.py:32-38: f = alpha (A(x) (x W) Wout - x) + beta x0.  Wout sits between the aggregate
// z = A(x) (x W) and the "- x", so the aggregation cannot carry the epilogue as it does for every other function; this kernel
// carries it instead, and an evaluation stays projection + attention + aggregation + ONE more launch with no elementwise pass
// over the state (csrc/solver.hip, enqueue_rhs, GNPDE_RHS_MIX_FEATURES).
//
// The product runs on the fp32 matrix cores exactly as in linear.hip: one wavefront owns 16 consecutive rows and all d output
// columns, 64 columns (four 16 x 16 accumulators) at a time; lane (r, kq) feeds z[row0 + r][kb + 4 kq + i] and
// Wout_t[col0 + r][kb + 4 kq + i] to the i-th MFMA of a 16-wide K block.  The K order of an output element is fixed (blocks
// ascending, i = 0..3 inside a block), so results are the same bits from run to run and between an eager launch and a graph replay.
//
// The accumulators leave the MFMA column-per-lane (col = lane & 15, row = 4 (lane >> 4) + reg) while every streaming operand of
// the epilogue (u, x0, y, k1..k3, prev[j], out_k, out_y) is row-contiguous: the 16 x 64 block goes through a wave-private LDS slab
// (no workgroup barrier: the LDS operations of a wave execute in order) and comes back as 16-byte row lanes for epilogue<4, .>;
// widths without 16-byte lanes come back as 64 consecutive floats of one row per instruction for epilogue<1, .>.
#include "common.h"
#include "epilogue.h"

namespace gnpde {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGroupTiles = 4;                   // 16-column tiles a wave accumulates at a time
constexpr int kGroupCols = 16 * kGroupTiles;
constexpr int kSlabLd = kGroupCols + 4;          // 272-byte slab rows: 16-byte aligned, and the four row quarters of a store hit distinct banks

// four consecutive K elements of a row of z or Wout_t (A % 4 == 0: a 4-wide piece is whole or absent)
__device__ __forceinline__ f32x4 load_k4(const float* __restrict__ row, int k, int kmax, bool ok, bool vec) {
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (!ok || k >= kmax) return r;
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(row + k);
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = row[k + i];
  }
  return r;
}

// VEC = 4: columns [0, wcols) of every state-shaped operand in 16-byte lanes (wcols = d, or d rounded up to 4 over padding columns);
// VEC = 1: scalar lanes over [0, d).  vec_in: z and Wout_t rows are 16-byte aligned.
template <int VEC>
__global__ __launch_bounds__(kBlock) void out_proj_kernel(const float* __restrict__ z, int n, int A, int ldz,
                                                          const float* __restrict__ W, int d, int ldw,
                                                          const float* __restrict__ u, int ld, int wcols, int vec_in,
                                                          const gnpde_epilogue_t ep) {
  __shared__ __attribute__((aligned(16))) float slab[kWavesPerBlock][16 * kSlabLd];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const long long tile = static_cast<long long>(blockIdx.x) * kWavesPerBlock + wave;
  const long long row0 = tile * 16;
  if (row0 >= n) return;
  const int r = lane & 15;       // row within the tile (A operand) / column within a 16-column tile (B operand)
  const int kq = lane >> 4;      // which 4-wide quarter of the 16-wide K block
  const long long arow = row0 + r < n ? row0 + r : n - 1;      // ragged last tile: clamp reads, mask the epilogue
  const float* zrow = z + static_cast<size_t>(arow) * ldz;
  const bool vin = vec_in != 0;
  float* my = slab[wave];
  const float alpha = alpha_of(ep);
  const float beta = ep.x0 != nullptr ? *ep.beta : 0.0f;

  for (int c0 = 0; c0 < d; c0 += kGroupCols) {
    f32x4 acc[kGroupTiles];
#pragma unroll
    for (int t = 0; t < kGroupTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* wrow[kGroupTiles];
    bool wok[kGroupTiles];
#pragma unroll
    for (int t = 0; t < kGroupTiles; ++t) {
      const int col = c0 + 16 * t + r;
      wok[t] = col < d;
      wrow[t] = W + static_cast<size_t>(wok[t] ? col : 0) * ldw;
    }
#pragma unroll 2
    for (int kb = 0; kb < A; kb += 16) {
      const int k = kb + 4 * kq;
      const f32x4 av = load_k4(zrow, k, A, true, vin);
      f32x4 bv[kGroupTiles];
#pragma unroll
      for (int t = 0; t < kGroupTiles; ++t) bv[t] = load_k4(wrow[t], k, A, wok[t], vin);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < kGroupTiles; ++t)
          if (c0 + 16 * t < d)      // (wave-uniform: a column tile is present or absent)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[t][i], acc[t], 0, 0, 0);
    }
    // C/D layout of a 16 x 16 tile: col = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
    for (int t = 0; t < kGroupTiles; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) my[(4 * kq + i) * kSlabLd + 16 * t + r] = acc[t][i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if constexpr (VEC == 4) {
      // a load instruction covers four rows x 64 columns: lane -> (row it * 4 + lane / 16, columns 4 (lane % 16) .. + 3)
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        const int rr = it * 4 + kq;
        const int col = c0 + 4 * r;
        const long long row = row0 + rr;
        if (row < n && col < wcols) {
          const float4 t4 = *reinterpret_cast<const float4*>(&my[rr * kSlabLd + 4 * r]);
          const float ax[4] = {t4.x, t4.y, t4.z, t4.w};
          const size_t off = static_cast<size_t>(row) * ld + col;
          float ui[4];
          load_vec<4>(u + off, ui);
          epilogue<4, true>(ep, alpha, beta, off, ax, ui);
        }
      }
    } else {
      // scalar lanes: 64 consecutive floats of one row per instruction
      for (int rr = 0; rr < 16; ++rr) {
        const int col = c0 + lane;
        const long long row = row0 + rr;
        if (row < n && col < d) {
          const float ax[1] = {my[rr * kSlabLd + lane]};
          const size_t off = static_cast<size_t>(row) * ld + col;
          float ui[1];
          load_vec<1>(u + off, ui);
          epilogue<1, false>(ep, alpha, beta, off, ax, ui);
        }
      }
    }
    __builtin_amdgcn_wave_barrier();     // the slab reads above precede the next column group's slab writes
  }
}

}  // namespace

bool linear_epilogue_supported(int A, int d) { return A >= 4 && A <= 256 && A % 4 == 0 && d >= 1 && d <= 256; }

// u is read only by the lane that writes the same element, so an output may be u (check_epilogue's rule for a gathered operand is
// applied to z, whose rows a whole wave reads).
int launch_linear_epilogue(const float* z, int n, int A, int ldz, const float* W, int d, int ldw, const float* u, int ld,
                           const gnpde_epilogue_t& e, bool padded_rows, hipStream_t s) {
  GNPDE_CHECK_ARG(z && W && u, GNPDE_EINVAL, "linear_epilogue: null pointer");
  GNPDE_CHECK_ARG(n >= 0 && A >= 1 && d >= 1 && ldz >= A && ldw >= A && ld >= d, GNPDE_EINVAL,
                  "linear_epilogue: bad shape n=%d A=%d d=%d ldz=%d ldw=%d ldu=%d", n, A, d, ldz, ldw, ld);
  GNPDE_CHECK_ARG(linear_epilogue_supported(A, d), GNPDE_ESHAPE,
                  "linear_epilogue: A = %d, d = %d outside the kernel's shapes (A a multiple of 4 up to 256, d up to 256)", A, d);
  if (const int rc = check_epilogue("linear_epilogue", e, z, kEpilogueStagesAll)) return rc;
  GNPDE_CHECK_ARG(e.stage != GNPDE_STAGE_LINCOMB || e.out_k != nullptr || e.out_y != nullptr, GNPDE_EINVAL, "linear_epilogue: LINCOMB without output");
  if (n == 0) return 0;
  const bool vec_in = ldz % 4 == 0 && ldw % 4 == 0 && aligned(z, 16) && aligned(W, 16);
  const bool lanes16 = (d % 4 == 0 || padded_rows) && on_lanes(16, ld, u, nullptr, nullptr, &e);
  const long long tiles = (static_cast<long long>(n) + 15) / 16;
  const dim3 grid(static_cast<unsigned>((tiles + kWavesPerBlock - 1) / kWavesPerBlock)), block(kBlock);
  if (lanes16) {
    const int wcols = (d + 3) / 4 * 4;      // d % 4 != 0: the last lane covers up to 3 padding columns (<= ld: ld % 4 == 0)
    hipLaunchKernelGGL((out_proj_kernel<4>), grid, block, 0, s, z, n, A, ldz, W, d, ldw, u, ld, wcols, vec_in ? 1 : 0, e);
  } else {
    hipLaunchKernelGGL((out_proj_kernel<1>), grid, block, 0, s, z, n, A, ldz, W, d, ldw, u, ld, d, vec_in ? 1 : 0, e);
  }
  GNPDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace gnpde

extern "C" int gnpde_linear_epilogue(const float* z, int32_t n, int32_t A, int32_t ldz, const float* Wout_t, int32_t d, int32_t ldw,
                                     const float* u, int32_t ldu, const gnpde_epilogue_t* epi, void* stream) {
  GNPDE_CHECK_ARG(epi != nullptr, GNPDE_EINVAL, "linear_epilogue: null epilogue");
  return gnpde::launch_linear_epilogue(z, n, A, ldz, Wout_t, d, ldw, u, ldu, *epi, false, static_cast<hipStream_t>(stream));
}
