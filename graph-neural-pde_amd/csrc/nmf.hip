// NMF compression of positional encodings (reference src/pos_enc_factorisation.py: sklearn.decomposition.NMF, solver 'cd', Frobenius
// loss, no regularisation, shuffle off): one half-sweep of the coordinate descent.  include/gnpde.h has the definition.
//   nmf_cd_sweep_kernel   one wave per row; lane l holds the components l, l + 64, ... (C = ceil(k / 64) registers of W_i and of
//                         q = W_i G - P_i).  The wave forms q itself (row s of G times the wave-uniform W[i, s], ascending s), then
//                         walks t in order: grad = lane (t mod 64)'s q, read as a wave-uniform value; one IEEE division;
//                         delta = new - old; every lane adds G[t, r] delta to its q_r.  Nothing is reduced inside the sequential loop.
//                         Rows of G are read by consecutive lanes: from LDS (staged once per persistent workgroup) for k <= 128 --
//                         every row of W reads all of G twice, 128 KiB at k = 128 against 1 KiB of its own data -- and from memory
//                         (L2) above that, where G (up to 256 KiB) does not fit.  1024 threads per workgroup so that two workgroups
//                         with 64 KiB of G each fill a CU's 32 wave slots.
//                         The loops over s and t have no data-dependent branch (G[t, t] == 0 selects delta = 0) and are unrolled by
//                         hand, so the reads of G's rows run ahead of the sequential chain.  Row t of G also holds G[t, t], in lane
//                         t mod 64.
//                         Padding lanes (r >= k) read a valid address, hold zeros and store nothing.
//   violation             |pg| summed per row in double (the wave-uniform value, component order), one double per row with a plain
//                         store; then chunks of 4096 rows and the chunk sums are added in a fixed order (block_sum_double).  No
//                         atomics: bit-identical from run to run and independent of the sweep's grid.
#include "common.h"
#include "embedded_pair.h"

namespace gnpde {
namespace {

constexpr int kNmfMaxK = 256;
constexpr int kNmfLdsK = 128;                 // G staged in LDS up to this k (64 KiB)
constexpr int kNmfBlock = 1024;
constexpr int kNmfWaves = kNmfBlock / kWave;
constexpr int kNmfChunk = 4096;               // rows per partial sum of the violation

__device__ __forceinline__ float uniform_lane(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

template <int C, bool LDS>
__global__ __launch_bounds__(kNmfBlock) void nmf_cd_sweep_kernel(float* __restrict__ W, long long ldw, const float* __restrict__ G,
                                                                const float* __restrict__ P, long long ldp, long long n, int k,
                                                                double* __restrict__ row_violation) {
  extern __shared__ __attribute__((aligned(16))) float g_lds[];
  constexpr int kUnroll = LDS ? 4 : 2;      // rows of G in flight (1024 threads leave 128 VGPRs; the rows from memory cost C registers each)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < k * k; i += kNmfBlock) g_lds[i] = G[i];
    __syncthreads();
  }
  auto g_at = [&](int idx) -> float {
    if constexpr (LDS) return g_lds[idx];
    else return G[idx];
  };
  const long long stride = static_cast<long long>(gridDim.x) * kNmfWaves;
  for (long long row = static_cast<long long>(blockIdx.x) * kNmfWaves + wave; row < n; row += stride) {
    float* wr = W + row * ldw;
    const float* pr = P + row * ldp;
    float w[C], q[C];
    int rc[C];                                   // the lane's components, clamped: a padding lane reads a valid address and keeps zeros
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int r = lane + 64 * c;
      rc[c] = r < k ? r : k - 1;
      w[c] = r < k ? wr[r] : 0.0f;
      q[c] = 0.0f;
    }
    // q = W_i G - P_i.  The loops over s and t are unrolled by hand (a loop that holds a readlane is not unrolled for a run-time
    // trip count), so that the reads of the next rows of G are issued ahead of the chain.
#pragma unroll
    for (int cs = 0; cs < C; ++cs) {
      const int lim = k - 64 * cs < 64 ? k - 64 * cs : 64;
      auto add_row = [&](int ss) {
        const float ws = uniform_lane(w[cs], ss);
        const int s = 64 * cs + ss;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float g = g_at(s * k + rc[c]);
          q[c] = fmaf(ws, lane + 64 * c < k ? g : 0.0f, q[c]);
        }
      };
      int ss = 0;
      for (; ss + kUnroll <= lim; ss += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) add_row(ss + u);
      }
      for (; ss < lim; ++ss) add_row(ss);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int r = lane + 64 * c;
      if (r < k) q[c] -= pr[r];
    }
    double violation = 0.0;
#pragma unroll
    for (int ct = 0; ct < C; ++ct) {
      const int lim = k - 64 * ct < 64 ? k - 64 * ct : 64;
      auto component = [&](int tt) {
        const int t = 64 * ct + tt;
        float g_row[C];                          // row t of G: the update of q, and its diagonal entry in lane tt
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float g = g_at(t * k + rc[c]);
          g_row[c] = lane + 64 * c < k ? g : 0.0f;
        }
        const float grad = uniform_lane(q[ct], tt), w_old = uniform_lane(w[ct], tt), gtt = uniform_lane(g_row[ct], tt);
        const float pg = w_old == 0.0f ? fminf(0.0f, grad) : grad;
        violation += static_cast<double>(fabsf(pg));
        const float w_new = gtt != 0.0f ? fmaxf(w_old - grad / gtt, 0.0f) : w_old;      // G[t, t] == 0 gives delta = 0
        const float delta = w_new - w_old;
        if (lane == tt) w[ct] = w_new;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = fmaf(g_row[c], delta, q[c]);
      };
      int tt = 0;
      for (; tt + kUnroll <= lim; tt += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) component(tt + u);
      }
      for (; tt < lim; ++tt) component(tt);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int r = lane + 64 * c;
      if (r < k) wr[r] = w[c];
    }
    if (lane == 0) row_violation[row] = violation;
  }
}

// block b: the sum of in[b * kNmfChunk .. min(n, (b + 1) * kNmfChunk)) -- thread t adds its entries t, t + 256, ... in order, then the tree
__global__ __launch_bounds__(kBlock) void nmf_sum_chunks_kernel(const double* __restrict__ in, long long n, double* __restrict__ out) {
  __shared__ double red[kBlock];
  const long long begin = static_cast<long long>(blockIdx.x) * kNmfChunk;
  const long long end = begin + kNmfChunk < n ? begin + kNmfChunk : n;
  double s = 0.0;
  for (long long i = begin + threadIdx.x; i < end; i += kBlock) s += in[i];
  s = block_sum_double(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

__global__ __launch_bounds__(kBlock) void nmf_sum_kernel(const double* __restrict__ in, long long n, double* __restrict__ out) {
  __shared__ double red[kBlock];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += kBlock) s += in[i];
  s = block_sum_double(s, red);
  if (threadIdx.x == 0) *out = s;
}

inline long long nmf_chunks(long long n) { return (n + kNmfChunk - 1) / kNmfChunk; }

template <int C>
int launch_sweep(float* W, long long ldw, const float* G, const float* P, long long ldp, long long n, int k, double* row_violation,
                 hipStream_t s) {
  long long blocks = (n + kNmfWaves - 1) / kNmfWaves;
  if (blocks > 512) blocks = 512;           // persistent: two workgroups of 1024 threads per CU; the rows are dealt wave by wave
  const dim3 grid(static_cast<unsigned>(blocks)), block(kNmfBlock);
  if (k <= kNmfLdsK) {
    if constexpr (C <= kNmfLdsK / 64) {
      hipLaunchKernelGGL((nmf_cd_sweep_kernel<C, true>), grid, block, static_cast<size_t>(k) * k * sizeof(float), s, W, ldw, G, P, ldp, n, k,
                         row_violation);
    }
  } else {
    hipLaunchKernelGGL((nmf_cd_sweep_kernel<C, false>), grid, block, 0, s, W, ldw, G, P, ldp, n, k, row_violation);
  }
  GNPDE_LAUNCH_CHECK();
  return 0;
}

// byte ranges of two matrices (rows x cols floats, row stride ld) intersect
inline bool overlap(const float* a, long long rows_a, long long lda, const float* b, long long rows_b, long long ldb, int cols) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + (static_cast<uintptr_t>(rows_a - 1) * lda + cols) * sizeof(float);
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + (static_cast<uintptr_t>(rows_b - 1) * ldb + cols) * sizeof(float);
  return a0 < b1 && b0 < a1;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_nmf_cd_sweep_workspace_bytes(int64_t n) {
  if (n < 1 || n > INT32_MAX) return 0;
  return align_up(static_cast<size_t>(n) * sizeof(double), 256) + align_up(static_cast<size_t>(nmf_chunks(n)) * sizeof(double), 256);
}

extern "C" int gnpde_nmf_cd_sweep(float* W, int64_t ldw, const float* G, const float* P, int64_t ldp, int64_t n, int32_t k,
                                  double* violation, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(k >= 1 && k <= kNmfMaxK, GNPDE_ESHAPE, "nmf_cd_sweep: k = %d outside 1 .. %d", k, kNmfMaxK);
  GNPDE_CHECK_ARG(n >= 1 && n <= INT32_MAX, GNPDE_ESHAPE, "nmf_cd_sweep: n = %lld outside 1 .. INT32_MAX", static_cast<long long>(n));
  GNPDE_CHECK_ARG(W && G && P && violation, GNPDE_EINVAL, "nmf_cd_sweep: null pointer (W, G, P or violation)");
  GNPDE_CHECK_ARG(ldw >= k && ldp >= k, GNPDE_EINVAL, "nmf_cd_sweep: row strides %lld / %lld are below k = %d", static_cast<long long>(ldw),
                  static_cast<long long>(ldp), k);
  GNPDE_CHECK_ARG(!overlap(W, n, ldw, P, n, ldp, k), GNPDE_EINVAL, "nmf_cd_sweep: W and P alias (W is updated in place while P is read)");
  GNPDE_CHECK_ARG(!overlap(W, n, ldw, G, k, k, k), GNPDE_EINVAL, "nmf_cd_sweep: W and G alias (W is updated in place while G is read)");
  const size_t need = gnpde_nmf_cd_sweep_workspace_bytes(n);
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "nmf_cd_sweep: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, need);
  hipStream_t s = static_cast<hipStream_t>(stream);
  double* row_violation = static_cast<double*>(workspace);
  double* chunk_sums = reinterpret_cast<double*>(static_cast<char*>(workspace) + align_up(static_cast<size_t>(n) * sizeof(double), 256));
  int rc;
  switch ((k + 63) / 64) {
    case 1: rc = launch_sweep<1>(W, ldw, G, P, ldp, n, k, row_violation, s); break;
    case 2: rc = launch_sweep<2>(W, ldw, G, P, ldp, n, k, row_violation, s); break;
    case 3: rc = launch_sweep<3>(W, ldw, G, P, ldp, n, k, row_violation, s); break;
    default: rc = launch_sweep<4>(W, ldw, G, P, ldp, n, k, row_violation, s); break;
  }
  if (rc != 0) return rc;
  const long long chunks = nmf_chunks(n);
  hipLaunchKernelGGL(nmf_sum_chunks_kernel, dim3(static_cast<unsigned>(chunks)), dim3(kBlock), 0, s, row_violation, static_cast<long long>(n),
                     chunk_sums);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(nmf_sum_kernel, dim3(1), dim3(kBlock), 0, s, chunk_sums, chunks, violation);
  GNPDE_LAUNCH_CHECK();
  return 0;
}
