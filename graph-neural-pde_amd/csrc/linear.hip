// out[n, m] = x[n, d] * W[m, d]^T + b[m]  on the fp32 matrix cores.
//
// The only GEMM-shaped work on the path: nn.Linear Q and K of SpGraphTransAttentionLayer
// (reference src/function_transformer_attention.py:174-175, fused into one [N,d]x[d,2A] product;
// V is skipped, its result is dead when mix_features is false, :34-35) and torch.mm(x, W) of the
// GAT layer (src/function_GAT_attention.py:106).  Tall-skinny: N = 1e5..1e6 rows, d and m <= 256,
// so it is bound by reading x once; v_mfma_f32_16x16x4_f32 is exact fp32 (bit-equal to an fmaf
// chain) and keeps the VALU free.
//
// One wavefront owns 16 consecutive rows and all m output columns (m/16 accumulators).  Every lane
// loads ONE float4 of x per 16-wide K block -- x[row0 + (l&15)][kb + 4*(l>>4) .. +3] -- and uses its
// i-th component as the A operand of the i-th MFMA of that block; the matching B operand is the i-th
// component of the float4 W[col0 + (l&15)][kb + 4*(l>>4) .. +3].  The k index of an MFMA step is thus
// {kb+i, kb+4+i, kb+8+i, kb+12+i}: a permutation of the K order, which a dot product does not care
// about, and it makes both operand loads 16-byte vector loads straight from row-major memory with no
// LDS transpose.
#include "common.h"

namespace gnpde {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// relu on the A operand (the decoder of the reference's GNN.forward applies F.relu to the state before m2)
__device__ __forceinline__ f32x4 relu_if(f32x4 v, int relu) {
  if (relu) {
    v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
  }
  return v;
}

template <bool ALIGNED>
__device__ __forceinline__ f32x4 load4_guard(const float* __restrict__ base, int k, int kmax, bool row_ok) {
  f32x4 r = {0.f, 0.f, 0.f, 0.f};
  if (!row_ok) return r;
  if constexpr (ALIGNED) {
    if (k + 3 < kmax) {
      const float4 t = *reinterpret_cast<const float4*>(base + k);
      r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
      return r;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (k + i < kmax) r[i] = base[k + i];
  return r;
}

// MT = number of 16-column output tiles kept in registers by one wave.
// FULL: every column tile is complete and d % 16 == 0 -> no guards on the operand loads (rows past the end
// are clamped to the last row and only their stores are masked), so the loads of a K batch are
// straight-line code the scheduler can issue back to back, and one launch covers the ragged last tile.
template <int MT, bool ALIGNED, bool FULL, int KUV = (MT <= 2 ? 4 : 2)>
__global__ __launch_bounds__(kBlock) void linear_kernel(const float* __restrict__ x, int n, int d, int ldx,
                                                        const float* __restrict__ W, int m, int ldw,
                                                        const float* __restrict__ b, float* __restrict__ out,
                                                        int ldo, int col_base, int row_base, int relu) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const long long tile = static_cast<long long>(blockIdx.x) * kWavesPerBlock + wave;
  const int row0 = row_base + static_cast<int>(tile * 16);
  if (row0 >= n) return;
  col_base += static_cast<int>(blockIdx.y) * (MT * 16);     // 2-D launches: grid.y walks the column groups (small n, below)
  const int r = lane & 15;       // row within the tile (A operand) / column within a 16-col tile (B)
  const int kq = lane >> 4;      // which 4-wide K quarter of the 16-wide K block
  const int arow = row0 + r;
  const bool arow_ok = arow < n;
  const float* xrow = x + static_cast<size_t>(arow_ok ? arow : (FULL ? n - 1 : 0)) * ldx;

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // KU 16-wide K blocks per iteration: all operand loads of an iteration are issued before the first
  // MFMA so that several HBM round trips overlap (a wave has only d/16 dependent-free blocks to hide
  // ~2 us of latency behind)
  constexpr int KU = KUV;
  for (int kb = 0; kb < d; kb += 16 * KU) {
    f32x4 av[KU];
    f32x4 bv[KU][MT];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k = kb + 16 * u + 4 * kq;
      if constexpr (FULL) {
        if (kb + 16 * u < d) {  // d % 16 == 0: a K block is complete or absent -- a scalar (wave-uniform) test
          const float4 ta = *reinterpret_cast<const float4*>(xrow + k);
          av[u] = relu_if(f32x4{ta.x, ta.y, ta.z, ta.w}, relu);
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const float4 tb = *reinterpret_cast<const float4*>(W + static_cast<size_t>(col_base + t * 16 + r) * ldw + k);
            bv[u][t] = f32x4{tb.x, tb.y, tb.z, tb.w};
          }
        } else {
          av[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < MT; ++t) bv[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      } else {
        av[u] = relu_if(load4_guard<ALIGNED>(xrow, k, d, arow_ok), relu);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const int col = col_base + t * 16 + r;
          const bool ok = col < m;
          bv[u][t] = load4_guard<ALIGNED>(W + static_cast<size_t>(ok ? col : 0) * ldw, k, d, ok);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < MT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][i], bv[u][t][i], acc[t], 0, 0, 0);
  }

  // C/D layout of the 16x16 tile: col = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int col = col_base + t * 16 + r;
    if constexpr (!FULL) {
      if (col >= m) continue;
    }
    const float bias = b != nullptr ? b[col] : 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int orow = row0 + 4 * kq + i;
      if (orow < n) out[static_cast<size_t>(orow) * ldo + col] = acc[t][i] + bias;
    }
  }
}

// Persistent variant for the projection shapes of the hot path (d = 16*KB <= 128 wide, m = 16*MT <= 32 columns):
// the whole B operand (all of W) stays in registers for the life of the wavefront, wavefronts stride over the
// 16-row tiles, and the A operand of the NEXT tile is in flight while the MFMAs of the current one issue, so
// the kernel streams x at memory speed instead of paying one HBM round trip per tile.
template <int MT, int KB>
__global__ __launch_bounds__(kBlock) void linear_persistent_kernel(const float* __restrict__ x, int n, int ldx,
                                                                   const float* __restrict__ W, int ldw,
                                                                   const float* __restrict__ b, float* __restrict__ out,
                                                                   int ldo, int col_base, int relu) {
  const int lane = threadIdx.x & (kWave - 1);
  const int r = lane & 15, kq = lane >> 4;
  const long long n_tiles = (static_cast<long long>(n) + 15) / 16;
  const long long stride = static_cast<long long>(gridDim.x) * kWavesPerBlock;
  long long tile = static_cast<long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;

  f32x4 bv[KB][MT];
#pragma unroll
  for (int u = 0; u < KB; ++u)
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const float4 tb = *reinterpret_cast<const float4*>(W + static_cast<size_t>(col_base + t * 16 + r) * ldw + 16 * u + 4 * kq);
      bv[u][t] = f32x4{tb.x, tb.y, tb.z, tb.w};
    }
  float bias[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) bias[t] = b != nullptr ? b[col_base + t * 16 + r] : 0.0f;

  auto load_tile = [&](long long tl, f32x4 (&av)[KB]) {
    long long row = tl * 16 + r;
    if (row >= n) row = n - 1;  // ragged last tile: clamp reads, mask writes
    const float* xr = x + static_cast<size_t>(row) * ldx + 4 * kq;
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const float4 ta = *reinterpret_cast<const float4*>(xr + 16 * u);
      av[u] = relu_if(f32x4{ta.x, ta.y, ta.z, ta.w}, relu);
    }
  };

  f32x4 cur[KB], nxt[KB];
  load_tile(tile, cur);
  while (true) {
    const long long next = tile + stride;
    const bool more = next < n_tiles;
    if (more) load_tile(next, nxt);
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][i], bv[u][t][i], acc[t], 0, 0, 0);
    const long long row0 = tile * 16;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long orow = row0 + 4 * kq + i;
        if (orow < n) out[static_cast<size_t>(orow) * ldo + col_base + t * 16 + r] = acc[t][i] + bias[t];
      }
    if (!more) break;
#pragma unroll
    for (int u = 0; u < KB; ++u) cur[u] = nxt[u];
    tile = next;
  }
}


// Wide projections (m >= 64 output columns, e.g. the R-MAT configuration's [N,256] x [256,128]): linear_kernel re-reads all of
// W (128 KB) from L2 for every 16-row tile -- 8x the bytes of the tile itself, 2.84 ms where the fp32 MFMA time is 0.9 ms.
// Here W is staged ONCE per workgroup in LDS (rows padded by 4 floats, so the 16 lanes of a ds_read_b128 group hit 16
// different 16-byte slots) and the 8 waves of the workgroup stride over the row tiles: per 16-K block a wave issues MT
// B-operand reads from LDS and 4 MT MFMAs, with the A operands of the next K batch in flight from HBM.
template <int MT, int DMAX>
__global__ __launch_bounds__(512) void linear_lds_kernel(const float* __restrict__ x, int n, int d, int ldx,
                                                         const float* __restrict__ W, int ldw, const float* __restrict__ b,
                                                         float* __restrict__ out, int ldo, int col_base, int relu) {
  constexpr int LDL = DMAX + 4;
  constexpr int KU = 4;                                  // 16-wide K blocks per batch
  __shared__ float lds[MT * 16 * LDL];
  const int d4 = d >> 2;
  for (int idx = threadIdx.x; idx < MT * 16 * d4; idx += 512) {
    const int row = idx / d4, c4 = idx - row * d4;
    *reinterpret_cast<float4*>(&lds[row * LDL + 4 * c4]) =
        *reinterpret_cast<const float4*>(W + static_cast<size_t>(col_base + row) * ldw + 4 * c4);
  }
  __syncthreads();
  const int lane = threadIdx.x & (kWave - 1);
  const int r = lane & 15, kq = lane >> 4;
  float bias[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) bias[t] = b != nullptr ? b[col_base + t * 16 + r] : 0.0f;
  const long long n_tiles = (static_cast<long long>(n) + 15) / 16;
  const long long stride = static_cast<long long>(gridDim.x) * 8;
  const int nkb = d >> 4;
  for (long long tile = static_cast<long long>(blockIdx.x) * 8 + (threadIdx.x >> 6); tile < n_tiles; tile += stride) {
    long long row = tile * 16 + r;
    if (row >= n) row = n - 1;                           // ragged last tile: clamp reads, mask writes
    const float* xr = x + static_cast<size_t>(row) * ldx + 4 * kq;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 cur[KU], nxt[KU];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const float4 ta = u < nkb ? *reinterpret_cast<const float4*>(xr + 16 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
      cur[u] = relu_if(f32x4{ta.x, ta.y, ta.z, ta.w}, relu);
    }
    for (int u0 = 0; u0 < nkb; u0 += KU) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {                     // next batch's A operands (wave-uniform guard)
        const int kb = u0 + KU + u;
        const float4 ta = kb < nkb ? *reinterpret_cast<const float4*>(xr + 16 * kb) : make_float4(0.f, 0.f, 0.f, 0.f);
        nxt[u] = relu_if(f32x4{ta.x, ta.y, ta.z, ta.w}, relu);
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        if (u0 + u < nkb) {
#pragma unroll
          for (int t = 0; t < MT; ++t) {
            const float4 tb = *reinterpret_cast<const float4*>(&lds[(t * 16 + r) * LDL + 16 * (u0 + u) + 4 * kq]);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][0], tb.x, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][1], tb.y, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][2], tb.z, acc[t], 0, 0, 0);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[u][3], tb.w, acc[t], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < KU; ++u) cur[u] = nxt[u];
    }
    const long long row0 = tile * 16;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long orow = row0 + 4 * kq + i;
        if (orow < n) out[static_cast<size_t>(orow) * ldo + col_base + t * 16 + r] = acc[t][i] + bias[t];
      }
  }
}

// Round 3: the same persistent kernel with the A operand fetched in FULL LINES and transposed through LDS.  The kernel above
// loads fragment-shaped -- lane (r, kq) reads 16 bytes of row r, so one load instruction touches 16 rows x 64 B, half a cache
// line each -- and streams x at 3.7 TB/s with the MFMA pipe 30 % busy.  Here lane l of load `it` reads chunk it * 64 + l of the
// tile's 16 x d floats (two whole rows, 1 KB contiguous, per instruction), the wave writes the chunks into its own LDS slab
// (chunk (r, j) at r * d/4 + (j ^ (r & 7)): the xor keeps both the row-linear writes and the column-strided fragment reads
// free of bank conflicts) and reads the fragments back as ds_read_b128.  Wave-private slabs: no barrier, LDS operations of a
// wave execute in order.  Same MFMA sequence, same k order, same results bit for bit.
template <int MT, int KB>
__global__ __launch_bounds__(kBlock) void linear_staged_kernel(const float* __restrict__ x, int n, int ldx,
                                                               const float* __restrict__ W, int ldw,
                                                               const float* __restrict__ b, float* __restrict__ out,
                                                               int ldo, int col_base, int relu) {
  constexpr int CPR = KB * 4;                 // 16-byte chunks per row (d = 16 KB floats)
  constexpr int CHUNKS = 16 * CPR;            // per tile
  constexpr int PER_LANE = CHUNKS / kWave;    // = KB
  __shared__ f32x4 slab[kWavesPerBlock][CHUNKS];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const long long n_tiles = (static_cast<long long>(n) + 15) / 16;
  const long long stride = static_cast<long long>(gridDim.x) * kWavesPerBlock;   // every wave strides over the table by the grid
  long long tile = static_cast<long long>(blockIdx.x) * kWavesPerBlock + wave;
  if (tile >= n_tiles) return;

  f32x4 bv[KB][MT];
#pragma unroll
  for (int u = 0; u < KB; ++u)
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const float4 tb = *reinterpret_cast<const float4*>(W + static_cast<size_t>(col_base + t * 16 + r) * ldw + 16 * u + 4 * kq);
      bv[u][t] = f32x4{tb.x, tb.y, tb.z, tb.w};
    }
  float bias[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) bias[t] = b != nullptr ? b[col_base + t * 16 + r] : 0.0f;

  // chunk c = it * 64 + lane of a tile: row c / CPR, column chunk c % CPR
  auto load_tile = [&](long long tl, f32x4 (&g)[PER_LANE]) {
#pragma unroll
    for (int it = 0; it < PER_LANE; ++it) {
      const int c = it * kWave + lane;
      long long row = tl * 16 + c / CPR;
      if (row >= n) row = n - 1;               // ragged last tile: clamp reads, mask writes
      g[it] = *reinterpret_cast<const f32x4*>(x + static_cast<size_t>(row) * ldx + 4 * (c % CPR));
    }
  };
  f32x4* my = slab[wave];
  f32x4 g[PER_LANE];
  load_tile(tile, g);
  while (true) {
#pragma unroll
    for (int it = 0; it < PER_LANE; ++it) {
      const int c = it * kWave + lane;
      const int rr = c / CPR, j = c % CPR;
      my[rr * CPR + (j ^ (rr & 7))] = g[it];
    }
    const long long next = tile + stride;
    const bool more = next < n_tiles;
    if (more) load_tile(next, g);              // in flight during the MFMAs of this tile
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragments two K blocks at a time: the reads of the next pair are in flight during the MFMAs of this one
#pragma unroll
    for (int u = 0; u < KB; u += 2) {
      f32x4 cu[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) cu[q] = relu_if(my[r * CPR + ((4 * (u + q) + kq) ^ (r & 7))], relu);
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cu[q][i], bv[u + q][t][i], acc[t], 0, 0, 0);
    }
    const long long row0 = tile * 16;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long long orow = row0 + 4 * kq + i;
        if (orow < n) out[static_cast<size_t>(orow) * ldo + col_base + t * 16 + r] = acc[t][i] + bias[t];
      }
    if (!more) break;
    __builtin_amdgcn_wave_barrier();           // the fragment reads above precede the next tile's slab writes
    tile = next;
  }
}

// The staged kernel for the q||k projection shape (MT = 2: m = 32 output columns) with PAIRED columns: column tile t of lane r is output
// column 2 r + t, so a lane's two accumulators of an output row are ADJACENT columns and leave as one 8-byte store: a store instruction
// writes four complete 128-byte output rows (the kernel above writes every output line as two 64-byte halves by two different
// instructions).  Same MFMA sequence and k order per output element: bit-identical results.  (Two row tiles of x in flight per wave
// measured slower, 28.0 vs 25.8 us: profiles/r06_linear_*.txt.)
template <int KB>
__global__ __launch_bounds__(kBlock) void linear_staged2_kernel(const float* __restrict__ x, int n, int ldx,
                                                                const float* __restrict__ W, int ldw,
                                                                const float* __restrict__ b, float* __restrict__ out,
                                                                int ldo, int col_base, int relu, float* __restrict__ out2 = nullptr,
                                                                int split = 0) {
  // out2 / split (round 6): output columns >= split go to out2[row * ldo + col - split] -- the q||k projection as TWO tables [n, A] when a
  // key row is shorter than a cache line (A <= 16: the attention's gathers of 64-byte k rows then fetch no q halves of 128-byte lines)
  constexpr int MT = 2;
  constexpr int CPR = KB * 4;
  constexpr int CHUNKS = 16 * CPR;
  constexpr int PER_LANE = CHUNKS / kWave;
  __shared__ f32x4 slab[kWavesPerBlock][CHUNKS];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  const int r = lane & 15, kq = lane >> 4;
  const long long n_tiles = (static_cast<long long>(n) + 15) / 16;
  const long long stride = static_cast<long long>(gridDim.x) * kWavesPerBlock;
  long long tile = static_cast<long long>(blockIdx.x) * kWavesPerBlock + wave;
  if (tile >= n_tiles) return;

  int wcol[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) wcol[t] = col_base + (2 * r + t);
  f32x4 bv[KB][MT];
#pragma unroll
  for (int u = 0; u < KB; ++u)
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const float4 tb = *reinterpret_cast<const float4*>(W + static_cast<size_t>(wcol[t]) * ldw + 16 * u + 4 * kq);
      bv[u][t] = f32x4{tb.x, tb.y, tb.z, tb.w};
    }
  float bias[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) bias[t] = b != nullptr ? b[wcol[t]] : 0.0f;

  // chunk c = it * 64 + lane of a tile: row c / CPR = it * (64 / CPR) + lane / CPR, column chunk j = lane % CPR (CPR = 16 or 32 divides 64):
  // one per-lane offset, the rest are compile-time multiples of the row stride
  constexpr int RPI = kWave / CPR;               // rows per load instruction
  const int lr = lane / CPR, j = lane % CPR;
  auto load_tile = [&](long long tl, f32x4 (&g)[PER_LANE]) {
    const long long row0 = tl * 16;
    const int rmax = static_cast<int>(n - 1 - row0 < 15 ? n - 1 - row0 : 15);       // (wave-uniform) ragged last tile: clamp reads, mask writes
    const float* base = x + static_cast<size_t>(row0) * ldx + 4 * j;
#pragma unroll
    for (int it = 0; it < PER_LANE; ++it) {
      const int rr = it * RPI + lr;
      g[it] = *reinterpret_cast<const f32x4*>(base + static_cast<size_t>(rr < rmax ? rr : rmax) * ldx);
    }
  };
  f32x4* my = slab[wave];
  auto consume = [&](const f32x4 (&g)[PER_LANE]) {
#pragma unroll
    for (int it = 0; it < PER_LANE; ++it) {
      const int rr = it * RPI + lr;
      my[rr * CPR + (j ^ (rr & 7))] = g[it];
    }
  };
  auto compute = [&](long long tl) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KB; u += 2) {
      f32x4 cu[2];
#pragma unroll
      for (int q = 0; q < 2; ++q) cu[q] = relu_if(my[r * CPR + ((4 * (u + q) + kq) ^ (r & 7))], relu);
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(cu[q][i], bv[u + q][t][i], acc[t], 0, 0, 0);
    }
    const long long row0 = tl * 16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long orow = row0 + 4 * kq + i;
      if (orow < n) {
        const int c0 = col_base + 2 * r;
        float* dst = (split > 0 && c0 >= split) ? out2 + static_cast<size_t>(orow) * ldo + (c0 - split) : out + static_cast<size_t>(orow) * ldo + c0;
        *reinterpret_cast<float2*>(dst) = make_float2(acc[0][i] + bias[0], acc[1][i] + bias[1]);
      }
    }
    __builtin_amdgcn_wave_barrier();           // the fragment reads above precede the next tile's slab writes
  };
  f32x4 g[PER_LANE];
  load_tile(tile, g);
  while (true) {
    consume(g);
    const long long next = tile + stride;
    const bool more = next < n_tiles;
    if (more) load_tile(next, g);                // in flight during the MFMAs of this tile
    compute(tile);
    if (!more) break;
    tile = next;
  }
}

// ---- The launch decision -----------------------------------------------------------------------------------------------------
// ONE function decides which kernel instantiation a launch takes, over which columns and on what grid; the launchers below switch on
// its result and gnpde_linear_plan hands the same result to tests and A/B scripts, so the two cannot drift apart.  A launch is
// (family, mt, param): the template arguments of the kernel (gnpde_linear_launch_t in include/gnpde.h).
struct LinearShape {
  long long n;
  int d, m, ldo;
  bool aligned;        // 16-byte operand loads: ldx % 4 == 0, ldw % 4 == 0, x and W 16-byte aligned
  uintptr_t out;       // only its alignment is read
};

unsigned capped_grid(long long blocks, long long need) { return static_cast<unsigned>(blocks > need ? need : blocks); }

// the launch of MT column tiles from column `col` on
gnpde_linear_launch_t plan_tile(const LinearShape& p, int MT, int col) {
  gnpde_linear_launch_t L = {};
  L.mt = MT;
  L.col_base = col;
  L.cols = p.m - col < 16 * MT ? p.m - col : 16 * MT;
  L.grid_y = 1;
  L.block = kBlock;
  // complete 16-row tiles with complete column tiles and d % 16 == 0 take the unguarded kernel
  const bool full_cols = p.aligned && (p.d % 16 == 0) && (col + 16 * MT <= p.m);
  const long long tiles = (p.n + 15) / 16;
  const long long need = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;
  if (MT <= 2 && full_cols && p.d <= 128) {
    // persistent grid: enough wavefronts to fill the chip (8 per SIMD at these register counts would be
    // ideal; W fragments + double-buffered A cost ~150 VGPRs -> 3 per SIMD), each striding over tiles
    L.grid_x = capped_grid(256LL * 3, need);
    L.param = p.d / 16;
    // d = 64 / 128 (4 or 8 chunks per lane and tile): full-line loads transposed through LDS (linear_staged_kernel)
    if (p.d == 128 || p.d == 64) {
      if (MT == 2 && p.ldo % 2 == 0 && col % 2 == 0 && p.out % 8 == 0) {
        // paired columns on a grid of 4 workgroups per CU (3 resident: the fourth starts as one ends) -- 24.4 -> 24.0 us in the
        // headline solve, 26.9 -> 25.8 us stand-alone (profiles/r06_linear_*.txt)
        L.family = GNPDE_LINEAR_STAGED2;
        L.grid_x = capped_grid(256LL * 4, need);
      } else {
        L.family = GNPDE_LINEAR_STAGED;
      }
    } else {
      L.family = GNPDE_LINEAR_PERSISTENT;
    }
    return L;
  }
  if (MT >= 4 && full_cols && p.d <= 256) {   // W staged in LDS, persistent workgroups of 8 waves
    const long long need8 = (tiles + 7) / 8;
    L.family = GNPDE_LINEAR_LDS;
    L.block = 512;
    if (p.d <= 128) {
      L.param = 128;
      L.grid_x = capped_grid(256LL * (MT == 4 ? 4 : 2), need8);
    } else {
      L.param = 256;
      L.grid_x = capped_grid(256LL * (MT == 4 ? 2 : 1), need8);
    }
    return L;
  }
  L.family = GNPDE_LINEAR_TILE;
  L.param = 2 * (p.aligned ? 1 : 0) + (full_cols ? 1 : 0);
  L.grid_x = static_cast<unsigned>(need);
  return L;
}

// Small n (Cora: 2 708 rows, [n,80] x [80,256]): the persistent / LDS-staged kernels above are built to stream a tall x -- at 170 row
// tiles they put 22 workgroups on the chip, each staging 40 KB of W first, and need one launch per 128 output columns: 2 x 9.8 us
// per evaluation, two thirds of a launch-bound GRAND-nl evaluation on such a graph.  Here ONE launch covers all of [n, m]: a
// wavefront per (16-row tile, 32-column group), operands straight from L2, EIGHT 16-wide K blocks in flight per batch (d <= 128:
// every operand load of the wave is issued before its first MFMA -- the launch is a few dependent round trips long, nothing
// else).  Same MFMA sequence and k order per output element as
// every other variant (bit-identical results).
constexpr long long kSmallLinearTiles = 2048;      // n <= 32 768 rows

// The launch that starts at column `col` (col < m); the next one starts at col + 16 * mt of what this returns, until that reaches m.
gnpde_linear_launch_t plan_next(const LinearShape& p, int col) {
  const long long tiles = (p.n + 15) / 16;
  if (p.aligned && col == 0 && tiles <= kSmallLinearTiles && p.d % 16 == 0 && p.m % 16 == 0) {
    gnpde_linear_launch_t L = {};
    L.family = GNPDE_LINEAR_SMALL;
    L.mt = p.m % 32 == 0 ? 2 : 1;
    L.cols = p.m;
    L.grid_x = static_cast<unsigned>((tiles + kWavesPerBlock - 1) / kWavesPerBlock);
    L.grid_y = static_cast<unsigned>(p.m / (16 * L.mt));
    L.block = kBlock;
    return L;
  }
  const int rem = (p.m - col + 15) / 16;
  return plan_tile(p, rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1, col);
}

int columns_advanced(const gnpde_linear_launch_t& L) { return L.family == GNPDE_LINEAR_SMALL ? L.cols : 16 * L.mt; }

// Launch what the plan says: nothing here looks at the shape again.
int launch_planned(const gnpde_linear_launch_t& L, const float* x, int n, int d, int ldx, const float* W, int m, int ldw, const float* b,
                   float* out, int ldo, hipStream_t s, int relu, float* out2 = nullptr, int split = 0) {
  const dim3 grid(L.grid_x, L.grid_y), block(L.block);
  const int col = L.col_base;
  const int key = L.mt * 1000 + L.param;
#define GNPDE_LK(KEY, ...) \
  case KEY: hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, s, x, n, d, ldx, W, m, ldw, b, out, ldo, col, 0, relu); return 0
#define GNPDE_LP(KEY, ...) \
  case KEY: hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, s, x, n, ldx, W, ldw, b, out, ldo, col, relu); return 0
#define GNPDE_LL(KEY, ...) \
  case KEY: hipLaunchKernelGGL((__VA_ARGS__), grid, block, 0, s, x, n, d, ldx, W, ldw, b, out, ldo, col, relu); return 0
  switch (L.family) {
    case GNPDE_LINEAR_SMALL:
      switch (key) {
        GNPDE_LK(1000, linear_kernel<1, true, true, 8>);
        GNPDE_LK(2000, linear_kernel<2, true, true, 8>);
        default: break;
      }
      break;
    case GNPDE_LINEAR_STAGED2:
      switch (key) {
        case 2004: hipLaunchKernelGGL((linear_staged2_kernel<4>), grid, block, 0, s, x, n, ldx, W, ldw, b, out, ldo, col, relu, out2, split); return 0;
        case 2008: hipLaunchKernelGGL((linear_staged2_kernel<8>), grid, block, 0, s, x, n, ldx, W, ldw, b, out, ldo, col, relu, out2, split); return 0;
        default: break;
      }
      break;
    case GNPDE_LINEAR_STAGED:
      switch (key) {
        GNPDE_LP(1004, linear_staged_kernel<1, 4>);
        GNPDE_LP(1008, linear_staged_kernel<1, 8>);
        GNPDE_LP(2004, linear_staged_kernel<2, 4>);
        GNPDE_LP(2008, linear_staged_kernel<2, 8>);
        default: break;
      }
      break;
    case GNPDE_LINEAR_PERSISTENT:
      switch (key) {
        GNPDE_LP(1001, linear_persistent_kernel<1, 1>);
        GNPDE_LP(1002, linear_persistent_kernel<1, 2>);
        GNPDE_LP(1003, linear_persistent_kernel<1, 3>);
        GNPDE_LP(1005, linear_persistent_kernel<1, 5>);
        GNPDE_LP(1006, linear_persistent_kernel<1, 6>);
        GNPDE_LP(1007, linear_persistent_kernel<1, 7>);
        GNPDE_LP(2001, linear_persistent_kernel<2, 1>);
        GNPDE_LP(2002, linear_persistent_kernel<2, 2>);
        GNPDE_LP(2003, linear_persistent_kernel<2, 3>);
        GNPDE_LP(2005, linear_persistent_kernel<2, 5>);
        GNPDE_LP(2006, linear_persistent_kernel<2, 6>);
        GNPDE_LP(2007, linear_persistent_kernel<2, 7>);
        default: break;
      }
      break;
    case GNPDE_LINEAR_LDS:
      switch (key) {
        GNPDE_LL(4128, linear_lds_kernel<4, 128>);
        GNPDE_LL(4256, linear_lds_kernel<4, 256>);
        GNPDE_LL(8128, linear_lds_kernel<8, 128>);
        GNPDE_LL(8256, linear_lds_kernel<8, 256>);
        default: break;
      }
      break;
    case GNPDE_LINEAR_TILE:
      switch (key) {   // param = 2 * ALIGNED + FULL
        GNPDE_LK(1003, linear_kernel<1, true, true>);
        GNPDE_LK(1002, linear_kernel<1, true, false>);
        GNPDE_LK(1000, linear_kernel<1, false, false>);
        GNPDE_LK(2003, linear_kernel<2, true, true>);
        GNPDE_LK(2002, linear_kernel<2, true, false>);
        GNPDE_LK(2000, linear_kernel<2, false, false>);
        GNPDE_LK(4003, linear_kernel<4, true, true>);
        GNPDE_LK(4002, linear_kernel<4, true, false>);
        GNPDE_LK(4000, linear_kernel<4, false, false>);
        GNPDE_LK(8003, linear_kernel<8, true, true>);
        GNPDE_LK(8002, linear_kernel<8, true, false>);
        GNPDE_LK(8000, linear_kernel<8, false, false>);
        default: break;
      }
      break;
    default: break;
  }
#undef GNPDE_LK
#undef GNPDE_LP
#undef GNPDE_LL
  set_error("linear: the plan names no kernel (family %d, mt %d, param %d)", L.family, L.mt, L.param);
  return GNPDE_ESHAPE;
}

bool operands_aligned(uintptr_t x, int ldx, uintptr_t W, int ldw) { return ldx % 4 == 0 && ldw % 4 == 0 && x % 16 == 0 && W % 16 == 0; }

// the one launch of gnpde_linear_split: the paired-column staged kernel over both tables
gnpde_linear_launch_t plan_split(long long n, int d) {
  gnpde_linear_launch_t L = {};
  const long long tiles = (n + 15) / 16;
  L.family = GNPDE_LINEAR_STAGED2;
  L.mt = 2;
  L.param = d / 16;
  L.split = 1;
  L.cols = 32;
  L.grid_x = capped_grid(256LL * 4, (tiles + kWavesPerBlock - 1) / kWavesPerBlock);
  L.grid_y = 1;
  L.block = kBlock;
  return L;
}

}  // namespace

// The q||k projection as two tables (q [n, A], k [n, A]): offered where a key row is shorter than a 128-byte line and the launch would
// take the staged kernel anyway (tall x, d = 64 / 128, 2A = 32 output columns, 16-byte aligned operands).
bool linear_split_supported(const float* x, long long n, int d, int ldx, const float* W, int m, int ldw, int split) {
  const long long tiles = (n + 15) / 16;
  return m == 32 && split == 16 && (d == 64 || d == 128) && tiles > kSmallLinearTiles &&
         operands_aligned(reinterpret_cast<uintptr_t>(x), ldx, reinterpret_cast<uintptr_t>(W), ldw) && g_tune[GNPDE_TUNE_KEY_TABLE] != 1;
}

int launch_linear_split(const float* x, int n, int d, int ldx, const float* W, int m, int ldw, const float* b, float* out_q, float* out_k,
                        int split, hipStream_t s) {
  GNPDE_CHECK_ARG(x && W && out_q && out_k && linear_split_supported(x, n, d, ldx, W, m, ldw, split) &&
                  reinterpret_cast<uintptr_t>(out_q) % 8 == 0 && reinterpret_cast<uintptr_t>(out_k) % 8 == 0, GNPDE_ESHAPE,
                  "linear_split: shape without a two-table kernel (see linear_split_supported)");
  if (int rc = launch_planned(plan_split(n, d), x, n, d, ldx, W, m, ldw, b, out_q, split, s, 0, out_k, split)) return rc;
  GNPDE_LAUNCH_CHECK();
  return 0;
}

int launch_linear_any(const float* x, int n, int d, int ldx, const float* W, int m, int ldw, const float* b, float* out,
                      int ldo, hipStream_t s, int relu) {
  GNPDE_CHECK_ARG(x && W && out, GNPDE_EINVAL, "linear: null pointer");
  GNPDE_CHECK_ARG(n >= 0 && d >= 1 && m >= 1 && ldx >= d && ldw >= d && ldo >= m, GNPDE_EINVAL,
                  "linear: bad shape n=%d d=%d m=%d ldx=%d ldw=%d ldo=%d", n, d, m, ldx, ldw, ldo);
  if (n == 0) return 0;
  const LinearShape p = {n, d, m, ldo, operands_aligned(reinterpret_cast<uintptr_t>(x), ldx, reinterpret_cast<uintptr_t>(W), ldw),
                         reinterpret_cast<uintptr_t>(out)};
  for (int col = 0; col < m;) {
    const gnpde_linear_launch_t L = plan_next(p, col);
    if (int rc = launch_planned(L, x, n, d, ldx, W, m, ldw, b, out, ldo, s, relu)) return rc;
    col += columns_advanced(L);
  }
  GNPDE_LAUNCH_CHECK();
  return 0;
}

int linear_plan(uintptr_t x, int n, int d, int ldx, uintptr_t W, int m, int ldw, uintptr_t out, int ldo, gnpde_linear_launch_t* plan, int cap) {
  GNPDE_CHECK_ARG(n >= 0 && d >= 1 && m >= 1 && ldx >= d && ldw >= d && ldo >= m, GNPDE_EINVAL,
                  "linear_plan: bad shape n=%d d=%d m=%d ldx=%d ldw=%d ldo=%d", n, d, m, ldx, ldw, ldo);
  GNPDE_CHECK_ARG(cap >= 0 && (plan != nullptr || cap == 0), GNPDE_EINVAL, "linear_plan: cap = %d entries without a buffer", cap);
  if (n == 0) return 0;
  const LinearShape p = {n, d, m, ldo, operands_aligned(x, ldx, W, ldw), out};
  int count = 0;
  for (int col = 0; col < m; ++count) {
    const gnpde_linear_launch_t L = plan_next(p, col);
    if (count < cap) plan[count] = L;
    col += columns_advanced(L);
  }
  return count;
}

int linear_split_plan(uintptr_t x, int n, int d, int ldx, uintptr_t W, int m, int ldw, uintptr_t out_q, uintptr_t out_k, int split,
                      gnpde_linear_launch_t* plan) {
  GNPDE_CHECK_ARG(plan != nullptr, GNPDE_EINVAL, "linear_split_plan: null plan");
  GNPDE_CHECK_ARG(linear_split_supported(reinterpret_cast<const float*>(x), n, d, ldx, reinterpret_cast<const float*>(W), m, ldw, split) &&
                  out_q % 8 == 0 && out_k % 8 == 0, GNPDE_ESHAPE,
                  "linear_split_plan: shape without a two-table kernel (see linear_split_supported)");
  *plan = plan_split(n, d);
  return 1;
}

}  // namespace gnpde

extern "C" int gnpde_linear(const float* x, int32_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw,
                            const float* b, float* out, int32_t ldo, void* stream) {
  return gnpde::launch_linear_any(x, n, d, ldx, W, m, ldw, b, out, ldo, static_cast<hipStream_t>(stream), 0);
}

extern "C" int gnpde_linear_split_supported(const float* x, int64_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw, int32_t split) {
  return gnpde::linear_split_supported(x, n, d, ldx, W, m, ldw, split) ? 1 : 0;
}

extern "C" int gnpde_linear_split(const float* x, int32_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw, const float* b,
                                  float* out_q, float* out_k, int32_t split, void* stream) {
  return gnpde::launch_linear_split(x, n, d, ldx, W, m, ldw, b, out_q, out_k, split, static_cast<hipStream_t>(stream));
}

extern "C" int gnpde_linear_plan(uint64_t x_addr, int32_t n, int32_t d, int32_t ldx, uint64_t w_addr, int32_t m, int32_t ldw, uint64_t out_addr,
                                 int32_t ldo, gnpde_linear_launch_t* plan, int32_t cap) {
  return gnpde::linear_plan(static_cast<uintptr_t>(x_addr), n, d, ldx, static_cast<uintptr_t>(w_addr), m, ldw, static_cast<uintptr_t>(out_addr), ldo,
                            plan, cap);
}

extern "C" int gnpde_linear_split_plan(uint64_t x_addr, int32_t n, int32_t d, int32_t ldx, uint64_t w_addr, int32_t m, int32_t ldw,
                                       uint64_t out_q_addr, uint64_t out_k_addr, int32_t split, gnpde_linear_launch_t* plan) {
  return gnpde::linear_split_plan(static_cast<uintptr_t>(x_addr), n, d, ldx, static_cast<uintptr_t>(w_addr), m, ldw,
                                  static_cast<uintptr_t>(out_q_addr), static_cast<uintptr_t>(out_k_addr), split, plan);
}

extern "C" int gnpde_relu_linear(const float* x, int32_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw,
                                 const float* b, float* out, int32_t ldo, void* stream) {
  return gnpde::launch_linear_any(x, n, d, ldx, W, m, ldw, b, out, ldo, static_cast<hipStream_t>(stream), 1);
}
