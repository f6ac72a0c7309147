// Approximate personalised PageRank by forward push (Andersen-Chung-Lang), the `exact = False` branch of graph diffusion rewiring
// (reference src/graph_rewiring.py:389-392 -> torch_geometric's GDC.diffusion_matrix_approx / __calc_ppr__).  One workgroup per
// source; nothing of size n x n exists.  include/gnpde.h defines the result; DESIGN.md section 4d has the error bound.
//
//   numbers    estimates p and residuals r are 64-bit FIXED-POINT integers, one quantum = 2^-60.  Integer adds commute, so the
//              integer atomics below give one result whatever order the adds arrive in.  No floating-point arithmetic happens
//              before the single conversion of an output value to fp32.
//   rounds     synchronous: (A) every touched node u whose residual is >= alpha eps deg(u) (the source unconditionally in round 0)
//              moves its residual res to p(u) and is listed; barrier; (B) every listed node adds floor(floor((1 - alpha) res) /
//              deg(u)) to the residual of each node of its row; barrier.  The active set of a round is a function of the state
//              at its start and phase B is a sum of integers: the state after every round, hence the result, is a function of
//              (graph, source, alpha, eps) alone -- not of the launch geometry, the batch or the store.
//   fast       the state of a source is an LDS hash (2048 slots, linear probing, at most 1536 distinct nodes; 16-lane groups walk
//              the rows of the listed nodes).  Cleared per source: O(slots), never O(n).
//   slow       a source whose support outgrows the hash is listed and a second kernel of the SAME call runs it again from the start
//              on a per-workgroup scratch in global memory (dense r / p / stamp arrays with a touched list; cleared once per call by the groups that have work, reset through that list per source).
//              Same integers, same rounds: bit-identical to what the fast store would have given.
//   output     count pass: entries with p > 0 per source.  fill pass (the push again): those nodes sorted ascending (bitonic sort
//              by the workgroup) -> (s, u, fp32(p)) at offsets[s].  residual pass: fp32(r) scattered into a dense [n_src, n] array.
#include "common.h"
#include <cmath>

namespace gnpde {
namespace {

typedef unsigned long long u64;

constexpr int kPushSlots = 2048;            // hash slots of the fast store (a power of two)
constexpr int kPushHashShift = 32 - 11;
constexpr int kPushMaxFill = 1536;          // distinct nodes the fast store accepts; a thread inserts at most one node past
                                            // that before it sees the overflow flag: 1536 + 256 < 2048, probing always ends
constexpr int kPushGroup = 16;              // lanes that share the row of one listed node
constexpr int kPushFrac = 60;               // one quantum = 2^-60
constexpr unsigned kPushEmpty = 0xffffffffu;
constexpr int kPushMaxRounds = 1 << 22;     // never reached (every push moves >= 1 quantum into p); a guard against a hang
constexpr int kPushMaxBlocks = 2048;
constexpr int kPushMaxSlowGroups = 1024;
constexpr long long kPushResidMaxN = 4096;

enum { PUSH_COUNT = 0, PUSH_FILL = 1, PUSH_RESID = 2 };
enum { PUSH_ST_ROUNDS = 1, PUSH_ST_INDEX = 2, PUSH_ST_OFFSETS = 4 };

struct PushArgs {
  const int* rowptr;
  const int* col;
  long long n, s0, n_src;
  u64 alpha_fx, beta64, thr_unit;
  int max_fill, mode;
  long long* counts;
  const long long* offsets;
  long long* out_ei;
  long long out_ld;
  float* out_p;
  float* resid;
  int* n_overflow;
  int* overflow_list;
  u64* info;                // [0] += sources on the slow path, [1] |= PUSH_ST_*
};

__device__ __forceinline__ float push_to_float(u64 q) { return __ull2float_rn(q) * 0x1p-60f; }   // one rounding

// ascending bitonic sort of b[0 .. P) (P a power of two >= 2) by the whole workgroup; b in LDS or global memory
__device__ __forceinline__ void block_sort(unsigned* b, long long P, int tid) {      // 64-bit: P reaches 2^31 for n near INT32_MAX
  for (long long size = 2; size <= P; size <<= 1) {
    for (long long stride = size >> 1; stride > 0; stride >>= 1) {
      for (long long q = tid; q < (P >> 1); q += kBlock) {
        const long long i = ((q & ~(stride - 1)) << 1) | (q & (stride - 1));
        const long long j = i | stride;
        const bool up = (i & size) == 0;
        const unsigned a = b[i], c = b[j];
        if ((a > c) == up) {
          b[i] = c;
          b[j] = a;
        }
      }
      __syncthreads();
    }
  }
}

struct PushShared {
  int nact, fill, ovf, cnt;
};

// LDS hash: slot = position in the table
struct FastStore {
  unsigned* keys;
  u64* r;
  u64* p;
  unsigned short* aslot;
  u64* ares;
  PushShared* sh;
  int max_fill;

  __device__ __forceinline__ int iter_count() const { return kPushSlots; }
  __device__ __forceinline__ unsigned node_at(int i) const { return keys[i]; }
  __device__ __forceinline__ unsigned slot_of(int i, unsigned) const { return static_cast<unsigned>(i); }
  __device__ __forceinline__ u64 load_r(unsigned s) const { return r[s]; }
  __device__ __forceinline__ void store_r(unsigned s, u64 v) { r[s] = v; }
  __device__ __forceinline__ void add_r(unsigned s, u64 v) { atomicAdd(&r[s], v); }
  __device__ __forceinline__ u64 load_p(unsigned s) const { return p[s]; }
  __device__ __forceinline__ void store_p(unsigned s, u64 v) { p[s] = v; }
  __device__ __forceinline__ void list(int a, unsigned s, unsigned, u64 res) {
    aslot[a] = static_cast<unsigned short>(s);
    ares[a] = res;
  }
  __device__ __forceinline__ unsigned listed_slot(int a) const { return aslot[a]; }
  __device__ __forceinline__ unsigned listed_node(int a) const { return keys[aslot[a]]; }
  __device__ __forceinline__ u64 listed_res(int a) const { return ares[a]; }
  __device__ __forceinline__ unsigned* sort_buffer() { return reinterpret_cast<unsigned*>(ares); }   // 1536 * 8 >= 2048 * 4 bytes
  __device__ __forceinline__ unsigned find(unsigned w) const {
    unsigned h = (w * 2654435761u) >> kPushHashShift;
    while (keys[h] != w) h = (h + 1) & (kPushSlots - 1);       // w is in the table
    return h;
  }
  __device__ __forceinline__ unsigned insert(unsigned w) {
    unsigned h = (w * 2654435761u) >> kPushHashShift;
    for (;;) {
      unsigned k = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (k == kPushEmpty) {
        k = atomicCAS(&keys[h], kPushEmpty, w);
        if (k == kPushEmpty) {
          if (atomicAdd(&sh->fill, 1) >= max_fill) sh->ovf = 1;
          return h;
        }
      }
      if (k == w) return h;
      h = (h + 1) & (kPushSlots - 1);
    }
  }
  __device__ __forceinline__ void reset(int tid) {
    for (int i = tid; i < kPushSlots; i += kBlock) {
      keys[i] = kPushEmpty;
      r[i] = 0;
      p[i] = 0;
    }
  }
};

// per-workgroup scratch in global memory: slot = node.  r / p / stamp are all zero between sources.  Values other waves of the
// workgroup have changed through atomics are read with agent-scope loads.
struct SlowStore {
  u64* r;
  u64* p;
  u64* ares;
  unsigned* stamp;
  unsigned* touched;
  unsigned* anode;          // listed nodes; the sort buffer of the fill pass (npad entries)
  PushShared* sh;

  __device__ __forceinline__ int iter_count() const { return sh->fill; }
  __device__ __forceinline__ unsigned node_at(int i) const { return touched[i]; }
  __device__ __forceinline__ unsigned slot_of(int, unsigned node) const { return node; }
  __device__ __forceinline__ u64 load_r(unsigned s) const { return __hip_atomic_load(&r[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void store_r(unsigned s, u64 v) { __hip_atomic_store(&r[s], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void add_r(unsigned s, u64 v) { atomicAdd(&r[s], v); }
  __device__ __forceinline__ u64 load_p(unsigned s) const { return p[s]; }
  __device__ __forceinline__ void store_p(unsigned s, u64 v) { p[s] = v; }
  __device__ __forceinline__ void list(int a, unsigned, unsigned node, u64 res) {
    anode[a] = node;
    ares[a] = res;
  }
  __device__ __forceinline__ unsigned listed_slot(int a) const { return anode[a]; }
  __device__ __forceinline__ unsigned listed_node(int a) const { return anode[a]; }
  __device__ __forceinline__ u64 listed_res(int a) const { return ares[a]; }
  __device__ __forceinline__ unsigned* sort_buffer() { return anode; }
  __device__ __forceinline__ unsigned find(unsigned w) const { return w; }
  __device__ __forceinline__ unsigned insert(unsigned w) {
    if (atomicExch(&stamp[w], 1u) == 0u) touched[atomicAdd(&sh->fill, 1)] = w;
    return w;
  }
  __device__ __forceinline__ void reset(int tid) {
    const int nt = sh->fill;
    for (int i = tid; i < nt; i += kBlock) {
      const unsigned v = touched[i];
      store_r(v, 0);
      p[v] = 0;
      __hip_atomic_store(&stamp[v], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};

// The push of source s_local (node a.s0 + s_local) on `st` (empty on entry, left as the push ends) and its output.  Returns false
// when the store overflowed (nothing is written then).  Every thread of the workgroup calls it with the same arguments.
template <class Store>
__device__ bool push_source(const PushArgs& a, Store& st, long long s_local, int tid) {
  PushShared* sh = st.sh;
  const unsigned src = static_cast<unsigned>(a.s0 + s_local);
  if (tid == 0) {
    sh->nact = 0;
    sh->fill = 0;
    sh->ovf = 0;
    sh->cnt = 0;
  }
  __syncthreads();
  if (tid == 0) st.store_r(st.insert(src), a.alpha_fx);
  __syncthreads();
  if (sh->ovf) return false;
  unsigned status = 0;
  bool done = false;
  for (int round = 0; round < kPushMaxRounds; ++round) {
    // (A) the round's active set: residual -> estimate, listed with the amount to spread
    const int ni = st.iter_count();
    for (int i = tid; i < ni; i += kBlock) {
      const unsigned v = st.node_at(i);
      if (v == kPushEmpty) continue;
      const unsigned s = st.slot_of(i, v);
      const u64 res = st.load_r(s);
      if (res == 0) continue;
      bool active = round == 0;               // only the source is in the store then
      if (!active) {
        const u64 deg = static_cast<u64>(a.rowptr[v + 1] - a.rowptr[v]);
        active = __umul64hi(a.thr_unit, deg) == 0 && res >= a.thr_unit * deg;
      }
      if (active) {
        st.store_p(s, st.load_p(s) + res);
        st.store_r(s, 0);
        st.list(atomicAdd(&sh->nact, 1), s, v, res);
      }
    }
    __syncthreads();
    const int na = sh->nact;
    if (na == 0) {
      done = true;
      break;
    }
    // (B) spread: 16 lanes per listed node
    const int lane = tid & (kPushGroup - 1);
    for (int q = tid / kPushGroup; q < na; q += kBlock / kPushGroup) {
      const unsigned v = st.listed_node(q);
      const int b = a.rowptr[v], e = a.rowptr[v + 1];
      if (e <= b) continue;
      const u64 share = __umul64hi(st.listed_res(q), a.beta64) / static_cast<u64>(e - b);
      if (share == 0) continue;
      for (int i = b + lane; i < e; i += kPushGroup) {
        // an overflowing source is abandoned: stop inserting, so that a thread adds at most one node past the limit
        if (__hip_atomic_load(&sh->ovf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
        const unsigned w = static_cast<unsigned>(a.col[i]);
        if (static_cast<long long>(w) >= a.n) {
          status |= PUSH_ST_INDEX;
          continue;
        }
        st.add_r(st.insert(w), share);
      }
    }
    __syncthreads();
    if (sh->ovf) break;
    if (tid == 0) sh->nact = 0;
    __syncthreads();
  }
  if (sh->ovf) {
    if (status) atomicOr(&a.info[1], static_cast<u64>(status));
    return false;
  }
  if (!done) status |= PUSH_ST_ROUNDS;
  // output
  const int ni = st.iter_count();
  if (a.mode == PUSH_RESID) {
    for (int i = tid; i < ni; i += kBlock) {
      const unsigned v = st.node_at(i);
      if (v != kPushEmpty) a.resid[s_local * a.n + v] = push_to_float(st.load_r(st.slot_of(i, v)));
    }
  } else {
    unsigned* buf = st.sort_buffer();
    for (int i = tid; i < ni; i += kBlock) {
      const unsigned v = st.node_at(i);
      if (v == kPushEmpty || st.load_p(st.slot_of(i, v)) == 0) continue;
      const int at = atomicAdd(&sh->cnt, 1);
      if (a.mode == PUSH_FILL) buf[at] = v;
    }
    __syncthreads();
    const int cnt = sh->cnt;
    if (a.mode == PUSH_COUNT) {
      if (tid == 0) a.counts[s_local] = cnt;
    } else {
      const long long off = a.offsets[s_local];
      if (a.offsets[s_local + 1] - off != cnt) {
        status |= PUSH_ST_OFFSETS;            // not the offsets of this push's count pass: nothing is written
      } else if (cnt > 0) {
        long long P = 2;
        while (P < cnt) P <<= 1;
        for (long long i = static_cast<long long>(cnt) + tid; i < P; i += kBlock) buf[i] = kPushEmpty;
        __syncthreads();
        block_sort(buf, P, tid);
        for (int i = tid; i < cnt; i += kBlock) {
          const unsigned v = buf[i];
          a.out_ei[off + i] = static_cast<long long>(src);
          a.out_ei[a.out_ld + off + i] = static_cast<long long>(v);
          a.out_p[off + i] = push_to_float(st.load_p(st.find(v)));
        }
      }
    }
  }
  if (status) atomicOr(&a.info[1], static_cast<u64>(status));
  __syncthreads();
  return true;
}

__global__ __launch_bounds__(kBlock) void gdc_push_fast_kernel(PushArgs a) {
  __shared__ unsigned keys[kPushSlots];
  __shared__ u64 r[kPushSlots];
  __shared__ u64 p[kPushSlots];
  __shared__ u64 ares[kPushMaxFill];
  __shared__ unsigned short aslot[kPushMaxFill];
  __shared__ PushShared sh;
  const int tid = threadIdx.x;
  FastStore st{keys, r, p, aslot, ares, &sh, a.max_fill};
  for (long long s = blockIdx.x; s < a.n_src; s += gridDim.x) {
    st.reset(tid);
    __syncthreads();
    const bool ok = push_source(a, st, s, tid);
    if (!ok && tid == 0) a.overflow_list[atomicAdd(a.n_overflow, 1)] = static_cast<int>(s);
    __syncthreads();
  }
}

struct SlowLayout {
  size_t r, p, ares, stamp, touched, anode, per_group;
};

__host__ __device__ inline size_t push_align(size_t v) { return (v + 255) / 256 * 256; }

__host__ __device__ inline SlowLayout slow_layout(long long n) {
  size_t npad = 2;
  while (npad < static_cast<size_t>(n)) npad <<= 1;
  SlowLayout L;
  const size_t N = static_cast<size_t>(n);
  L.r = 0;
  L.p = L.r + push_align(N * 8);
  L.ares = L.p + push_align(N * 8);
  L.stamp = L.ares + push_align(N * 8);
  L.touched = L.stamp + push_align(N * 4);
  L.anode = L.touched + push_align(N * 4);
  L.per_group = L.anode + push_align(npad * 4);
  return L;
}

__global__ __launch_bounds__(kBlock) void gdc_push_slow_kernel(PushArgs a, char* scratch) {
  __shared__ PushShared sh;
  const int tid = threadIdx.x;
  const SlowLayout L = slow_layout(a.n);
  char* base = scratch + static_cast<size_t>(blockIdx.x) * L.per_group;
  SlowStore st{reinterpret_cast<u64*>(base + L.r), reinterpret_cast<u64*>(base + L.p), reinterpret_cast<u64*>(base + L.ares),
               reinterpret_cast<unsigned*>(base + L.stamp), reinterpret_cast<unsigned*>(base + L.touched),
               reinterpret_cast<unsigned*>(base + L.anode), &sh};
  const int total = *a.n_overflow;
  if (blockIdx.x == 0 && tid == 0 && a.mode == PUSH_COUNT) a.info[0] += static_cast<u64>(total);
  if (static_cast<int>(blockIdx.x) >= total) return;       // no work: this group's scratch is not touched at all
  // r / p / stamp start all zero and every source leaves them so: O(n) once per call and group, only for groups that have work
  for (long long i = tid; i < a.n; i += kBlock) {
    st.r[i] = 0;
    st.p[i] = 0;
    st.stamp[i] = 0u;
  }
  __threadfence();
  __syncthreads();
  for (int i = blockIdx.x; i < total; i += gridDim.x) {
    push_source(a, st, static_cast<long long>(a.overflow_list[i]), tid);      // (this store cannot overflow)
    st.reset(tid);
    __syncthreads();
  }
}

struct PushWs {
  size_t list, scratch, total;
};

PushWs push_ws(long long n, long long n_src, int groups) {
  PushWs W;
  W.list = 256;
  W.scratch = W.list + push_align(static_cast<size_t>(n_src) * sizeof(int));
  W.total = W.scratch + static_cast<size_t>(groups) * slow_layout(n).per_group;
  return W;
}

bool push_fixed_point(double alpha, double eps, PushArgs* a) {
  const long double one = ldexpl(1.0L, kPushFrac);
  a->alpha_fx = static_cast<u64>(floorl(static_cast<long double>(alpha) * one));
  a->beta64 = static_cast<u64>(floorl(ldexpl(1.0L - static_cast<long double>(alpha), 64)));
  long double t = floorl(static_cast<long double>(alpha) * static_cast<long double>(eps) * one);
  if (t > one) t = one;                    // more than the whole mass: only the source is ever pushed
  a->thr_unit = static_cast<u64>(t);
  return a->thr_unit >= 1 && a->alpha_fx >= 1;
}

int push_run(const char* what, int mode, const gnpde_graph_t* g, long long s0, long long n_src, double alpha, double eps, int capacity,
             int slow_groups, long long* counts, const long long* offsets, long long* out_ei, long long out_ld, float* out_p,
             float* resid, long long* info, void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(g != nullptr && g->n >= 1 && g->rowptr != nullptr && (g->colidx != nullptr || g->e == 0), GNPDE_EINVAL,
                  "%s: no graph / no nodes", what);
  GNPDE_CHECK_ARG(g->row_begin == 0, GNPDE_EINVAL, "%s: the graph is a row range of a partitioned graph", what);
  GNPDE_CHECK_ARG(s0 >= 0 && n_src >= 1 && s0 <= g->n - n_src, GNPDE_EINVAL, "%s: sources [%lld, %lld + %lld) outside [0, %d)", what, s0,
                  s0, n_src, g->n);
  GNPDE_CHECK_ARG(alpha > 0.0 && alpha < 1.0, GNPDE_EINVAL, "%s: alpha = %g outside (0, 1)", what, alpha);
  GNPDE_CHECK_ARG(eps > 0.0 && std::isfinite(eps), GNPDE_EINVAL, "%s: eps = %g is not a positive finite number", what, eps);
  GNPDE_CHECK_ARG(capacity >= -1, GNPDE_EINVAL, "%s: capacity = %d (-1: the built-in %d, 0: every source on the slow path)", what, capacity,
                  kPushMaxFill);
  GNPDE_CHECK_ARG(slow_groups >= 1 && slow_groups <= kPushMaxSlowGroups, GNPDE_ESHAPE, "%s: slow_groups = %d outside 1 .. %d", what,
                  slow_groups, kPushMaxSlowGroups);
  PushArgs a;
  GNPDE_CHECK_ARG(push_fixed_point(alpha, eps, &a), GNPDE_EINVAL, "%s: alpha eps = %g is below the fixed-point quantum 2^-%d", what,
                  alpha * eps, kPushFrac);
  GNPDE_CHECK_ARG(info != nullptr, GNPDE_EINVAL, "%s: null info", what);
  if (mode == PUSH_COUNT) GNPDE_CHECK_ARG(counts != nullptr, GNPDE_EINVAL, "%s: null counts", what);
  if (mode == PUSH_FILL)
    GNPDE_CHECK_ARG(offsets != nullptr && out_ei != nullptr && out_p != nullptr && out_ld >= 0, GNPDE_EINVAL, "%s: null pointer", what);
  if (mode == PUSH_RESID) {
    GNPDE_CHECK_ARG(g->n <= kPushResidMaxN, GNPDE_ESHAPE, "%s: the dense [n_sources, n] residual read-out is for n <= %lld (n = %d)", what,
                    kPushResidMaxN, g->n);
    GNPDE_CHECK_ARG(resid != nullptr, GNPDE_EINVAL, "%s: null residuals", what);
  }
  const PushWs W = push_ws(g->n, n_src, slow_groups);
  GNPDE_CHECK_ARG(workspace != nullptr && workspace_bytes >= W.total, GNPDE_EWS, "%s: workspace too small", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  a.rowptr = g->rowptr;
  a.col = g->colidx;
  a.n = g->n;
  a.s0 = s0;
  a.n_src = n_src;
  a.max_fill = capacity < 0 || capacity > kPushMaxFill ? kPushMaxFill : capacity;
  a.mode = mode;
  a.counts = counts;
  a.offsets = offsets;
  a.out_ei = out_ei;
  a.out_ld = out_ld;
  a.out_p = out_p;
  a.resid = resid;
  a.n_overflow = reinterpret_cast<int*>(ws);
  a.overflow_list = reinterpret_cast<int*>(ws + W.list);
  a.info = reinterpret_cast<u64*>(info);
  GNPDE_HIP(hipMemsetAsync(ws, 0, 256, s));       // the overflow counter; the slow kernel clears the scratch of the groups it uses
  if (mode == PUSH_RESID) GNPDE_HIP(hipMemsetAsync(resid, 0, static_cast<size_t>(n_src) * static_cast<size_t>(g->n) * sizeof(float), s));
  const unsigned blocks = static_cast<unsigned>(n_src < kPushMaxBlocks ? n_src : kPushMaxBlocks);
  hipLaunchKernelGGL(gdc_push_fast_kernel, dim3(blocks), dim3(kBlock), 0, s, a);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(gdc_push_slow_kernel, dim3(static_cast<unsigned>(slow_groups)), dim3(kBlock), 0, s, a, ws + W.scratch);
  GNPDE_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

extern "C" size_t gnpde_gdc_push_workspace_bytes(int64_t n, int64_t n_sources, int32_t slow_groups) {
  if (n < 1 || n > INT32_MAX || n_sources < 1 || n_sources > n || slow_groups < 1 || slow_groups > kPushMaxSlowGroups) return 0;
  return push_ws(n, n_sources, slow_groups).total;
}

extern "C" int gnpde_gdc_push_count(const gnpde_graph_t* g, int64_t s0, int64_t n_sources, double alpha, double eps, int32_t capacity,
                                    int32_t slow_groups, int64_t* counts, int64_t* info, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return push_run("gdc_push_count", PUSH_COUNT, g, s0, n_sources, alpha, eps, capacity, slow_groups, reinterpret_cast<long long*>(counts),
                  nullptr, nullptr, 0, nullptr, nullptr, reinterpret_cast<long long*>(info), workspace, workspace_bytes, stream);
}

extern "C" int gnpde_gdc_push_fill(const gnpde_graph_t* g, int64_t s0, int64_t n_sources, double alpha, double eps, int32_t capacity,
                                   int32_t slow_groups, const int64_t* offsets, int64_t* out_edge_index, int64_t out_ld, float* out_p,
                                   int64_t* info, void* workspace, size_t workspace_bytes, void* stream) {
  return push_run("gdc_push_fill", PUSH_FILL, g, s0, n_sources, alpha, eps, capacity, slow_groups, nullptr,
                  reinterpret_cast<const long long*>(offsets), reinterpret_cast<long long*>(out_edge_index), out_ld, out_p, nullptr,
                  reinterpret_cast<long long*>(info), workspace, workspace_bytes, stream);
}

extern "C" int gnpde_gdc_push_residuals(const gnpde_graph_t* g, int64_t s0, int64_t n_sources, double alpha, double eps, int32_t capacity,
                                        int32_t slow_groups, float* residuals, int64_t* info, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  return push_run("gdc_push_residuals", PUSH_RESID, g, s0, n_sources, alpha, eps, capacity, slow_groups, nullptr, nullptr, nullptr, 0,
                  nullptr, residuals, reinterpret_cast<long long*>(info), workspace, workspace_bytes, stream);
}
