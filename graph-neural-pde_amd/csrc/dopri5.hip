// dopri5 with the step-size controller on the device (see gnpde.h, gnpde_dopri5_*): torchdiffeq 0.2.1's
// RKAdaptiveStepsizeODESolver / Dopri5Solver as the reference reaches it with its default opt['method'] = 'dopri5'
// (src/block_constant.py:57-62, src/block_transformer_attention.py:58-63; re-stated in src/early_stop_solver.py:30-128).
//
// torchdiffeq runs the accept / reject decision and the step-size update in Python: one device->host read of the error ratio and
// ~40 eager launches per trial step.  Here ONE trial step is ONE hipGraph of 6 evaluations of f + 3 small kernels, which take
// everything that depends on the step size from a 64-byte controller record in device memory:
//     5 x f         k_i = f(u_i), the epilogue forms u_{i+1} = y + sum_j (b_ij h) k_j      (u_6 = y1; coef_scale -> h)
//     f             k6 = f(y1)                                                              (first-same-as-last)
//     error norm    block partial sums of ((sum_j e_j h k_j) / (atol + rtol max(|y|, |y1|)))^2
//     control       fold -> ratio; the decision of embedded_pair.h (step_decide: accept, end point reached -> interpolation fraction
//                   and done, t, dt in float64); h' = fl32(dt) for the next trial step
//     finish        (end point in this step) y_out = quartic through y, y1, y_mid, k0, k6 at t1;
//                   u_1 = y' + (b10 h') k0' of the NEXT trial step, (y', k0') = (y1, k6) if accepted else (y, k0)
// The graph exists in two parities that the host launches in turn: h and h' alternate between two slots of the record, and so
// do the roles of the buffer pairs (y, y1) and (k0, k6) -- an accepted step hands its y1 / k6 to the next trial step as y / k0
// without a copy; only a REJECTED step copies y and k0 across (finish kernel), which is the rare case.
// The host queues as many trial steps as cannot overshoot the end point even if every one of them were accepted with the
// largest growth the controller allows (factor 10), then reads the record once: no trial step is ever wasted, and a solve
// of N trial steps synchronises O(log N) + (number near the end point) times instead of N.
#include <cmath>
#include <vector>
#include "common.h"
#include "embedded_pair.h"
#include "epilogue.h"
#include "graph_capture.h"
#include "rhs.h"

namespace gnpde {
namespace {

struct Ctl {            // the controller record (device; copied to the host once per batch of trial steps)
  double t, dt, t1;
  float h[2];           // fl32(dt) of the trial step in flight (slot = parity of the trial) and of the next one
  float ratio;
  float x;              // interpolation fraction (t1 - t) / dt of the step that contains the end point
  int accept, interp, done;
  int trials, accepted, rejected;
  // early stopping (gnpde_dopri5_set_early_stop): the test-time integrator of the reference evaluates the decoder after EVERY
  // trial step and gives up after max_test_steps of them (src/early_stop_solver.py:82-98)
  int max_trials;       // 0: no limit
  int stopped;          // the trial budget ran out: y_out = the state where it stopped, not an interpolation
  int eval_now;         // gate of the evaluator kernels appended to this trial step
  int eval_tag;         // step tag of that evaluation: number of accepted steps (0 = the initial state)
  int initial_done;     // the initial state has been evaluated (trials rejected before the first accept do that once)
  int pad_[3];
};
static_assert(sizeof(Ctl) == 96, "controller record");

// fold of the error partial sums (as rk_error_final_kernel of misc.hip) + the controller's decision (embedded_pair.h); around it what is
// this solve's own: the no-op past the end point, the counters, the trial budget and the gate of the evaluator kernels
__global__ __launch_bounds__(kBlock) void control_kernel(const double* __restrict__ ws, int nblocks, double count, Ctl* c,
                                                        int parity, double* __restrict__ times, int times_capacity, int order) {
  __shared__ double red[kBlock];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += kBlock) acc += ws[i];      // block partials in double (misc.hip, rk_error_partial_kernel)
  const double sum = block_sum_double(acc, red);
  if (threadIdx.x != 0) return;
  const float ratio32 = static_cast<float>(sqrt(sum / count));
  c->ratio = ratio32;
  if (c->done) {                      // replayed past the end point (never queued by gnpde_dopri5_run): change nothing
    c->accept = 0;
    c->interp = 0;
    c->eval_now = 0;
    c->h[1 - parity] = c->h[parity];
    return;
  }
  const StepDecision dec = step_decide(c->t, c->dt, c->t1, ratio32, order);
  c->trials += 1;
  const int accept = dec.accept;
  int interp = dec.done;
  if (accept) {
    if (dec.done) {
      c->x = dec.x;
      c->done = 1;
    }
    c->t = dec.t_next;
    c->accepted += 1;
  } else {
    c->rejected += 1;
  }
  c->dt = dec.dt_next;
  c->h[1 - parity] = static_cast<float>(dec.dt_next);
  // early stopping: which state the evaluator kernels behind this trial step see.  Accepted: the new state, tagged with the
  // number of accepted steps (its time goes to times[tag]).  Rejected: the unchanged previous state -- counted already, it
  // cannot win the strict `val > best` -- except before the first accept, when it is the INITIAL state (tag 0), once.
  int eval_now = 0;
  if (c->max_trials > 0) {
    if (accept) {
      eval_now = 1;
      c->eval_tag = c->accepted;
      if (times != nullptr && c->accepted < times_capacity) times[c->accepted] = c->t;
    } else if (c->accepted == 0 && !c->initial_done) {
      eval_now = 1;
      c->eval_tag = 0;
      c->initial_done = 1;
    }
    if (c->trials >= c->max_trials) {   // the budget of trial steps is spent: the result is the state reached, as it stands
      c->done = 1;
      c->stopped = 1;
      interp = 0;
    }
  }
  c->eval_now = eval_now;
  c->accept = accept;
  c->interp = interp;
}

// Initial step size, torchdiffeq misc.py _select_initial_step (Hairer, Norsett & Wanner II.4) with its float32 / float64 mix:
//   d0 = rms(y / tol), d1 = rms(f0 / tol), h0 = 0.01 d0 / d1 (1e-6 if either is tiny), d2 = rms((f(y + h0 f0) - f0) / tol) / h0,
//   h1 = (0.01 / max(d1, d2))^(1/5), dt = min(100 h0, h1).  The three norms land in `Init` straight from the error-norm kernels.
struct Init {
  float d0, d1, d2, h0;
};

__global__ void init_h0_kernel(Init* q) {
  const double d0 = static_cast<double>(q->d0), d1 = static_cast<double>(q->d1);
  q->h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6f : 0.01f * q->d0 / q->d1;
}

__global__ void init_dt_kernel(const Init* q, Ctl* c, double t0, double t1, int max_trials, double* times, int times_capacity, int order) {
  const double h0 = static_cast<double>(q->h0), d1 = static_cast<double>(q->d1);
  const double d2 = static_cast<double>(q->d2) / h0;
  double h1;
  if (d1 <= 1e-15 && d2 <= 1e-15) {
    h1 = fmax(1e-6, h0 * 1e-3);
  } else {
    const float big = static_cast<float>(fmax(d1, d2));
    h1 = static_cast<double>(static_cast<float>(pow(static_cast<double>(0.01f / big), static_cast<double>(1.0f / order))));
  }
  c->t = t0;
  c->t1 = t1;
  c->dt = fmin(100.0 * h0, h1);
  c->h[0] = static_cast<float>(c->dt);
  c->h[1] = 0.f;
  c->ratio = 0.f;
  c->x = 0.f;
  c->accept = c->interp = c->done = 0;
  c->trials = c->accepted = c->rejected = 0;
  c->max_trials = max_trials;
  c->stopped = c->eval_now = c->eval_tag = c->initial_done = 0;
  if (times != nullptr && times_capacity > 0) times[0] = t0;
}

// the row copy of misc.hip (launch_copy_rows) through a row map: gather != 0: dst[r] = src[map[r]] (state in: solver row r holds the caller's row map[r]);
// gather == 0: dst[map[r]] = src[r] (result out).  Folds the node relabelling of graph.LocalityView into the two copies a solve makes
// anyway (two index_select launches, a state-sized temporary and their host gaps per forward otherwise).
__global__ __launch_bounds__(kBlock) void copy_rows_map_kernel(const float* __restrict__ src, int ld_src, float* __restrict__ dst, int ld_dst,
                                                              long long n, int d, const int* __restrict__ map, int gather) {
  const long long total = n * d;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    const long long r = i / d;
    const int c = static_cast<int>(i - r * d);
    const long long m = map[r];
    const long long rs = gather ? m : r, rd = gather ? r : m;
    dst[static_cast<size_t>(rd) * ld_dst + c] = src[static_cast<size_t>(rs) * ld_src + c];
  }
}

struct FinishArgs {
  const float* y; float* y1;      // the next trial step reads its y from the y1 buffer and its k0 from the k6 buffer:
  float* k[7];                    // written here only when this step was rejected
  float* yout; float* u1;
  float mid[7];                   // fl32(c_mid_j)
  int n_k, last;                  // derivatives of the pair (7 / 2), index of the last one (the next step's first if accepted)
  float b10;
  long long n;
  int d, ld;
  const Ctl* c;
  int parity;
};

// torchdiffeq's quartic end-point interpolation (embedded_pair.h, as dopri5_interp_kernel of misc.hip), the commit
// of an accepted step and the first stage input of the next trial step, one pass over the state
__global__ __launch_bounds__(kBlock) void finish_kernel(const FinishArgs a) {
  const int accept = a.c->accept, interp = a.c->interp, stopped = a.c->stopped;
  const float h = a.c->h[a.parity], hn = a.c->h[1 - a.parity], x = a.c->x;
  const float cn = a.b10 * hn;
  // flat over the padded storage (ld % 4 == 0, buffers 256-byte aligned; the padding columns hold zeros and stay zero)
  const long long total4 = a.n * a.ld / 4;
  typedef float f4 __attribute__((ext_vector_type(4)));
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < total4;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
    // (accept / interp are the same for every thread of the grid: an accepted step that does not contain the end point -- the common
    //  case -- reads y1 and k6 only, a rejected one y and k0 only; two of the four streams of the old unconditional form)
    f4 ya = {0.f, 0.f, 0.f, 0.f}, yb = ya, fa = ya, fb = ya;
    if (interp || !accept) {
      ya = reinterpret_cast<const f4*>(a.y)[i];
      fa = reinterpret_cast<const f4*>(a.k[0])[i];
    }
    if (interp || accept) {
      yb = reinterpret_cast<const f4*>(a.y1)[i];
      fb = reinterpret_cast<const f4*>(a.k[a.last])[i];
    }
    if (interp) {
      f4 ym = ya;
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const float m = j < a.n_k ? a.mid[j] * h : 0.0f;
        if (m != 0.0f) ym += reinterpret_cast<const f4*>(a.k[j])[i] * m;
      }
      reinterpret_cast<f4*>(a.yout)[i] = quartic(ya, yb, fa, fb, ym, h, x);
    }
    const f4 yn = accept ? yb : ya, fn = accept ? fb : fa;
    if (stopped) reinterpret_cast<f4*>(a.yout)[i] = yn;     // trial budget spent: the state where the integration stopped
    if (!accept) {
      reinterpret_cast<f4*>(a.y1)[i] = yn;
      reinterpret_cast<f4*>(a.k[a.last])[i] = fn;
    }
    f4 u;
#pragma unroll
    for (int t = 0; t < 4; ++t) u[t] = fmaf(cn, fn[t], yn[t]);
    reinterpret_cast<f4*>(a.u1)[i] = u;
  }
}

// Recorded solve (training without the adjoint method): an ACCEPTED trial step leaves its stage inputs on the tape -- slot
// `accepted - 1` receives u_0 = y and u_1..u_5, slot `accepted` receives u_0 = y1 (the next step's y, or the end state) -- and its
// step size.  Runs between the control kernel and the finish kernel (which overwrites u_1 with the next trial step's).
struct TapeArgs {
  const float* src[7];      // y, u_1..u_5, y1
  float* slots;             // [capacity + 1][6][stride]
  float* h;                 // [capacity]
  int* overflow;
  const Ctl* c;
  long long n4;             // float4s per state buffer (n * ld / 4)
  long long stride;         // floats between consecutive buffers of the tape
  int capacity, parity;
};

__global__ __launch_bounds__(kBlock) void tape_store_kernel(const TapeArgs a) {
  if (!a.c->accept) return;
  const int slot = a.c->accepted - 1;
  if (slot >= a.capacity) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.overflow = 1;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) a.h[slot] = a.c->h[a.parity];
  typedef float f4 __attribute__((ext_vector_type(4)));
  float* base = a.slots + static_cast<size_t>(slot) * 6 * a.stride;
  for (long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x; i < a.n4;
       i += static_cast<long long>(gridDim.x) * blockDim.x) {
#pragma unroll
    for (int b = 0; b < 6; ++b) reinterpret_cast<f4*>(base + b * a.stride)[i] = reinterpret_cast<const f4*>(a.src[b])[i];
    reinterpret_cast<f4*>(base + 6 * a.stride)[i] = reinterpret_cast<const f4*>(a.src[6])[i];     // u_0 of the next slot
  }
}

// Outputs at several times (gnpde_dopri5_set_outputs).  The stepping never looks at them: an ACCEPTED trial step [t_prev, t] writes out[j]
// = its quartic interpolant at x = fl32((t_out[j] - t_prev) / (t - t_prev)) for every pending j < n_out - 1 with t_out[j] <= t (the last
// output is the end point: the finish kernel's).  Runs between the control kernel (the record already holds the new time) and the finish
// kernel (which overwrites what a rejected step hands on).  The pending index and the start time of the step are carried in a record of
// their own, in two slots like Ctl::h: a trial step reads slot `parity` and its one-thread tail writes slot 1 - parity for the next
// one, so no thread of the grid reads what the tail writes.
struct OutRec {
  double t_prev[2];
  int next_out[2];
  int n_out, pad_;
};
static_assert(sizeof(OutRec) == 32, "output record");

__global__ void emit_init_kernel(OutRec* q, double t0, int n_out) {
  q->t_prev[0] = q->t_prev[1] = t0;
  q->next_out[0] = q->next_out[1] = 0;
  q->n_out = n_out;
}

struct EmitArgs {
  const float* y; const float* y1;
  const float* k[7];
  float mid[7];                   // fl32(c_mid_j)
  int n_k, last;
  long long n;
  int d, ld;
  float* out; int ld_out;         // [n_out][n, ld_out]
  const int* order;               // solver row r -> the caller's row order[r] (null: r)
  const double* t_out;            // [n_out], ascending, t_out[n_out - 1] = t1
  OutRec* rec;
  const Ctl* c;
  int parity;
};

template <bool VEC4>
__global__ __launch_bounds__(kBlock) void emit_outputs_kernel(const EmitArgs a) {
  constexpr int W = VEC4 ? 4 : 1;
  const int accept = a.c->accept;
  const double t = a.c->t, t_prev = a.rec->t_prev[a.parity];
  const int j0 = a.rec->next_out[a.parity], n_out = a.rec->n_out;
  // (everything the bound depends on is read from device memory written by earlier kernels: the same for every thread of the grid)
  int j1 = j0;
  if (accept)
    while (j1 < n_out - 1 && a.t_out[j1] <= t) ++j1;
  if (j1 > j0) {
    const float h = a.c->h[a.parity];
    const int groups = a.d / W;
    const long long total = a.n * groups;
    const size_t slab = static_cast<size_t>(a.n) * a.ld_out;
    for (long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += static_cast<long long>(gridDim.x) * kBlock) {
      const long long row = i / groups;
      const int col = static_cast<int>(i - row * groups) * W;
      const size_t off = static_cast<size_t>(row) * a.ld + col;
      const long long orow = a.order != nullptr ? static_cast<long long>(a.order[row]) : row;
      float ya[W], yb[W], fa[W], fb[W], ym[W];
      load_vec<W>(a.y + off, ya);
      load_vec<W>(a.y1 + off, yb);
      load_vec<W>(a.k[0] + off, fa);
      load_vec<W>(a.k[a.last] + off, fb);
#pragma unroll
      for (int c = 0; c < W; ++c) ym[c] = ya[c];
#pragma unroll
      for (int j = 0; j < 7; ++j) {
        const float m = j < a.n_k ? a.mid[j] * h : 0.0f;
        if (m != 0.0f) {
          float kj[W];
          load_vec<W>(a.k[j] + off, kj);
#pragma unroll
          for (int c = 0; c < W; ++c) ym[c] += kj[c] * m;
        }
      }
      float* o = a.out + static_cast<size_t>(orow) * a.ld_out + col;
      for (int j = j0; j < j1; ++j) {
        const float x = static_cast<float>((a.t_out[j] - t_prev) / (t - t_prev));
        float v[W];
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = quartic(ya[c], yb[c], fa[c], fb[c], ym[c], h, x);
        store_vec<W>(o + j * slab, v);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {      // the tail: what the next trial step (the other parity) starts from
    a.rec->next_out[1 - a.parity] = j1;
    a.rec->t_prev[1 - a.parity] = accept ? t : t_prev;
  }
}

// sum over the per-wave dots of every launch of the reverse sweep: sum d1 - sum d2 in double, fixed order -- kTapeFoldBlocks blocks over
// contiguous ranges, then one wave over their partial sums
constexpr int kTapeFoldBlocks = 128;

__global__ __launch_bounds__(kBlock) void tape_dots_partial_kernel(const float* __restrict__ dots, long long n_pairs, double* __restrict__ part) {
  __shared__ double red[kBlock];
  const long long per = (n_pairs + gridDim.x - 1) / gridDim.x;
  const long long b0 = per * blockIdx.x, b1 = b0 + per < n_pairs ? b0 + per : n_pairs;
  double acc = 0.0;
  for (long long i = b0 + threadIdx.x; i < b1; i += kBlock) {
    const float2 v = reinterpret_cast<const float2*>(dots)[i];
    acc += static_cast<double>(v.x) - static_cast<double>(v.y);
  }
  const double sum = block_sum_double(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kTapeFoldBlocks) void tape_dots_fold_kernel(const double* __restrict__ part, float* __restrict__ out) {
  __shared__ double red[kTapeFoldBlocks];
  red[threadIdx.x] = part[threadIdx.x];
  __syncthreads();
  for (int s = kTapeFoldBlocks / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = static_cast<float>(red[0]);
}

}  // namespace
}  // namespace gnpde

using namespace gnpde;

struct gnpde_dopri5 {
  gnpde_rhs_t rhs;
  gnpde_graph_t graph;
  gnpde_graph_t graph_t;
  RhsLayout L;
  float rtol, atol;
  char* ws;
  size_t ws_bytes;
  size_t state_bytes;     // one [n, ld] buffer, rounded up to 256 bytes
  size_t off_ctl, off_err, off_rhs, off_state;
  hipStream_t cap_stream = nullptr;
  hipGraph_t graph_obj[2] = {nullptr, nullptr};    // the trial step in its two parities (which slot of Ctl::h it reads)
  hipGraphExec_t exec[2] = {nullptr, nullptr};
  bool padding_cleared = false;
  Ctl* host_ctl = nullptr;   // pinned
  int n_evals = 0, n_accepted = 0, n_rejected = 0, n_launches = 0, n_syncs = 0;
  // buffers inside the workspace
  float* Y[2];  float* KA[2];  float* km[5];  float* u[2];  float* yout;   // (y, y1) and (k0, k6) swap roles with the parity
  Ctl* ctl;  float* err_ws;  Init* init;
  // early stopping
  bool early = false;
  gnpde_decoder_t dec{};
  int* early_state = nullptr;
  int* early_trace = nullptr;
  int early_trace_capacity = 0;
  double* times = nullptr;
  int times_capacity = 0;
  int max_trials = 0;
  // recorded solve (gnpde_dopri5_set_tape)
  float* tape = nullptr;        // [3 extra stage-input buffers][capacity + 1 slots x 6 buffers][h: capacity][overflow flag]
  int tape_capacity = 0;
  float* tape_x[3] = {nullptr, nullptr, nullptr};
  float* tape_slots = nullptr;
  float* tape_h = nullptr;
  int* tape_overflow = nullptr;
  float* host_h = nullptr;      // pinned copy of the accepted steps' sizes, read once behind a recorded solve
  int host_h_capacity = 0;
  const int* row_order = nullptr;   // gnpde_dopri5_set_row_order: solver row r <-> caller's row row_order[r]
  // outputs at several times (gnpde_dopri5_set_outputs)
  const double* t_out = nullptr;    // device, [n_out]
  int n_out = 0;
  double t_out_last = 0.0;          // host copy of t_out[n_out - 1]: the t1 of the runs
  float* out = nullptr;
  int ld_out = 0;
  OutRec* out_rec = nullptr;
  // Row-partitioned solve (gnpde_dopri5_create_sharded): the evaluations go through the exchange engine (its stage buffers hold the four
  // states that are ever an evaluation's input: Y[0], Y[1], u[0], u[1]), the error norms are summed over the ranks inside the stream
  int pair = GNPDE_ADAPTIVE_DOPRI5;   // gnpde_dopri5_set_pair: the embedded pair (Dormand-Prince 5(4) / torchdiffeq's adaptive_heun 2(1))
  gnpde_sharded_solver_t* shard = nullptr;
  long long n_rows = 0;             // rows the element-wise kernels of this rank cover (all rows / the owned rows)
  double count = 0.0;               // elements of the WHOLE state: the mean of the error norm is over every rank's rows
  float last_x = 0.f;           // interpolation fraction of the last accepted step of the last run
  int tape_steps = 0;           // accepted steps of the last recorded run (0: nothing to differentiate)
};

namespace {

size_t dopri5_layout(const gnpde_rhs_t& r, gnpde_dopri5* s) {
  const size_t state = align_up(static_cast<size_t>(r.graph->n) * r.ld * 4, 256);
  size_t off = 0;
  const size_t off_ctl = off;   off += 256;                 // Ctl + one scalar for the initial-step norms
  const size_t off_err = off;   off += 4096 * 4;
  const RhsLayout L = rhs_layout(r);
  const size_t off_rhs = off;   off += align_up(L.total, 256);
  const size_t off_state = off; off += 12 * state;
  if (s) {
    s->state_bytes = state;
    s->off_ctl = off_ctl; s->off_err = off_err; s->off_rhs = off_rhs; s->off_state = off_state;
  }
  return off;
}

// one evaluation of f at u with the given epilogue: the whole graph, or -- partitioned -- exchange + interior + boundary rows
int enqueue_f(gnpde_dopri5* s, float* u, const gnpde_epilogue_t& e, hipStream_t st) {
  if (s->shard != nullptr) return sharded_enqueue_eval(s->shard, u, e, st);
  return enqueue_rhs(s->rhs, u, e, s->ws + s->off_rhs, s->L, st);
}

__global__ void root_mean_kernel(const double* __restrict__ sum, double count, float* __restrict__ out) {
  *out = static_cast<float>(sqrt(sum[0] / count));
}

int enqueue_trial(gnpde_dopri5* s, int parity, hipStream_t st) {
  const gnpde_rhs_t& r = s->rhs;
  const long long n = s->n_rows;
  const float* h = &s->ctl->h[parity];
  float* y = s->Y[parity];
  float* y1 = s->Y[1 - parity];
  const Tableau& tab = *tableau_of(s->pair);
  const int S = tab.S, n_k = S + 1;
  float* k[7];                          // K_0 (carried over), the middle stages, K_S (carried on); entries past S repeat K_S
  k[0] = s->KA[parity];
  for (int j = 1; j < 7; ++j) k[j] = j < S ? s->km[j - 1] : s->KA[1 - parity];
  // stage inputs u_1..u_5: two alternating buffers -- or, when the solve is recorded, five distinct ones that survive the trial step
  float* ui[5] = {s->u[0], s->u[1], s->u[0], s->u[1], s->u[0]};
  if (s->tape != nullptr) { ui[2] = s->tape_x[0]; ui[3] = s->tape_x[1]; ui[4] = s->tape_x[2]; }
  float ce[7], cmid[7];
  for (int j = 0; j < 7; ++j) { ce[j] = static_cast<float>(tab.c_err[j]); cmid[j] = static_cast<float>(tab.c_mid[j]); }
  // (u_1 = y + (a00 h) k0 was written by the previous trial step's finish kernel)
  float* cur = s->u[0];
  for (int rr = 1; rr <= S; ++rr) {
    gnpde_epilogue_t e = base_epilogue(r);
    e.stage = GNPDE_STAGE_RHS;
    e.out_k = k[rr];
    const double* w = nullptr;          // weights of the state this evaluation's epilogue forms from K_0..K_rr, if any
    if (rr < S) {                       // the input of stage rr + 1 (of a first-same-as-last pair the last one IS the solution)
      w = tab.a[rr];
      e.out_y = tab.fsal && rr == S - 1 ? y1 : ui[rr];
    } else if (!tab.fsal) {             // the solution from every stage derivative
      w = tab.c_sol;
      e.out_y = y1;
    }
    if (w != nullptr) {
      e.stage = GNPDE_STAGE_LINCOMB;
      e.y = y;
      // (earlier derivatives with a zero weight -- k1 in the solution row -- are not streamed: fma(k, 0, o) = o for every finite k)
      int np = 0;
      for (int j = 0; j < rr; ++j) {
        const float c = static_cast<float>(w[j]);
        if (c == 0.0f) continue;
        e.prev[np] = k[j];
        e.coef[np] = c;
        ++np;
      }
      e.n_prev = np;
      e.coef[np] = static_cast<float>(w[rr]);
      e.coef_scale = h;
    }
    if (int rc = enqueue_f(s, cur, e, st)) return rc;
    if (w != nullptr) cur = e.out_y;
  }
  int nblocks = 0;
  if (int rc = launch_rk_error_ratio(y, y1, k, ce, n_k, s->atol, s->rtol, n, r.d, r.ld, nullptr, s->err_ws, st, h, &nblocks))
    return rc;
  if (s->shard != nullptr) {      // the squares of every rank's rows: one double all-reduced inside the stream
    if (int rc = sharded_enqueue_sum(s->shard, reinterpret_cast<double*>(s->err_ws), nblocks, st)) return rc;
    nblocks = 1;
  }
  hipLaunchKernelGGL(control_kernel, dim3(1), dim3(kBlock), 0, st, reinterpret_cast<const double*>(s->err_ws), nblocks, s->count, s->ctl, parity,
                     s->early ? s->times : nullptr, s->early ? s->times_capacity : 0, tab.order);
  GNPDE_LAUNCH_CHECK();
  if (s->t_out != nullptr) {
    EmitArgs ea{};
    ea.y = y; ea.y1 = y1;
    for (int j = 0; j < 7; ++j) {
      ea.k[j] = k[j];
      ea.mid[j] = cmid[j];
    }
    ea.n_k = n_k; ea.last = S;
    ea.n = n; ea.d = r.d; ea.ld = r.ld;
    ea.out = s->out; ea.ld_out = s->ld_out; ea.order = s->row_order; ea.t_out = s->t_out; ea.rec = s->out_rec; ea.c = s->ctl; ea.parity = parity;
    // (the state side always allows 16-byte lanes: ld % 4 == 0 is checked at creation and every buffer is a 256-byte aligned slice of the
    //  workspace, as the finish kernel relies on; what varies is the width and the caller's output)
    const bool v4 = r.d % 4 == 0 && s->ld_out % 4 == 0 && reinterpret_cast<uintptr_t>(s->out) % 16 == 0;
    long long eb = (n * (v4 ? r.d / 4 : r.d) + kBlock - 1) / kBlock;
    if (eb > 4096) eb = 4096;
    if (eb < 1) eb = 1;
    if (v4) hipLaunchKernelGGL((emit_outputs_kernel<true>), dim3(static_cast<unsigned>(eb)), dim3(kBlock), 0, st, ea);
    else hipLaunchKernelGGL((emit_outputs_kernel<false>), dim3(static_cast<unsigned>(eb)), dim3(kBlock), 0, st, ea);
    GNPDE_LAUNCH_CHECK();
  }
  if (s->tape != nullptr) {
    TapeArgs ta{};
    ta.src[0] = y;
    for (int j = 0; j < 5; ++j) ta.src[1 + j] = ui[j];
    ta.src[6] = y1;
    ta.slots = s->tape_slots; ta.h = s->tape_h; ta.overflow = s->tape_overflow; ta.c = s->ctl;
    ta.n4 = n * r.ld / 4; ta.stride = static_cast<long long>(s->state_bytes / 4);
    ta.capacity = s->tape_capacity; ta.parity = parity;
    long long tb = (ta.n4 + kBlock - 1) / kBlock;
    if (tb > 2048) tb = 2048;
    if (tb < 1) tb = 1;
    hipLaunchKernelGGL(tape_store_kernel, dim3(static_cast<unsigned>(tb)), dim3(kBlock), 0, st, ta);
    GNPDE_LAUNCH_CHECK();
  }
  FinishArgs fa{};
  fa.y = y; fa.y1 = y1; fa.yout = s->yout; fa.u1 = s->u[0];
  for (int j = 0; j < 7; ++j) {
    fa.k[j] = k[j];
    fa.mid[j] = cmid[j];
  }
  fa.n_k = n_k; fa.last = S;
  fa.b10 = static_cast<float>(tab.a[0][0]);
  fa.n = n; fa.d = r.d; fa.ld = r.ld; fa.c = s->ctl; fa.parity = parity;
  long long blocks = (n * r.ld / 4 + kBlock - 1) / kBlock;
  if (blocks > 4096) blocks = 4096;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(finish_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, st, fa);
  GNPDE_LAUNCH_CHECK();
  if (s->early) {
    // After the finish kernel the y1 buffer holds the state the NEXT trial step starts from, whatever was decided: the
    // accepted y1, or the copy of y.  The evaluator kernels read it; the controller's gate and tag decide if and as what.
    if (int rc = enqueue_early_stop_eval(s->dec, y1, r.ld, static_cast<int>(n), 0, s->early_state, s->early_trace,
                                         s->early_trace_capacity, st, &s->ctl->eval_now, &s->ctl->eval_tag))
      return rc;
  }
  return 0;
}

// rms(sum_j c_j v_j / (atol + rtol |y|)) -> *out (device)
int scaled_rms(gnpde_dopri5* s, const float* const* v, const float* c, int n_v, hipStream_t st, float* out) {
  const gnpde_rhs_t& r = s->rhs;
  if (s->shard != nullptr) {
    int nblocks = 0;
    if (int rc = launch_rk_error_ratio(s->Y[0], s->Y[0], v, c, n_v, s->atol, s->rtol, s->n_rows, r.d, r.ld, nullptr, s->err_ws, st, nullptr,
                                       &nblocks))
      return rc;
    if (int rc = sharded_enqueue_sum(s->shard, reinterpret_cast<double*>(s->err_ws), nblocks, st)) return rc;
    hipLaunchKernelGGL(root_mean_kernel, dim3(1), dim3(1), 0, st, reinterpret_cast<const double*>(s->err_ws), s->count, out);
    GNPDE_LAUNCH_CHECK();
    return 0;
  }
  return launch_rk_error_ratio(s->Y[0], s->Y[0], v, c, n_v, s->atol, s->rtol, s->n_rows, r.d, r.ld, out, s->err_ws, st, nullptr,
                               nullptr);
}

}  // namespace

extern "C" size_t gnpde_dopri5_workspace_bytes(const gnpde_rhs_t* rhs) {
  if (check_rhs(rhs)) return 0;
  return dopri5_layout(*rhs, nullptr);
}

extern "C" int gnpde_dopri5_create(gnpde_dopri5_t** out, const gnpde_rhs_t* rhs, float rtol, float atol, void* workspace,
                                   size_t workspace_bytes) {
  GNPDE_CHECK_ARG(out != nullptr, GNPDE_EINVAL, "dopri5_create: out is null");
  *out = nullptr;
  if (int rc = check_rhs(rhs)) return rc;
  GNPDE_CHECK_ARG(rtol >= 0.f && atol >= 0.f && rtol + atol > 0.f, GNPDE_EINVAL, "dopri5_create: bad tolerances");
  GNPDE_CHECK_ARG(rhs->ld % 4 == 0, GNPDE_ESHAPE, "dopri5_create: the state row stride must be a multiple of 4 (pad the rows)");
  gnpde_dopri5* s = new gnpde_dopri5();
  s->rhs = *rhs;
  s->graph = *rhs->graph;
  s->rhs.graph = &s->graph;
  if (s->rhs.att.graph_t != nullptr) {   // (the descriptor's transposed graph is copied as well: the caller's structs may go away)
    s->graph_t = *s->rhs.att.graph_t;
    s->rhs.att.graph_t = &s->graph_t;
  }
  s->rtol = rtol;
  s->atol = atol;
  s->L = rhs_layout(s->rhs);
  const size_t need = dopri5_layout(s->rhs, s);
  if (!(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 256 == 0)) {
    set_error("dopri5_create: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, need);
    delete s;
    return GNPDE_EWS;
  }
  s->ws = static_cast<char*>(workspace);
  s->ws_bytes = workspace_bytes;
  s->ctl = reinterpret_cast<Ctl*>(s->ws + s->off_ctl);
  s->init = reinterpret_cast<Init*>(s->ws + s->off_ctl + 128);
  s->out_rec = reinterpret_cast<OutRec*>(s->ws + s->off_ctl + 160);
  s->err_ws = reinterpret_cast<float*>(s->ws + s->off_err);
  float* base = reinterpret_cast<float*>(s->ws + s->off_state);
  const size_t stride = s->state_bytes / 4;
  s->Y[0] = base; s->Y[1] = base + stride; s->u[0] = base + 2 * stride; s->u[1] = base + 3 * stride;
  s->KA[0] = base + 4 * stride; s->KA[1] = base + 5 * stride;
  for (int j = 0; j < 5; ++j) s->km[j] = base + (6 + j) * stride;
  s->yout = base + 11 * stride;
  s->n_rows = s->graph.n;
  s->count = static_cast<double>(s->graph.n) * s->rhs.d;
  if (hipHostMalloc(reinterpret_cast<void**>(&s->host_ctl), sizeof(Ctl), hipHostMallocDefault) != hipSuccess) {
    set_error("dopri5_create: pinned allocation failed");
    delete s;
    return GNPDE_EINVAL;
  }
  *out = s;
  return 0;
}

// Row-partitioned: [controller record | error partials | k0, k6, five k's, y_out of the owned rows]; the evaluation scratch is the engine's
namespace {
size_t dopri5_sharded_layout(const ShardedShape& h, gnpde_dopri5* s) {
  const size_t state = align_up(static_cast<size_t>(h.n_own > 0 ? h.n_own : 1) * h.ld * 4, 256);
  size_t off = 0;
  const size_t off_ctl = off;   off += 256;
  const size_t off_err = off;   off += 4096 * 4;
  const size_t off_state = off; off += 8 * state;
  if (s) {
    s->state_bytes = state;
    s->off_ctl = off_ctl; s->off_err = off_err; s->off_rhs = off_state; s->off_state = off_state;
  }
  return off;
}
}  // namespace

extern "C" size_t gnpde_dopri5_sharded_workspace_bytes(gnpde_sharded_solver_t* engine) {
  if (engine == nullptr) return 0;
  return dopri5_sharded_layout(sharded_shape(engine), nullptr);
}

extern "C" int gnpde_dopri5_create_sharded(gnpde_dopri5_t** out, gnpde_sharded_solver_t* engine, float rtol, float atol,
                                           int64_t n_rows_total, void* workspace, size_t workspace_bytes) {
  GNPDE_CHECK_ARG(out != nullptr, GNPDE_EINVAL, "dopri5_create_sharded: out is null");
  *out = nullptr;
  GNPDE_CHECK_ARG(engine != nullptr, GNPDE_EINVAL, "dopri5_create_sharded: engine is null");
  GNPDE_CHECK_ARG(rtol >= 0.f && atol >= 0.f && rtol + atol > 0.f, GNPDE_EINVAL, "dopri5_create_sharded: bad tolerances");
  const ShardedShape h = sharded_shape(engine);
  GNPDE_CHECK_ARG(h.p2p && h.n_buffers >= 4, GNPDE_ESTATE, "dopri5_create_sharded: the engine needs the P2P transport with 4 shared stage buffers");
  GNPDE_CHECK_ARG(h.ld % 4 == 0, GNPDE_ESHAPE, "dopri5_create_sharded: the state row stride must be a multiple of 4");
  GNPDE_CHECK_ARG(n_rows_total >= h.n_own && h.n_own >= 1, GNPDE_EINVAL, "dopri5_create_sharded: %lld rows in total, %d owned",
                  static_cast<long long>(n_rows_total), h.n_own);
  if (int rc = sharded_prepare_adaptive(engine)) return rc;
  gnpde_dopri5* s = new gnpde_dopri5();
  s->shard = engine;
  s->rhs = *h.rhs;                 // alpha / beta / x0 / widths of the owned rows (the evaluations themselves are the engine's)
  s->graph = *h.rhs->graph;
  s->rhs.graph = &s->graph;
  s->rhs.att.graph_t = nullptr;
  s->rtol = rtol;
  s->atol = atol;
  s->n_rows = h.n_own;
  s->count = static_cast<double>(n_rows_total) * h.d;
  const size_t need = dopri5_sharded_layout(h, s);
  if (!(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 256 == 0)) {
    set_error("dopri5_create_sharded: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, need);
    delete s;
    return GNPDE_EWS;
  }
  s->ws = static_cast<char*>(workspace);
  s->ws_bytes = workspace_bytes;
  s->ctl = reinterpret_cast<Ctl*>(s->ws + s->off_ctl);
  s->init = reinterpret_cast<Init*>(s->ws + s->off_ctl + 128);
  s->out_rec = reinterpret_cast<OutRec*>(s->ws + s->off_ctl + 160);
  s->err_ws = reinterpret_cast<float*>(s->ws + s->off_err);
  // every state that is ever an evaluation's input lives in a shared stage buffer: the peers push their boundary rows into its halo rows
  s->Y[0] = sharded_stage_buffer(engine, 0); s->Y[1] = sharded_stage_buffer(engine, 1);
  s->u[0] = sharded_stage_buffer(engine, 2); s->u[1] = sharded_stage_buffer(engine, 3);
  float* base = reinterpret_cast<float*>(s->ws + s->off_state);
  const size_t stride = s->state_bytes / 4;
  s->KA[0] = base; s->KA[1] = base + stride;
  for (int j = 0; j < 5; ++j) s->km[j] = base + (2 + j) * stride;
  s->yout = base + 7 * stride;
  if (hipHostMalloc(reinterpret_cast<void**>(&s->host_ctl), sizeof(Ctl), hipHostMallocDefault) != hipSuccess) {
    set_error("dopri5_create_sharded: pinned allocation failed");
    delete s;
    return GNPDE_EINVAL;
  }
  *out = s;
  return 0;
}

extern "C" int gnpde_dopri5_run(gnpde_dopri5_t* s, const float* y0, int32_t ld_y0, double t0, double t1, float* y_out,
                                int32_t ld_out, int32_t trials_per_sync, int32_t max_evals, int32_t* finished, void* stream) {
  GNPDE_CHECK_ARG(s && y0 && y_out, GNPDE_EINVAL, "dopri5_run: null argument");
  const gnpde_rhs_t& r = s->rhs;
  GNPDE_CHECK_ARG(ld_y0 >= r.d && ld_out >= r.d && t1 > t0, GNPDE_EINVAL, "dopri5_run: bad strides or time span");
  GNPDE_CHECK_ARG(s->t_out == nullptr || t1 == s->t_out_last, GNPDE_EINVAL, "dopri5_run: t1 = %.17g but the last output time is %.17g", t1,
                  s->t_out_last);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (trials_per_sync < 1) trials_per_sync = 1;
  const int n = static_cast<int>(s->n_rows);
  s->n_evals = s->n_accepted = s->n_rejected = s->n_launches = s->n_syncs = 0;
  s->tape_steps = 0;
  if (finished) *finished = 0;
  if (s->tape != nullptr) GNPDE_HIP(hipMemsetAsync(s->tape_overflow, 0, sizeof(int), st));
  if (s->early) GNPDE_HIP(hipMemsetAsync(s->early_state, 0, 8 * sizeof(int32_t), st));
  if (!s->padding_cleared) {   // once: the padding columns [d, ld) are never written with anything but what they hold
    GNPDE_HIP(hipMemsetAsync(s->ws + s->off_state, 0, (s->shard != nullptr ? 8 : 12) * s->state_bytes, st));
    s->padding_cleared = true;
  }
  const Tableau& tab = *tableau_of(s->pair);
  // state in / result out: dst rows = src rows, through the row map if one is set
  auto copy_rows = [&](const float* src, int ld_src, float* dst, int ld_dst, int gather) -> int {
    if (s->row_order == nullptr) return launch_copy_rows(src, ld_src, dst, ld_dst, n, r.d, st);
    hipLaunchKernelGGL(copy_rows_map_kernel, dim3(copy_rows_grid(n, r.d)), dim3(kBlock), 0, st, src, ld_src, dst, ld_dst,
                       static_cast<long long>(n), r.d, s->row_order, gather);
    GNPDE_LAUNCH_CHECK();
    return 0;
  };
  if (int rc = copy_rows(y0, ld_y0, s->Y[0], r.ld, 1)) return rc;
  auto feval = [&](float* src, float* dst) -> int {
    gnpde_epilogue_t e = base_epilogue(r);
    e.stage = GNPDE_STAGE_RHS;
    e.out_k = dst;
    s->n_evals += 1;
    return enqueue_f(s, src, e, st);
  };
  if (int rc = feval(s->Y[0], s->KA[0])) return rc;
  // initial step size, entirely on the device (no read-back): see init_h0_kernel / init_dt_kernel
  const float one = 1.0f, minus = -1.0f;
  const long long flat = static_cast<long long>(n) * r.ld;
  {
    const float* v[1] = {s->Y[0]};
    if (int rc = scaled_rms(s, v, &one, 1, st, &s->init->d0)) return rc;
    const float* w[1] = {s->KA[0]};
    if (int rc = scaled_rms(s, w, &one, 1, st, &s->init->d1)) return rc;
    hipLaunchKernelGGL(init_h0_kernel, dim3(1), dim3(1), 0, st, s->init);
    GNPDE_LAUNCH_CHECK();
    if (int rc = launch_lincomb(s->Y[0], w, &one, 1, flat, s->u[0], st, &s->init->h0)) return rc;   // y + h0 f0
    if (int rc = feval(s->u[0], s->km[0])) return rc;
    const float* dk[2] = {s->km[0], s->KA[0]};
    const float cw[2] = {one, minus};
    if (int rc = scaled_rms(s, dk, cw, 2, st, &s->init->d2)) return rc;
    hipLaunchKernelGGL(init_dt_kernel, dim3(1), dim3(1), 0, st, s->init, s->ctl, t0, t1, s->early ? s->max_trials : 0,
                       s->early ? s->times : nullptr, s->early ? s->times_capacity : 0, tab.order);
    GNPDE_LAUNCH_CHECK();
    if (s->t_out != nullptr) {
      hipLaunchKernelGGL(emit_init_kernel, dim3(1), dim3(1), 0, st, s->out_rec, t0, s->n_out);
      GNPDE_LAUNCH_CHECK();
    }
    // first stage input of the first trial step (later ones come out of the finish kernel)
    const float c[1] = {static_cast<float>(tab.a[0][0])};
    if (int rc = launch_lincomb(s->Y[0], w, c, 1, flat, s->u[0], st, &s->ctl->h[0])) return rc;
  }
  for (int parity = 0; parity < 2; ++parity) {
    if (s->exec[parity] != nullptr) continue;
    if (int rc = capture_into(&s->cap_stream, &s->graph_obj[parity], &s->exec[parity], [&](hipStream_t cs) { return enqueue_trial(s, parity, cs); }))
      return rc;
  }
  const int base_evals = s->n_evals;
  bool have_record = false;   // nothing is known about dt on the host before the first read: one trial step, then look
  for (;;) {
    // as many trial steps as cannot pass t1 (plan_batch, embedded_pair.h), then one read of the record
    const Ctl& hc = *s->host_ctl;
    int batch = plan_batch(hc.t, hc.dt, hc.t1, trials_per_sync, have_record);
    if (have_record && hc.max_trials > 0 && batch > hc.max_trials - hc.trials) batch = hc.max_trials - hc.trials;   // trial budget
    if (batch < 1) batch = 1;
    for (int b = 0; b < batch; ++b) GNPDE_HIP(hipGraphLaunch(s->exec[(s->n_launches + b) & 1], st));
    s->n_launches += batch;
    GNPDE_HIP(hipMemcpyAsync(s->host_ctl, s->ctl, sizeof(Ctl), hipMemcpyDeviceToHost, st));
    GNPDE_HIP(hipStreamSynchronize(st));
    s->n_syncs += 1;
    have_record = true;
    s->n_evals = base_evals + tab.S * hc.trials;
    s->n_accepted = hc.accepted;
    s->n_rejected = hc.rejected;
    if (s->shard != nullptr) {    // a peer that never arrived: its share of the norms is missing, nothing behind this point means anything
      int lost = 0;
      if (int rc = sharded_lost_peer(s->shard, &lost)) return rc;
      GNPDE_CHECK_ARG(!lost, GNPDE_ESTATE, "dopri5_run: a peer never published its rows or its share of the error norm (wait timed out)");
    }
    if (hc.done) break;
    GNPDE_CHECK_ARG(hc.t + hc.dt > hc.t, GNPDE_EINVAL, "dopri5_run: underflow in dt %g at t %g", hc.dt, hc.t);
    if (max_evals > 0 && s->n_evals > max_evals) return 0;   // *finished stays 0
  }
  if (int rc = copy_rows(s->yout, r.ld, y_out, ld_out, 0)) return rc;
  if (s->tape != nullptr) {
    GNPDE_CHECK_ARG(s->n_accepted <= s->tape_capacity, GNPDE_EWS, "dopri5_run: %d accepted steps do not fit the tape (%d slots)",
                    s->n_accepted, s->tape_capacity);
    if (s->n_accepted > 0)
      GNPDE_HIP(hipMemcpyAsync(s->host_h, s->tape_h, sizeof(float) * s->n_accepted, hipMemcpyDeviceToHost, st));
  }
  GNPDE_HIP(hipStreamSynchronize(st));
  if (s->tape != nullptr) {
    s->tape_steps = s->host_ctl->interp || s->host_ctl->done ? s->n_accepted : 0;
    s->last_x = s->host_ctl->x;
  }
  if (finished) *finished = 1;
  return 0;
}

extern "C" int gnpde_dopri5_set_early_stop(gnpde_dopri5_t* s, const gnpde_decoder_t* dec, int32_t* state, int32_t* trace,
                                           int32_t trace_capacity, double* times, int32_t times_capacity, int32_t max_trial_steps) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "dopri5_set_early_stop: solver is null");
  for (int p = 0; p < 2; ++p) {      // the evaluator kernels are part of the captured trial step
    drop_capture(&s->graph_obj[p], &s->exec[p]);
  }
  if (dec == nullptr) {
    s->early = false;
    return 0;
  }
  GNPDE_CHECK_ARG(s->t_out == nullptr, GNPDE_EINVAL,
                  "dopri5_set_early_stop: not together with outputs at several times (detach them first: gnpde_dopri5_set_outputs(s, NULL, 0, NULL, 0))");
  GNPDE_CHECK_ARG(s->shard == nullptr, GNPDE_ESTATE, "dopri5_set_early_stop: not on a row-partitioned solve (the split counts are over all rows)");
  if (int rc = check_decoder(dec, s->rhs.d)) return rc;
  GNPDE_CHECK_ARG(state != nullptr && max_trial_steps >= 1, GNPDE_EINVAL, "dopri5_set_early_stop: state is null or no trial steps allowed");
  GNPDE_CHECK_ARG((trace != nullptr || trace_capacity == 0) && (times != nullptr || times_capacity == 0) && trace_capacity >= 0 &&
                  times_capacity >= 0, GNPDE_EINVAL, "dopri5_set_early_stop: capacity without an array");
  s->dec = *dec;
  s->early_state = state;
  s->early_trace = trace;
  s->early_trace_capacity = trace_capacity;
  s->times = times;
  s->times_capacity = times_capacity;
  s->max_trials = max_trial_steps;
  s->early = true;
  return 0;
}

extern "C" int gnpde_dopri5_set_pair(gnpde_dopri5_t* s, int32_t pair) {
  GNPDE_CHECK_ARG(s != nullptr && (pair == GNPDE_ADAPTIVE_DOPRI5 || pair == GNPDE_ADAPTIVE_HEUN), GNPDE_EINVAL, "dopri5_set_pair: bad argument");
  GNPDE_CHECK_ARG(pair == GNPDE_ADAPTIVE_DOPRI5 || s->tape == nullptr, GNPDE_ESTATE, "dopri5_set_pair: the recorded solve is Dormand-Prince's");
  if (pair == s->pair) return 0;
  for (int p = 0; p < 2; ++p) {      // the trial step is captured per pair
    drop_capture(&s->graph_obj[p], &s->exec[p]);
  }
  s->pair = pair;
  return 0;
}

extern "C" int gnpde_dopri5_set_row_order(gnpde_dopri5_t* s, const int32_t* order) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "dopri5_set_row_order: solver is null");
  GNPDE_CHECK_ARG(order == nullptr || s->shard == nullptr, GNPDE_ESTATE, "dopri5_set_row_order: not on a row-partitioned solve");
  if (s->t_out != nullptr && order != s->row_order) {      // (with outputs attached the captured emit kernel writes through the map)
    for (int p = 0; p < 2; ++p) drop_capture(&s->graph_obj[p], &s->exec[p]);
  }
  s->row_order = order;      // (otherwise read by the copy kernels of gnpde_dopri5_run only: the captured trial steps are untouched)
  return 0;
}

extern "C" int gnpde_dopri5_set_outputs(gnpde_dopri5_t* s, const double* t_out, int32_t n_out, float* out, int32_t ld_out) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "dopri5_set_outputs: solver is null");
  GNPDE_CHECK_ARG(n_out >= 0, GNPDE_EINVAL, "dopri5_set_outputs: n_out = %d", n_out);
  auto drop = [&]() {      // the emit kernel and its pointers are part of the captured trial step
    for (int p = 0; p < 2; ++p) drop_capture(&s->graph_obj[p], &s->exec[p]);
  };
  if (n_out == 0 || t_out == nullptr) {
    if (s->t_out != nullptr) drop();
    s->t_out = nullptr;
    s->out = nullptr;
    s->n_out = 0;
    return 0;
  }
  GNPDE_CHECK_ARG(s->shard == nullptr, GNPDE_EINVAL, "dopri5_set_outputs: not on a row-partitioned solve (it has two output times)");
  GNPDE_CHECK_ARG(s->tape == nullptr, GNPDE_EINVAL, "dopri5_set_outputs: a recorded solve has two output times (detach the tape first)");
  GNPDE_CHECK_ARG(!s->early, GNPDE_EINVAL, "dopri5_set_outputs: not together with the early-stopping evaluator (detach it first)");
  GNPDE_CHECK_ARG(out != nullptr && ld_out >= s->rhs.d, GNPDE_EINVAL, "dopri5_set_outputs: out is null or ld_out %d < d %d", ld_out, s->rhs.d);
  double last = 0.0;
  GNPDE_HIP(hipMemcpy(&last, t_out + (n_out - 1), sizeof(double), hipMemcpyDeviceToHost));
  if (t_out != s->t_out || out != s->out || ld_out != s->ld_out) drop();      // (n_out and the times themselves are read from device memory)
  s->t_out = t_out;
  s->n_out = n_out;
  s->t_out_last = last;
  s->out = out;
  s->ld_out = ld_out;
  return 0;
}

extern "C" int gnpde_dopri5_stats(const gnpde_dopri5_t* s, int32_t* n_evals, int32_t* n_accepted, int32_t* n_rejected,
                                  int32_t* n_launches, int32_t* n_syncs) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "dopri5_stats: solver is null");
  store_stats(s, n_evals, n_accepted, n_rejected, n_launches, n_syncs);
  return 0;
}

extern "C" int gnpde_dopri5_destroy(gnpde_dopri5_t* s) {
  if (!s) return 0;
  for (int p = 0; p < 2; ++p) {
    drop_capture(&s->graph_obj[p], &s->exec[p]);
  }
  if (s->cap_stream) (void)hipStreamDestroy(s->cap_stream);
  if (s->host_ctl) (void)hipHostFree(s->host_ctl);
  if (s->host_h) (void)hipHostFree(s->host_h);
  delete s;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Recorded solve + reverse sweep: training with opt['adjoint'] = False (the reference's default and its Cora / Citeseer
// best_params; src/base_classes.py:44-47): autograd runs back through every accepted step of torchdiffeq's dopri5.  Here the forward
// is the device-controlled solve above leaving the accepted steps' stage inputs on a tape, and the backward is ONE call that walks
// the tape with the fused row kernel of the adjoint stage (spmm.hip, launch_adjoint_rows) -- per evaluation k_i = f(u_i), ONE launch
// on the transposed graph forms W_i = a (A^T G_i - G_i) (+ the incoming dL/dy1 as its source term in stage 6), the next G_{i-1} =
// h sum_m a_{m,i-1} W_m in its epilogue, the edge products r_e += u_i[row'] . G_i[col'] and the dot <u_i, W_i> = <G_i, k_i - b x0>.
// The algebra is written out and pinned against torch autograd in oracle/tape_reverse.py / tests/test_tape_reverse_cpu.py.
// The record (gnpde_dopri5_set_tape, _tape_bytes, _tape_slots, _tape_record) serves the Laplacian, transformer and GAT functions alike: stage
// inputs only.  The sweep below is GRAND-l's (f linear in u; the weights are constants of the solve that carry gradients: attention
// block); GRAND-nl and GAT records are swept by csrc/adjoint.hip (gnpde_adjoint_set_dopri5_tape, the walk of tape_reverse.h).
// ------------------------------------------------------------------------------------------------
extern "C" size_t gnpde_dopri5_tape_bytes(const gnpde_rhs_t* rhs, int32_t capacity_steps) {
  if (check_rhs(rhs) || capacity_steps < 1) return 0;
  const size_t state = align_up(static_cast<size_t>(rhs->graph->n) * rhs->ld * 4, 256);
  return (3 + 6 * (static_cast<size_t>(capacity_steps) + 1) + 1) * state + align_up(sizeof(float) * capacity_steps, 256) + 256;
}

extern "C" int gnpde_dopri5_set_tape(gnpde_dopri5_t* s, void* tape, size_t tape_bytes, int32_t capacity_steps) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "dopri5_set_tape: solver is null");
  for (int p = 0; p < 2; ++p) {      // the store kernel and the stage-input buffers are part of the captured trial step
    drop_capture(&s->graph_obj[p], &s->exec[p]);
  }
  s->tape = nullptr;
  s->tape_steps = 0;
  if (tape == nullptr) return 0;
  GNPDE_CHECK_ARG(s->t_out == nullptr, GNPDE_EINVAL,
                  "dopri5_set_tape: a recorded solve has two output times (detach the outputs first: gnpde_dopri5_set_outputs(s, NULL, 0, NULL, 0))");
  GNPDE_CHECK_ARG(s->shard == nullptr, GNPDE_ESTATE, "dopri5_set_tape: not on a row-partitioned solve");
  GNPDE_CHECK_ARG(s->pair == GNPDE_ADAPTIVE_DOPRI5, GNPDE_ESTATE, "dopri5_set_tape: the recorded solve is Dormand-Prince's");
  // (the store kernel copies stage inputs whatever f is; GRAND-nl / GAT records are swept by gnpde_adjoint_set_dopri5_tape, which
  //  recomputes q||k and the weights of every evaluation -- nothing of an evaluation is recorded inside a trial step that may be rejected)
  GNPDE_CHECK_ARG(s->rhs.kind == GNPDE_RHS_LAPLACIAN || s->rhs.kind == GNPDE_RHS_TRANSFORMER || s->rhs.kind == GNPDE_RHS_GAT, GNPDE_EINVAL,
                  "dopri5_set_tape: the recorded solve covers the Laplacian, transformer and GAT functions");
  GNPDE_CHECK_ARG(capacity_steps >= 1 && reinterpret_cast<uintptr_t>(tape) % 256 == 0, GNPDE_EINVAL, "dopri5_set_tape: bad capacity or alignment");
  const size_t need = gnpde_dopri5_tape_bytes(&s->rhs, capacity_steps);
  GNPDE_CHECK_ARG(tape_bytes >= need, GNPDE_EWS, "dopri5_set_tape: %zu bytes (need %zu)", tape_bytes, need);
  if (s->host_h_capacity < capacity_steps) {
    if (s->host_h) (void)hipHostFree(s->host_h);
    s->host_h = nullptr;
    GNPDE_HIP(hipHostMalloc(reinterpret_cast<void**>(&s->host_h), sizeof(float) * capacity_steps, hipHostMallocDefault));
    s->host_h_capacity = capacity_steps;
  }
  const size_t stride = s->state_bytes / 4;
  float* base = static_cast<float*>(tape);
  for (int j = 0; j < 3; ++j) s->tape_x[j] = base + j * stride;
  s->tape_slots = base + 3 * stride;
  s->tape_h = s->tape_slots + (6 * (static_cast<size_t>(capacity_steps) + 1) + 1) * stride;
  s->tape_overflow = reinterpret_cast<int*>(reinterpret_cast<char*>(s->tape_h) + align_up(sizeof(float) * capacity_steps, 256));
  s->tape_capacity = capacity_steps;
  s->tape = base;
  // (the caller hands over zero-filled memory: the padding columns of the extra stage-input buffers are read by 16-byte lanes)
  return 0;
}

extern "C" int gnpde_dopri5_tape_steps(const gnpde_dopri5_t* s) { return s ? s->tape_steps : 0; }

extern "C" int gnpde_dopri5_tape_slots(const gnpde_dopri5_t* s, const float** slots, size_t* slot_stride) {
  GNPDE_CHECK_ARG(s != nullptr && s->tape != nullptr && slots != nullptr && slot_stride != nullptr, GNPDE_EINVAL, "dopri5_tape_slots: no recorded solve");
  *slots = s->tape_slots;
  *slot_stride = s->state_bytes / 4;
  return 0;
}

extern "C" int gnpde_dopri5_tape_record(const gnpde_dopri5_t* s, float* h_out, int32_t capacity, float* x_out) {
  GNPDE_CHECK_ARG(s != nullptr && s->tape != nullptr && (h_out != nullptr || capacity == 0), GNPDE_EINVAL, "dopri5_tape_record: no recorded solve");
  for (int i = 0; i < s->tape_steps && i < capacity; ++i) h_out[i] = s->host_h[i];
  if (x_out) *x_out = s->last_x;
  return 0;
}

namespace {
// buffers of the reverse sweep inside its workspace
struct SweepLayout {
  size_t off_one, off_dots, off_part, off_state, total;
  size_t dots_floats, part_bytes;
  int slots;
};

SweepLayout sweep_layout(const gnpde_dopri5* s, const gnpde_graph_t* gt, int steps) {
  SweepLayout L{};
  const gnpde_rhs_t& r = s->rhs;
  L.slots = adjoint_rows_dot_slots(gt, r.d);
  L.dots_floats = 2 * static_cast<size_t>(L.slots) * (6 * static_cast<size_t>(steps) + 1);
  L.part_bytes = static_cast<size_t>(gt->n_long_chunks) * align_up(static_cast<size_t>(r.d), 4) * sizeof(float);
  size_t off = 0;
  L.off_one = off;   off += 2048;                              // 1.0f, then the fold's 128 partial sums (double)
  L.off_dots = off;  off += align_up(L.dots_floats * sizeof(float), 256);
  L.off_part = off;  off += align_up(L.part_bytes, 256);
  L.off_state = off; off += 18 * s->state_bytes;
  L.total = off;
  return L;
}
}  // namespace

extern "C" size_t gnpde_dopri5_tape_backward_workspace_bytes(const gnpde_dopri5_t* s, const gnpde_graph_t* graph_t) {
  if (s == nullptr || graph_t == nullptr || s->tape == nullptr) return 0;
  return sweep_layout(s, graph_t, s->tape_steps > 0 ? s->tape_steps : s->tape_capacity).total;
}

extern "C" int gnpde_dopri5_tape_backward(gnpde_dopri5_t* s, const gnpde_graph_t* graph_t, const float* w_t, const float* grad_out,
                                          int32_t ld_go, float* grad_y0, int32_t ld_gy0, float* r_t, float* sum_g, float* dot_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  GNPDE_CHECK_ARG(s && graph_t && grad_out && grad_y0 && r_t && sum_g && dot_out && (w_t || graph_t->e == 0), GNPDE_EINVAL,
                  "dopri5_tape_backward: null argument");
  GNPDE_CHECK_ARG(s->tape != nullptr && s->tape_steps >= 1, GNPDE_EINVAL, "dopri5_tape_backward: no recorded solve to differentiate");
  GNPDE_CHECK_ARG(s->rhs.kind == GNPDE_RHS_LAPLACIAN, GNPDE_EINVAL, "dopri5_tape_backward: the Laplacian function's sweep (f linear in the state); "
                  "GRAND-nl and GAT records: gnpde_adjoint_set_dopri5_tape");
  const gnpde_rhs_t& r = s->rhs;
  GNPDE_CHECK_ARG(graph_t->n == r.graph->n && graph_t->e == r.graph->e, GNPDE_ESHAPE, "dopri5_tape_backward: the transposed graph does not match");
  GNPDE_CHECK_ARG(ld_go >= r.d && ld_gy0 >= r.d && r.ld % 4 == 0 && r.d <= 256, GNPDE_ESHAPE, "dopri5_tape_backward: bad strides / width");
  const int S = s->tape_steps;
  const SweepLayout L = sweep_layout(s, graph_t, S);
  GNPDE_CHECK_ARG(workspace && workspace_bytes >= L.total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0, GNPDE_EWS,
                  "dopri5_tape_backward: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, L.total);
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* ws = static_cast<char*>(workspace);
  const long long n = r.graph->n;
  const long long flat = n * r.ld;
  const size_t stride = s->state_bytes / 4;
  const bool padded = (r.flags & GNPDE_RHS_PADDED_ROWS) != 0;
  float* one = reinterpret_cast<float*>(ws + L.off_one);
  float* dots = reinterpret_cast<float*>(ws + L.off_dots);
  void* part = L.part_bytes ? static_cast<void*>(ws + L.off_part) : nullptr;
  float* sb = reinterpret_cast<float*>(ws + L.off_state);
  float* Z = sb;                       // zeros: the base of every linear combination formed here
  float* GO = sb + 1 * stride;         // dL/d(out) in the state layout
  float* W[7] = {nullptr, sb + 2 * stride, sb + 3 * stride, sb + 4 * stride, sb + 5 * stride, sb + 6 * stride, sb + 7 * stride};
  float* Gk[6] = {nullptr, sb + 8 * stride, sb + 9 * stride, sb + 10 * stride, sb + 11 * stride, sb + 12 * stride};
  float* gk_io[2] = {sb + 13 * stride, sb + 14 * stride};    // G_k6 coming in / G_k0 going out, alternating
  float* gy_io[2] = {sb + 15 * stride, sb + 16 * stride};    // G_y1 coming in / G_y going out
  float* GY0 = sb + 17 * stride;
  GNPDE_HIP(hipMemsetAsync(Z, 0, 2 * s->state_bytes, st));                         // Z and GO (its padding columns stay zero)
  GNPDE_HIP(hipMemsetAsync(sum_g, 0, static_cast<size_t>(flat) * sizeof(float), st));
  if (graph_t->e > 0) GNPDE_HIP(hipMemsetAsync(r_t, 0, static_cast<size_t>(graph_t->e) * sizeof(float), st));
  GNPDE_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(one), 0x3f800000, 1, st));     // 1.0f: weight of the source term
  if (int rc = launch_copy_rows(grad_out, ld_go, GO, r.ld, n, r.d, st)) return rc;
  auto slot_u = [&](int step, int i) -> const float* {       // stage input u_i of accepted step `step` (u_6 = u_0 of the next slot)
    return i < 6 ? s->tape_slots + (static_cast<size_t>(step) * 6 + i) * stride : s->tape_slots + (static_cast<size_t>(step) + 1) * 6 * stride;
  };
  int launch = 0;
  auto stage = [&](const float* g_in, const float* u_in, const float* source, float* out_w, float* out_g, const float* const* prev,
                   const float* coef, int n_prev) -> int {
    gnpde_epilogue_t e = base_epilogue(r);
    e.beta = source ? one : nullptr;
    e.x0 = source;
    e.stage = GNPDE_STAGE_LINCOMB;
    e.y = Z;
    e.out_k = out_w;
    e.out_y = out_g;
    e.n_prev = n_prev;
    for (int j = 0; j < n_prev; ++j) { e.prev[j] = prev[j]; e.coef[j] = coef[j]; }
    e.coef[n_prev] = coef[n_prev];
    e.coef_scale = nullptr;
    float* d = dots + 2 * static_cast<size_t>(L.slots) * launch;
    ++launch;
    return launch_adjoint_rows(graph_t, w_t, g_in, u_in, r.d, r.ld, &e, r_t, d, part, L.part_bytes, st, padded, true);
  };
  int io = 0;       // gk_io[io] / gy_io[io] hold what comes in from the later step
  for (int step = S - 1; step >= 0; --step) {
    const float h = s->host_h[step];
    const bool last = step == S - 1;
    float cD[7] = {0, 0, 0, 0, 0, 0, 0};
    float cDy = 0.f;
    if (last) {
      // torchdiffeq interp.py: out = y + x cd + x^2 cc + x^3 cb + x^4 ca; every operand enters linearly (oracle/tape_reverse.py)
      const double x = static_cast<double>(s->last_x), x2 = x * x, x3 = x2 * x, x4 = x3 * x, hd = static_cast<double>(h);
      const double p_ym = 16 * x2 - 32 * x3 + 16 * x4, p_y = 1 - 11 * x2 + 18 * x3 - 8 * x4, p_y1 = -5 * x2 + 14 * x3 - 8 * x4;
      const double p_k0 = hd * (x - 4 * x2 + 5 * x3 - 2 * x4), p_k6 = hd * (x2 - 3 * x3 + 2 * x4);
      for (int j = 0; j < 7; ++j) cD[j] = static_cast<float>(p_ym * hd * kDopri5.c_mid[j]);
      cD[0] = static_cast<float>(p_ym * hd * kDopri5.c_mid[0] + p_k0);
      cDy = static_cast<float>(p_y + p_ym);
      const float* v[1] = {GO};
      const float c1[1] = {static_cast<float>(p_y1)};
      if (int rc = launch_lincomb(Z, v, c1, 1, flat, gy_io[io], st, nullptr)) return rc;
      const float c6[1] = {static_cast<float>(p_ym * hd * kDopri5.c_mid[6] + p_k6)};
      if (int rc = launch_lincomb(Z, v, c6, 1, flat, gk_io[io], st, nullptr)) return rc;
    }
    float* gk_in = gk_io[io];
    float* gy_in = gy_io[io];
    float* gk_out = gk_io[1 - io];
    float* gy_out = gy_io[1 - io];
    for (int i = 6; i >= 1; --i) {
      // after this launch: W_i, and G_{i-1} = D_{i-1} + h sum_{m >= i} a_{m,i-1} W_m   (a_{m,j} = kDopri5.a[m-1][j]; its row 5 = b)
      const float* prev[GNPDE_MAX_PREV];
      float coef[GNPDE_MAX_PREV + 1];
      int np = 0;
      for (int m = 6; m > i; --m) { prev[np] = W[m]; coef[np] = static_cast<float>(kDopri5.a[m - 1][i - 1]) * h; ++np; }
      if (last && cD[i - 1] != 0.f) { prev[np] = GO; coef[np] = cD[i - 1]; ++np; }
      coef[np] = static_cast<float>(kDopri5.a[i - 1][i - 1]) * h;
      const float* g_in = i == 6 ? gk_in : Gk[i];
      float* g_next = i == 1 ? gk_out : Gk[i - 1];
      if (int rc = stage(g_in, slot_u(step, i), i == 6 ? gy_in : nullptr, W[i], g_next, prev, coef, np)) return rc;
    }
    {   // G_y = D_y + sum_m W_m
      const float* v[7] = {W[1], W[2], W[3], W[4], W[5], W[6], GO};
      const float c[7] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, cDy};
      if (int rc = launch_lincomb(Z, v, c, last && cDy != 0.f ? 7 : 6, flat, gy_out, st, nullptr)) return rc;
    }
    {   // sum of the gradients that reached k_1..k_6 of this step (d beta = <that sum, x0>)
      const float* v[6] = {gk_in, Gk[5], Gk[4], Gk[3], Gk[2], Gk[1]};
      const float c[6] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
      if (int rc = launch_lincomb(sum_g, v, c, 6, flat, sum_g, st, nullptr)) return rc;
    }
    io = 1 - io;
  }
  {   // the first evaluation k_0 = f(y0):  dL/dy0 = G_y + a (A^T G_k0 - G_k0)
    const float c0[1] = {0.f};
    if (int rc = stage(gk_io[io], slot_u(0, 0), gy_io[io], GY0, nullptr, nullptr, c0, 0)) return rc;
    const float* v[1] = {gk_io[io]};
    const float c[1] = {1.f};
    if (int rc = launch_lincomb(sum_g, v, c, 1, flat, sum_g, st, nullptr)) return rc;
  }
  if (int rc = launch_copy_rows(GY0, r.ld, grad_y0, ld_gy0, n, r.d, st)) return rc;
  double* fold_part = reinterpret_cast<double*>(ws + L.off_one + 64);       // (behind the 1.0f of the source weight)
  hipLaunchKernelGGL(tape_dots_partial_kernel, dim3(kTapeFoldBlocks), dim3(kBlock), 0, st, dots, static_cast<long long>(L.slots) * launch, fold_part);
  GNPDE_LAUNCH_CHECK();
  hipLaunchKernelGGL(tape_dots_fold_kernel, dim3(1), dim3(kTapeFoldBlocks), 0, st, fold_part, dot_out);
  GNPDE_LAUNCH_CHECK();
  return 0;
}
