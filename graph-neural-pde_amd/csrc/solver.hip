// One right-hand-side evaluation f(u) composed from the kernels of this library, and the
// fixed-step solver loop (torchdiffeq 0.2.1 `euler` / `rk4` == 3/8 rule) with the stage algebra
// fused into the aggregation epilogue and the whole time grid captured in ONE hipGraph.
//
// Replaces ODEFunc.forward (reference src/function_laplacian_diffusion.py:38-51,
// src/function_transformer_attention.py:38-53, src/function_GAT_attention.py:45-65) and the Python
// solver loop reached from ODEblock.forward (src/block_constant.py:57-62,
// src/block_transformer_attention.py:58-63): ~30 launches + ~10 elementwise launches per stage there,
// 1 (GRAND-l) or 5 (GRAND-nl) launches per stage here and a single graph launch per forward pass.
#include <atomic>
#include <vector>
#include "common.h"
#include "fixed_grid.h"
#include "graph_capture.h"
#include "rhs.h"

namespace gnpde {

int launch_linear_any(const float* x, int n, int d, int ldx, const float* W, int m, int ldw, const float* b, float* out,
                      int ldo, hipStream_t s, int relu = 0);
int launch_edge_attention(const gnpde_graph_t* g, const gnpde_attention_t* at, float* w_mean_csr, float* att_edge,
                          float* prods_edge, void* ws, size_t ws_bytes, hipStream_t stream, const Fork* fork);
int launch_normalise_heads(float* qk, long long n, int ld, int att_dim, int heads, bool centre, hipStream_t s, float* inv_out = nullptr);
size_t attention_workspace_bytes(const gnpde_graph_t* g, int h, bool gat);
size_t attention_workspace_bytes_rows(const gnpde_graph_t* g, int h, bool gat, int key_rows);
size_t fused_attn_workspace_bytes(const gnpde_graph_t* g, int d, int heads);
bool fused_attn_supported(const gnpde_attention_t& at, int d, int ld, const void* u, const gnpde_epilogue_t* epi);
int launch_attn_rhs_fused(const gnpde_graph_t* g, const gnpde_attention_t* at, const float* proj_w, const float* proj_b,
                          const float* u, int d, int ld, const gnpde_epilogue_t* epi, void* ws, size_t ws_bytes,
                          hipStream_t stream);


// The projection comes FIRST so that two descriptors over the same state rows (interior / boundary pass of a
// partitioned graph) that are handed the same workspace see the SAME q||k buffer; the regions behind it are
// scratch that each pass overwrites (the passes are ordered on one stream).
RhsLayout rhs_layout(const gnpde_rhs_t& r) {
  RhsLayout L{};
  const gnpde_graph_t& g = *r.graph;
  size_t off = 0;
  if (r.kind != GNPDE_RHS_LAPLACIAN) {
    const size_t prow = r.n_state_rows > g.n ? r.n_state_rows : g.n;
    L.proj = off;  off += align_up(prow * r.proj_m * 4, 256);
  }
  // mix_features: the aggregation gathers rows of the projection table (A wide) instead of state rows (d wide); the workspace is
  // sized for the wider of the two
  const bool mix = rhs_mix_features(r);
  L.spmm = off;
  L.spmm_bytes = gnpde_spmm_workspace_bytes(&g, mix && r.att.att_dim > r.d ? r.att.att_dim : r.d);
  off += align_up(L.spmm_bytes, 256);
  if (r.kind != GNPDE_RHS_LAPLACIAN) {
    L.wmean = off; off += align_up(static_cast<size_t>(g.e) * 4, 256);
    L.att = off;
    L.att_bytes = attention_workspace_bytes_rows(&g, r.att.heads, r.kind == GNPDE_RHS_GAT, r.n_state_rows);
    off += align_up(L.att_bytes, 256);
    if (r.kind == GNPDE_RHS_TRANSFORMER) {
      L.fused = off;
      L.fused_bytes = fused_attn_workspace_bytes(&g, r.d, r.att.heads);
      off += align_up(L.fused_bytes, 256);
    }
  }
  if (mix) {   // the aggregate z = A(x) (x W) that gnpde_linear_epilogue reads (without the flag no offset above or below moves)
    L.z = off; off += align_up(static_cast<size_t>(g.n) * r.att.att_dim * 4, 256);
  }
  // the aggregation's hub-row tickets (they belong to the partials; LAST, so that every other region keeps its offset)
  L.tickets = off;
  L.ticket_bytes = gnpde_spmm_ticket_bytes(&g);
  off += align_up(L.ticket_bytes, 256);
  L.total = off;
  return L;
}

int check_rhs(const gnpde_rhs_t* r) {
  GNPDE_CHECK_ARG(r && r->graph, GNPDE_EINVAL, "rhs: null descriptor");
  GNPDE_CHECK_ARG(r->kind >= GNPDE_RHS_LAPLACIAN && r->kind <= GNPDE_RHS_GAT, GNPDE_EINVAL, "rhs: bad kind %d", r->kind);
  GNPDE_CHECK_ARG(r->d >= 1 && r->ld >= r->d, GNPDE_EINVAL, "rhs: bad d/ld");
  GNPDE_CHECK_ARG(r->alpha != nullptr, GNPDE_EINVAL, "rhs: alpha is null");
  GNPDE_CHECK_ARG(r->x0 == nullptr || r->beta != nullptr, GNPDE_EINVAL, "rhs: x0 without beta");
  if (r->kind == GNPDE_RHS_LAPLACIAN) {
    GNPDE_CHECK_ARG(r->w_csr != nullptr || r->graph->e == 0, GNPDE_EINVAL, "rhs: laplacian needs w_csr");
  } else {
    GNPDE_CHECK_ARG(r->proj_w != nullptr && r->proj_m >= 1, GNPDE_EINVAL, "rhs: projection weights missing");
    const int need = r->kind == GNPDE_RHS_TRANSFORMER ? 2 * r->att.att_dim : r->att.att_dim;
    GNPDE_CHECK_ARG(r->proj_m == need, GNPDE_EINVAL, "rhs: proj_m=%d but attention needs %d", r->proj_m, need);
  }
  if (rhs_mix_features(*r)) {
    GNPDE_CHECK_ARG(r->kind == GNPDE_RHS_GAT, GNPDE_EINVAL, "rhs: GNPDE_RHS_MIX_FEATURES is the GAT function's (kind %d)", r->kind);
    GNPDE_CHECK_ARG(r->out_w != nullptr && r->out_ld >= r->att.att_dim, GNPDE_EINVAL, "rhs: mix_features needs out_w [d, A] with out_ld >= A");
    GNPDE_CHECK_ARG(r->proj_row_end == 0 && r->n_state_rows <= r->graph->n, GNPDE_ESHAPE,
                    "rhs: mix_features on a partitioned descriptor (whole-graph descriptors only)");
    GNPDE_CHECK_ARG(linear_epilogue_supported(r->att.att_dim, r->d), GNPDE_ESHAPE,
                    "rhs: mix_features with attention_dim = %d, d = %d (attention_dim a multiple of 4 up to 256, d up to 256)", r->att.att_dim, r->d);
  }
  return 0;
}

// evaluations enqueued in the one-launch attention form (gnpde_one_launch_evaluations: the tests read the launch decision from it)
static std::atomic<long long> g_one_launch_evals{0};

// Enqueue f(u) with the given epilogue.  `ws` follows rhs_layout.
int enqueue_rhs(const gnpde_rhs_t& r, const float* u, const gnpde_epilogue_t& epi, char* ws, const RhsLayout& L,
                hipStream_t s, const Fork* fork, const RhsRecord* record, const LoPair* lo, bool tickets) {
  const gnpde_graph_t* g = r.graph;
  const bool padded = (r.flags & GNPDE_RHS_PADDED_ROWS) != 0 && r.ld % 4 == 0;
  SpmmOptions opt;      // of the aggregation that ends the evaluation
  opt.padded_rows = padded;
  opt.tickets = tickets && L.ticket_bytes > 0 ? ws + L.tickets : nullptr;
  opt.ticket_bytes = L.ticket_bytes;
  const float* w = r.w_csr;
  if (record != nullptr && rhs_record_stride(r) == 0) record = nullptr;
  if (lo != nullptr && lo->u_lo == nullptr) lo = nullptr;
  // bf16 gather operand: the routes with the attention inside the aggregation kernel are not taken (separate launches run)
  if (lo == nullptr && record == nullptr && r.kind == GNPDE_RHS_TRANSFORMER && fused_attn_supported(r.att, r.d, r.ld, u, &epi) &&
      reinterpret_cast<uintptr_t>(r.proj_w) % 16 == 0) {
    // scaled-dot attention, softmax over rows: projection + attention + aggregation + epilogue in one pass
    return launch_attn_rhs_fused(g, &r.att, r.proj_w, r.proj_b, u, r.d, r.ld, &epi, ws + L.fused, L.fused_bytes, s);
  }
  if (r.kind != GNPDE_RHS_LAPLACIAN) {
    float* proj = record ? record->proj : reinterpret_cast<float*>(ws + L.proj);
    float* wmean = record ? record->wmean : reinterpret_cast<float*>(ws + L.wmean);
    int p0 = 0, p1 = r.n_state_rows > g->n ? r.n_state_rows : g->n;   // keys of halo rows are recomputed locally
    if (r.proj_row_end > 0) {  // this pass projects only a slice of the state rows
      p0 = r.proj_row_begin;
      p1 = r.proj_row_end;
    }
    const bool key_table = rhs_key_table(r, u);       // q and k as two tables: the k gathers of the attention fetch whole lines of keys
    int rc = 0;
    if (key_table) rc = launch_linear_split(u, g->n, r.d, r.ld, r.proj_w, r.proj_m, r.d, r.proj_b, proj, proj + static_cast<size_t>(g->n) * r.att.att_dim,
                                            r.att.att_dim, s);
    else if (p1 > p0) rc = launch_linear_any(u + static_cast<size_t>(p0) * r.ld, p1 - p0, r.d, r.ld, r.proj_w, r.proj_m, r.d,
                                             r.proj_b, proj + static_cast<size_t>(p0) * r.proj_m, r.proj_m, s);
    if (rc) return rc;
    gnpde_attention_t at = r.att;
    at.ldqk = key_table ? r.att.att_dim : r.proj_m;
    at.q = proj;
    at.k = key_table ? proj + static_cast<size_t>(g->n) * r.att.att_dim : (r.kind == GNPDE_RHS_TRANSFORMER ? proj + r.att.att_dim : proj);
    if (r.kind == GNPDE_RHS_TRANSFORMER && (at.type == GNPDE_ATT_COSINE || at.type == GNPDE_ATT_PEARSON) &&
        at.heads >= 1 && at.att_dim % at.heads == 0) {
      // cosine_sim / pearson (reference src/function_transformer_attention.py:198-206) = the scaled dot product of unit (mean-centred)
      // head vectors: the rows just projected are normalised in place (the query side times sqrt(d_k)) and everything behind --
      // fused row kernels with their hub phases, the fused normalisers over columns / squareplus, attention inside the aggregation
      // kernel on small graphs -- is the scaled-dot path
      rc = launch_normalise_heads(proj + static_cast<size_t>(p0) * r.proj_m, p1 > p0 ? p1 - p0 : 0, r.proj_m, at.att_dim, at.heads,
                                  at.type == GNPDE_ATT_PEARSON, s);
      if (rc) return rc;
      at.type = GNPDE_ATT_SCALED_DOT;
    }
    at.n_key_rows = r.n_state_rows > g->n ? r.n_state_rows : 0;     // halo rows: the GAT node terms cover them
    if (lo == nullptr && record == nullptr && r.kind == GNPDE_RHS_TRANSFORMER && fork == nullptr && r.proj_row_end == 0 && r.n_state_rows <= g->n &&
        (r.d % 4 == 0 || padded) && attn_spmm_supported(g, at, r.d, r.ld, u, epi)) {
      // scaled-dot row softmax: the short rows are attended inside the aggregation kernel; only the hub rows' weights are
      // computed ahead (two small launches)
      rc = launch_hub_attention(g, &at, wmean, ws + L.att, L.att_bytes, s);
      if (rc) return rc;
      return launch_attn_spmm(g, &at, wmean, u, r.d, r.ld, &epi, ws + L.spmm, L.spmm_bytes, s, padded);
    }
    // Whole-graph GRAND-nl with the plain scaled-dot row softmax, fp32 gather, aggregation next on this stream: the row attention is
    // ONE launch, and the hub-chunk items of the aggregation normalise the hub rows (HubDefer) -- the weight buffer is complete after the
    // aggregation, so a recorded solve takes this form too.  Here stand the conditions that are the evaluation's -- among them the
    // score type the CALLER named: cosine_sim / pearson reach the attention as scaled_dot (above) and keep their two launches.  The
    // attention's own conditions are its plan's: the deferred launcher plans once, runs what the plan says (the plain launcher's launches
    // where that is not the one launch) and reports in defer.taken which it was.
    if (lo == nullptr && fork == nullptr && r.kind == GNPDE_RHS_TRANSFORMER && r.att.type == GNPDE_ATT_SCALED_DOT && r.proj_row_end == 0 &&
        r.n_state_rows <= g->n && spmm_hub_defer_supported(g, u, r.d, r.ld, epi, ws + L.spmm, padded)) {
      HubDefer defer;
      rc = launch_edge_attention_deferred(g, &at, wmean, ws + L.att, L.att_bytes, s, &defer);
      if (rc) return rc;
      if (defer.taken) g_one_launch_evals.fetch_add(1, std::memory_order_relaxed);
      opt.defer = &defer;
      return launch_spmm_rhs(g, wmean, u, r.d, r.ld, &epi, nullptr, ws + L.spmm, L.spmm_bytes, s, opt);
    }
    if (rhs_mix_features(r)) {
      // f = alpha' (A(x) (x W) Wout - x) + beta x0: the plain aggregation gathers rows of the projection table (its normal hub-row
      // handling, one stream, fp32), and the out-projection carries the caller's epilogue
      rc = launch_edge_attention(g, &at, wmean, nullptr, nullptr, ws + L.att, L.att_bytes, s, nullptr);
      if (rc) return rc;
      float* z = reinterpret_cast<float*>(ws + L.z);
      rc = launch_spmm_rhs(g, wmean, proj, r.att.att_dim, r.proj_m, nullptr, z, ws + L.spmm, L.spmm_bytes, s);
      if (rc) return rc;
      return launch_linear_epilogue(z, g->n, r.att.att_dim, r.att.att_dim, r.out_w, r.d, r.out_ld, u, r.ld, epi, padded, s);
    }
    rc = launch_edge_attention(g, &at, wmean, nullptr, nullptr, ws + L.att, L.att_bytes, s, fork);
    if (rc) return rc;
    w = wmean;
  }
  opt.fork = fork;
  opt.lo = lo;
  return launch_spmm_rhs(g, w, u, r.d, r.ld, &epi, nullptr, ws + L.spmm, L.spmm_bytes, s, opt);
}

bool rhs_gather_lo_supported(const gnpde_rhs_t& r) {
  const bool padded = (r.flags & GNPDE_RHS_PADDED_ROWS) != 0;
  return !rhs_mix_features(r) && r.ld % 4 == 0 && (r.d % 4 == 0 || padded) && r.d <= 1024 && r.n_state_rows <= r.graph->n && r.proj_row_end == 0 &&
         r.graph->row_begin == 0;
}

gnpde_epilogue_t base_epilogue(const gnpde_rhs_t& r) {
  gnpde_epilogue_t e{};
  e.alpha = r.alpha;
  e.beta = r.beta;
  e.x0 = r.x0;
  e.alpha_sigmoid = r.alpha_sigmoid;
  return e;
}

}  // namespace gnpde

using namespace gnpde;

struct gnpde_solver {
  gnpde_rhs_t rhs;
  gnpde_graph_t graph;
  gnpde_graph_t graph_t;
  int method;
  std::vector<float> dts;
  char* ws;
  size_t ws_bytes;
  RhsLayout L;
  size_t off_k1, off_k2, off_k3, off_ua, off_ub, off_rhs;
  hipStream_t cap_stream = nullptr;
  Fork fork;                 // second stream + events for the hub-row branch
  hipGraph_t graph_obj = nullptr;
  hipGraphExec_t exec = nullptr;
  float* captured_y = nullptr;
  int n_evals = 0;
  bool early = false;        // early-stopping evaluator after every step
  gnpde_decoder_t dec{};
  int* early_state = nullptr;
  int* early_trace = nullptr;
  int early_trace_capacity = 0;
  float* tape = nullptr;     // recorded solve (gnpde_solver_set_tape): n_evals + 1 state-sized slots, the stage inputs in evaluation order
  float* tape_rec = nullptr; // ... followed by one RhsRecord per evaluation (GRAND-nl with scaled-dot scores: q||k and the weights)
  uint16_t* lo = nullptr;    // bf16 gather operand (gnpde_solver_set_gather): one shadow per stage-input buffer, caller's memory
  // outputs at several times (gnpde_solver_set_outputs): output j is taken after step out_step[j] (1-based, non-decreasing) at the
  // fraction out_frac[j] of that step; a step with an output strictly inside it keeps its start state in out_scratch
  std::vector<int> out_step;
  std::vector<float> out_frac;
  float* out = nullptr;
  int ld_out = 0;
  float* out_scratch = nullptr;
  const int* out_order = nullptr;
};

namespace {

// one bf16 shadow per stage-input buffer (stage_input_buffers of fixed_grid.h)
size_t lo_stride(const gnpde_rhs_t& r) { return align_up(static_cast<size_t>(r.graph->n) * r.ld * 2, 256); }

size_t solver_layout(const gnpde_rhs_t& r, int method, gnpde_solver* s) {
  const size_t state = align_up(static_cast<size_t>(r.graph->n) * r.ld * 4, 256);
  size_t off = 0;
  size_t k1 = 0, k2 = 0, k3 = 0, ua = 0, ub = 0;
  ua = off; off += state;
  if (method == GNPDE_METHOD_RK4) {
    ub = off; off += state;
    k1 = off; off += state;
    k2 = off; off += state;
    k3 = off; off += state;
  }
  const size_t rhs_off = off;
  off += rhs_layout(r).total;
  if (s) {
    s->off_ua = ua; s->off_ub = ub; s->off_k1 = k1; s->off_k2 = k2; s->off_k3 = k3; s->off_rhs = rhs_off;
  }
  return off;
}

int ensure_fork(gnpde_solver* s) {
  if (s->fork.aux != nullptr) return 0;
  GNPDE_HIP(hipStreamCreateWithFlags(&s->fork.aux, hipStreamNonBlocking));
  GNPDE_HIP(hipEventCreateWithFlags(&s->fork.e_fork, hipEventDisableTiming));
  GNPDE_HIP(hipEventCreateWithFlags(&s->fork.e_join, hipEventDisableTiming));
  return 0;
}

int enqueue_solve(gnpde_solver* s, float* y, hipStream_t st) {
  const gnpde_rhs_t& r = s->rhs;
  const Fork* fk = (s->rhs.graph->n_long_rows > 0 && g_tune[GNPDE_TUNE_FORK] == 1) ? &s->fork : nullptr;  // opt-in: cross-stream joins cost more than they hide
  if (fk != nullptr) {
    const int frc = ensure_fork(s);
    if (frc) return frc;
  }
  char* rws = s->ws + s->off_rhs;
  float* ua = reinterpret_cast<float*>(s->ws + s->off_ua);
  int step = 0;
  auto evaluate = [&](const float* state) -> int {
    ++step;
    if (!s->early) return 0;
    return enqueue_early_stop_eval(s->dec, state, r.ld, r.graph->n, step, s->early_state,
                                   s->early_trace, s->early_trace_capacity, st);
  };
  // outputs at several times: before a step with an output strictly inside it the start state goes to the scratch buffer (the stage
  // buffers are recycled inside the step), after a step every output that falls into it is one snapshot launch
  size_t next_out = 0;
  auto interior = [](float f) { return f != 1.0f; };
  auto before_step = [&](int i, const float* state) -> int {      // i: the 1-based number of the step about to run
    for (size_t j = next_out; j < s->out_step.size() && s->out_step[j] == i; ++j)
      if (interior(s->out_frac[j])) {
        GNPDE_HIP(hipMemcpyAsync(s->out_scratch, state, static_cast<size_t>(r.graph->n) * r.ld * 4, hipMemcpyDeviceToDevice, st));
        break;
      }
    return 0;
  };
  auto after_step = [&](int i, const float* state) -> int {
    for (; next_out < s->out_step.size() && s->out_step[next_out] == i; ++next_out) {
      const float f = s->out_frac[next_out];
      float* dst = s->out + next_out * static_cast<size_t>(r.graph->n) * s->ld_out;
      if (int rc = launch_snapshot_rows(interior(f) ? s->out_scratch : nullptr, state, f, r.graph->n, r.d, r.ld, dst, s->ld_out, s->out_order, st))
        return rc;
    }
    return 0;
  };
  if (s->early) GNPDE_HIP(hipMemsetAsync(s->early_state, 0, 8 * sizeof(int32_t), st));
  // hub-row tickets of the aggregation launches: zero at the head of the solve (a memset node of a captured one); every launch that uses
  // them leaves them zero
  if (s->L.ticket_bytes > 0) GNPDE_HIP(hipMemsetAsync(rws + s->L.tickets, 0, s->L.ticket_bytes, st));
  // bf16 gather operand: shadow b belongs to one stage-input buffer; the kernel that writes a stage input writes its shadow, so
  // only y0's is filled by a pass of its own.  pair(from, to): gather from shadow `from`, write the shadow of out_y to `to`.
  const bool lo_on = s->lo != nullptr;
  auto shadow = [&](int b) { return reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(s->lo) + b * lo_stride(r)); };
  LoPair lo_store{};
  auto pair = [&](int from, int to) -> const LoPair* {
    if (!lo_on) return nullptr;
    lo_store.u_lo = shadow(from);
    lo_store.out_y_lo = shadow(to);
    return &lo_store;
  };
  if (lo_on) {
    const int crc = launch_to_bf16(y, r.graph->n, r.d, r.ld, shadow(0), st);
    if (crc) return crc;
  }
  const size_t nbytes = static_cast<size_t>(r.graph->n) * r.ld * 4;
  const gnpde_epilogue_t base = base_epilogue(r);
  // y, u2 (ua), u3 (ub) and u4 (the k1 slot) of the compact rk4, whose k1..k3 are never materialised; y and ua for euler and midpoint
  float* const bufs[4] = {y, ua, reinterpret_cast<float*>(s->ws + s->off_ub), reinterpret_cast<float*>(s->ws + s->off_k1)};
  if (s->method == GNPDE_METHOD_RK4 && s->tape == nullptr && g_tune[GNPDE_TUNE_RK4_CLASSIC] != 0) {
    // the classic form with k1..k3 stored (A/B against the compact one; a recorded solve is always compact)
    float *ub = bufs[2], *k1 = bufs[3];
    float* k2 = reinterpret_cast<float*>(s->ws + s->off_k2);
    float* k3 = reinterpret_cast<float*>(s->ws + s->off_k3);
    for (float dt : s->dts) {
      gnpde_epilogue_t e = base;
      e.dt = dt; e.y = y;
      e.stage = GNPDE_STAGE_RK1; e.out_k = k1; e.out_y = ua;
      int rc = before_step(step + 1, y);
      if (rc) return rc;
      rc = enqueue_rhs(r, y, e, rws, s->L, st, fk, nullptr, pair(0, 1), true);
      if (rc) return rc;
      e.stage = GNPDE_STAGE_RK2; e.k1 = k1; e.out_k = k2; e.out_y = ub;
      rc = enqueue_rhs(r, ua, e, rws, s->L, st, fk, nullptr, pair(1, 2), true);
      if (rc) return rc;
      e.stage = GNPDE_STAGE_RK3; e.k2 = k2; e.out_k = k3; e.out_y = ua;
      rc = enqueue_rhs(r, ub, e, rws, s->L, st, fk, nullptr, pair(2, 1), true);
      if (rc) return rc;
      e.stage = GNPDE_STAGE_RK4; e.k3 = k3; e.out_k = nullptr; e.out_y = y;
      rc = enqueue_rhs(r, ua, e, rws, s->L, st, fk, nullptr, pair(1, 0), true);
      if (rc) return rc;
      rc = evaluate(y);
      if (rc) return rc;
      rc = after_step(step, y);
      if (rc) return rc;
    }
    return 0;
  }
  // Every other solve runs the schedule of fixed_grid.h; what differs is where the stage inputs u[0..S] of a step lie.  Recycled buffers:
  // the step starts in the buffer the last one ended in and walks the ring from there -- midpoint and rk4 end in place on y, euler
  // alternates between y and ua; idx[] also names the bf16 shadows.  Recorded solve (s->tape): the same launches, every stage input
  // written to a slot of its own -- the record costs no extra pass over the state.  Slot 0 = y0, slot i = the input of evaluation i
  // (rk4: u1..u4 of step n at 4n..4n+3), the last slot = y(T), copied back into y.
  const int S = evals_per_step(s->method), B = stage_input_buffers(s->method);
  const size_t stride = align_up(nbytes, 256) / 4;
  auto slot = [&](size_t i) { return s->tape + i * stride; };
  RhsRecord rec_store{};
  auto rec = [&](size_t eval) -> const RhsRecord* {
    if (s->tape_rec == nullptr) return nullptr;
    rec_store = rhs_record_at(r, s->tape_rec, eval);
    return &rec_store;
  };
  float* u[5];
  int idx[5];
  int first = 0;     // ring position of the step's start
  float* result = y;
  if (s->tape != nullptr) {
    result = slot(0);
    GNPDE_HIP(hipMemcpyAsync(result, y, nbytes, hipMemcpyDeviceToDevice, st));
  }
  size_t at = 0;     // evaluations so far
  for (float dt : s->dts) {
    for (int i = 0; i <= S; ++i) {
      idx[i] = (first + i) % B;
      u[i] = s->tape != nullptr ? slot(at + i) : bufs[idx[i]];
    }
    int rc = before_step(step + 1, u[0]);
    if (rc) return rc;
    rc = enqueue_step(base, s->method, dt, u, [&](int j, const float* in, const gnpde_epilogue_t& e) {
      return enqueue_rhs(r, in, e, rws, s->L, st, fk, rec(at + j), pair(idx[j], idx[j + 1]), true);
    });
    if (rc) return rc;
    at += S;
    first = idx[S];
    result = u[S];
    rc = evaluate(result);
    if (rc) return rc;
    rc = after_step(step, result);
    if (rc) return rc;
  }
  if (result != y) GNPDE_HIP(hipMemcpyAsync(y, result, nbytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

void drop_graph(gnpde_solver* s) {
  drop_capture(&s->graph_obj, &s->exec);
  s->captured_y = nullptr;
}

}  // namespace

extern "C" int64_t gnpde_one_launch_evaluations(void) { return gnpde::g_one_launch_evals.load(std::memory_order_relaxed); }

extern "C" size_t gnpde_rhs_workspace_bytes(const gnpde_rhs_t* rhs) {
  if (check_rhs(rhs)) return 0;
  return rhs_layout(*rhs).total;
}

extern "C" int gnpde_rhs_eval(const gnpde_rhs_t* rhs, const float* u, float* out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  int rc = check_rhs(rhs);
  if (rc) return rc;
  GNPDE_CHECK_ARG(u && out && u != out, GNPDE_EINVAL, "rhs_eval: bad u/out");
  const RhsLayout L = rhs_layout(*rhs);
  GNPDE_CHECK_ARG(L.total == 0 || (workspace && workspace_bytes >= L.total), GNPDE_EWS, "rhs_eval: workspace %zu < %zu bytes",
                  workspace_bytes, L.total);
  gnpde_epilogue_t e = base_epilogue(*rhs);
  e.stage = GNPDE_STAGE_RHS;
  e.out_k = out;
  return enqueue_rhs(*rhs, u, e, static_cast<char*>(workspace), L, static_cast<hipStream_t>(stream));
}

extern "C" int gnpde_rhs_stage(const gnpde_rhs_t* rhs, const float* u, const gnpde_epilogue_t* epi, void* workspace,
                               size_t workspace_bytes, void* stream) {
  int rc = check_rhs(rhs);
  if (rc) return rc;
  GNPDE_CHECK_ARG(u && epi, GNPDE_EINVAL, "rhs_stage: null argument");
  const RhsLayout L = rhs_layout(*rhs);
  GNPDE_CHECK_ARG(L.total == 0 || (workspace && workspace_bytes >= L.total), GNPDE_EWS, "rhs_stage: workspace %zu < %zu bytes",
                  workspace_bytes, L.total);
  gnpde_epilogue_t e = *epi;
  e.alpha = rhs->alpha;
  e.beta = rhs->beta;
  e.x0 = rhs->x0;
  e.alpha_sigmoid = rhs->alpha_sigmoid;
  return enqueue_rhs(*rhs, u, e, static_cast<char*>(workspace), L, static_cast<hipStream_t>(stream));
}

extern "C" size_t gnpde_solver_workspace_bytes(const gnpde_rhs_t* rhs, int32_t method) {
  if (check_rhs(rhs)) return 0;
  if (method != GNPDE_METHOD_EULER && method != GNPDE_METHOD_RK4 && method != GNPDE_METHOD_MIDPOINT) return 0;
  return solver_layout(*rhs, method, nullptr);
}

extern "C" int gnpde_solver_create(gnpde_solver_t** out, const gnpde_rhs_t* rhs, int32_t method, const float* dts,
                                   int32_t n_steps, void* workspace, size_t workspace_bytes) {
  GNPDE_CHECK_ARG(out != nullptr, GNPDE_EINVAL, "solver_create: out is null");
  *out = nullptr;
  int rc = check_rhs(rhs);
  if (rc) return rc;
  GNPDE_CHECK_ARG(method == GNPDE_METHOD_EULER || method == GNPDE_METHOD_RK4 || method == GNPDE_METHOD_MIDPOINT, GNPDE_EINVAL,
                  "solver_create: bad method %d", method);
  GNPDE_CHECK_ARG(n_steps >= 0 && (dts || n_steps == 0), GNPDE_EINVAL, "solver_create: bad time grid");
  gnpde_solver* s = new gnpde_solver();
  s->rhs = *rhs;
  s->graph = *rhs->graph;
  s->rhs.graph = &s->graph;
  if (s->rhs.att.graph_t != nullptr) {   // (the descriptor's transposed graph is copied as well: the caller's structs may go away)
    s->graph_t = *s->rhs.att.graph_t;
    s->rhs.att.graph_t = &s->graph_t;
  }
  s->method = method;
  s->dts.assign(dts, dts + n_steps);
  s->L = rhs_layout(s->rhs);
  const size_t need = solver_layout(s->rhs, method, s);
  if (!(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 256 == 0)) {
    set_error("solver_create: workspace %zu bytes (need %zu, 256-byte aligned)", workspace_bytes, need);
    delete s;
    return GNPDE_EWS;
  }
  s->ws = static_cast<char*>(workspace);
  s->ws_bytes = workspace_bytes;
  s->n_evals = n_steps * evals_per_step(method);
  *out = s;
  return 0;
}

extern "C" int gnpde_solver_run(gnpde_solver_t* s, float* y, int32_t use_graph, void* stream) {
  GNPDE_CHECK_ARG(s && y, GNPDE_EINVAL, "solver_run: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!use_graph) return enqueue_solve(s, y, st);
  if (s->exec == nullptr || s->captured_y != y) {
    drop_graph(s);
    if (int rc = capture_into(&s->cap_stream, &s->graph_obj, &s->exec, [&](hipStream_t cs) { return enqueue_solve(s, y, cs); })) return rc;
    s->captured_y = y;
  }
  GNPDE_HIP(hipGraphLaunch(s->exec, st));
  return 0;
}

extern "C" size_t gnpde_solver_tape_bytes(const gnpde_rhs_t* rhs, int32_t method, int32_t n_steps) {
  if (check_rhs(rhs) || n_steps < 0) return 0;
  if (method != GNPDE_METHOD_EULER && method != GNPDE_METHOD_RK4 && method != GNPDE_METHOD_MIDPOINT) return 0;
  const size_t state = align_up(static_cast<size_t>(rhs->graph->n) * rhs->ld * 4, 256);
  const size_t per = evals_per_step(method);
  return (per * static_cast<size_t>(n_steps) + 1) * state + per * static_cast<size_t>(n_steps) * rhs_record_stride(*rhs) * 4;
}

extern "C" int gnpde_solver_set_tape(gnpde_solver_t* s, void* tape, size_t tape_bytes) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "solver_set_tape: solver is null");
  GNPDE_CHECK_ARG(tape == nullptr || s->lo == nullptr, GNPDE_EINVAL,
                  "solver_set_tape: a recorded solve keeps the fp32 gather operand (detach the bf16 one first: gnpde_solver_set_gather(s, 0, NULL, 0))");
  GNPDE_CHECK_ARG(tape == nullptr || s->out_step.empty(), GNPDE_EINVAL,
                  "solver_set_tape: a recorded solve has two output times (detach the outputs first: gnpde_solver_set_outputs(s, 0, ...))");
  drop_graph(s);
  s->tape = nullptr;
  s->tape_rec = nullptr;
  if (tape == nullptr) return 0;
  GNPDE_CHECK_ARG(!rhs_mix_features(s->rhs), GNPDE_ESHAPE,
                  "solver_set_tape: no reverse sweep differentiates the mix_features form of the GAT function; it is not recorded");
  const size_t need = gnpde_solver_tape_bytes(&s->rhs, s->method, static_cast<int32_t>(s->dts.size()));
  GNPDE_CHECK_ARG(reinterpret_cast<uintptr_t>(tape) % 256 == 0 && tape_bytes >= need, GNPDE_EWS,
                  "solver_set_tape: %zu bytes (need %zu, 256-byte aligned, zero-filled)", tape_bytes, need);
  s->tape = static_cast<float*>(tape);
  const size_t state = align_up(static_cast<size_t>(s->rhs.graph->n) * s->rhs.ld * 4, 256);
  s->tape_rec = rhs_record_stride(s->rhs) > 0 ? s->tape + (static_cast<size_t>(s->n_evals) + 1) * (state / 4) : nullptr;
  return 0;
}

extern "C" size_t gnpde_solver_gather_bytes(const gnpde_rhs_t* rhs, int32_t method) {
  if (check_rhs(rhs)) return 0;
  if (method != GNPDE_METHOD_EULER && method != GNPDE_METHOD_RK4 && method != GNPDE_METHOD_MIDPOINT) {
    set_error("solver_gather_bytes: bad method %d", method);
    return 0;
  }
  if (!rhs_gather_lo_supported(*rhs)) {
    set_error("solver_gather_bytes: the bf16 gather operand needs 16-byte lanes of a whole-graph state (d %% 4 == 0, or "
              "GNPDE_RHS_PADDED_ROWS; ld %% 4 == 0): d=%d ld=%d", rhs->d, rhs->ld);
    return 0;
  }
  return stage_input_buffers(method) * lo_stride(*rhs);
}

extern "C" int gnpde_solver_set_gather(gnpde_solver_t* s, int32_t dtype, void* mem, size_t bytes) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "solver_set_gather: solver is null");
  GNPDE_CHECK_ARG(dtype == GNPDE_GATHER_FP32 || dtype == GNPDE_GATHER_BF16, GNPDE_EINVAL, "solver_set_gather: bad dtype %d", dtype);
  if (dtype == GNPDE_GATHER_FP32) {
    drop_graph(s);
    s->lo = nullptr;
    return 0;
  }
  GNPDE_CHECK_ARG(s->tape == nullptr, GNPDE_EINVAL,
                  "solver_set_gather: a recorded solve keeps the fp32 gather operand (detach the tape first: gnpde_solver_set_tape(s, NULL, 0))");
  const size_t need = gnpde_solver_gather_bytes(&s->rhs, s->method);
  if (need == 0) return GNPDE_ESHAPE;
  GNPDE_CHECK_ARG(mem != nullptr && reinterpret_cast<uintptr_t>(mem) % 256 == 0 && bytes >= need, GNPDE_EWS,
                  "solver_set_gather: %zu bytes (need %zu, 256-byte aligned)", bytes, need);
  drop_graph(s);
  s->lo = static_cast<uint16_t*>(mem);
  return 0;
}

extern "C" int gnpde_solver_set_early_stop(gnpde_solver_t* s, const gnpde_decoder_t* dec, int32_t* state, int32_t* trace,
                                           int32_t trace_capacity) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "solver_set_early_stop: solver is null");
  GNPDE_CHECK_ARG(dec == nullptr || s->out_step.empty(), GNPDE_EINVAL,
                  "solver_set_early_stop: not together with outputs at several times (detach them first: gnpde_solver_set_outputs(s, 0, ...))");
  drop_graph(s);
  if (dec == nullptr) {
    s->early = false;
    return 0;
  }
  int rc = check_decoder(dec, s->rhs.d);
  if (rc) return rc;
  GNPDE_CHECK_ARG(state != nullptr, GNPDE_EINVAL, "solver_set_early_stop: state is null");
  GNPDE_CHECK_ARG(trace != nullptr || trace_capacity == 0, GNPDE_EINVAL, "solver_set_early_stop: trace capacity without a trace");
  s->dec = *dec;
  s->early_state = state;
  s->early_trace = trace;
  s->early_trace_capacity = trace_capacity;
  s->early = true;
  return 0;
}

extern "C" int gnpde_solver_set_outputs(gnpde_solver_t* s, int32_t n_out, const int32_t* step, const float* frac, float* out, int32_t ld_out,
                                        float* scratch) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "solver_set_outputs: solver is null");
  GNPDE_CHECK_ARG(n_out >= 0, GNPDE_EINVAL, "solver_set_outputs: n_out = %d", n_out);
  if (n_out == 0) {
    drop_graph(s);
    s->out_step.clear();
    s->out_frac.clear();
    s->out = s->out_scratch = nullptr;
    return 0;
  }
  GNPDE_CHECK_ARG(s->tape == nullptr, GNPDE_EINVAL, "solver_set_outputs: a recorded solve has two output times (detach the tape first)");
  GNPDE_CHECK_ARG(!s->early, GNPDE_EINVAL, "solver_set_outputs: not together with the early-stopping evaluator (detach it first)");
  const gnpde_rhs_t& r = s->rhs;
  GNPDE_CHECK_ARG(r.n_state_rows <= r.graph->n && r.proj_row_end == 0 && r.graph->row_begin == 0, GNPDE_EINVAL,
                  "solver_set_outputs: not on a partitioned descriptor (the row-partitioned engine has two output times)");
  GNPDE_CHECK_ARG(step && frac && out && ld_out >= r.d, GNPDE_EINVAL, "solver_set_outputs: null array or ld_out %d < d %d", ld_out, r.d);
  bool any_interior = false;
  for (int j = 0; j < n_out; ++j) {
    GNPDE_CHECK_ARG(step[j] >= 1 && step[j] <= static_cast<int>(s->dts.size()) && (j == 0 || step[j] >= step[j - 1]), GNPDE_EINVAL,
                    "solver_set_outputs: step[%d] = %d (1..%d, non-decreasing)", j, step[j], static_cast<int>(s->dts.size()));
    GNPDE_CHECK_ARG(frac[j] >= 0.0f && frac[j] <= 1.0f, GNPDE_EINVAL, "solver_set_outputs: frac[%d] = %g (0..1)", j, static_cast<double>(frac[j]));
    any_interior = any_interior || frac[j] != 1.0f;
  }
  GNPDE_CHECK_ARG(!any_interior || scratch != nullptr, GNPDE_EINVAL, "solver_set_outputs: an output inside a step needs the scratch state buffer");
  drop_graph(s);
  s->out_step.assign(step, step + n_out);
  s->out_frac.assign(frac, frac + n_out);
  s->out = out;
  s->ld_out = ld_out;
  s->out_scratch = scratch;
  return 0;
}

extern "C" int gnpde_solver_set_output_order(gnpde_solver_t* s, const int32_t* order) {
  GNPDE_CHECK_ARG(s != nullptr, GNPDE_EINVAL, "solver_set_output_order: solver is null");
  if (order != s->out_order) drop_graph(s);
  s->out_order = order;
  return 0;
}

extern "C" int gnpde_solver_num_rhs_evals(const gnpde_solver_t* s) { return s ? s->n_evals : 0; }

extern "C" int gnpde_solver_destroy(gnpde_solver_t* s) {
  if (!s) return 0;
  drop_graph(s);
  if (s->cap_stream) (void)hipStreamDestroy(s->cap_stream);
  if (s->fork.aux) (void)hipStreamDestroy(s->fork.aux);
  if (s->fork.e_fork) (void)hipEventDestroy(s->fork.e_fork);
  if (s->fork.e_join) (void)hipEventDestroy(s->fork.e_join);
  delete s;
  return 0;
}
