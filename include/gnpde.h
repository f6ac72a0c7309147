/*
 * gnpde.h -- C ABI of libgnpde_hip.so: the MI355X (gfx950) implementation of the GRAND / BLEND
 * ODE right-hand side f(t,x) = alpha * (A(x) x - x) + beta * x0 and of the fixed-step solver loop
 * around it.
 *
 * The reference (twitter-research/graph-neural-pde) has no FFI: its boundary for this path is the
 * Python protocol ODEFunc.forward(t, x) / ODEblock.forward(x) (src/base_classes.py:32-95).  The
 * entry points below are what a binding for that path binds; each cites the reference code it
 * replaces (paths relative to the reference root).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - every pointer marked "device" is HBM memory owned by the caller; nothing here allocates
 *     device memory, synchronises the device or touches the default stream (safe inside hipGraph
 *     capture), except the gnpde_solver_* objects which own their hipGraphExec;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every function returns 0 on success, a hipError_t (> 0) for runtime failures, or a negative
 *     GNPDE_E* code for bad arguments; gnpde_last_error() returns a thread-local message;
 *   - all floating point is IEEE fp32 (no fast-math), all device indices int32;
 *   - learnable scalars (alpha_train, beta_train, ...) are read from DEVICE pointers so that no
 *     host synchronisation is needed between optimiser steps and solves.
 */
#ifndef GNPDE_H
#define GNPDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNPDE_ABI_VERSION 26  /* 26: gnpde_solver_set_outputs, gnpde_solver_set_output_order, gnpde_dopri5_set_outputs, gnpde_snapshot_rows (native solves with several output times);  25: GNPDE_RHS_MIX_FEATURES, gnpde_rhs_t.out_w / out_ld appended, gnpde_linear_epilogue (no-grad solves of the GAT function's mix_features form);  24: gnpde_attention_rows_bwd_dq, gnpde_head_rowsum, gnpde_hub_bwd_workspace_floats, gnpde_head_rowsum_supported, gnpde_attention_rows_bwd_dq_supported (the adjoint stage's row kernels as entry points of their own);  23: gnpde_attention_plan, gnpde_attention_launch_t, GNPDE_ATT_ROUTE_* / _ROWS16_* / _GMAX_* / _HUBS_* / _PLAN_* (the row attention's launch decision);  22: gnpde_spmm_plan, gnpde_spmm_launch_t, GNPDE_SPMM_* (the aggregation's launch decision), gnpde_adjoint_rows_dot_slots;  21: gnpde_spmm_ticket_bytes, gnpde_spmm_rhs_tickets, gnpde_in_kernel_fold_launches, gnpde_agg_fold_launch (hub rows folded inside the row-pair aggregation launch);  20: gnpde_adjoint_set_dopri5_tape, gnpde_dopri5_tape_slots, GNPDE_METHOD_DOPRI5_TAPE (GRAND-nl / GAT dopri5 training: sweep over a recorded solve), gnpde_dopri5_set_tape takes transformer and GAT descriptors;  19: gnpde_poincare_step(_workspace_bytes) (hyperbolic positional encodings: row-normalised Riemannian SGD on the Poincare ball);  18: gnpde_linear_plan, gnpde_linear_split_plan, gnpde_linear_launch_t, GNPDE_LINEAR_* (the projection's launch decision);  17: gnpde_nmf_cd_sweep(_workspace_bytes) (NMF compression of positional encodings);  16: gnpde_one_launch_evaluations (gnpde_tune(21, .): row attention of an evaluation in one launch);  15: gnpde_random_walks, gnpde_negative_walks, gnpde_random_permutation(_workspace_bytes), gnpde_deepwalk_step(_workspace_bytes), GNPDE_DEEPWALK_* (DeepWalk positional encodings);  14: gnpde_gdc_push_workspace_bytes, gnpde_gdc_push_count, gnpde_gdc_push_fill, gnpde_gdc_push_residuals (approximate PPR by forward push), gnpde_rank_select_begin, gnpde_rank_select_hist, gnpde_rank_select_pick, gnpde_rank_select_values (threshold by avg_degree);  13: gnpde_philox_words, gnpde_random_nodes, gnpde_node_importance, gnpde_sample_nodes(_workspace_bytes), gnpde_edge_union(_workspace_bytes), gnpde_select_edges(_workspace_bytes), gnpde_full_adjacency, GNPDE_SAMPLING_* (edge-sampling rewiring of the fully-adjacent layer);  12: gnpde_knn_metric, gnpde_radius_workspace_bytes, gnpde_radius_quantile, gnpde_radius_count, gnpde_radius_fill, GNPDE_METRIC_* (positional-distance rewiring: Poincare k-NN and radius graphs);  11: gnpde_gdc_workspace_bytes, gnpde_gdc_block, gnpde_gdc_topk, gnpde_gdc_emit, gnpde_gdc_threshold_count, gnpde_gdc_threshold_fill, gnpde_gdc_segment_sums, gnpde_gdc_dense (graph diffusion rewiring);  10: gnpde_split_kernel_grads, gnpde_split_kernel_grad_floats (BLEND split kernel on the native VJP stage), exp-kernel stage to attention_dim 256;  9: gnpde_knn, gnpde_knn_workspace_bytes (k-nearest-neighbour rewiring);  8: optional bf16 gather operand (gnpde_to_bf16, gnpde_spmm_lo, gnpde_spmm_rhs_lo, gnpde_solver_gather_bytes, gnpde_solver_set_gather);  7: gnpde_dopri5_create_sharded (device controller over the row partition), gnpde_dopri5_set_pair, gnpde_sharded_solver_set_general, gnpde_graph_build_device;  6: gnpde_adjoint_set_tape takes csr_from_t, gnpde_adjoint_tape_swapped, gnpde_linear_split;  5: gnpde_solver_set_tape / gnpde_adjoint_set_tape (recorded fixed-grid solve);  4: gnpde_dopri5_set_tape / _tape_backward, gnpde_adjoint_adaptive_*, GNPDE_METHOD_MIDPOINT;  2: gnpde_graph_t.xcd_deal appended, gnpde_xcd_row_map; 3: gnpde_attention_t.graph_t / t_from_csr appended,
                                 gnpde_adjoint_*, gnpde_stream_read; gnpde_graph_t.n_bin_le64 and gnpde_attention_t.n_key_rows in what was
                                 padding (struct sizes unchanged) */

#define GNPDE_EINVAL   (-1)  /* bad argument                                  */
#define GNPDE_ESHAPE   (-2)  /* shape not supported by any kernel variant     */
#define GNPDE_EWS      (-3)  /* workspace too small                           */
#define GNPDE_ESTATE   (-4)  /* object used in the wrong state                */

/* Rows with more than GNPDE_LONG_ROW non-zeros are split into chunks of that many edges so that a
 * hub node (ogbn-arxiv: degree 13k) is spread over many wavefronts. */
#define GNPDE_LONG_ROW 512

int         gnpde_abi_version(void);
const char* gnpde_last_error(void);
/* Select a kernel variant for A/B measurements; 0 = default.  Keys 0, 8 and 13 are retired: any value but 0 is GNPDE_EINVAL. */
int         gnpde_tune(int32_t key, int32_t value);
/* Evaluations enqueued so far (by any solver or gnpde_rhs_eval / gnpde_rhs_stage of this process; a captured solve counts once per
 * enqueued evaluation, not per replay) whose row attention took the one-launch form with the hub rows normalised by the aggregation's
 * chunk items -- whole-graph GRAND-nl, scaled-dot row softmax, 1 / 2 / 4 heads, fp32 gather, d = 68..128 on a graph of mostly short
 * rows (the row-pair aggregation kernel); gnpde_tune(21, 1) keeps the two launches.  The launch decision, for tests and A/B scripts. */
int64_t     gnpde_one_launch_evaluations(void);

/* ------------------------------------------------------------------------------------------------
 * Graph preparation (host, C++).  Replaces the implicit COO handling of torch_sparse.spmm /
 * torch_scatter (reference call sites: src/function_transformer_attention.py:35,190-191,213;
 * src/function_laplacian_diffusion.py:31-35): COO int64 [2,E] in ANY order, duplicates allowed
 * -> CSR with a stable permutation, a CSC view, and the long-row chunk list.
 * ---------------------------------------------------------------------------------------------- */

/* Number of long rows / long-row chunks / long columns the edge list produces (sizes of the arrays
 * below).  `col` may be NULL (then *n_long_cols = 0). */
int gnpde_graph_count_long(const int64_t* row, const int64_t* col, int64_t n_edges, int32_t n_nodes,
                           int32_t* n_long_rows, int32_t* n_long_chunks, int32_t* n_long_cols);

/* All arrays are HOST memory, caller allocated:
 *   rowptr[n+1], colidx[E], perm[E] (CSR position -> index into the caller's edge list; stable, so
 *   duplicates keep their relative order), rowidx[E] (row of each CSR position),
 *   cscptr[n+1], cscpos[E] (for every column, the CSR positions of its entries, ascending)  -- may
 *   both be NULL;  long_rows[n_long_rows], long_chunk_ptr[n_long_rows+1],
 *   long_chunk_row/begin/end/first[n_long_chunks] (first = index of the first chunk of the same row),
 *   long_cols[n_long_cols] (NULL without the CSC view);
 *   bin_rows[4n]: one int32x4 record {row, first CSR position, length, 0} per listed row, grouped by
 *   degree class -- first the rows with 1..16 entries, then those with 17..GNPDE_LONG_ROW (empty and
 *   long rows are not listed); bin_counts[2] = sizes of the two classes.  The first class is in ascending row
 *   order, the second LONGEST FIRST (ties in row order): a wavefront takes one such row, and the long ones should start the
 *   row-attention launch, not end it.  (One 16-byte load replaces the rowptr indirection in the row-attention kernels.)
 * Returns GNPDE_EINVAL if an index is outside [0, n_nodes). */
int gnpde_graph_build(const int64_t* row, const int64_t* col, int64_t n_edges, int32_t n_nodes,
                      int32_t* rowptr, int32_t* colidx, int32_t* perm, int32_t* rowidx,
                      int32_t* cscptr, int32_t* cscpos,
                      int32_t* long_rows, int32_t* long_chunk_ptr, int32_t* long_chunk_row,
                      int32_t* long_chunk_begin, int32_t* long_chunk_end, int32_t* long_cols,
                      int32_t* bin_rows, int32_t* bin_counts, int32_t* long_chunk_first);

/* The same arrays built ON THE DEVICE from an edge list that already lives there (blocks that hand over a new edge set every training
 * forward: reference src/block_transformer_hard_attention.py:55-61, src/block_transformer_rewiring.py), element for element what
 * gnpde_graph_build gives.  Two calls around ONE host read:
 *   gnpde_graph_build_device       row / col: device int64 [E]; fills rowptr[n+1], colidx / perm / rowidx / cscpos [E], cscptr[n+1],
 *                                  bin_rows[4n] and counts[16] (device): [0] != 0: an index outside [0, n); [1] rows with 1..16 entries,
 *                                  [2] with 17..GNPDE_LONG_ROW, [3] of those with <= 64, [4] long rows, [5] long columns, [6] 512-entry
 *                                  chunks of the long rows, [7] / [8] longest row / column.
 *   gnpde_graph_build_device_long  (after the caller read counts and allocated the lists) long_rows[n_long_rows],
 *                                  long_chunk_ptr[n_long_rows+1], long_chunk_row / begin / end / first[n_long_chunks],
 *                                  long_cols[n_long_cols]; scratch_count: one device word.
 * Workspace: gnpde_graph_build_device_workspace_bytes(E, n) device bytes, 256-byte aligned, the same block for both calls. */
size_t gnpde_graph_build_device_workspace_bytes(int64_t n_edges, int32_t n_nodes);
int gnpde_graph_build_device(const int64_t* row, const int64_t* col, int64_t n_edges, int32_t n_nodes, int32_t* rowptr, int32_t* colidx,
                             int32_t* perm, int32_t* rowidx, int32_t* cscptr, int32_t* cscpos, int32_t* bin_rows, int32_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream);
int gnpde_graph_build_device_long(const int32_t* rowptr, const int32_t* cscptr, int32_t n_nodes, int32_t n_long_rows, int32_t n_long_chunks,
                                  int32_t n_long_cols, int32_t* long_rows, int32_t* long_chunk_ptr, int32_t* long_chunk_row,
                                  int32_t* long_chunk_begin, int32_t* long_chunk_end, int32_t* long_cols, int32_t* long_chunk_first,
                                  int32_t* scratch_count, void* workspace, size_t workspace_bytes, void* stream);

/* Balanced k-way row partition for the multi-GPU path (no METIS offline; no reference equivalent): size-capped
 * label-propagation clusters packed into parts, then node-level refinement under the balance constraint.  The parts are
 * balanced (3 %) on  entries + row_weight  per row -- 1 follows the aggregation time, larger values even out the node counts --
 * and the clusters are capped at a part's work / cluster_div.  part[n] receives values in [0, n_parts).  Host only,
 * deterministic for given arguments.  gnpde_partition_rows = row_weight 1, cluster_div 4.  The outcome of the heuristic moves
 * by tens of per cent with these two; the Python layer scores a few combinations by the busiest xGMI link and the busiest
 * rank they produce and keeps the cheapest (distributed.PartitionPlan). */
int gnpde_partition_rows(const int32_t* rowptr, const int32_t* colidx, int32_t n_nodes,
                         int32_t n_parts, int32_t refine_iters, uint64_t seed, int32_t* part);
int gnpde_partition_rows_ex(const int32_t* rowptr, const int32_t* colidx, int32_t n_nodes, int32_t n_parts,
                            int32_t refine_iters, uint64_t seed, int32_t row_weight, int32_t cluster_div, int32_t* part);

/* Communication refinement of a row partition (no reference equivalent).  A partitioned evaluation waits for the rows each rank
 * RECEIVES, not for cut edges: M[r][q] = distinct nodes of part q referenced by rows of part r = rows on the link q -> r per
 * evaluation.  Hill climbing on single-node moves with exact bookkeeping: phase 1 lowers the total of M without raising the
 * busiest link, phase 2 lowers the excess of the links above 90 % of the busiest; the parts stay inside the balance window of
 * gnpde_partition_rows_ex (entries + row_weight per row).  part[n] in / out.  stats (nullable, int64[5]): busiest link before /
 * after, total received rows before / after, moves.  Host only, deterministic. */
int gnpde_partition_refine_links(const int32_t* rowptr, const int32_t* colidx, int32_t n_nodes, int32_t n_parts,
                                 int32_t row_weight, int32_t max_passes, int32_t* part, int64_t* stats);

/* Device view of a prepared graph (all pointers device memory). */
typedef struct gnpde_graph {
  int32_t n;                         /* nodes (square operator)                              */
  int32_t e;                         /* stored entries                                       */
  const int32_t* rowptr;             /* [n+1]                                                */
  const int32_t* colidx;             /* [e]  CSR order                                       */
  const int32_t* rowidx;             /* [e]  row of each CSR position                        */
  const int32_t* perm;               /* [e]  CSR position -> caller edge id                  */
  const int32_t* cscptr;             /* [n+1] or NULL                                        */
  const int32_t* cscpos;             /* [e]   or NULL                                        */
  int32_t n_long_rows;
  int32_t n_long_chunks;
  const int32_t* long_rows;          /* [n_long_rows]                                        */
  const int32_t* long_chunk_ptr;     /* [n_long_rows+1]                                      */
  const int32_t* long_chunk_row;     /* [n_long_chunks]                                      */
  const int32_t* long_chunk_begin;   /* [n_long_chunks]                                      */
  const int32_t* long_chunk_end;     /* [n_long_chunks]                                      */
  int32_t n_long_cols;               /* columns with more than GNPDE_LONG_ROW entries        */
  int32_t n_bin16;                   /* rows with 1..16 entries                              */
  int32_t n_bin64;                   /* rows with 17..GNPDE_LONG_ROW entries                 */
  int32_t max_row_len;               /* longest row                                          */
  int32_t max_col_len;               /* longest column (0 without the CSC view)              */
  int32_t row_begin;                 /* aggregation covers rows [row_begin, n) (0 normally; the boundary
                                        pass of a row-partitioned graph starts after the interior rows) */
  const int32_t* long_cols;          /* [n_long_cols] or NULL                                */
  const int32_t* bin_rows;           /* [(n_bin16 + n_bin64) * 4] records {row, begin, len, 0} */
  const int32_t* long_chunk_first;   /* [n_long_chunks] index of the first chunk of the same row */
  int32_t xcd_deal;                  /* how the aggregation launches deal the rows to the 8 XCDs (gnpde_xcd_row_map):
                                        GNPDE_XCD_CONTIGUOUS or GNPDE_XCD_HASHED; chosen per graph by whoever builds it */
  int32_t n_bin_le64;                /* (ABI 3) how many records of the second degree class (17..GNPDE_LONG_ROW entries, longest
                                        first) have at most 64 entries: they TRAIL that class, and the backward kernels give them a
                                        one-pass launch of their own (one entry per lane); 0: the whole class in one launch */
} gnpde_graph_t;

/* gnpde_graph_t.xcd_deal.  CONTIGUOUS: XCD x takes the x-th eighth of the rows -- neighbouring rows share an XCD's L2, and the
 * deal is balanced as long as the row length does not depend on the row id.  HASHED: blocks of 16 .. 128 consecutive rows, the
 * eight blocks of a group taken by the eight XCDs in an order rotated by a hash of the group -- balanced whatever the ids mean
 * (R-MAT: the expected degree falls 3x with every set id bit, contiguous eighths leave the launch 1.46x out of balance; ids in
 * order of time, crawl or degree do the same to real graphs).  The Python layer measures the contiguous deal's imbalance when it
 * builds a graph (work model: entries + 3 per row) and switches to HASHED above 3 %. */
#define GNPDE_XCD_CONTIGUOUS 0
#define GNPDE_XCD_HASHED     1

/* ------------------------------------------------------------------------------------------------
 * Epilogue of one right-hand-side evaluation, optionally fused with the solver's stage algebra.
 *   k      = alpha' * (A u - u_i) [+ beta * x0_i]      alpha' = sigmoid(*alpha) or *alpha
 *            (src/function_laplacian_diffusion.py:43-51 == function_transformer_attention.py:46-53
 *             == function_GAT_attention.py:56-64)
 * and then, per `stage` (torchdiffeq 0.2.1 fixed-grid solvers, called from
 * src/block_constant.py:57-62; rk4 == 3/8-rule rk4_alt_step_func, cf. src/early_stop_solver.py:150-155):
 *   GNPDE_STAGE_RHS    out_k = k
 *   GNPDE_STAGE_EULER  out_y = y + dt * k                       (u == y here, so out_y must differ)
 *   GNPDE_STAGE_RK1    out_k = k1 ; out_y = y + dt*k1*(1/3)
 *   GNPDE_STAGE_RK2    out_k = k2 ; out_y = y + dt*(k2 - k1*(1/3))
 *   GNPDE_STAGE_RK3    out_k = k3 ; out_y = y + dt*(k1 - k2 + k3)
 *   GNPDE_STAGE_RK4               ; out_y = y + (k1 + 3*(k2+k3) + k4)*dt*0.125   (in place on y)
 *   Compact rk4 (same step, stage states expressed through the previous stage INPUTS so that k1..k3 are
 *   never stored or re-read: 16 instead of 24 state-sized streams per step; u2 = y + dt k1/3 etc.):
 *   GNPDE_STAGE_RK1C   out_y = u + dt*k1*(1/3)                          (u == y)
 *   GNPDE_STAGE_RK2C   out_y = (2*y - u) + dt*k2                        (u == u2;  == y + dt*(k2 - k1/3))
 *   GNPDE_STAGE_RK3C   out_y = (2*a - u) + dt*k3      a = u2  (field k1)  (u == u3;  == y + dt*(k1 - k2 + k3))
 *   GNPDE_STAGE_RK4C   out_y = ((6*a + 3*u - y) + dt*k4)*0.125   a = u3  (u == u4; in place on y)
 *   General explicit Runge-Kutta stage (adaptive solvers: dopri5 of torchdiffeq, reference default method):
 *   GNPDE_STAGE_LINCOMB  out_k = k (if non-NULL) ;
 *                        out_y = y + sum_{j < n_prev} coef[j] * prev[j] + coef[n_prev] * k   (if non-NULL)
 *                        with coef[j] = fl32(beta_j) * fl32(dt) prepared by the caller (torchdiffeq's
 *                        k.matmul(beta * dt) rounding), or coef[j] = fl32(beta_j) and coef_scale -> fl32(dt) on the device.
 * `u` is the stage input the operator is applied to, `y` the state at the start of the step.
 * ---------------------------------------------------------------------------------------------- */
enum {
  GNPDE_STAGE_RHS = 0, GNPDE_STAGE_EULER = 1,
  GNPDE_STAGE_RK1 = 2, GNPDE_STAGE_RK2 = 3, GNPDE_STAGE_RK3 = 4, GNPDE_STAGE_RK4 = 5,
  GNPDE_STAGE_RK1C = 6, GNPDE_STAGE_RK2C = 7, GNPDE_STAGE_RK3C = 8, GNPDE_STAGE_RK4C = 9,
  GNPDE_STAGE_LINCOMB = 10
};
#define GNPDE_MAX_PREV 7

typedef struct gnpde_epilogue {
  const float* alpha;      /* device scalar (alpha_train)                                   */
  const float* beta;       /* device scalar (beta_train); used iff x0 != NULL               */
  const float* x0;         /* [n, ld] device or NULL (opt['add_source'] false)              */
  int32_t alpha_sigmoid;   /* 1: alpha' = sigmoid(alpha)  (opt['no_alpha_sigmoid'] false)   */
  int32_t stage;           /* GNPDE_STAGE_*                                                 */
  float   dt;              /* step size for the fused stage algebra                         */
  const float* y;          /* [n, ld] state at step start (stages != RHS)                   */
  const float* k1;         /* [n, ld] (RK2..RK4)                                            */
  const float* k2;         /* [n, ld] (RK3, RK4)                                            */
  const float* k3;         /* [n, ld] (RK4)                                                 */
  float* out_k;            /* [n, ld] (RHS, RK1..RK3)                                       */
  float* out_y;            /* [n, ld] (all but RHS)                                         */
  int32_t n_prev;          /* LINCOMB: number of earlier stage derivatives                  */
  int32_t pad_;
  const float* prev[GNPDE_MAX_PREV];   /* LINCOMB: [n, ld] each                             */
  float coef[GNPDE_MAX_PREV + 1];      /* LINCOMB: weights of prev[0..n_prev-1], then of k  */
  const float* coef_scale; /* LINCOMB: NULL, or a DEVICE scalar every coef[] is multiplied by when the kernel runs
                              (fl32 product): coef[] = fl32(beta_j), *coef_scale = fl32(dt) kept on the device by the
                              adaptive controller (gnpde_dopri5_*), so that a captured step serves every step size */
} gnpde_epilogue_t;

/* Host-side query of the work distribution of the aggregation launches (no reference equivalent; used by the host tests and
 * by tools/xcd_balance.py).  Workgroup b of a launch runs on XCD b % 8; every XCD walks its own list of rows.  deal =
 * GNPDE_XCD_HASHED: the rows [row_begin, row_end) are dealt in blocks of 2^*row_shift consecutive rows, eight consecutive blocks
 * form a group and XCD x takes block 8 j + ((x + hash(j)) mod 8) of group j; GNPDE_XCD_CONTIGUOUS: *row_shift = -1, XCD x takes
 * the x-th eighth (gnpde_tune(10, 1 / 2) overrides the argument with CONTIGUOUS / HASHED, as it overrides gnpde_graph_t.xcd_deal
 * in the launches).  *rows_per_xcd: length of every XCD's list; map (NULL, or [8 * *rows_per_xcd]): map[x * *rows_per_xcd + r]
 * = the r-th row of XCD x, or -1 past the end.  Every row appears exactly once; the two rows of an even-aligned pair (r, r + 1)
 * are consecutive. */
int gnpde_xcd_row_map(int32_t row_begin, int32_t row_end, int32_t deal, int32_t* row_shift, int32_t* rows_per_xcd, int32_t* map);

/* Bytes of scratch gnpde_spmm_rhs needs for the long-row partial sums (0 if no long rows). */
size_t gnpde_spmm_workspace_bytes(const gnpde_graph_t* g, int32_t d);

/* Hub-row tickets of an aggregation launch that folds its long rows itself: one 32-bit arrival counter per long row, in long_rows
 * order (0 bytes without long rows).  The caller zeroes them once; a launch that uses them leaves them zero again.  Where the
 * row-pair kernel runs (16-byte lanes, d = 68..128, a graph of mostly short rows) with an epilogue over the whole graph from the fp32
 * table, the chunk items of a hub row publish their partial sums, count themselves on the row's ticket, and the item that arrives last
 * folds the row in chunk order -- the float sequence of the fold launch, so the same bits -- and that launch is not enqueued;
 * gnpde_agg_fold_launch(1) keeps it (0, the default: fold in the kernel; a process-wide switch for A/B runs and bit references, as gnpde_tune).  Every other route ignores the tickets.  gnpde_in_kernel_fold_launches: aggregation launches enqueued
 * so far in this process that took the in-kernel form (a captured solve counts once per enqueued launch, not per replay). */
size_t  gnpde_spmm_ticket_bytes(const gnpde_graph_t* g);
int64_t gnpde_in_kernel_fold_launches(void);
int     gnpde_agg_fold_launch(int32_t keep);
/* gnpde_spmm_rhs with tickets (NULL: exactly gnpde_spmm_rhs); GNPDE_EWS when ticket_bytes < gnpde_spmm_ticket_bytes(g). */
int gnpde_spmm_rhs_tickets(const gnpde_graph_t* g, const float* w_csr, const float* u, int32_t d, int32_t ld,
                           const gnpde_epilogue_t* epi, void* workspace, size_t workspace_bytes, void* tickets, size_t ticket_bytes,
                           void* stream);

/* K7+K8 of SURVEY.md: ax[i] = sum_{e in row i} w[e] * u[col_e]  (torch_sparse.spmm, src/
 * function_laplacian_diffusion.py:31-35, function_transformer_attention.py:35) followed by the
 * epilogue above.  w is in CSR order.  u, x0, y, k*, out_* are [n, ld] row-major with ld >= d.
 * Deterministic (no atomics). */
int gnpde_spmm_rhs(const gnpde_graph_t* g, const float* w_csr, const float* u, int32_t d, int32_t ld,
                   const gnpde_epilogue_t* epi, void* workspace, size_t workspace_bytes, void* stream);

/* Plain aggregation out[i] = sum_e w[e] * u[col_e] without the diffusion epilogue (GAT
 * mix_features path, src/function_GAT_attention.py:33-36). */
int gnpde_spmm(const gnpde_graph_t* g, const float* w_csr, const float* u, int32_t d, int32_t ld,
               float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Optional bf16 GATHER operand (mixed precision, opt-in).  The aggregation is bound by the bytes of the neighbour rows it gathers;
 * these entry points gather them from a bf16 "shadow" of the stage input -- [n, ld] bf16 bit patterns (round to nearest even) with
 * the state's ld, 8-byte aligned rows -- and keep everything else fp32: the accumulation, the row's own -u_i term (read from `u`),
 * the source term, the stage algebra, the outputs.  One evaluation differs from the fp32 one by at most
 * alpha' * 2^-8 * sum_e |w_e| |u[col_e]| per element.  Only 16-byte lanes: ld % 4 == 0 and 16-byte aligned fp32 operands, anything else
 * returns GNPDE_ESHAPE.  A width d % 4 != 0 is taken with ld % 4 == 0 under the contract of GNPDE_RHS_PADDED_ROWS: the columns [d, ld) of
 * EVERY operand, shadows and outputs included, are padding of whole [n, ld] allocations that may be read and overwritten.
 *   gnpde_to_bf16      dst[i, j] = bf16(src[i, j]) for j < d; row stride ld on both sides, padding columns are left alone
 *   gnpde_spmm_lo      out[i] = sum_e w[e] * u_lo[col_e]                       (plain aggregation from a given shadow)
 *   gnpde_spmm_rhs_lo  gnpde_spmm_rhs with the neighbour rows gathered from u_lo; out_y_lo (NULL, or a shadow other than u_lo)
 *                      receives the bf16 rounding of epi->out_y, written by the same kernel from the registers that hold out_y */
int gnpde_to_bf16(const float* src, int64_t n, int32_t d, int32_t ld, void* dst, void* stream);
int gnpde_spmm_lo(const gnpde_graph_t* g, const float* w_csr, const void* u_lo, int32_t d, int32_t ld,
                  float* out, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_spmm_rhs_lo(const gnpde_graph_t* g, const float* w_csr, const float* u, const void* u_lo, int32_t d, int32_t ld,
                      const gnpde_epilogue_t* epi, void* out_y_lo, void* workspace, size_t workspace_bytes, void* stream);

/* Sampled dense-dense product on the graph pattern: out_csr[p] = s * a[row_p] . b[col_p], with
 * s = 1 (scale NULL), *scale, or sigmoid(*scale).  This is the gradient of gnpde_spmm_rhs w.r.t. the
 * per-edge weights (d w_e = alpha' g_row . u_col) that autograd needs when the reference's blocks hand
 * attention_weights with gradients (training, src/block_transformer_attention.py:38-39). */
int gnpde_sddmm(const gnpde_graph_t* g, const float* a, int32_t lda, const float* b, int32_t ldb, int32_t d,
                const float* scale, int32_t scale_sigmoid, float* out_csr, void* stream);

/* Backward of the row softmax + head mean of gnpde_edge_attention (scaled-dot, attention_norm_idx 0):
 *   ds[p,h] = s (a[p,h] / H) (dw[p] - sum_{p' in row} a[p',h] dw[p'])   [* edge_w[p] if given]
 * with s = 1 (scale NULL), *scale, or sigmoid(*scale) (device scalar: the alpha of the epilogue, so that dw can be
 * the UNSCALED g_row . x_col, which also yields d alpha).  att_edge is the [E,h] attention in the caller's edge
 * order, dw_csr / ds_csr are in CSR order.  Rows longer than GNPDE_LONG_ROW are taken by whole blocks. */
int gnpde_softmax_rows_bwd(const gnpde_graph_t* g, const float* att_edge, int32_t heads, const float* dw_csr,
                           const float* edge_w_csr, const float* scale, int32_t scale_sigmoid, float* ds_csr,
                           void* stream);

/* Head-wise weighted segment sum over the graph pattern (d q / d k of the attention scores):
 *   out[i, c] = scale * sum_{p in row i} ds[p, head(c)] * feat[col_p, c]           (by_column = 0)
 *   out[j, c] = scale * sum_{p in column j} ds[p, head(c)] * feat[row_p, c]        (by_column = 1, CSC view)
 * c < A = heads*dk, head(c) = c / dk; heads >= 1, dk >= 1, A <= 256, ldf >= A, ldo >= A, feat and out 4-byte aligned, any
 * leading dimension (feat may be the k half of a q||k row with A odd).  Every row of out is written (zeros for an empty
 * segment); fixed summation order, no atomics, no allocation.  dk % 4 == 0 with A/4 a power of two, 16-byte-aligned
 * operands and ld % 4 == 0 take the float4 kernel, every other shape a generic one (float2 or scalar lanes). */
int gnpde_head_spmm(const gnpde_graph_t* g, int32_t by_column, const float* ds_csr, int32_t heads, int32_t dk,
                    const float* feat, int32_t ldf, float scale, float* out, int32_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense feature mixing on the fp32 matrix cores (v_mfma_f32_16x16x4_f32):
 *   out[n, m] = x[n, d] * W[m, d]^T + b[m]          (b may be NULL)
 * Replaces nn.Linear Q and K of SpGraphTransAttentionLayer (src/function_transformer_attention.py:
 * 174-175; pass W = [Q.weight; K.weight] to get q||k in one pass, V is skipped because its result
 * is unused when mix_features is false, :34-35) and torch.mm(x, W) of the GAT layer
 * (src/function_GAT_attention.py:106; pass W^T).
 * ---------------------------------------------------------------------------------------------- */
int gnpde_linear(const float* x, int32_t n, int32_t d, int32_t ldx, const float* W, int32_t m,
                 int32_t ldw, const float* b, float* out, int32_t ldo, void* stream);

/* Out-projection with the diffusion epilogue and the stage algebra behind it (the GAT function's mix_features form,
 * src/function_GAT_attention.py:32-38; GNPDE_RHS_MIX_FEATURES):
 *   ax[i, c] = sum_k z[i, k] * Wout_t[c, k]        z [n, A] (ldz >= A), Wout_t [d, A] row-major (ldw >= A)
 *   k        = alpha' * (ax - u_i) + beta * x0_i   and then epi->stage, every GNPDE_STAGE_* (see gnpde_epilogue_t above)
 * u and every operand of the epilogue are [n, ldu] with ldu >= d.  Same matrix-core product as gnpde_linear (one wavefront owns 16
 * rows and all d columns, fixed K order: bit-identical from run to run); the accumulator tile is brought to row-contiguous lanes
 * through LDS before the epilogue streams its operands.  Shapes: A % 4 == 0, A <= 256, d <= 256, n >= 0; GNPDE_ESHAPE otherwise,
 * before any launch.  d % 4 == 0 with ldu % 4 == 0 and 16-byte aligned state operands takes 16-byte lanes, anything else scalar
 * lanes; columns [d, ldu) of the outputs are never written.  (A descriptor with GNPDE_RHS_PADDED_ROWS also takes 16-byte lanes for
 * d % 4 != 0, over its padding columns.)  An output may be u itself (the stage runs element by element) but not z. */
int gnpde_linear_epilogue(const float* z, int32_t n, int32_t A, int32_t ldz, const float* Wout_t, int32_t d, int32_t ldw,
                          const float* u, int32_t ldu, const gnpde_epilogue_t* epi, void* stream);

/* out = relu(x) W^T + b: the decoder of the reference's GNN.forward (F.relu -> [dropout, identity at test time] -> m2,
 * src/GNN.py:61-71) in one pass; same kernels as gnpde_linear with the activation applied to the A operand. */
int gnpde_relu_linear(const float* x, int32_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw,
                      const float* b, float* out, int32_t ldo, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge attention: per-edge scores -> per-node normalisation -> head-mean weights.
 * Replaces SpGraphTransAttentionLayer.forward (src/function_transformer_attention.py:190-213),
 * SpGraphAttentionLayer.forward (src/function_GAT_attention.py:111-114),
 * torch_geometric.utils.softmax and utils.squareplus (src/utils.py:179-208).
 * ---------------------------------------------------------------------------------------------- */
enum {
  GNPDE_ATT_SCALED_DOT = 0,  /* sum_c q k / sqrt(d_k)                     (:196)               */
  GNPDE_ATT_COSINE     = 1,  /* cosine similarity, eps 1e-5               (:198-199)           */
  GNPDE_ATT_PEARSON    = 2,  /* mean-centred cosine                       (:201-206)           */
  GNPDE_ATT_EXP_KERNEL = 3,  /* var^2 exp(-|q-k|^2 / (2 l^2))             (:194)               */
  GNPDE_ATT_GAT        = 4   /* LeakyReLU(a_src.h_i + a_dst.h_j)          (GAT :111-113)       */
};

typedef struct gnpde_attention {
  int32_t type;              /* GNPDE_ATT_*                                                    */
  int32_t heads;             /* h                                                              */
  int32_t att_dim;           /* A = h * d_k                                                    */
  int32_t norm_idx;          /* opt['attention_norm_idx']: 0 normalise over row, 1 over column */
  int32_t square_plus;       /* opt['square_plus']                                             */
  float   leaky_slope;       /* GAT only                                                       */
  const float* q;            /* [n, ldqk] device: row-side projection (GAT: h = x W)           */
  const float* k;            /* [n, ldqk] device: column-side projection (GAT: same as q)      */
  int32_t ldqk;
  int32_t n_key_rows;        /* rows of q / k the COLUMNS may address when that is more than the graph's n (a row-partitioned
                              * graph's halo rows lie behind its row range); 0: n.  ABI 3, in what was padding.  The GAT node
                              * terms (:111-114) are formed for all of them                    */
  const float* gat_a;        /* [2*d_k] device (GAT only)                                      */
  const float* output_var;   /* device scalar (exp_kernel)                                     */
  const float* lengthscale;  /* device scalar (exp_kernel)                                     */
  const float* edge_w_csr;   /* [e] CSR order or NULL: opt['reweight_attention'] (:208-209)    */
  /* optional (norm_idx == 1, scaled-dot scores): the transposed graph over the SAME edge list and, for every position of it, the
   * CSR position of that entry in the graph the call is made on.  With them the normalisation over the COLUMNS runs as the fused
   * row kernel over the rows of graph_t (scores, statistics and weights in one pass, weights scattered to their CSR positions)
   * instead of three passes with an [E,h] score round trip; NULL: the three passes. */
  const struct gnpde_graph* graph_t;
  const int32_t* t_from_csr;
} gnpde_attention_t;

/* Scratch: scores [e,h] + segment statistics [n,2h] + global max + GAT node terms [n,2h]. */
size_t gnpde_attention_workspace_bytes(const gnpde_graph_t* g, const gnpde_attention_t* a);

/* Outputs (all optional except at least one):
 *   w_mean_csr [e]    mean over heads of the normalised attention, CSR order (feeds gnpde_spmm_rhs)
 *   att_edge   [E,h]  attention in the CALLER's edge order (what the reference returns, :214)
 *   prods_edge [E,h]  un-normalised scores in the caller's edge order (:214)                  */
int gnpde_edge_attention(const gnpde_graph_t* g, const gnpde_attention_t* a,
                         float* w_mean_csr, float* att_edge, float* prods_edge,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The general attention path one pass at a time, for callers that must exchange between the passes (the row-partitioned solver,
 * SURVEY 8e):  pass 1 scores [e,h] into the workspace (+ the global maximum for squareplus, an order-preserving uint32 word),
 * pass 2 segment statistics m[n,h], den[n,h] (per row for attention_norm_idx 0, per column for 1; den includes the + 1e-16),
 * pass 3 normalise with the statistics / maximum CURRENTLY in the workspace and write w_mean_csr.  Same kernels and arithmetic
 * as gnpde_edge_attention's general path (reference src/function_transformer_attention.py:190-213, src/utils.py:179-208).
 * gnpde_attention_workspace_regions: byte offsets {scores, seg_m, seg_den, gmax} inside the workspace.
 * gnpde_segment_stats_merge: (m, den)[rows[i]] <- merge with (m_in, den_in)[i], i < n_rows (rows NULL: i itself) -- softmax:
 * M = max(m, m_in), den = den e^(m-M) + den_in e^(m_in-M); squareplus: den += den_in.  Partial statistics of a column whose
 * entries live on several ranks are combined with it, peer by peer in a fixed order. */
int gnpde_edge_attention_pass(const gnpde_graph_t* g, const gnpde_attention_t* a, int32_t pass, float* w_mean_csr,
                              void* workspace, size_t workspace_bytes, void* stream);
int gnpde_attention_workspace_regions(const gnpde_graph_t* g, const gnpde_attention_t* a, size_t* offsets);
int gnpde_segment_stats_merge(float* seg_m, float* seg_den, const int32_t* rows, int32_t n_rows, int32_t heads,
                              const float* m_in, const float* den_in, int32_t square_plus, void* stream);

/* The launch decision of gnpde_edge_attention, gnpde_edge_attention_pass, the backward's forward passes and the attention inside
 * gnpde_rhs_eval / the solvers, as gnpde_spmm_plan gives the aggregation's: route, template line of the row kernels, sweeps, grids and how
 * the hub rows (more than GNPDE_LONG_ROW entries) are handled.  Nothing is launched, no device is needed and no address is dereferenced:
 * workspace_addr and the pointer fields of *a (q, k, gat_a, output_var, lengthscale, edge_w_csr, t_from_csr) are read for their alignment
 * and for being null only; *g and a->graph_t are host structs whose counts and non-null arrays are read.  The launchers of the library
 * switch on the very same result, so a plan is what runs.  request_flags: GNPDE_ATT_PLAN_W_MEAN / _ATT_EDGE / _PRODS_EDGE the outputs
 * wanted, _FORK a second stream is given for the hub rows, _DEFER an aggregation follows that can normalise the hub rows (the solver's
 * evaluation), _HUBS_ONLY the hub rows' weights alone, _STATS_ONLY general passes 1-2 alone (the backward); pass: 0, or 1..3 as
 * gnpde_edge_attention_pass.  Returns what the launch would return for these operands: 0, or GNPDE_EINVAL / GNPDE_EWS (workspace
 * null) with gnpde_last_error set; the workspace SIZE is not part of the question.
 *   vec4     d_k % 4 == 0, ldqk % 4 == 0, q and k 16-byte aligned
 *   route    by the first line that holds (h in {1,2,4,8} for every line but the last; "rows alone" = head-mean weights alone,
 *            attention_norm_idx 0, no squareplus, the graph has bin_rows, GAT or vec4):
 *     GNPDE_ATT_ROUTE_NONE       no node or no edge
 *     GNPDE_ATT_ROUTE_HUBS_ONLY  rows alone, _HUBS_ONLY: hub chunk statistics + hub_normalise_kernel (hubs = OWN), nothing without hub rows
 *     GNPDE_ATT_ROUTE_SD_ROWS    row_attention_sd_kernel<h, dk4, .., MODE, SCATTER>, one launch per row class and sweep, the hub chunks in
 *                                their first blocks (hubs = IN_ROWS); needs one stream, the graph's long_chunk_first, gnpde_tune(4, 0):
 *                                  rows alone, GAT without edge weights: gat_terms = 2 (node terms + their 4-wide table), dk4 1, MODE 3
 *                                  rows alone, scaled_dot / exp_kernel, d_k in {4,8,16}: MODE 0 / MODE 4
 *                                  weights alone, scaled_dot, vec4, d_k in {4,8,16}, squareplus and / or attention_norm_idx 1 (graph_t and
 *                                  t_from_csr given, no edge weights: swapped = scatter = 1, the rows of graph_t with q and k exchanged):
 *                                  MODE 0, or the sweeps MODE 2 (global maximum) then MODE 1 for squareplus
 *     GNPDE_ATT_ROUTE_SD_ONE     _DEFER, rows alone, scaled_dot, d_k in {4,8,16}, h <= 4, whole graph, no halo rows, no edge weights, no
 *                                fork, gnpde_tune(21, 0), (4, 0), (17, 0): row_attention_sd_one_kernel, ONE launch (grid[0][0]); hubs =
 *                                DEFERRED: the aggregation forms the hub entries' weights.  Tested before the scaled_dot line of SD_ROWS.
 *     GNPDE_ATT_ROUTE_ROWS       rows alone, whatever is left: one launch per row class -- row_attention_sd_kernel without hub blocks
 *                                (dk4 != 0: scaled_dot, d_k in {4,8,16}, gnpde_tune(4, 0); reached with _FORK or without long_chunk_first)
 *                                or row_attention_kernel<type, h> (dk4 = 0) -- and the hub rows in two launches of their own (hubs = OWN,
 *                                or OWN_FORKED on the second stream)
 *     GNPDE_ATT_ROUTE_GENERAL    everything else: the passes of the bit mask `passes` (1 scores_kernel, 2 segment statistics --
 *                                seg_stats_heads = 1: seg_stats_heads_kernel<h> -- plus, hubs = LONG_STATS, two launches over the n_long
 *                                long segments x max_chunks chunks, 4 normalise_kernel); a row sub-range (row_begin > 0): GNPDE_EINVAL
 *   rows16   lane mapping of the rows of <= 16 entries: QUARTER 16 lanes a row, two rows interleaved (h = 4, d_k 4 or 16 on the SD
 *            kernels), LANES 16 h lanes (at most a wave), WHOLE_WAVE the A/B form of gnpde_tune(17, 9) (QUARTER's cases, MODE 0, no SCATTER)
 *   gmax     squareplus' global maximum: PER_WAVE one word per wave of the MODE 2 sweep (gmax_count of them), folded by the second sweep
 *            (no hub rows, at most 8192 waves, gnpde_tune(16, 0)); SLOTS_FOLD memset + slot atomics + gmax_fold_kernel; ATOMIC memset +
 *            atomics in scores_kernel (GENERAL, pass 0 or 1)
 *   grid     [sweep][0] rows of <= 16 entries: ceil(n_bin16 / rows per workgroup) + hub blocks, rows per workgroup = 4 x (64 / lanes a row)
 *            x rows interleaved (SD kernels: 4 at d_k 4, else 2, where one pass covers 16 entries x h; 1 where not; row_attention_kernel: 1);
 *            [sweep][1] rows of 17..GNPDE_LONG_ROW entries: ceil(n_bin64 / 4) + hub blocks (none in a MODE 2 sweep); 0: no launch
 *   hub_fold 2 under gnpde_tune(11, 2), else 0;  launches: kernel launches in all (memsets not counted) */
#define GNPDE_ATT_ROUTE_NONE      0
#define GNPDE_ATT_ROUTE_HUBS_ONLY 1
#define GNPDE_ATT_ROUTE_SD_ONE    2
#define GNPDE_ATT_ROUTE_SD_ROWS   3
#define GNPDE_ATT_ROUTE_ROWS      4
#define GNPDE_ATT_ROUTE_GENERAL   5
#define GNPDE_ATT_ROWS16_NONE       0
#define GNPDE_ATT_ROWS16_QUARTER    1
#define GNPDE_ATT_ROWS16_LANES      2
#define GNPDE_ATT_ROWS16_WHOLE_WAVE 3
#define GNPDE_ATT_GMAX_NONE       0
#define GNPDE_ATT_GMAX_PER_WAVE   1
#define GNPDE_ATT_GMAX_SLOTS_FOLD 2
#define GNPDE_ATT_GMAX_ATOMIC     3
#define GNPDE_ATT_HUBS_NONE       0
#define GNPDE_ATT_HUBS_IN_ROWS    1
#define GNPDE_ATT_HUBS_DEFERRED   2
#define GNPDE_ATT_HUBS_OWN        3
#define GNPDE_ATT_HUBS_OWN_FORKED 4
#define GNPDE_ATT_HUBS_LONG_STATS 5
#define GNPDE_ATT_PLAN_W_MEAN     1u
#define GNPDE_ATT_PLAN_ATT_EDGE   2u
#define GNPDE_ATT_PLAN_PRODS_EDGE 4u
#define GNPDE_ATT_PLAN_FORK       8u
#define GNPDE_ATT_PLAN_DEFER      16u
#define GNPDE_ATT_PLAN_HUBS_ONLY  32u
#define GNPDE_ATT_PLAN_STATS_ONLY 64u
typedef struct gnpde_attention_launch_t {
  int32_t  route;            /* GNPDE_ATT_ROUTE_* */
  int32_t  vec4;
  int32_t  h, dk4;           /* heads; d_k / 4 of the SD row kernels' template line (1 for GAT's table), 0 where none runs */
  int32_t  n_sweeps, mode[2];/* sweeps over the rows and the MODE of each */
  int32_t  scatter, swapped; /* SCATTER (weights stored through t_from_csr); q and k exchanged */
  int32_t  rows16;           /* GNPDE_ATT_ROWS16_* */
  int32_t  gmax, gmax_count; /* GNPDE_ATT_GMAX_* */
  int32_t  hubs, n_hub;      /* GNPDE_ATT_HUBS_*; hub chunks of the walked graph */
  int32_t  hub_fold;
  int32_t  gat_terms;        /* 0, 1 gat_terms_kernel, 2 with its table */
  int32_t  passes, seg_stats_heads, n_long, max_chunks;   /* GENERAL */
  int32_t  launches;
  uint32_t grid[2][2];
} gnpde_attention_launch_t;
int gnpde_attention_plan(const gnpde_graph_t* g, const gnpde_attention_t* a, uint32_t request_flags, int32_t pass, uint64_t workspace_addr,
                         gnpde_attention_launch_t* plan);

/* Backward of the normalisation + head mean of gnpde_edge_attention for EVERY normaliser the reference has (softmax or
 * squareplus, opt['attention_norm_idx'] 0 or 1; reference src/function_transformer_attention.py:210-213, src/utils.py:179-208,
 * torch_geometric.utils.softmax):  dw_csr[p] = g_row . x_col (gnpde_sddmm without scale, CSR order);
 *   ds_csr[p,h] = dL / d prods[p,h]   (the raw scores, before att->edge_w_csr is applied), scaled by s / H with
 * s = 1 (scale NULL), *scale, or sigmoid(*scale).  squareplus: the global maximum's gradient goes evenly to the entries that
 * attain it, as autograd's `src.max()` does.  The scores and segment statistics are recomputed from att->q / att->k
 * (any att->type).  Feed ds to gnpde_head_spmm for the scaled-dot score's d q / d k. */
size_t gnpde_attention_bwd_workspace_bytes(const gnpde_graph_t* g, const gnpde_attention_t* a);
int gnpde_edge_attention_bwd(const gnpde_graph_t* g, const gnpde_attention_t* a, const float* dw_csr, const float* scale,
                             int32_t scale_sigmoid, float* ds_csr, void* workspace, size_t workspace_bytes, void* stream);

/* The same backward for a gradient that arrives PER HEAD in the caller's edge order (datt_edge [E,h]: what autograd hands back
 * for the [E,h] attention a block computes once per forward, reference src/block_transformer_attention.py:38-39), with the
 * factor that turns d L / d score into what the score function's own derivative needs:
 *   post 0: ds = d L / d raw score (times att->edge_w_csr)                      -- scaled dot, cosine, pearson
 *   post 1: ds = (d L / d score) * score  -- the common factor of every derivative of var^2 exp(-|q-k|^2 / 2 l^2)
 *   post 2: ds = (d L / d score) * LeakyReLU'(pre-activation)                   -- GAT */
int gnpde_edge_attention_bwd_heads(const gnpde_graph_t* g, const gnpde_attention_t* a, const float* datt_edge, int32_t post,
                                   float* ds_csr, void* workspace, size_t workspace_bytes, void* stream);

/* The same ds as gnpde_softmax_rows_bwd, but computed from q and k in ONE pass (scores, row softmax and its
 * backward; no [E,h] attention array): att->type must be GNPDE_ATT_SCALED_DOT with norm_idx 0 and no squareplus,
 * heads in {1,2,4,8}, d_k in {4,8,16} (GNPDE_ESHAPE otherwise: use gnpde_edge_attention + gnpde_softmax_rows_bwd).
 * r_csr[p] = g_row . x_col (gnpde_sddmm without scale); att->edge_w_csr is honoured. */
int gnpde_attention_rows_bwd(const gnpde_graph_t* g, const gnpde_attention_t* att, const float* r_csr, const float* scale,
                             int32_t scale_sigmoid, float* ds_csr, void* stream);

/* The row kernels of the adjoint stage (csrc/adjoint.hip) as entry points of their own; plain forwards.
 * gnpde_attention_rows_bwd_dq: gnpde_attention_rows_bwd with its three optional operands --
 *   rpos    (NULL or [E] int32) r is stored in another order: the kernel reads r[rpos[p]] for CSR position p;
 *   dq      (NULL or [n, lddq]) also d q[row, 0:A] = (1 / sqrt d_k) sum_{p in row} ds[p, head] k[col_p, :], for the head shapes of
 *           gnpde_attention_rows_bwd_dq_supported (heads * d_k <= 32; GNPDE_ESHAPE otherwise).  Rows without entries are not written;
 *   hub_ws  (NULL or gnpde_hub_bwd_workspace_floats(g, heads, att_dim) floats) rows longer than GNPDE_LONG_ROW as 512-entry chunks
 *           over the whole chip (three kernels) instead of one 1024-thread block per row.
 * gnpde_head_rowsum: out[seg, 0:A] = scale * sum over the rows of g (entry t: ds[pos ? pos[t] : t, head], feat[colidx[t], :]) with a
 *   lane per entry, for the head shapes of gnpde_head_rowsum_supported (GNPDE_ESHAPE otherwise); feat and ds 16-byte aligned,
 *   ldf % 4 == 0; rows without entries are not written; hub_ws as above (heads * dk floats per chunk are used). */
size_t gnpde_hub_bwd_workspace_floats(const gnpde_graph_t* g, int32_t heads, int32_t att_dim);
int gnpde_head_rowsum_supported(int32_t heads, int32_t dk);
int gnpde_attention_rows_bwd_dq_supported(int32_t heads, int32_t dk);
int gnpde_attention_rows_bwd_dq(const gnpde_graph_t* g, const gnpde_attention_t* att, const float* r, const int32_t* rpos,
                                const float* scale, int32_t scale_sigmoid, float* ds_csr, float* dq, int32_t lddq, float* hub_ws,
                                void* stream);
int gnpde_head_rowsum(const gnpde_graph_t* g, const int32_t* pos, const float* ds, int32_t heads, int32_t dk, const float* feat,
                      int32_t ldf, float scale, float* out, int32_t ldo, float* hub_ws, void* stream);


/* ------------------------------------------------------------------------------------------------
 * GRAND-nl evaluation in ONE pass (the solver's hot case): scaled-dot attention, softmax over the row
 * (attention_norm_idx 0, no squareplus), head-mean aggregation, epilogue and solver stage.
 * Replaces the whole of ODEFuncTransformerAtt.forward (src/function_transformer_attention.py:38-53,
 * incl. the Q/K Linear layers :174-175) with a single gather of every neighbour row: the score is
 * evaluated as ((W_k,h^T q_i,h) . x_j + q_i,h . b_k,h) / sqrt(d_k), so neither the [N,2A] projection nor
 * [E,h] scores nor [E] weights are materialised.  proj_w = [Q.weight; K.weight] ([2A, d], 16-byte
 * aligned), proj_b = [Q.bias; K.bias] or NULL.  att->q / att->k are ignored; att->edge_w_csr is honoured.
 * gnpde_attn_rhs_fused_supported tells whether the configuration is covered (else use gnpde_linear +
 * gnpde_edge_attention + gnpde_spmm_rhs, which compute the same function).
 * ---------------------------------------------------------------------------------------------- */
size_t gnpde_attn_rhs_fused_workspace_bytes(const gnpde_graph_t* g, int32_t d, int32_t heads);
int gnpde_attn_rhs_fused_supported(const gnpde_attention_t* att, int32_t d, int32_t ld);
int gnpde_attn_rhs_fused(const gnpde_graph_t* g, const gnpde_attention_t* att, const float* proj_w,
                         const float* proj_b, const float* u, int32_t d, int32_t ld,
                         const gnpde_epilogue_t* epi, void* workspace, size_t workspace_bytes, void* stream);

/* w_csr[p] = mean_h src[perm[p], :]   (src [E,h] in the caller's edge order; h = 1: plain gather).
 * Used when a block hands attention_weights / edge_weight in edge order
 * (src/function_laplacian_diffusion.py:29-35). */
int gnpde_edge_to_csr_mean(const gnpde_graph_t* g, const float* src_edge, int32_t h, float* w_csr,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fixed-step solver (torchdiffeq `euler` / `rk4` fixed grid, src/block_constant.py:57-62,
 * src/block_transformer_attention.py:58-63) with the whole time loop captured in one hipGraph.
 * ---------------------------------------------------------------------------------------------- */
enum { GNPDE_RHS_LAPLACIAN = 0, GNPDE_RHS_TRANSFORMER = 1, GNPDE_RHS_GAT = 2 };
/* flags of gnpde_rhs_t.  PADDED_ROWS: ld is a multiple of 4 and the columns [d, ld) of EVERY state-shaped operand (stage
 * input, x0, y, k*, outputs) are padding that may be read and overwritten -- lets a state width that is not a multiple of
 * 4 (BLEND ogbn-arxiv: d = 162, reference best_params feat_hidden_dim 64 + pos_enc_hidden_dim 98) use 16-byte lanes. */
#define GNPDE_RHS_PADDED_ROWS 1
/* MIX_FEATURES (kind GNPDE_RHS_GAT only; GNPDE_EINVAL on another kind): the second form of the reference's GAT function
 * (src/function_GAT_attention.py:32-38, opt['mix_features']):  f = alpha' (A(x) (x W) Wout - x) + beta x0.  out_w is Wout TRANSPOSED,
 * [d, A] row-major with row stride out_ld >= A (A = att.att_dim).  An evaluation is the projection and the attention of the plain GAT
 * form, the plain aggregation z = A(x) (x W) of rows of the projection table into a workspace region [n, A], and
 * gnpde_linear_epilogue over z, which carries the diffusion epilogue and the stage algebra (Wout sits between the aggregate and
 * "- x", so the aggregation cannot).  Shapes: A % 4 == 0, A <= 256, d <= 256, whole-graph descriptors (proj_row_end == 0,
 * n_state_rows <= graph->n); GNPDE_ESHAPE otherwise.  Covered by gnpde_rhs_eval / gnpde_rhs_stage, gnpde_solver_* (early stopping
 * included) and gnpde_dopri5_* on one GPU.  NOT covered, and refused with GNPDE_ESHAPE: the adjoint objects (gnpde_adjoint_create,
 * every method; gnpde_adjoint_adaptive_create), the recorded solve (gnpde_solver_set_tape), the bf16 gather operand
 * (gnpde_solver_gather_bytes returns 0) and the row-partitioned solver -- none of them differentiates or shards this function. */
#define GNPDE_RHS_MIX_FEATURES 2
/* MIDPOINT (torchdiffeq fixed_grid.py Midpoint, advertised by the reference at src/run_GNN.py:330): y + dt f(y + (dt / 2) f(y)),
 * two evaluations per step, both as GNPDE_STAGE_LINCOMB stages; gnpde_solver_* only.
 * DOPRI5_TAPE: no method of a solve -- gnpde_adjoint_create only: the object sweeps a recorded Dormand-Prince solve
 * (gnpde_adjoint_set_dopri5_tape). */
enum { GNPDE_METHOD_EULER = 0, GNPDE_METHOD_RK4 = 1, GNPDE_METHOD_MIDPOINT = 2, GNPDE_METHOD_DOPRI5_TAPE = 3 };

typedef struct gnpde_rhs {
  int32_t kind;               /* GNPDE_RHS_*                                                   */
  const gnpde_graph_t* graph;
  int32_t d, ld;              /* state width and leading dimension                             */
  int32_t n_state_rows;       /* rows of the state incl. halo rows of a row-partitioned graph (0: graph->n);
                                 the projection covers all of them, the aggregation only graph->n rows */
  int32_t proj_row_begin;     /* with proj_row_end > 0: project only rows [proj_row_begin, proj_row_end)
                                 (interior / boundary passes overlapping the halo exchange) */
  int32_t proj_row_end;
  int32_t flags;              /* GNPDE_RHS_PADDED_ROWS | GNPDE_RHS_MIX_FEATURES, or 0 */
  /* epilogue scalars */
  const float* alpha; const float* beta; const float* x0; int32_t alpha_sigmoid;
  /* LAPLACIAN: fixed weights, CSR order */
  const float* w_csr;
  /* TRANSFORMER / GAT: projection W [m, d] (+ bias), m = 2A (q||k) or A (GAT), and the attention
   * descriptor (its q/k/ldqk fields are filled by the solver from its workspace)               */
  const float* proj_w; const float* proj_b; int32_t proj_m;
  gnpde_attention_t att;
  /* GNPDE_RHS_MIX_FEATURES: Wout transposed, [d, att.att_dim] row-major, row stride out_ld (appended in ABI 25: every field above
   * keeps its offset) */
  const float* out_w; int32_t out_ld;
} gnpde_rhs_t;

typedef struct gnpde_solver gnpde_solver_t;

/* Workspace (device) the solver needs: stage buffers k1..k3, two stage inputs, projections,
 * attention scratch, spmm scratch. */
size_t gnpde_solver_workspace_bytes(const gnpde_rhs_t* rhs, int32_t method);

/* dts[n_steps] are the step sizes of the time grid (host array; the last one may be short).
 * The descriptor, and the device arrays it points to, must stay alive as long as the solver. */
int gnpde_solver_create(gnpde_solver_t** out, const gnpde_rhs_t* rhs, int32_t method,
                        const float* dts, int32_t n_steps, void* workspace, size_t workspace_bytes);

/* Integrates y (in place, [n, ld]) over the whole grid.  With use_graph != 0 the launches are
 * captured once into a hipGraph (keyed on the y pointer) and replayed. */
int gnpde_solver_run(gnpde_solver_t* s, float* y, int32_t use_graph, void* stream);

/* Recorded solve -- training with opt['adjoint'] off through a fixed-grid method (the reference's default: src/base_classes.py:44-47
 * picks torchdiffeq.odeint, run_GNN.py:62-96 calls loss.backward() through its Python loop; src/block_constant.py:45-62).  With a tape
 * attached every stage input of the following runs is written to a slot of its own (n_evals + 1 state-sized slots, 256-byte aligned
 * strides: slot 0 = y0, slot i = the input of evaluation i, the last slot = y(T)) instead of a recycled stage buffer, so the record
 * costs no extra pass over the state.  GRAND-nl with scaled-dot scores also records, behind the slots, every evaluation's q||k
 * projection [n, 2A] and head-mean weights [e] (the evaluation writes them there instead of into its scratch regions), so that the
 * reverse sweep runs neither the projection nor the attention again.  The caller hands over ZERO-FILLED memory (padding columns are
 * read by 16-byte lanes).
 * tape == NULL detaches.  The reverse sweep is gnpde_adjoint_set_tape + gnpde_adjoint_run below. */
size_t gnpde_solver_tape_bytes(const gnpde_rhs_t* rhs, int32_t method, int32_t n_steps);
int    gnpde_solver_set_tape(gnpde_solver_t* s, void* tape, size_t tape_bytes);

/* bf16 gather operand of a fixed-step solve (see gnpde_spmm_rhs_lo): with dtype = GNPDE_GATHER_BF16 every stage-input buffer of
 * euler / midpoint / rk4 gets a shadow in `mem` (caller's device memory, 256-byte aligned, gnpde_solver_gather_bytes bytes); the kernel
 * that writes a stage input writes its shadow, y0's is filled by gnpde_to_bf16 at the start of a run, and a stage never writes the
 * shadow it gathers from.  The attention then always runs in launches of its own.  The state the caller gets back is fp32;
 * results are deterministic but differ from the fp32 solve by the rounding of the gathered rows.  dtype = GNPDE_GATHER_FP32
 * detaches.  Either call drops a captured hipGraph.  Excludes a tape: GNPDE_EINVAL while one is attached, and
 * gnpde_solver_set_tape refuses while the mode is on.  gnpde_solver_gather_bytes returns 0 with gnpde_last_error set when the
 * shape is out of scope (no 16-byte lanes, partitioned descriptors). */
#define GNPDE_GATHER_FP32 0
#define GNPDE_GATHER_BF16 1
size_t gnpde_solver_gather_bytes(const gnpde_rhs_t* rhs, int32_t method);
int    gnpde_solver_set_gather(gnpde_solver_t* s, int32_t dtype, void* mem, size_t bytes);

/* Outputs at several times of a fixed-grid solve  [torchdiffeq 0.2.1 FixedGridODESolver.integrate: output j comes from the first step
 * [ta, tb] with tb >= t[j], as y_next (t[j] == tb), y (t[j] == ta) or the linear interpolation y + frac (y_next - y)].  The caller plans
 * on the host: output j is taken after step step[j] (1-based, non-decreasing) at the fraction frac[j] in [0, 1] of that step (1: the
 * state after the step) and lands in out + j * n * ld_out, rows of stride ld_out >= d.  Before a step with an output strictly inside it the
 * solver copies its start state to `scratch` (one [n, ld] state buffer; may be NULL when every frac is 1); after the step one
 * gnpde_snapshot_rows launch per output.  Copies and snapshots are nodes of the captured hipGraph and of the eager path alike; without
 * outputs the solver enqueues exactly what it did before.  n_out == 0 detaches.  Drops a captured hipGraph.  GNPDE_EINVAL with a
 * message together with a tape, the early-stopping evaluator (either order of the calls) or a partitioned descriptor.  The bf16 gather
 * operand composes: outputs read the fp32 state only.
 * gnpde_solver_set_output_order: solver row r is written to row order[r] of every output (device int32 [n], must outlive the runs; the
 * relabelled graph of graph.LocalityView); NULL: row r. */
int gnpde_solver_set_outputs(gnpde_solver_t* s, int32_t n_out, const int32_t* step, const float* frac, float* out, int32_t ld_out,
                             float* scratch);
int gnpde_solver_set_output_order(gnpde_solver_t* s, const int32_t* order);
/* out[m(r), 0:d] = ya[r, 0:d] + frac (yb[r, 0:d] - ya[r, 0:d]), one fused multiply-add per element; state rows of stride ld, output rows
 * of stride ld_out; m(r) = order[r] (device int32 [n]) or r when order is NULL.  frac == 1 is the copy of yb through the same map (ya may
 * be NULL).  16-byte lanes where d, both strides and every address allow them, element by element otherwise. */
int gnpde_snapshot_rows(const float* ya, const float* yb, float frac, int64_t n, int32_t d, int32_t ld, float* out, int32_t ld_out,
                        const int32_t* order, void* stream);

/* The q||k projection of SpGraphTransAttentionLayer (nn.Linear Q and K, reference src/function_transformer_attention.py:174-175) as TWO
 * tables q [n, A], k [n, A] instead of interleaved rows [n, 2A]: when a key row is shorter than a 128-byte cache line (A <= 16) the
 * attention's gathers of k rows otherwise fetch the q half of every line.  Offered (gnpde_linear_split_supported != 0) for tall x,
 * d = 64 / 128, m = 2A = 32, 16-byte aligned operands; the fixed-step / dopri5 solvers use it by themselves for whole-graph GRAND-nl
 * descriptors with scaled-dot scores (gnpde_attention_t.q / k / ldqk already describe either layout). */
int gnpde_linear_split_supported(const float* x, int64_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw, int32_t split);
int gnpde_linear_split(const float* x, int32_t n, int32_t d, int32_t ldx, const float* W, int32_t m, int32_t ldw, const float* b,
                       float* out_q, float* out_k, int32_t split, void* stream);

/* The launch decision of gnpde_linear / gnpde_relu_linear, for tests and A/B scripts: which kernel instantiation each launch of a call
 * with these operands takes, over which output columns and on what grid.  Nothing is launched and no address is dereferenced: x_addr,
 * w_addr and out_addr are the operand addresses as integers and only their alignment is read (16 bytes for x and W, 8 for out).  The
 * launchers of the library switch on the very same result, so a plan is what runs.  A launch is (family, mt, param):
 *   GNPDE_LINEAR_SMALL       n <= 32 768, aligned operands, d % 16 == 0 and m % 16 == 0: ONE launch over all of [n, m] on a 2-D grid
 *                            (grid_y walks groups of 16 * mt columns); mt = 2 when m % 32 == 0, else 1; param 0
 *   GNPDE_LINEAR_STAGED2     d = 64 / 128, 32 complete columns, even ldo and column base, 8-byte aligned out: x in whole lines through
 *                            LDS, paired output columns in 8-byte stores; mt = 2, param = KB = d / 16; split = 1 when it writes two
 *                            tables (gnpde_linear_split)
 *   GNPDE_LINEAR_STAGED      d = 64 / 128 otherwise (16 or 32 complete columns); mt = 1 / 2, param = KB = d / 16
 *   GNPDE_LINEAR_PERSISTENT  every other d = 16 * KB <= 128 on 16 or 32 complete columns: W in registers; mt = 1 / 2, param = KB
 *   GNPDE_LINEAR_LDS         64 or 128 complete columns, d % 16 == 0, d <= 256: W staged in LDS by workgroups of 512; mt = 4 / 8,
 *                            param = DMAX = 128 (d <= 128) or 256
 *   GNPDE_LINEAR_TILE        everything else, one wavefront per 16-row tile; mt = 1 / 2 / 4 / 8, param = 2 * ALIGNED + FULL: 3 = 16-byte
 *                            loads without guards (complete columns, d % 16 == 0), 2 = 16-byte loads with guards (ragged columns or
 *                            ragged K), 0 = scalar loads (operands without 16-byte alignment)
 * A call whose rows exceed the small rule covers its columns left to right in launches of 128, 64, 32 or 16 (mt = 8, 4, 2, 1) by the
 * number of 16-column tiles still to go.  gnpde_linear_plan writes the first min(count, cap) launches in launch order to plan and
 * returns count (0 for n = 0), or GNPDE_EINVAL for a shape gnpde_linear refuses.  gnpde_linear_split_plan writes the one launch of
 * gnpde_linear_split and returns 1, or GNPDE_ESHAPE where gnpde_linear_split refuses. */
#define GNPDE_LINEAR_SMALL      0
#define GNPDE_LINEAR_STAGED2    1
#define GNPDE_LINEAR_STAGED     2
#define GNPDE_LINEAR_PERSISTENT 3
#define GNPDE_LINEAR_LDS        4
#define GNPDE_LINEAR_TILE       5
typedef struct gnpde_linear_launch_t {
  int32_t  family;    /* GNPDE_LINEAR_* */
  int32_t  mt;        /* 16-column tiles per wavefront */
  int32_t  param;     /* KB, DMAX or 2 * ALIGNED + FULL, by family (above) */
  int32_t  split;     /* 1: the two-table form of gnpde_linear_split */
  int32_t  col_base;  /* first output column of the launch */
  int32_t  cols;      /* output columns it writes */
  uint32_t grid_x, grid_y, block;
} gnpde_linear_launch_t;
int gnpde_linear_plan(uint64_t x_addr, int32_t n, int32_t d, int32_t ldx, uint64_t w_addr, int32_t m, int32_t ldw, uint64_t out_addr,
                      int32_t ldo, gnpde_linear_launch_t* plan, int32_t cap);
int gnpde_linear_split_plan(uint64_t x_addr, int32_t n, int32_t d, int32_t ldx, uint64_t w_addr, int32_t m, int32_t ldw,
                            uint64_t out_q_addr, uint64_t out_k_addr, int32_t split, gnpde_linear_launch_t* plan);

/* The launch decision of gnpde_spmm_rhs / gnpde_spmm and their _lo and _tickets forms, as gnpde_linear_plan gives the projection's: the
 * kernel a call with these operands takes, its grid, and how its hub rows (more than GNPDE_LONG_ROW entries) are folded.  Nothing is
 * launched, no device is needed and no address is dereferenced: u_addr, plain_out_addr, workspace_addr and the pointer fields of *epi are
 * read for their alignment (and for being null) only.  Exactly one of epi / plain_out_addr is given.  The launchers of the library
 * switch on the very same result, so a plan is what runs.  flags: GNPDE_SPMM_PLAN_LO a bf16 gather operand is given (shadows taken as
 * 16-byte aligned), _TICKETS a ticket buffer is given, _DEFER the hub-chunk items are to form their entries' weights (the one-launch row
 * attention), _FORK the hub-row work is to run on a second stream.  Returns what the launch would return for these operands:
 * 0, or GNPDE_EINVAL / GNPDE_ESHAPE with gnpde_last_error set (workspace and ticket SIZES are not part of the question).
 *   lane_bytes  16 where d % 4 == 0 (or padded_rows), ld % 4 == 0 and u, plain_out, the workspace and every epilogue operand are 16-byte
 *               aligned; 8 by the same rule with 2 and 8 bytes; else 4.  A bf16 operand needs 16 (GNPDE_ESHAPE otherwise).
 *   the kernel  by slots = lanes that cover a row = ceil(d / (lane_bytes / 4)):
 *     slots <= 8          GNPDE_SPMM_ROWS (L, K, U) = (8, 1, 4)             <= 16          ROWS (16, 1, 4)
 *     17 .. 64, 16-byte   GNPDE_SPMM_PAIR (L 32, U 16) where slots <= 32 and at least half of the rows have <= 16 entries (with a bf16
 *                         operand and gnpde_tune(18, 2), d % 8 == 0: GNPDE_SPMM_QUAD_LO, L 16, U 16); else GNPDE_SPMM_WIDE, L = 32 or 64,
 *                         U 8; full = 1 where d == 4 L (no column predicate; never for QUAD_LO)
 *     17 .. 64, narrower  ROWS (16, 2, 4) for slots <= 32, else ROWS (32, 2, 4)
 *     <= 128 / 192 / 256  ROWS (64, 2, 2) / (64, 3, 1) / (64, 4, 1)            more: GNPDE_ESHAPE
 *     L lanes cover one neighbour row (K column tiles of them), U gathers are in flight; ROWS runs workgroups of 256 (four waves, a row
 *     each), the others of 64; PAIR takes two and QUAD_LO four rows per wave.  lo = 1: the instantiation that gathers bf16.
 *   grid        8 * max(1, ceil((ceil(chunks / 8) + ceil(rows_per_xcd / rows per wave)) / waves per workgroup)), rows_per_xcd as
 *               gnpde_xcd_row_map gives it for [row_begin, n); forked = 1: the hub chunks run in a second launch of the same kernel on the
 *               other stream (chunks = 0 here)
 *   the pair kernel alone (whole graph, one stream, fp32 table, gnpde_tune(9, 0)) can take _DEFER (defer = 1 where the graph has hub
 *   rows; GNPDE_EINVAL on any other route) and fold the hub rows itself
 *   fold        GNPDE_SPMM_FOLD_NONE no hub rows; _IN_KERNEL tickets given, the pair kernel alone, stage RHS, EULER or RK1C..RK4C,
 *               gnpde_agg_fold_launch(0); else a launch of its own: _REDUCE4_LO with a bf16 operand, _REDUCE4 on 16-byte lanes, _SCALAR */
#define GNPDE_SPMM_ROWS    0
#define GNPDE_SPMM_WIDE    1
#define GNPDE_SPMM_PAIR    2
#define GNPDE_SPMM_QUAD_LO 3
#define GNPDE_SPMM_FOLD_NONE       0
#define GNPDE_SPMM_FOLD_IN_KERNEL  1
#define GNPDE_SPMM_FOLD_REDUCE4    2
#define GNPDE_SPMM_FOLD_REDUCE4_LO 3
#define GNPDE_SPMM_FOLD_SCALAR     4
#define GNPDE_SPMM_PLAN_LO      1u
#define GNPDE_SPMM_PLAN_TICKETS 2u
#define GNPDE_SPMM_PLAN_DEFER   4u
#define GNPDE_SPMM_PLAN_FORK    8u
typedef struct gnpde_spmm_launch_t {
  int32_t  family;      /* GNPDE_SPMM_* */
  int32_t  lane_bytes;  /* 16, 8 or 4 */
  int32_t  L, K, U;     /* template line of the kernel (above) */
  int32_t  full, lo, defer;
  uint32_t grid, block;
  int32_t  forked;
  int32_t  fold;        /* GNPDE_SPMM_FOLD_* */
} gnpde_spmm_launch_t;
int gnpde_spmm_plan(const gnpde_graph_t* g, uint64_t u_addr, int32_t d, int32_t ld, const gnpde_epilogue_t* epi, uint64_t plain_out_addr,
                    uint64_t workspace_addr, int32_t padded_rows, uint32_t flags, gnpde_spmm_launch_t* plan);

/* One un-fused evaluation out = f(u) of the same descriptor (what ODEFunc.forward returns). */
int gnpde_rhs_eval(const gnpde_rhs_t* rhs, const float* u, float* out, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t gnpde_rhs_workspace_bytes(const gnpde_rhs_t* rhs);

/* ------------------------------------------------------------------------------------------------
 * Native adjoint solve: the backward pass of ODEblock.forward under opt['adjoint'] (reference src/base_classes.py:44-47,
 * src/block_constant.py:45-55 -> torchdiffeq.odeint_adjoint) for the fixed-grid adjoint methods (opt['adjoint_method'] euler /
 * rk4 == 3/8 rule, opt['adjoint_step_size']).  torchdiffeq integrates  y' = f,  a' = -a^T df/dy,  g' = -a^T df/dtheta  backwards
 * in time (s = -t) and gets f and the vector-Jacobian products from autograd through ODEFunc.forward
 * (src/function_transformer_attention.py:38-53, src/function_laplacian_diffusion.py:38-51); here one stage is a fixed sequence
 * of this library's kernels (projection, attention, aggregation with the NEXT stage input formed in its epilogue, SDDMM,
 * normaliser backward, head-SpMMs, aggregation on the transposed CSR, one pass for the parameter gradients) and the whole
 * backward solve is one captured hipGraph.  rhs: GNPDE_RHS_LAPLACIAN (constant weights) or GNPDE_RHS_TRANSFORMER with
 * scaled-dot scores (any normaliser), alpha_sigmoid = 1, d <= 256 in 16-byte lanes; exp_kernel scores up to attention_dim = 256, 8 heads
 * (grads then carries two more slots behind d[bq;bk]: d output_var, d lengthscale).
 *   graph_t      CSR of the transposed operator over the SAME edge list;
 *   t_from_csr   [e] device (GRAND-nl): CSR position in rhs->graph of the entry stored at position p of graph_t;
 *   proj_wt      [d, 2A] device (GRAND-nl): rhs->proj_w transposed;   w_t_csr  [e] device (GRAND-l): the weights in graph_t's order.
 * gnpde_adjoint_run: y [n, ld] in: y(t1), out: the state integrated back to t0;  a [n, ld] in: dL/dy(t1), out: dL/dy(t0);
 * grads [gnpde_adjoint_grad_floats] out: GRAND-nl  d[Wq;Wk] [2A, d], d[bq;bk] [2A], d alpha_train, d beta_train;
 *                                        GRAND-l   d alpha_train, d beta_train.
 * dts[n_steps]: the step sizes of the reversed-time grid (torchdiffeq's fixed grid over [-t1, -t0]). */
typedef struct gnpde_adjoint gnpde_adjoint_t;
int    gnpde_adjoint_grad_floats(const gnpde_rhs_t* rhs);
size_t gnpde_adjoint_workspace_bytes(const gnpde_rhs_t* rhs, const gnpde_graph_t* graph_t, int32_t method);
/* Per-wave dot-product slots the adjoint stage's row kernel writes over g (part of the workspace above): its grid -- one wave per work
 * item, the aggregation's grid formula (gnpde_spmm_plan) with one row per wave and one wave per workgroup -- plus one per hub row. */
int32_t gnpde_adjoint_rows_dot_slots(const gnpde_graph_t* g, int32_t d);
int    gnpde_adjoint_create(gnpde_adjoint_t** out, const gnpde_rhs_t* rhs, const gnpde_graph_t* graph_t, const int32_t* t_from_csr,
                            const float* proj_wt, const float* w_t_csr, int32_t method, const float* dts, int32_t n_steps,
                            void* workspace, size_t workspace_bytes);
int    gnpde_adjoint_run(gnpde_adjoint_t* s, float* y, float* a, float* grads, int32_t use_graph, void* stream);
/* Reverse sweep through a RECORDED forward solve (gnpde_solver_set_tape; what autograd does through torchdiffeq's fixed-grid loop,
 * fixed_grid.py / rk_common.py rk4_alt_step_func, when opt['adjoint'] is off).  The object is created with the FORWARD method
 * (euler, midpoint or rk4) and the forward grid's dts; with a tape attached gnpde_adjoint_run ignores y's contents and maps
 * a = dL/dy(T) to dL/dy0, grads as above.  r_acc (GRAND-l, nullable) [e]: receives sum over the evaluations of
 * (b_j h) u_a[row] . u_y[col] in the CSR order of rhs->graph -- times alpha' the gradient of the edge weights (attention block).
 * tape == NULL detaches. */
int    gnpde_adjoint_set_tape(gnpde_adjoint_t* s, const void* tape, size_t tape_bytes, float* r_acc, const int32_t* csr_from_t);
/* csr_from_t (nullable) [e] device: position in graph_t of the entry stored at CSR position q of rhs->graph (the inverse of t_from_csr).  With
 * it -- and always for GRAND-l -- the sweep gathers the COTANGENT rows only: per recorded evaluation one row kernel on graph_t with the roles
 * exchanged (S = alpha' (A^T u_a - u_a), the edge products in graph_t's order, <u_y, S>), the attention backward, and one pass that closes
 * the stage algebra with S + P; the recorded state rows are read as own rows, never gathered.  gnpde_adjoint_tape_swapped: 1 when that
 * form runs -- r_acc then holds the products in GRAPH_T's order. */
int    gnpde_adjoint_tape_swapped(const gnpde_adjoint_t* s);
/* Reverse sweep through a RECORDED DORMAND-PRINCE solve of GRAND-nl or GAT  [replaces what torch autograd does when the reference trains
 * `--function transformer` (or GAT) with its defaults -- opt['adjoint'] = False, method dopri5 (src/run_GNN.py:336, best_params) --
 * i.e. loss.backward() through every accepted step of torchdiffeq's dopri5 loop (rk_common.py _runge_kutta_step, interp.py) and, per
 * evaluation, through ODEFuncTransformerAtt.forward / ODEFuncAtt.forward; the step sizes are constants of the backward pass].  The
 * object is created with method GNPDE_METHOD_DOPRI5_TAPE (dts NULL, n_steps 0; GNPDE_RHS_TRANSFORMER / GNPDE_RHS_GAT descriptors within
 * the limits above, t_from_csr and proj_wt as there) and given, per run and without being re-created, the record of the forward solve:
 *   slots        the stage inputs gnpde_dopri5_set_tape left (gnpde_dopri5_tape_slots): buffer 6 s + i = u_i of accepted step s, [n, ld]
 *                each, slot_stride floats apart (a multiple of 64, at least one state buffer), 256-byte aligned, device;
 *   h[n_steps]   HOST array, the accepted steps' sizes (copied);  x_last in (0, 1]: the fraction of the last step at which t1 lies
 *                (gnpde_dopri5_tape_record);   csr_from_t  as gnpde_adjoint_set_tape (nullable).
 * gnpde_adjoint_run (use_graph = 0: the number of accepted steps changes from run to run, nothing is captured; y is not read) then maps
 * a [n, ld] = dL/d(y_out) to dL/dy0 in place and fills grads as above (GAT: d W^T [A, d], d a in the first 2 d_k of the A slots behind it)
 * with one VJP stage per recorded evaluation, 6 n_steps + 1 in all -- projection and attention RECOMPUTED at u_i (nothing but stage inputs
 * is recorded), the next cotangent formed in the stage's GNPDE_STAGE_LINCOMB epilogue -- and one linear combination per step: a plain
 * sequence of launches on `stream`, no allocation, no float atomics (bit-identical from run to run), and -- after the object's first run,
 * which zero-fills the workspace and synchronises once as every gnpde_adjoint_run does -- no host synchronisation.  The walk is
 * stated in csrc/tape_reverse.h.  slots == NULL detaches.  Refused: an object of another method, GNPDE_RHS_LAPLACIAN (its sweep is
 * gnpde_dopri5_tape_backward), n_steps < 1, x_last outside (0, 1], use_graph != 0; gnpde_adjoint_set_tape refuses such an object. */
int    gnpde_adjoint_set_dopri5_tape(gnpde_adjoint_t* s, const float* slots, size_t slot_stride, const float* h, int32_t n_steps,
                                     float x_last, const int32_t* csr_from_t);
int    gnpde_adjoint_num_rhs_evals(const gnpde_adjoint_t* s);
int    gnpde_adjoint_destroy(gnpde_adjoint_t* s);

/* The BLEND split kernel (reference src/function_transformer_attention.py:133-171: beltrami + exp_kernel -- an exp kernel on the feature
 * and label columns with Qx, Kx, lengthscale_x, output_var_x times one on the positional columns with Qp, Kp, lengthscale_p,
 * output_var_p) runs here as ONE exp kernel of heads of width 2 d_k over a derived projection
 *   Wcat [4A, d], bcat [4A]: per head the d_k rows of Qx / l_x on the feature columns [0, f0) and the label columns [f0 + p0, d), then the
 *                            d_k rows of Qp / l_p on the positional columns [f0, f0 + p0); rows [0, 2A) from Qx / Qp, rows [2A, 4A) from Kx / Kp;
 *   output_var = ov_x ov_p, lengthscale = 1
 * (att_dim = 2A, proj_m = 4A; the adjoint solve and the recorded sweep take it up to att_dim = 256 like the plain exp kernel).
 * gnpde_split_kernel_grads is the chain rule from what gnpde_adjoint_run leaves in `grads` for that descriptor back to the layer's
 * twelve parameters, one launch, capturable (no allocation, no synchronisation, the scalars read from device memory):
 *   grads_cat  [4A d + 4A + 2] device: d Wcat, d bcat, d output_var, (d lengthscale: the derived 1 is no parameter);
 *   wcat, bcat the derived operands the solve used;   lengthscale_x / _p, output_var_x / _p: device scalars;
 *   out        [gnpde_split_kernel_grad_floats = 2A (d + 2) + 4] device:
 *              d Qx.weight [A, d - p0], d Qx.bias [A], d Kx.weight, d Kx.bias, d Qp.weight [A, p0], d Qp.bias [A], d Kp.weight, d Kp.bias,
 *              d lengthscale_x, d lengthscale_p, d output_var_x, d output_var_p, with
 *                d Qx.weight[h d_k + c, j] = d Wcat[h 2 d_k + c, j < f0 ? j : p0 + j] / l_x,   d Qp.weight[h d_k + c, j] = d Wcat[h 2 d_k + d_k + c, f0 + j] / l_p
 *                (entries of d Wcat where Wcat is structurally zero are dropped), the k half and the biases likewise,
 *                d l_x = -(1 / l_x) sum (d Wcat . Wcat + d bcat . bcat) over the feature rows of both halves (double, fixed order), d l_p over the
 *                positional rows,   d ov_x = d output_var ov_p,   d ov_p = d output_var ov_x.
 * Returns GNPDE_EINVAL before any launch for null pointers, heads * d_k > 256 or f0 + p0 > d. */
int gnpde_split_kernel_grad_floats(int32_t heads, int32_t d_k, int32_t d);
int gnpde_split_kernel_grads(const float* grads_cat, const float* wcat, const float* bcat, const float* lengthscale_x,
                             const float* lengthscale_p, const float* output_var_x, const float* output_var_p, int32_t heads, int32_t d_k,
                             int32_t d, int32_t f0, int32_t p0, float* out, void* stream);

/* f(u) of a descriptor with an arbitrary epilogue / stage (building block of host-controlled adaptive
 * solvers); the epilogue's alpha / beta / x0 / alpha_sigmoid fields are taken from the descriptor. */
int gnpde_rhs_stage(const gnpde_rhs_t* rhs, const float* u, const gnpde_epilogue_t* epi, void* workspace,
                    size_t workspace_bytes, void* stream);

/* Error ratio of an embedded Runge-Kutta step, on device (torchdiffeq _compute_error_ratio with the rms norm):
 *   err = sum_j coef[j] * k[j],  tol = atol + rtol * max(|y0|, |y1|),  *ratio = sqrt(mean((err / tol)^2)).
 * Deterministic two-level reduction with the squares summed in double (the norm does not depend on the order of the rows beyond
 * ~1e-16, so a solve on a relabelled graph takes the same decisions); workspace: 4096 floats (16 KB), 8-byte aligned. */
int gnpde_rk_error_ratio(const float* y0, const float* y1, const float* const* k, const float* coef, int32_t n_k,
                         float atol, float rtol, int64_t n, int32_t d, int32_t ld, float* ratio, float* workspace,
                         void* stream);

/* End-point interpolation of an accepted Dormand-Prince step (torchdiffeq _interp_fit / _interp_evaluate, the quartic
 * through y0, y1, the mid-point estimate and the two end slopes) in one pass:
 *   y_mid = y0 + sum_j mid_coef[j] * k[j]   (7 stage derivatives; mid_coef[j] = fl32(c_mid_j) * fl32(dt))
 *   out   = value of the quartic at fraction x = (t_out - t0) / (t1 - t0) of the step, h = fl32(dt). */
int gnpde_dopri5_interp(const float* y0, const float* y1, const float* const* k, const float* mid_coef, float h, float x,
                        int64_t n, int32_t d, int32_t ld, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Early-stopping evaluator  [replaces EarlyStopRK4.evaluate / EarlyStopDopri5.evaluate + test / test_OGB + the
 * best-validation bookkeeping, reference src/early_stop_solver.py:100-128, :156-157, :178-218]
 *
 * After a solver step: logits = relu(y[:, 0:d_dec]) W^T + b, prediction = first arg-max over the classes,
 * hits counted per split; the step with the strictly largest validation count so far is remembered.  No host
 * synchronisation: the counters live in a device `state` of GNPDE_EARLY_STATE_INTS int32:
 *   [0..2] train / val / test hits of the latest evaluation
 *   [3..5] train / val / test hits of the best step     [6] its `step` tag     [7] evaluations done
 *   [8..]  scratch: per-block partial counts (summed in a fixed order, no atomics)
 * Accuracies are hits / split size (the host knows the sizes).  `trace` (nullable, [trace_capacity][4] int32)
 * receives {train, val, test, step} of every evaluation, in order.
 * ---------------------------------------------------------------------------------------------- */
#define GNPDE_EARLY_STATE_INTS (8 + 3 * 2048)

typedef struct {
  const float* weight;    /* device [n_classes, d_dec] row-major: nn.Linear weight of the decoder m2              */
  const float* bias;      /* device [n_classes] or NULL                                                            */
  const int32_t* labels;  /* device [n]                                                                            */
  const uint8_t* split;   /* device [n]: bit 0 train_mask, bit 1 val_mask, bit 2 test_mask                         */
  int32_t n_classes;      /* <= 64                                                                                 */
  int32_t d_dec;          /* decoder input width; < d when the state is augmented (early_stop_solver.py:180-181)   */
} gnpde_decoder_t;

int gnpde_early_stop_reset(int32_t* state, void* stream);
int gnpde_early_stop_eval(const gnpde_decoder_t* dec, const float* y, int32_t d, int32_t ld, int32_t n, int32_t step,
                          int32_t* state, int32_t* trace, int32_t trace_capacity, void* stream);

/* Attach the evaluator to a fixed-step solver: every gnpde_solver_run then resets `state`, and evaluates the
 * state after each step (step tag = 1-based index into the time grid), all inside the same hipGraph.  Call
 * before the first run or between runs (drops a captured graph); dec == NULL detaches. */
int gnpde_solver_set_early_stop(gnpde_solver_t* s, const gnpde_decoder_t* dec, int32_t* state, int32_t* trace,
                                int32_t trace_capacity);

/* out[i] = base[i] + sum_j coef[j] * v[j][i]  for i < n, n_v <= GNPDE_MAX_PREV (host arrays of device pointers /
 * coefficients): the stage algebra of host-driven Runge-Kutta loops (adjoint solve) in one pass.  out may alias
 * base or any v[j]. */
int gnpde_lincomb(const float* base, const float* const* v, const float* coef, int32_t n_v, int64_t n, float* out,
                  void* stream);

int gnpde_solver_num_rhs_evals(const gnpde_solver_t* s);
int gnpde_solver_destroy(gnpde_solver_t* s);

/* ------------------------------------------------------------------------------------------------
 * dopri5 with the step-size controller ON THE DEVICE  [replaces torchdiffeq 0.2.1 Dopri5Solver / RKAdaptiveStepsizeODESolver as
 * reached from ODEblock.forward with the reference's default opt['method'] = 'dopri5' (src/block_constant.py:57-62,
 * src/block_transformer_attention.py:58-63; the loop the reference re-states in src/early_stop_solver.py:30-128)]
 *
 * One TRIAL step -- first stage input, five evaluations of f whose epilogues form the next stage input, f(y1) (first-same-
 * as-last), the error ratio, the controller (accept / reject, step-size update in float64, end-point test), the quartic
 * end-point interpolation and the commit of the accepted state -- is captured ONCE as a hipGraph: the step size, the time, the
 * accept flag and the interpolation fraction live in device memory, the stage kernels read fl32(dt) through
 * gnpde_epilogue_t.coef_scale, interpolation and commit are predicated on device flags.  gnpde_dopri5_run replays that graph
 * `trials_per_sync` times between two reads of the controller state (one 64-byte copy), so the host neither launches kernels nor
 * decides anything per step; trial steps replayed after the end point has been reached leave every result untouched (they are
 * not counted).  Same rule as torchdiffeq: rms error norm, safety 0.9, factor limits 0.2 / 10, no shrinking after an accepted
 * step, Shampine's error weights, initial step of Hairer's heuristic as torchdiffeq selects it.
 *   y0 [n, ld_y0] in, y_out [n, ld_out] out (may alias y0); integrates from t0 to t1 > t0.
 *   max_evals > 0: stop launching once more evaluations than that were spent (reference opt['max_nfe']); *finished tells.
 * Synchronises the stream. */
typedef struct gnpde_dopri5 gnpde_dopri5_t;
size_t gnpde_dopri5_workspace_bytes(const gnpde_rhs_t* rhs);
int gnpde_dopri5_create(gnpde_dopri5_t** out, const gnpde_rhs_t* rhs, float rtol, float atol, void* workspace,
                        size_t workspace_bytes);
enum { GNPDE_ADAPTIVE_HEUN = 0, GNPDE_ADAPTIVE_DOPRI5 = 1 };
/* The embedded pair of the following runs: GNPDE_ADAPTIVE_DOPRI5 (default) or GNPDE_ADAPTIVE_HEUN -- torchdiffeq 0.2.1's
 * `adaptive_heun` (adaptive_heun.py; reference `--method adaptive_heun`, src/run_GNN.py): one evaluation per trial step, k1 = f(y + h k0),
 * y1 = y + h (k0 + k1) / 2, error h (k0 - k1) / 2, order 2 in the step-size rule and the initial step, the quartic end-point
 * interpolant through y + h k0 / 2, and k1 as the next step's first derivative (rk_common.py takes f1 = k[..., -1] for every pair).
 * Same controller record, batching and early stopping; the recorded solve (gnpde_dopri5_set_tape) is Dormand-Prince's only. */
int gnpde_dopri5_set_pair(gnpde_dopri5_t* s, int32_t pair);
int gnpde_dopri5_run(gnpde_dopri5_t* s, const float* y0, int32_t ld_y0, double t0, double t1, float* y_out, int32_t ld_out,
                     int32_t trials_per_sync, int32_t max_evals, int32_t* finished, void* stream);
/* Early stopping on the device controller  [replaces EarlyStopDopri5.advance + evaluate, reference src/early_stop_solver.py:
 * 82-128: the decoder, arg-max and split accuracies after EVERY trial step with three .item() reads, and the max_test_steps
 * cut].  The evaluator kernels (gnpde_early_stop_eval) are appended to the captured trial step and gated by the controller
 * record: an accepted step evaluates the new state with tag = number of accepted steps and its time goes to times[tag]
 * (times[0] = t0); trial steps rejected before the first accept evaluate the initial state once (tag 0); other rejected steps
 * re-evaluate nothing (the unchanged state cannot win the strict `val > best`).  After max_trial_steps trial steps the solve
 * stops and y_out is the state reached (reference :93-98), not an interpolation.  The host still only replays graphs and reads
 * the 96-byte record once per batch.  state / trace as in gnpde_solver_set_early_stop; dec == NULL detaches.  Call between
 * runs (drops the captured trial steps). */
int gnpde_dopri5_set_early_stop(gnpde_dopri5_t* s, const gnpde_decoder_t* dec, int32_t* state, int32_t* trace,
                                int32_t trace_capacity, double* times, int32_t times_capacity, int32_t max_trial_steps);
/* Node relabelling folded into the solve's own copies (graph.LocalityView of the Python layer: the fused solves run on the graph with
 * its nodes relabelled; no reference equivalent): order[r] = the caller's row that solver row r holds (device, int32 [n], must outlive the
 * runs).  gnpde_dopri5_run then reads y0[order[r]] into its row r and writes its row r to y_out[order[r]] (y_out must not alias y0
 * then).  NULL restores the plain copies. */
int gnpde_dopri5_set_row_order(gnpde_dopri5_t* s, const int32_t* order);
/* Outputs at several times  [torchdiffeq 0.2.1 RKAdaptiveStepsizeODESolver: the steps are those of the solve from t0 to t1 -- they
 * never look at the output times -- and output j is the quartic interpolant (interp.py) of the first accepted step [t_prev, t_next] with
 * t_next >= t_out[j], at x = fl32((t_out[j] - t_prev) / (t_next - t_prev)), the quotient in float64].  t_out: device doubles [n_out],
 * strictly ascending, all behind the t0 of the runs, t_out[n_out - 1] == the t1 of the runs (gnpde_dopri5_run checks: GNPDE_EINVAL); out:
 * n_out slabs [n, ld_out].  An emit kernel between the control and the finish kernel of the captured trial step, predicated on the
 * controller record (a rejected step writes nothing), writes out[j] of every pending j < n_out - 1 with t_out[j] <= the new time -- any
 * number per step, through the row order if one is set; the pending index and the step's start time live in a 32-byte device record of
 * their own (the 96-byte controller record is unchanged).  The last output is y_out of gnpde_dopri5_run, as without outputs (slab
 * n_out - 1 is not written).  Both pairs.  t_out == NULL or n_out == 0 detaches.  Attaching, detaching or other pointers drop the captured
 * trial steps (other times behind the same pointers do not); reads t_out[n_out - 1] back (synchronises).  GNPDE_EINVAL with a message
 * together with a tape, the early-stopping evaluator (either order of the calls) or a row-partitioned solver. */
int gnpde_dopri5_set_outputs(gnpde_dopri5_t* s, const double* t_out, int32_t n_out, float* out, int32_t ld_out);
/* of the last run: evaluations of f, accepted and rejected steps, graph launches, host synchronisations */
int gnpde_dopri5_stats(const gnpde_dopri5_t* s, int32_t* n_evals, int32_t* n_accepted, int32_t* n_rejected, int32_t* n_launches,
                       int32_t* n_syncs);
int gnpde_dopri5_destroy(gnpde_dopri5_t* s);
/* Recorded solve + reverse sweep  [replaces what torch autograd does when the reference trains with opt['adjoint'] = False -- its
 * default, and its Cora / Citeseer best_params (src/base_classes.py:44-47, src/best_params.py) -- i.e. `loss.backward()` through
 * every accepted step of torchdiffeq's dopri5 (rk_common.py _runge_kutta_step, interp.py), with the step sizes constants of the
 * backward pass (misc.py _optimal_step_size runs under torch.no_grad)].  The sweep here is GRAND-l's (f linear in the state; the
 * edge weights are constants of the solve that carry gradients: src/block_transformer_attention.py:36-72); a GRAND-nl / GAT solve is
 * recorded the same way -- stage inputs only -- and swept by gnpde_adjoint_set_dopri5_tape + gnpde_adjoint_run.
 *   gnpde_dopri5_set_tape       ZERO-FILLED device memory of gnpde_dopri5_tape_bytes(rhs, capacity_steps) bytes, 256-byte aligned;
 *                               every ACCEPTED trial step of the following runs leaves its stage inputs u_0..u_5 (and y1 as u_0 of
 *                               the next slot) and its step size there (one copy kernel inside the captured trial step, gated by the
 *                               controller record).  A run that accepts more than capacity_steps steps returns GNPDE_EWS.  NULL
 *                               detaches.  Call between runs (drops the captured trial steps).
 *   gnpde_dopri5_tape_steps     accepted steps of the last recorded run that reached t1 (0: nothing to differentiate)
 *   gnpde_dopri5_tape_backward  given dL/d(y_out) of the LAST run (grad_out [n, ld_go]): dL/dy0 -> grad_y0 [n, ld_gy0];
 *                               r_t [e] = sum over all 6 S + 1 evaluations k = f(u) of  u[row'] . G[col']  in the CSR order of
 *                               graph_t (G = gradient reaching k): dL/dw_e = alpha' r; sum_g [n, ld] = sum of the G (dL/dbeta =
 *                               <sum_g, x0>); dot_out[0] = sum <G, k - beta x0> (dL/dalpha_train = that * (1 - alpha') under the
 *                               sigmoid).  graph_t / w_t: the transposed graph (gnpde_graph_t of the flipped edge list) and the weights
 *                               of the descriptor in ITS CSR order.  One launch of the fused row kernel per evaluation + two small
 *                               combinations per step, no host synchronisation; the algebra is written out in oracle/tape_reverse.py. */
size_t gnpde_dopri5_tape_bytes(const gnpde_rhs_t* rhs, int32_t capacity_steps);
int gnpde_dopri5_set_tape(gnpde_dopri5_t* s, void* tape, size_t tape_bytes, int32_t capacity_steps);
int gnpde_dopri5_tape_steps(const gnpde_dopri5_t* s);
/* host arrays: the float32 step sizes of the accepted steps of the last recorded run and the fraction of the last step at which t1 lies */
int gnpde_dopri5_tape_record(const gnpde_dopri5_t* s, float* h_out, int32_t capacity, float* x_out);
/* where the record lies: *slots = buffer 0 of the attached tape (buffer 6 s + i = u_i of accepted step s), *slot_stride = floats between
 * consecutive buffers; GNPDE_EINVAL without a tape */
int gnpde_dopri5_tape_slots(const gnpde_dopri5_t* s, const float** slots, size_t* slot_stride);
size_t gnpde_dopri5_tape_backward_workspace_bytes(const gnpde_dopri5_t* s, const gnpde_graph_t* graph_t);
int gnpde_dopri5_tape_backward(gnpde_dopri5_t* s, const gnpde_graph_t* graph_t, const float* w_t, const float* grad_out,
                               int32_t ld_go, float* grad_y0, int32_t ld_gy0, float* r_t, float* sum_g, float* dot_out,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adjoint with an ADAPTIVE adjoint method, the controller ON THE DEVICE  [replaces torchdiffeq 0.2.1's odeint_adjoint backward pass
 * with `adjoint_method` 'adaptive_heun' -- the reference's DEFAULT (src/run_GNN.py:334; best_params Pubmed) -- or 'dopri5' (best_params
 * CoauthorCS, Computers) as reached from src/base_classes.py:44-47: the augmented state (vjp_t, y, a, g_theta) integrated backwards as one
 * flat vector through autograd (adjoint.py augmented_dynamics), AdaptiveHeunSolver / Dopri5Solver with the mixed norm of misc.py]
 *
 * GRAND-l descriptors only: for f(u) = alpha' (A u - u) + beta x0 the system decouples (reversed time s = -t) into
 *   y' = -f(y),  a' = alpha' (A^T a - a),  g_alpha' = (1 - alpha') <a, f(y) - beta x0>,  g_beta' = <a, x0>.
 * One TRIAL step of the embedded pair = one hipGraph: per stage the fused row kernel on the graph (f at the stage input, the next stage
 * input in its epilogue, the dots) and the aggregation on the transposed graph, then two error norms, control, finish
 * (csrc/adjoint_adaptive.hip); accept / reject, step size (float64), mixed norm (largest of rms(y), rms(a), |g_alpha|, |g_beta| errors
 * over their tolerances), end-point interpolation decided by kernels from a 112-byte record the host reads once per batch of trial steps.
 * torchdiffeq's rule throughout (safety 0.9, factors 0.2 / 10, the pair's order, the last stage derivative carried over as the next
 * step's first).
 *   rhs: f on the graph (kind GNPDE_RHS_LAPLACIAN; x0 / beta optional); graph_t / w_t: the transposed graph and the weights in ITS CSR
 *   order; method: GNPDE_ADAPTIVE_*; rtol / atol: the adjoint tolerances.
 *   gnpde_adjoint_adaptive_run: y [n, ld_y] = the state at the LATER time (read), a [n, ld_a] in: dL/dy there, out: at the earlier time;
 *   g (device float[2]) in / out: accumulated (g_alpha, g_beta); integrates s from s0 to s1 > s0 (= -t) starting with step dt0 (the
 *   caller selects it: misc.py _select_initial_step, two evaluations).  max_evals / *finished as gnpde_dopri5_run.  Synchronises the stream
 *   while it runs (one read per batch); the final copies are queued behind. */
/* (GNPDE_ADAPTIVE_HEUN / GNPDE_ADAPTIVE_DOPRI5: declared with gnpde_dopri5_set_pair above) */
typedef struct gnpde_adjoint_adaptive gnpde_adjoint_adaptive_t;
size_t gnpde_adjoint_adaptive_workspace_bytes(const gnpde_rhs_t* rhs, const gnpde_graph_t* graph_t, int32_t method);
int gnpde_adjoint_adaptive_create(gnpde_adjoint_adaptive_t** out, const gnpde_rhs_t* rhs, const gnpde_graph_t* graph_t, const float* w_t,
                                  int32_t method, float rtol, float atol, void* workspace, size_t workspace_bytes);
int gnpde_adjoint_adaptive_run(gnpde_adjoint_adaptive_t* s, const float* y, int32_t ld_y, float* a, int32_t ld_a, float* g, double s0,
                               double s1, double dt0, int32_t trials_per_sync, int32_t max_evals, int32_t* finished, void* stream);
int gnpde_adjoint_adaptive_stats(const gnpde_adjoint_adaptive_t* s, int32_t* n_evals, int32_t* n_accepted, int32_t* n_rejected,
                                 int32_t* n_launches, int32_t* n_syncs);
int gnpde_adjoint_adaptive_destroy(gnpde_adjoint_adaptive_t* s);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU halo exchange helpers (row-partitioned graph, one process per GPU, RCCL between).
 * ---------------------------------------------------------------------------------------------- */
/* dst[i, 0:d] = src[idx[i], 0:d]  for i < count  (pack boundary rows into a send buffer)        */
int gnpde_gather_rows(const float* src, int32_t ld_src, const int32_t* idx, int32_t count, int32_t d,
                      float* dst, int32_t ld_dst, void* stream);

/* Measurement aid, no reference equivalent (bench.py's `roofline.ceiling`): out[i] = sum_{t<k} table[idx[i*k + t]] for
 * i < n_out -- a perfectly balanced gather of whole rows of d floats (d % 4 == 0, <= 256) with the row width, table and launch
 * geometry of the aggregation kernels and no arithmetic but the adds.  Its rate on the table and mean degree of a workload is
 * the ceiling the aggregation is reported against when the gathered table is cache-resident (torch_sparse.spmm's gather,
 * src/function_transformer_attention.py:25-36, stripped of everything else). */
int gnpde_gather_ceiling(const float* table, int32_t n_rows, int32_t d, int32_t ld, const int32_t* idx, int32_t k,
                         float* out, int32_t n_out, int32_t variant /* 0: ids loaded per lane, 1: coalesced + shuffle */, void* stream);

/* Measurement aid, no reference equivalent (bench.py's `roofline.stream_read_probe`): a coalesced streaming read of
 * n_floats floats, `passes` times inside one launch (16-byte lanes, grid stride, eight loads in flight per lane), one float
 * per workgroup written to sink
 * (n_sink >= 2048).  The rate the memory side delivers L2-cold lines of a table at -- the hardware ceiling next to which the
 * aggregation's gather of the same table (torch_sparse.spmm's index_select, src/function_transformer_attention.py:25-36) is
 * reported when that table is resident in the Infinity Cache. */
int gnpde_stream_read(const float* table, int64_t n_floats, int32_t passes, float* sink, int32_t n_sink, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge-set bookkeeping of the hard-attention / rewiring blocks (once per training forward):
 *   threshold = torch.quantile(score, q);  mask = score > threshold;  edge_index[:, mask];  kept scores renormalised by their
 *   sum per endpoint (reference src/block_transformer_hard_attention.py:48-66, src/block_transformer_rewiring.py:40-50,154-183).
 * gnpde_quantile: *out (device) = the q-quantile of v[0..n) with torch.quantile's default linear interpolation, evaluated in
 *   float32 exactly as torch does (rank = fl32(q) * fl32(n-1)); a radix select, no sort; n is not limited to 16 M.
 * gnpde_threshold_edges: stable compaction of the columns of edge_index ([2, n_edges] int64, row-major) whose score exceeds
 *   *threshold (device scalar) into out_edge_index ([2, n_edges] capacity, same row stride), out_weight[i] = score / (sum of the
 *   kept scores with the same endpoint edge_index[norm_idx] + 1e-16); *out_count (device int64) = number of kept edges.
 * ---------------------------------------------------------------------------------------------- */
size_t gnpde_quantile_workspace_bytes(void);
int gnpde_quantile(const float* v, int64_t n, double q, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The same radix select with the CALLER's two ranks (ascending, 0 = the smallest) over values fed piece by piece: begin; then for
 * pass = 0 .. 3: gnpde_rank_select_hist over every piece (it adds to the state), gnpde_rank_select_pick; then
 * gnpde_rank_select_values: out[0], out[1] (device) = the order statistics of rank k0, k1 among everything fed.  The pieces must be
 * the same in every pass; ranks at or past the number of values fed give an unspecified value.  The totals are counted in 64
 * bits (any number of pieces); one piece holds at most 2^32 values (GNPDE_ESHAPE).  Workspace: gnpde_quantile's.
 * (torch_geometric's GDC.__calculate_eps__ sorts all values; graph diffusion rewiring's threshold by avg_degree uses this.) */
int gnpde_rank_select_begin(int64_t k0, int64_t k1, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_rank_select_hist(const float* v, int64_t n, int32_t pass, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_rank_select_pick(int32_t pass, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_rank_select_values(float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t gnpde_threshold_edges_workspace_bytes(int64_t n_edges, int32_t n_nodes);
int gnpde_threshold_edges(const int64_t* edge_index, const float* score, int64_t n_edges, const float* threshold,
                          int32_t norm_idx, int32_t n_nodes, int64_t* out_edge_index, float* out_weight, int64_t* out_count,
                          void* workspace, size_t workspace_bytes, void* stream);

/* k-nearest-neighbour rewiring in feature space (BLEND, `--rewire_KNN`; reference src/graph_rewiring.py:120-126, a pykeops
 * LazyTensor.argKmin):  for every row i of x ([n, d] fp32, row stride ldx >= d) the k smallest D_ij = |x_i - x_j|^2 over ALL j, the
 * diagonal included, as idx [n, k] int64 and (dist != NULL) dist [n, k] fp32.  One fused kernel forms the distance tiles on the fp32
 * matrix cores (D = |x_i|^2 + |x_j|^2 - 2 x_i.x_j, clamped at 0, D_ii = 0 exactly) and selects in LDS; no [n, n] or [chunk, n] array
 * is written.  A row's result is ascending by the computed distance, equal distances by ascending column (KeOps leaves tie order
 * unspecified; this is this library's definition); no atomics: bit-identical from run to run.  For few rows the column range is
 * split S ways over workgroups (partial lists in the workspace, then a merge launch); S follows from n and the CU count, or from
 * gnpde_tune(19, S).  The workspace size depends on S: query it after any gnpde_tune call (it serves either metric of gnpde_knn_metric).
 * Limits: 1 <= k <= min(n, 128), d >= 1, n <= INT32_MAX; otherwise GNPDE_ESHAPE / GNPDE_EINVAL (gnpde_knn_workspace_bytes: 0). */
size_t gnpde_knn_workspace_bytes(int64_t n, int32_t d, int32_t k);
int gnpde_knn(const float* x, int32_t n, int32_t d, int32_t ldx, int32_t k, int64_t* idx, float* dist, void* workspace,
              size_t workspace_bytes, void* stream);

/* Positional-distance rewiring (BLEND, `--rewiring pos_enc_knn`; reference src/graph_rewiring.py:285-342 with
 * src/hyperbolic_distances.py:7-14 and src/distances_kNN.py: scipy pdist + squareform, a dense float64 [n, n] matrix, np.quantile and
 * sklearn's NearestNeighbors(metric='precomputed')).  Every selection here works on the KEY of a pair, formed tile by tile on the fp32
 * matrix cores and never stored:
 *   GNPDE_METRIC_SQEUCLIDEAN  key_ij = D_ij = (s_i + s_j) - 2 x_i.x_j clamped at 0, D_ii = 0 exactly; s_i the fp32 squared norm of the
 *                             pre-pass (gnpde_knn's key).  Distance: sqrt(D) (gnpde_knn itself returns D, as it always has).
 *   GNPDE_METRIC_POINCARE     key_ij = r_ij = fl(D_ij / fl(a_i a_j)), ONE IEEE fp32 division, with a_i = max(1 - s_i, 2^-24) (2^-24 is
 *                             the smallest positive value 1 - s takes in fp32; the reference clamps at the float64 epsilon), r_ii = +0.
 *                             The hyperbolic distance arccosh(1 + 2 r) is monotone in r, so selections order and compare keys and
 *                             never distances; where a distance is returned it is log1pf(2 r + 2 sqrtf(r (r + 1))).
 * Inputs must be finite.  Rows on or outside the unit ball get the clamp, as in the reference, not an error.  Keys are non-negative
 * floats: their bit patterns order as unsigned integers.  key_ij is bit-identical to key_ji: the products are the same, the k order
 * is the same and the additions commute.
 *
 * gnpde_knn_metric: gnpde_knn (below) on the keys of `metric`; dist holds the distance of the key as defined above (metric 0: D).
 * gnpde_knn forwards metric 0 and is bit for bit what it was.
 *
 * Radius graph: the edge set {(i, j) : key_ij <= tau}, self loops included, as edge_index [2, E] int64 sorted by (row, column) -- what
 * np.where(dist <= thresh) gives.  tau is the caller's key, or the quantile key: the key of rank lo = floor((n^2 - 1) q) (rank 0 is the
 * smallest; the arithmetic is in host double, as numpy does it) among all n^2 keys, the diagonal included.  That selects the set
 * np.quantile's linearly interpolated threshold t selects: t lies in [v_lo, v_lo+1) (it is v_lo + g (v_lo+1 - v_lo) with 0 <= g < 1) and
 * no key lies strictly between two consecutive order statistics, so {key <= t} = {key <= v_lo}.  The tau that is returned is that lower
 * order statistic v_lo, not numpy's interpolated number.
 *   gnpde_radius_quantile  three sweeps of the tile pipeline (radix select over 11 / 11 / 10 key bits; LDS histograms flushed with
 *                          64-bit integer atomics, whose sums do not depend on the order of arrival; a one-wave kernel between the
 *                          sweeps; no host read) -> tau_out (DEVICE, two floats: the key tau and its distance)
 *   gnpde_radius_count     rowptr [n + 1] (device int64; rowptr[n] = E) for tau = tau_dev[0] (device, e.g. tau_out) or, tau_dev NULL,
 *                          tau_key; the caller reads E and allocates
 *   gnpde_radius_fill      must follow the count of the SAME x, tau, workspace and gnpde_tune state on the same stream:
 *                          out_edge_index ([2, out_ld] int64, row-major, out_ld >= E), a row's columns ascending.  No atomics.
 * For few row tiles the column range is split S ways (gnpde_tune(19, S) forces S); per-split per-row counts place the entries, so the
 * result is a pure function of the input: bit-identical from run to run and for every S.  The workspace size depends on S.
 * Limits: n <= INT32_MAX, q in [0, 1], a known metric (GNPDE_ESHAPE otherwise; gnpde_radius_workspace_bytes: 0); the row scan of the
 * count is one workgroup (sized for graphs of up to a few million nodes). */
#define GNPDE_METRIC_SQEUCLIDEAN 0
#define GNPDE_METRIC_POINCARE    1
int gnpde_knn_metric(const float* x, int32_t n, int32_t d, int32_t ldx, int32_t k, int32_t metric, int64_t* idx, float* dist,
                     void* workspace, size_t workspace_bytes, void* stream);
size_t gnpde_radius_workspace_bytes(int64_t n, int32_t d);
int gnpde_radius_quantile(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t metric, double q, float* tau_out,
                          void* workspace, size_t workspace_bytes, void* stream);
int gnpde_radius_count(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t metric, const float* tau_dev, float tau_key,
                       int64_t* rowptr, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_radius_fill(const float* x, int64_t n, int32_t d, int32_t ldx, int32_t metric, const float* tau_dev, float tau_key,
                      int64_t* out_edge_index, int64_t out_ld, void* workspace, size_t workspace_bytes, void* stream);

/* Edge-sampling rewiring of BLEND's fully-adjacent layer (`--fa_layer`; reference src/graph_rewiring.py:150-241 add_edges /
 * add_outgoing_attention_edges / edge_sampling, called by src/GNN_KNN.py:65-83 inside every forward).  The reference composes
 * np.random.choice, torch.multinomial, torch.unique(dim=1), torch.quantile (16 M element limit) and a boolean mask.
 *
 * Random numbers: Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; the Random123 generator), written out in the kernel.
 *   key = (seed low word, seed high word);  counter = (block low word, block high word, stream, call);
 *   word i of a stream = word (i & 3) of block (i >> 2).  `stream` separates the two endpoints of a pair (0 = anchors / first
 *   endpoints, 1 = partners), `call` separates successive add_edges calls of one model.  A word is a pure function of
 *   (seed, stream, call, i): results do not depend on the launch shape and are the same on every device.
 *   gnpde_philox_words   out[w] = word (w & 3) of block first_block + (w >> 2), w in [0, n_words)   (for tests of the generator)
 *   gnpde_random_nodes   out[i] = (word_i * n) >> 32 in exact integer arithmetic: uniform over [0, n), 1 <= n <= INT32_MAX
 * gnpde_node_importance  out[j] = (sum of att_mean over the edges whose column is j) / (their number); att_mean [E] is in the
 *   caller's edge order, g the graph of that edge list with its CSC view.  One wave per column: lane l adds the column's entries
 *   l, l + 64, ... in CSC order, then a fixed butterfly adds the 64 partial sums, so a hub column is 64 fixed chunks combined in a
 *   fixed order.  No atomics on floats: bit-identical from run to run.  A column without entries (0 / 0 in the reference, which
 *   then fails inside multinomial) sets GNPDE_SAMPLING_EMPTY_COLUMN in *flag and gives 0.
 * gnpde_sample_nodes     `count` draws with replacement from softmax(logits) over n nodes, in fixed point:
 *     t_j = expf(s_j - max s) in fp32;  w_j = (uint64)(t_j 2^32)  (the scaling is exact; the maximum contributes exactly 2^32);
 *     C = inclusive prefix sums of w in uint64 -- integer addition is associative, so any scan order gives the same bits;
 *     draw i: r = (word 2i << 32) | word (2i + 1),  target = high 64 bits of r * C_n,  answer = the first j with C_j > target
 *     (binary search).  A node of weight 0 is never drawn.  A non-finite logit sets GNPDE_SAMPLING_NONFINITE, C_n == 0 sets
 *     GNPDE_SAMPLING_ZERO_MASS (the draws are then 0 and meaningless).
 * gnpde_edge_union       the ascending unique columns of cat(a, b) -- what torch.unique(cat, dim=1) returns: columns ordered by
 *   (row, col).  a [2, n_a], b [2, n_b] int64 row-major; keys row * n_nodes + col in 64 bits, radix sort, unique, decode.
 *   out_edge_index is [2, n_a + n_b] (row stride n_a + n_b), its first *out_count (device int64) columns are written.  An index
 *   outside [0, n_nodes) sets GNPDE_SAMPLING_INDEX_RANGE.
 * gnpde_select_edges     stable compaction of the columns of edge_index ([2, n_edges], row-major) whose score is >= *threshold
 *   (device scalar) into out_edge_index ([2, n_edges] capacity, same row stride); *out_count (device int64) = number kept.
 *   No weights and no renormalisation (gnpde_threshold_edges keeps its `>` and its renormalisation).  NaN scores are dropped.
 * gnpde_full_adjacency   out [2, n^2]: column i n + j = (i, j), the diagonal included (reference src/utils.py:161-167).
 * `flag` is ONE device int32 that the kernels OR bits into; the caller zeroes it and reads it.  Everything runs on the caller's
 * stream; argument errors return a code before any launch.  A workspace query returns 0 (and the entry point GNPDE_ESTATE) when
 * the sort's / scan's own temporary-storage query fails. */
#define GNPDE_SAMPLING_EMPTY_COLUMN 1
#define GNPDE_SAMPLING_NONFINITE    2
#define GNPDE_SAMPLING_ZERO_MASS    4
#define GNPDE_SAMPLING_INDEX_RANGE  8
int gnpde_philox_words(uint64_t seed, uint32_t stream_id, uint32_t call, uint64_t first_block, int64_t n_words, uint32_t* out,
                       void* stream);
int gnpde_random_nodes(int32_t n, int64_t count, uint64_t seed, uint32_t stream_id, uint32_t call, int64_t* out, void* stream);
int gnpde_node_importance(const gnpde_graph_t* g, const float* att_mean, float* out, int32_t* flag, void* stream);
size_t gnpde_sample_nodes_workspace_bytes(int32_t n);
int gnpde_sample_nodes(const float* logits, int32_t n, int64_t count, uint64_t seed, uint32_t stream_id, uint32_t call, int64_t* out,
                       int32_t* flag, void* workspace, size_t workspace_bytes, void* stream);
size_t gnpde_edge_union_workspace_bytes(int64_t n_a, int64_t n_b);
int gnpde_edge_union(const int64_t* a, int64_t n_a, const int64_t* b, int64_t n_b, int32_t n_nodes, int64_t* out_edge_index,
                     int64_t* out_count, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream);
size_t gnpde_select_edges_workspace_bytes(int64_t n_edges);
int gnpde_select_edges(const int64_t* edge_index, const float* score, int64_t n_edges, const float* threshold,
                       int64_t* out_edge_index, int64_t* out_count, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_full_adjacency(int32_t n, int64_t* out_edge_index, void* stream);

/* DeepWalk positional encodings (BLEND's `--pos_enc_type DW<d>`; reference src/deepwalk_embeddings.py: torch_geometric's Node2Vec
 * with p = q = 1, sparse embedding, torch.optim.SparseAdam).  This header is the authority; PyG and torch_cluster are no dependency.
 *
 * Graph.  CSR over n nodes: rowptr [n + 1] and col [n_edges] int32.  The out-neighbours of u are the `dst` of the caller's edges
 *   (u, dst), WITH multiplicity, ascending by dst (ops.walk_csr builds it).  A node of out-degree 0 stays where it is (torch_cluster).
 * Random numbers.  The Philox4x32-10 streams defined above.  Stream ids 0 and 1 belong to the edge sampling; the trainer uses
 *   16 (positive walks), 17 (negative walks) and 18 (epoch order).
 * Positive walk w, step t (0 <= t < L = walk_length, 1 <= L <= 127):
 *     word(w, t) = word (t & 3) of block  w * ceil(L / 4) + (t >> 2)  of stream (seed, stream_id, call)     (64-bit block number)
 *     next = col[rowptr[cur] + ((word * deg(cur)) >> 32)]
 *   out [n_walks, L + 1] int32, column 0 the start node.  Walk r of a call is w = first_walk + r and starts at starts[r % n_starts]
 *   (PyG's batch.repeat): batches of one epoch draw from disjoint counter ranges.
 * Negative walk: column 0 the start node, column t + 1 = (word(w, t) * n) >> 32, on a stream id of its own.
 * Epoch order.  gnpde_random_permutation: out = the indices i in [0, n) sorted by the 64-bit key (word i of the stream) << 32 | i
 *   (radix sort), int64.
 * Epoch e, batch b of size B (the last may be short): the start of walk r is perm[b B + (r mod |batch|)], r < |batch| walks_per_node
 *   positive and r < |batch| walks_per_node num_negative_samples negative walks; call = e; first_walk = b B walks_per_node for the
 *   positive walks and that times num_negative_samples for the negative ones.
 * Windows (C = context_size, walk_length >= C >= 2): J = L + 2 - C windows per walk; a walk contributes the position pairs (a, b)
 *   with 0 <= a < J and a < b <= a + C - 1 -- the pairs (first column, other column) of PyG's cat([rw[:, j:j + C] for j in range(J)]).
 * Loss of one step: x_ab = <e[rw[a]], e[rw[b]]>, EPS = 1e-15,
 *     loss = mean over all positive pairs of -log(sigma(x) + EPS)  +  mean over all negative pairs of -log(sigma(-x) + EPS).
 *   PyG writes the negative term as log(1 - sigma(x) + EPS); in fp32 that is log(EPS) once x > ~17.  The step follows the mathematics.
 * Update (torch.optim.SparseAdam): g = the gradient summed per distinct touched row (a pair with rw[a] == rw[b] contributes to that
 *   row twice); only touched rows change:  m <- m + (g - m)(1 - beta1),  v <- v + (g g - v)(1 - beta2),
 *     e <- e - lr sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps),   t = the global step count from 1.
 *   An untouched row keeps its e, m and v bit for bit.
 * gnpde_deepwalk_step: emb [n, d] (row stride ld), m and v [n, d] (row stride ld_mv) float32, 16-byte aligned, strides multiples of 4;
 *   pos_rw [r_pos, L + 1] and neg_rw [r_neg, L + 1] int32 (given, so that a test can feed walks); *loss_out (device float) = the loss.
 *   One wave per walk stages the walk's rows in LDS and writes ONE contribution row per walk position with plain stores; a radix
 *   sort of (node << 32 | slot) is the inverted index; per node the contribution rows are added in slot order.  No float atomics:
 *   results are bit-identical from run to run.  Nothing is read by the host.
 *   Limits (GNPDE_ESHAPE otherwise): d a multiple of 4 in 4 .. 256, L <= 127, 2 <= C <= L, (L + 1) d + J (C - 1) <= 16384 floats
 *   (64 KiB of LDS: the rows and the pair coefficients), (r_pos + r_neg)(L + 1) <= INT32_MAX.
 * `flag` is ONE device int32 that the kernels OR bits into; the caller zeroes it and reads it: a start node or a walk entry outside
 *   [0, n) (it then counts as node 0), a rowptr / col entry outside the graph (the walk then stays).
 * Everything runs on the caller's stream; argument errors return a code before any launch.  A workspace query returns 0 for
 * arguments the entry point refuses. */
#define GNPDE_DEEPWALK_BAD_START 1
#define GNPDE_DEEPWALK_BAD_GRAPH 2
#define GNPDE_DEEPWALK_BAD_WALK  4
int gnpde_random_walks(const int32_t* rowptr, const int32_t* col, int64_t n_edges, int32_t n, const int64_t* starts, int64_t n_starts,
                       int64_t n_walks, int32_t walk_length, uint64_t seed, uint32_t stream_id, uint32_t call, uint64_t first_walk,
                       int32_t* out, int32_t* flag, void* stream);
int gnpde_negative_walks(int32_t n, const int64_t* starts, int64_t n_starts, int64_t n_walks, int32_t walk_length, uint64_t seed,
                         uint32_t stream_id, uint32_t call, uint64_t first_walk, int32_t* out, int32_t* flag, void* stream);
size_t gnpde_random_permutation_workspace_bytes(int64_t n);
int gnpde_random_permutation(int64_t n, uint64_t seed, uint32_t stream_id, uint32_t call, int64_t* out, void* workspace,
                             size_t workspace_bytes, void* stream);
size_t gnpde_deepwalk_step_workspace_bytes(int64_t r_pos, int64_t r_neg, int32_t walk_length, int32_t context_size, int32_t d);
int gnpde_deepwalk_step(float* emb, int32_t ld, float* m, float* v, int32_t ld_mv, int32_t n, int32_t d, int32_t t,
                        const int32_t* pos_rw, int64_t r_pos, const int32_t* neg_rw, int64_t r_neg, int32_t walk_length,
                        int32_t context_size, float lr, float beta1, float beta2, float eps, float* loss_out, int32_t* flag,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Hyperbolic positional encodings (BLEND's `--pos_enc_type HYPS<dd>`; the reference loads such files and ships no program that
 * writes them).  This header is the authority: an embedding of the nodes in the Poincare ball, trained on DeepWalk's walks.
 *
 * State.  e [n, d] float32, every row strictly inside the unit ball.  No optimiser state.
 * Walks, negative walks, epoch order, batches and windows: the DeepWalk definitions above, word for word (gnpde_random_walks,
 *   gnpde_negative_walks, gnpde_random_permutation, the position pairs (a, b)), on stream ids of their own: 19 (positive walks),
 *   20 (negative walks), 21 (epoch order), so that a DeepWalk run and a hyperbolic run of one seed share no random numbers.
 * Pair (u, v) = (rw[a], rw[b]):
 *     s_u = |e_u|^2,  alpha = 1 - s_u,  beta = 1 - s_v,  q = |e_u - e_v|^2,  r = q / (alpha beta)     (the key of gnpde_knn_metric's
 *                                                                                                      GNPDE_METRIC_POINCARE)
 *     dist = arccosh(1 + 2 r), evaluated as 2 log(sqrt(r) + sqrt(1 + r))                               (no cancellation at small r)
 *     x = (R - dist) / T                                                                                (radius R, temperature T)
 *     d dist / d e_u = 1 / sqrt(r (1 + r)) * 2 / (alpha beta) * [(e_u - e_v) + (q / alpha) e_u],   and with u, v and alpha, beta
 *       exchanged for e_v.
 *   A pair with r == 0 exactly (the same node, or identical coordinates) has a zero gradient; its loss term counts with dist = 0.
 * Loss of one step (reported only), EPS = 1e-15:
 *     mean over all positive pairs of -log(sigma(x) + EPS)  +  mean over all negative pairs of -log(sigma(-x) + EPS).
 * Update: row-normalised Riemannian SGD.  For every touched row u
 *     g_u = the sum over all pair ends at u, positive and negative, of the derivative of THAT PAIR'S OWN loss term (EPS included,
 *           no 1 / count factor) with respect to e_u, added in a fixed order;
 *     c_u = the number of pair ends at u (a pair with rw[a] == rw[b] counts twice);
 *     e_u <- proj(e_u - lr (alpha_u^2 / 4) g_u / c_u),     proj(y) = y if |y| < 1 - 1e-5, else y (1 - 1e-5) / |y|.
 *   alpha_u^2 / 4 is the inverse of the ball's metric; the Euclidean length of d dist / d e_u is 2 / alpha_u and |d loss / d x| < 1,
 *   so one update moves a row by less than lr alpha_u / (2 T), whatever the batch size and however often the node occurs.
 *   An untouched row keeps its bits.
 * gnpde_poincare_step: emb [n, d] (row stride ld) float32; d = 2 (ld even, emb 8-byte aligned) or a multiple of 4 (ld a multiple
 *   of 4, emb 16-byte aligned); pos_rw [r_pos, L + 1] and neg_rw [r_neg, L + 1] int32; *loss_out (device float) = the loss.
 *   The layout of gnpde_deepwalk_step: one wave per walk stages the walk's rows in LDS (a width of 2 padded to 4), forms s per
 *   position and (q, coefficient) per pair, and writes ONE contribution row per walk position with plain stores; a radix sort of
 *   (node << 32 | slot) is the inverted index; per node the contribution rows are added in slot order and c_u is the sum of the
 *   slots' pair-end counts, a function of (position, L, C) alone.  No float atomics: results are bit-identical from run to run.
 *   Nothing is read by the host.  sqrt and the divisions are IEEE.  A walk entry outside [0, n) sets GNPDE_DEEPWALK_BAD_WALK in
 *   `flag` and counts as node 0.
 *   Limits (GNPDE_ESHAPE otherwise): d = 2 or a multiple of 4 in 4 .. 128, L <= 127, 2 <= C <= L, DeepWalk's 64 KiB of LDS per walk,
 *   which here hold (L + 1) max(d, 4) row floats, L + 1 norms and 2 J (C - 1) pair coefficients, each of the four blocks rounded up
 *   to 4 floats: at most 16384 floats together; (r_pos + r_neg)(L + 1) <= INT32_MAX.  lr >= 0 and T > 0 (GNPDE_EINVAL otherwise). */
size_t gnpde_poincare_step_workspace_bytes(int64_t r_pos, int64_t r_neg, int32_t walk_length, int32_t context_size, int32_t d);
int gnpde_poincare_step(float* emb, int32_t ld, int32_t n, int32_t d, const int32_t* pos_rw, int64_t r_pos, const int32_t* neg_rw,
                        int64_t r_neg, int32_t walk_length, int32_t context_size, float lr, float radius, float temperature,
                        float* loss_out, int32_t* flag, void* workspace, size_t workspace_bytes, void* stream);

/* NMF compression of positional encodings (reference src/pos_enc_factorisation.py: sklearn.decomposition.NMF(solver='cd',
 * beta_loss='frobenius'), no regularisation, shuffle off).  This header is the authority; sklearn is no dependency.
 *   X [n, m] >= 0 is approximated by W [n, k] H [k, m], W, H >= 0.  One iteration is two half-sweeps of one kind:
 *     update W  with  G = H H^T [k, k]  and  P = X H^T [n, k];      update H^T [m, k]  with  G = W^T W  and  P = X^T W.
 *   gnpde_nmf_cd_sweep is one half-sweep: for each component t = 0 .. k - 1 in order and for every row i
 *       grad = -P[i, t] + sum_r G[t, r] W[i, r]                   (W already updated for the components < t)
 *       pg   = W[i, t] == 0 ? min(0, grad) : grad;   *violation += |pg|
 *       if G[t, t] != 0:  W[i, t] = max(W[i, t] - grad / G[t, t], 0)                           (one IEEE division)
 *   Rows are independent.  The kernel keeps q = W_i G - P_i in registers (one wave per row, lane l the components l, l + 64, ...) and
 *   adds G[t, :] (new - old) to it after each component: the same mathematics with another float32 summation order.  G is a Gram
 *   matrix: the kernel reads row t of G where the update of q names column t, so G is to be symmetric.
 *   *violation (device double) = the sum over rows and components: per row in double in component order, one double per row in
 *   the workspace, then chunks of 4096 rows and the chunk sums in a fixed order.  No atomics: bit-identical from run to run.
 *   W [n, k] (row stride ldw, in place), G [k, k] contiguous, P [n, k] (row stride ldp), float32, unit column stride.
 *   Limits: 1 <= k <= 256 and 1 <= n <= INT32_MAX (GNPDE_ESHAPE); the byte range of W may meet neither P's nor G's (GNPDE_EINVAL;
 *   two column slices of ONE wider buffer count as meeting).  Inputs are to be finite and W, G[t, t] >= 0: nothing is checked on the
 *   device.  Everything runs on the caller's stream; the workspace query returns 0 for an n the entry point refuses. */
size_t gnpde_nmf_cd_sweep_workspace_bytes(int64_t n);
int gnpde_nmf_cd_sweep(float* W, int64_t ldw, const float* G, const float* P, int64_t ldp, int64_t n, int32_t k, double* violation,
                       void* workspace, size_t workspace_bytes, void* stream);

/* Two-hop densification of the rewiring block (new_edges = 'k_hop_att', reference src/block_transformer_rewiring.py:68-86):
 *   S = coalesce(A ++ offdiag(A A)) / 2, i.e. torch_sparse.spspmm(A, A) -> remove_self_loops -> cat with A -> / 2 ->
 *   torch_sparse.coalesce(op='add'), in one row-wise kernel without materialising the products.  A is given in CSR (rowptr [n+1],
 *   col, w in CSR order; duplicates allowed and summed).  Two phases, as the output size is data dependent:
 *   gnpde_two_hop_count -> out_rowptr [n+1] (device int64; out_rowptr[n] = nnz(S)); the caller reads the total and allocates
 *   gnpde_two_hop_fill  -> out_edge_index ([2, out_ld] int64, row-major, first nnz columns written) and out_weight, entries ordered
 *                          by (row, col) as coalesce orders them.  Sums are formed in CSR order: run-to-run identical. */
size_t gnpde_two_hop_workspace_bytes(int32_t n_nodes);
int gnpde_two_hop_count(const int32_t* rowptr, const int32_t* col, int32_t n_nodes, int64_t* out_rowptr, void* workspace,
                        size_t workspace_bytes, void* stream);
int gnpde_two_hop_fill(const int32_t* rowptr, const int32_t* col, const float* w, int32_t n_nodes, const int64_t* out_rowptr,
                       int64_t* out_edge_index, int64_t out_ld, float* out_weight, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Graph diffusion rewiring (GDC; `--rewiring gdc` and BLEND's `--pos_enc_type GDC`, reference src/graph_rewiring.py:51-90, 345-401,
 * a subclass of torch_geometric.transforms.GDC).  Definition (this header is the authority; PyG is no dependency):
 *   1. A = the caller's weighted edges, a loop of self_loop_weight appended to EVERY node when that weight is non-zero, duplicate
 *      (row, col) entries summed.
 *   2. T = normalise(A): 'sym' w_e deg[row]^-1/2 deg[col]^-1/2 with deg_i = sum over row_e = i of w_e; 'col' w_e / (sum of the
 *      column's weights); 'row' likewise over rows; the reciprocal of zero is 0.  (Steps 1-2 are the caller's: torch device ops.)
 *   3. S = sum_{m = 0 .. M} theta_m T^m: ppr theta_m = alpha (1 - alpha)^m, heat theta_m = e^-t t^m / m!, or a caller's list;
 *      M is the smallest with 1 - sum_{m <= M} theta_m <= tol (the caller's, Python gdc_terms).
 *   4. per column j of S: top-k keeps the k largest STRICTLY POSITIVE entries, ordered by value descending, equal values by
 *      ascending row; a column with fewer positive entries yields fewer.  threshold keeps the entries >= eps (eps > 0).  Zeros are
 *      never emitted (PyG's dense top-k also emits zero-weight edges, in arbitrary order: the one deliberate difference).
 *   5. output normalisation over the kept entries ('col': every non-empty column sums to 1), the same zero rule; no NaN / Inf.
 *   6. edge_index [2, E'] int64 with row = i, col = j for a kept S[i, j], grouped by ascending column; within a column as in 4
 *      (top-k) or by ascending row (threshold fill).  No atomics anywhere: bit-identical from run to run.
 * A column block S[:, j0 .. j0 + block) is a Horner recurrence on an [n, block] slab:  X = theta_M E, then M times X <- T X
 * (gnpde_spmm, as it is) and X[j0 + b, b] += theta_m.  theta is a DEVICE array of n_terms = M + 1 floats.  No [n, n] array
 * exists outside gnpde_gdc_dense.  g: the graph of T (row_begin = 0), w_csr its weights in CSR order.
 *   gnpde_gdc_block            slab [n, block] (row stride block) <- S[:, j0 .. j0 + block), columns past n are zero
 *   gnpde_gdc_topk             slab -> keys [n, k] uint64 (rows j0 .. of it: ~value bits << 32 | row, ascending = the order of 4,
 *                              padded with ~0) and counts[j0 + b] = kept entries of column j0 + b (int64)
 *   gnpde_gdc_emit             after the last block: offsets [n + 1] = exclusive scan of counts (the caller's) -> out_edge_index
 *                              ([2, out_ld] int64, row-major), out_weight = value (normalise = 0) or value / column sum (1);
 *                              the sum of a column is formed in a fixed order
 *   gnpde_gdc_threshold_count  slab -> counts [block] int64 (column j0 + b at b; columns past n are not written)
 *   gnpde_gdc_threshold_fill   must follow the count of the SAME block on the same stream and workspace: offsets [block + 1] =
 *                              exclusive scan of counts -> (row, col, value) at offsets[b] .., rows ascending
 *   gnpde_gdc_segment_sums     sums[s] = sum of w[offsets[s] .. offsets[s + 1]) in a fixed order (sums may be NULL); divide != 0:
 *                              the segment is divided by its sum in place (an empty sum gives 0): 'col' / 'row' / 'sym' sums
 *   gnpde_gdc_dense            dense [n, n] fp32: dense[i, j0 + b] = S[i, j0 + b] (normalise = 0) or / the column's sum (1);
 *                              GNPDE_ESHAPE when 4 n^2 > cap_bytes
 * Limits: block a multiple of 4 in 4 .. 256, 1 <= k <= 128, n <= INT32_MAX, 1 <= n_terms <= 4097 (M <= 4096), eps > 0; outside
 * them GNPDE_ESHAPE / GNPDE_EINVAL with gnpde_last_error set and nothing launched (gnpde_gdc_workspace_bytes: 0).  One workspace
 * (k = 0 when no top-k follows) serves every call of a block; it includes the aggregation's scratch. */
size_t gnpde_gdc_workspace_bytes(const gnpde_graph_t* g, int32_t block, int32_t k);
int gnpde_gdc_block(const gnpde_graph_t* g, const float* w_csr, const float* theta, int32_t n_terms, int64_t j0, int32_t block,
                    float* slab, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_gdc_topk(const gnpde_graph_t* g, const float* slab, int64_t j0, int32_t block, int32_t k, uint64_t* keys,
                   int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_gdc_emit(const uint64_t* keys, const int64_t* offsets, int32_t n, int32_t k, int32_t normalise,
                   int64_t* out_edge_index, int64_t out_ld, float* out_weight, void* stream);
int gnpde_gdc_threshold_count(const gnpde_graph_t* g, const float* slab, int64_t j0, int32_t block, float eps, int64_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream);
int gnpde_gdc_threshold_fill(const gnpde_graph_t* g, int64_t j0, int32_t block, float eps, const int64_t* offsets,
                             int64_t* out_edge_index, int64_t out_ld, float* out_weight, void* workspace, size_t workspace_bytes,
                             void* stream);
int gnpde_gdc_segment_sums(float* w, const int64_t* offsets, int64_t n_segments, float* sums, int32_t divide, void* stream);
int gnpde_gdc_dense(const gnpde_graph_t* g, const float* slab, int64_t j0, int32_t block, int32_t normalise, float* dense,
                    size_t cap_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* Approximate personalised PageRank by forward push (Andersen-Chung-Lang): the `exact = False` branch of graph diffusion rewiring
 * (reference src/graph_rewiring.py:389-392 -> torch_geometric's GDC.diffusion_matrix_approx).  g: the coalesced UNWEIGHTED graph with
 * the self loops already added (row_begin = 0; only n, rowptr and colidx are read), deg(u) = the length of row u.  For every
 * source s: p_s = 0, r_s = alpha e_s; a push at u with res = r_s(u) does p_s(u) += res, r_s(u) = 0, r_s(v) += (1 - alpha) res /
 * deg(u) for every v of row u.  The source is pushed once unconditionally, then every u with r_s(u) >= alpha eps deg(u), in
 * synchronous rounds, until none is left.  p and r are 64-bit fixed-point integers (quantum 2^-60; the two divisions of a push
 * round DOWN, so a push loses less than deg(u) + 2 quanta of mass and never creates any) accumulated with integer atomics: the
 * result is bit-identical from run to run and does not depend on the batch (s0, n_sources), the grid, `capacity` or `slow_groups`.
 * The state of a source lives in an LDS hash of `capacity` distinct nodes (-1: the built-in 1536, the maximum; 0: none); a source
 * whose support outgrows it is run again inside the same call on one of `slow_groups` per-workgroup scratch areas of the workspace
 * (36 n bytes each, cleared by the groups that have work, reset per source through a touched list) -- same integers, same result.  Nothing of size n x n exists.
 *   gnpde_gdc_push_count      counts[i] (int64, [n_sources]) = number of u with p_{s0 + i}(u) > 0
 *   gnpde_gdc_push_fill       offsets [n_sources + 1] = exclusive scan of those counts (the caller's) -> out_edge_index ([2, out_ld]
 *                             int64 row-major: row 0 = s, row 1 = u ascending) and out_p = fp32(p_s(u)) (one rounding) at offsets[i] ..
 *   gnpde_gdc_push_residuals  residuals [n_sources, n] fp32 (dense, zero-filled here) = fp32(r_s(u)); for tests, n <= 4096
 * info: int64[2] on the device, zeroed by the caller: info[0] += sources that took the slow path (count pass only), info[1] |=
 * 1 (round guard reached: never expected), 2 (a column index outside [0, n)), 4 (offsets are not those of this push's counts; that
 * source is not written).  Limits: n <= INT32_MAX, 0 < alpha < 1, eps > 0 finite, alpha eps >= 2^-60, 0 <= s0, s0 + n_sources <= n,
 * capacity >= -1, 1 <= slow_groups <= 1024; outside them GNPDE_EINVAL / GNPDE_ESHAPE / GNPDE_EWS with gnpde_last_error set and
 * nothing launched (gnpde_gdc_push_workspace_bytes: 0). */
size_t gnpde_gdc_push_workspace_bytes(int64_t n, int64_t n_sources, int32_t slow_groups);
int gnpde_gdc_push_count(const gnpde_graph_t* g, int64_t s0, int64_t n_sources, double alpha, double eps, int32_t capacity,
                         int32_t slow_groups, int64_t* counts, int64_t* info, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_gdc_push_fill(const gnpde_graph_t* g, int64_t s0, int64_t n_sources, double alpha, double eps, int32_t capacity,
                        int32_t slow_groups, const int64_t* offsets, int64_t* out_edge_index, int64_t out_ld, float* out_p,
                        int64_t* info, void* workspace, size_t workspace_bytes, void* stream);
int gnpde_gdc_push_residuals(const gnpde_graph_t* g, int64_t s0, int64_t n_sources, double alpha, double eps, int32_t capacity,
                             int32_t slow_groups, float* residuals, int64_t* info, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row-partitioned solve over the GPUs of one node: one process per GPU, RCCL point-to-point halo exchange once per
 * evaluation of f, the whole solve (pack, grouped send/recv on a second stream, interior rows, boundary rows, every
 * stage of every step) captured per rank in ONE hipGraph.  The reference has no counterpart (single device;
 * nn.DataParallel replicas in src/ray_tune.py:65-66); this is the multi-GPU form of the solver loop of
 * src/block_constant.py:57-62 that BASELINE.json's north star asks for.
 *
 * RCCL is bound at run time: gnpde_comm_load_library(path) names the librccl to use (NULL / never called: the first
 * of "librccl.so.1", "librccl.so" that loads; a library already in the process is reused).
 * Bootstrap: rank 0 calls gnpde_comm_get_unique_id, ships the GNPDE_COMM_ID_BYTES to the other ranks by any means
 * (the Python host broadcasts them through torch.distributed), every rank calls gnpde_comm_create (collective).
 * ---------------------------------------------------------------------------------------------- */
#define GNPDE_COMM_ID_BYTES 128
typedef struct gnpde_comm gnpde_comm_t;
int gnpde_comm_load_library(const char* path);
int gnpde_comm_get_unique_id(void* id_out /* GNPDE_COMM_ID_BYTES */);
int gnpde_comm_create(gnpde_comm_t** out, const void* id, int32_t rank, int32_t world);
int gnpde_comm_destroy(gnpde_comm_t* comm);

/* What this rank exchanges per evaluation.  Local row numbering of the state: [interior rows | boundary rows | halo rows
 * grouped by owning rank, ascending]; rows [0, n_own) are owned.  send_idx (device) lists, grouped by destination rank,
 * the owned rows each peer needs (send_counts[p] of them for rank p); recv_counts[p] rows arrive from rank p and land,
 * in rank order, in the halo region [n_own, n_own + n_halo) of the stage buffer -- nothing is unpacked. */
typedef struct gnpde_halo {
  int32_t world, rank;
  int32_t n_own, n_halo;
  const int32_t* send_idx;      /* device [sum(send_counts)]  */
  const int32_t* send_counts;   /* host [world]               */
  const int32_t* recv_counts;   /* host [world]               */
} gnpde_halo_t;

/* P2P transport (the default of the Python layer): the stage buffers of every rank live in IPC-shared device memory; a
 * push kernel stores this rank's boundary rows straight into the peers' halo regions over xGMI and raises an epoch flag
 * in each peer's flag array, a one-block wait kernel in front of the boundary pass polls the flags (bounded spin).  No
 * library call and no host involvement per evaluation: the per-rank hipGraph holds kernel and memcpy nodes only.
 * Several ranks may share one device (the processes map each other's memory the same way).
 *   gnpde_p2p_create      allocates n_buffers (4 for rk4, 2 for euler; a fifth for gnpde_sharded_solver_set_general) stage buffers of buffer_bytes >= (n_own + n_halo) * d * 4
 *                         and the flag array (fine-grained memory)
 *   gnpde_p2p_get_handle  -> GNPDE_P2P_HANDLE_BYTES to be all-gathered over the ranks by the host
 *   gnpde_p2p_connect     handles of ALL ranks, [world][GNPDE_P2P_HANDLE_BYTES]; maps the peers' memory */
#define GNPDE_P2P_HANDLE_BYTES 128
typedef struct gnpde_p2p gnpde_p2p_t;
int   gnpde_p2p_create(gnpde_p2p_t** out, int32_t rank, int32_t world, size_t buffer_bytes, int32_t n_buffers);
int   gnpde_p2p_get_handle(gnpde_p2p_t* p2p, void* handle_out);
int   gnpde_p2p_connect(gnpde_p2p_t* p2p, const void* handles);
void* gnpde_p2p_buffer(gnpde_p2p_t* p2p, int32_t b);      /* device pointer of local stage buffer b */
int   gnpde_p2p_destroy(gnpde_p2p_t* p2p);

typedef struct gnpde_sharded_solver gnpde_sharded_solver_t;

/* rhs_interior: descriptor over the graph view holding the rows without halo neighbours (graph->n = their count;
 * projection rows [0, n_own)); rhs_boundary: the view holding the other owned rows (graph->n = n_own, graph->row_begin =
 * number of interior rows; projection rows [n_own, n_own + n_halo)).  Both with n_state_rows = n_own + n_halo,
 * ld == d, the same kind / scalars / x0 ([n_own, d]).
 * gnpde_sharded_solver_create: RCCL transport (comm may be NULL when nothing is exchanged, world 1); EAGER launches only:
 * capturing the grouped send/recv on a forked stream crashes the HIP 7.0 runtime bundled with torch 2.10.
 * gnpde_sharded_solver_create_p2p: P2P transport; peer_halo_row0[p] = row of peer p's stage buffers where THIS rank's rows
 * start (= n_own of p + the recv counts of p for ranks below this one), peer_buffer_bytes[p] = p's buffer_bytes (aligned
 * up to 256). */
size_t gnpde_sharded_solver_workspace_bytes(const gnpde_halo_t* halo, const gnpde_rhs_t* rhs_interior,
                                            const gnpde_rhs_t* rhs_boundary, int32_t method, int32_t p2p);
int gnpde_sharded_solver_create(gnpde_sharded_solver_t** out, gnpde_comm_t* comm, const gnpde_halo_t* halo,
                                const gnpde_rhs_t* rhs_interior, const gnpde_rhs_t* rhs_boundary, int32_t method,
                                const float* dts, int32_t n_steps, void* workspace, size_t workspace_bytes);
int gnpde_sharded_solver_create_p2p(gnpde_sharded_solver_t** out, gnpde_p2p_t* p2p, const gnpde_halo_t* halo,
                                    const gnpde_rhs_t* rhs_interior, const gnpde_rhs_t* rhs_boundary, int32_t method,
                                    const float* dts, int32_t n_steps, const int64_t* peer_halo_row0,
                                    const int64_t* peer_buffer_bytes, void* workspace, size_t workspace_bytes);
/* y: device state whose first n_own rows are integrated in place over the whole grid (RCCL transport: [n_own + n_halo, d],
 * the halo rows are scratch; P2P: [>= n_own, d], copied into / out of the shared stage buffer).  use_graph != 0: captured
 * once per y pointer and replayed (P2P transport only).  Every rank must call it (the exchange is collective). */
int gnpde_sharded_solver_run(gnpde_sharded_solver_t* s, float* y, int32_t use_graph, void* stream);
/* Host-side: the order in which the P2P push walks a destination-grouped send list of send_counts[0..world) rows --
 * order[w] = slot copied by the w-th wavefront; the destinations are interleaved in proportion to their counts so that every
 * xGMI link of the rank is busy for the whole push (walked group by group, one link would carry it all while six idle).  A
 * permutation of [0, sum send_counts) that keeps each destination's rows in order.  What gnpde_sharded_solver_create_p2p uses;
 * exported for the host tests. */
int gnpde_push_order(const int32_t* send_counts, int32_t world, int32_t* order);
/* P2P transport: compute the boundary rows in n_chunks consecutive row ranges and push each range's rows of the stage OUTPUT --
 * the next evaluation's input -- into the peers' halo regions right behind it, on the side stream, while the next range is
 * computed; the last range's push raises the next evaluation's epoch.  The first evaluation of a solve still pushes its whole
 * input, the last one pushes nothing.  What is left to hide behind the next interior pass is one range's push instead of the
 * whole exchange.  rhs_chunks[c]: descriptor of range c (same kind / d / ld as the boundary descriptor; graph rows
 * [row_begin, n) continue where range c-1 ended, the ranges tile [n_interior, n_own); for the transformer kind range 0
 * projects the halo rows and the later ones an empty slice).  push_order: permutation of the send slots grouped by range --
 * slots [push_chunk_ptr[c], push_chunk_ptr[c+1]) hold the rows range c computes (rows of the interior pass that peers read
 * ride with range 0).  Same arithmetic in the same order as the unchunked solve: results are bit-identical.  n_chunks = 0
 * restores the single boundary pass.  GNPDE_EWS when the workspace has no room for a range's scratch
 * (gnpde_rhs_workspace_bytes of the range descriptors beyond the interior / boundary ones).  Drops a captured graph.
 * No reference equivalent (the reference is single-device). */
int gnpde_sharded_solver_set_boundary_chunks(gnpde_sharded_solver_t* s, const gnpde_rhs_t* const* rhs_chunks, int32_t n_chunks,
                                             const int32_t* push_order, const int32_t* push_chunk_ptr);
/* Exchange timing of the LAST run (P2P transport): for every evaluation four wall-clock stamps (s_memrealtime ticks, rate in
 * *ticks_per_second) written by the kernels themselves inside the hipGraph -- [0] the push kernel starts, [1] its last block has
 * published the epoch (all boundary rows stored into the peers' halo regions), [2] the main stream reaches the wait (interior
 * rows done), [3] every peer's rows have landed.  [1]-[0] = push duration (xGMI stores), [3]-[2] = time the boundary pass waited
 * for the exchange, i.e. the part of the exchange that compute did not hide.  With gnpde_sharded_solver_set_boundary_chunks the
 * rows of evaluation s travel during evaluation s - 1: [0] = the push behind the FIRST row range starts, [1] = the push behind
 * the last range has published the epoch, both stamped in the row of the evaluation whose INPUT they deliver.  stamps:
 * int64[capacity_evals][4]; *n_evals: the evaluations of a run (0 when the solver does not exchange).  Synchronises.  No reference
 * equivalent (measurement). */
int gnpde_sharded_solver_timing(gnpde_sharded_solver_t* s, int64_t* stamps, int32_t capacity_evals, int32_t* n_evals,
                                int64_t* ticks_per_second);

/* Synchronises.  *timed_out != 0: a wait kernel gave up polling a peer's epoch flag (results are invalid);
 * *epochs = evaluations this rank has published so far.  After the first time-out the waits of the evaluations still
 * queued return without polling (the flag is sticky for the lifetime of the gnpde_p2p_t), so a lost solve ends quickly. */
int gnpde_sharded_solver_status(gnpde_sharded_solver_t* s, int32_t* timed_out, int64_t* epochs);
int gnpde_sharded_solver_set_spin_limit(gnpde_sharded_solver_t* s, int64_t max_spins);
int gnpde_sharded_solver_num_rhs_evals(const gnpde_sharded_solver_t* s);
int gnpde_sharded_solver_destroy(gnpde_sharded_solver_t* s);

/* Normalisers that are not row-local over the row partition, inside the per-rank graph  [replaces the Python-driven evaluation that ran
 * until ABI 6: reference src/function_transformer_attention.py:190-213 with attention_norm_idx = 1 and / or squareplus
 * (src/utils.py:179-208), src/function_GAT_attention.py with attention_norm_idx = 1].  After this call every evaluation of the solver is:
 * push of the boundary rows; projection of own + halo rows into qk; pass 1 of gnpde_edge_attention_pass on att_graph (every local node
 * a segment) [squareplus: the MAXIMUM of the global score maximum over the ranks, one word exchanged through the flag blocks];
 * pass 2 [normalised over columns: the partial statistics of the halo columns are pushed into their owners' in_part rows, merged
 * there peer by peer in rank order (the arithmetic of gnpde_segment_stats_merge), and the totals are pushed back with the state's
 * pattern]; pass 3 into w; the aggregation over spmm_graph (the owned rows) with the solver's stage epilogue.  Every rank issues the
 * same pushes in the same order, so the one epoch sequence of the transport orders all of them.
 *   att: type / heads / att_dim / norm_idx / square_plus / leaky_slope / gat_a / output_var / lengthscale / edge_w_csr (att_graph's CSR
 *        order); q, k, ldqk are filled per evaluation (transformer: q = qk, k = qk + att_dim, ldqk = 2 att_dim; GAT: q = k = qk).
 *   qk [n_own + n_halo, proj_m], w [entries of att_graph], stats_send [n_halo, 2 heads], the two workspaces: device memory of the caller.
 *   stats_buffer: index (>= 4) of the shared buffer of gnpde_p2p_create that holds [S: (n_own + n_halo) x 2 heads | in_part: n_send x
 *        2 heads] on every rank; in_offset / peer_in_offset[p]: byte offset of in_part on this rank / on peer p (multiples of 256);
 *        peer_buffer_bytes[p] as in gnpde_sharded_solver_create_p2p; peer_rev_row0[p]: row of peer p's in_part where THIS rank's rows
 *        start (= the send counts of p for the ranks below this one).  Only read when att->norm_idx == 1 and world > 1. */
typedef struct gnpde_general {
  const gnpde_graph_t* att_graph;
  const gnpde_graph_t* spmm_graph;
  const gnpde_attention_t* att;
  float* qk; float* w; float* stats_send;
  void* att_ws; size_t att_ws_bytes;
  void* spmm_ws; size_t spmm_ws_bytes;
  int32_t stats_buffer;
  int64_t in_offset;
  const int64_t* peer_in_offset;
  const int64_t* peer_buffer_bytes;
  const int64_t* peer_rev_row0;
} gnpde_general_t;
int gnpde_sharded_solver_set_general(gnpde_sharded_solver_t* s, const gnpde_general_t* g);

/* dopri5 over the row partition with the controller on the device  [replaces, per rank, the Python controller that ran over
 * torch.distributed until ABI 6: reference src/block_constant.py:57-62 with opt['method'] = 'dopri5' on a graph no single GPU holds].
 * `engine`: a gnpde_sharded_solver_t created with gnpde_sharded_solver_create_p2p (method GNPDE_METHOD_RK4 -- four shared stage
 * buffers --, n_steps = 0): it stays the caller's, must outlive the dopri5 object and is used by nothing else meanwhile.  The trial
 * step of gnpde_dopri5_create is captured per rank with every evaluation as push + interior rows + wait + boundary rows, and the
 * error norm (and the three norms of the initial step size) as ONE double summed over the ranks inside the stream: every rank stores
 * its partial into every peer's fine-grained flag block, waits for the peers' and adds them in rank order, so every rank's
 * controller record holds the same bits and every rank takes the same accept / reject decisions and step sizes -- no host read per
 * trial step, no collective call.  n_rows_total: rows of the WHOLE graph (the mean of the norm).  gnpde_dopri5_run then takes and
 * returns the OWNED rows ([n_own, d]); early stopping, the tape and the row order are single-GPU features (GNPDE_ESTATE here). */
size_t gnpde_dopri5_sharded_workspace_bytes(gnpde_sharded_solver_t* engine);
int gnpde_dopri5_create_sharded(gnpde_dopri5_t** out, gnpde_sharded_solver_t* engine, float rtol, float atol, int64_t n_rows_total,
                                void* workspace, size_t workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GNPDE_H */
