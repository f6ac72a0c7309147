"""Every line of the row attention's dispatch (plan_attention / launch_planned in csrc/attention.hip) against a float64 oracle, judged segment by
segment (tests/row_cases.py: the metric, the staircase graphs, the cases).  Every case draws a standard-normal fp32 table directly (no
projection), asks ops.edge_attention for the head-mean weights and compares them in CSR order with the float64 head mean of
oracle/restate.py on the same table; helpers.TOL applies to every ROW (column for attention_norm_idx = 1), hub rows included.  Each case
runs twice, gnpde_tune(TUNE_ATT_GENERIC_ROWS, .) 0 and 1, and both runs are compared with float64, never with each other.  Which line a
run takes is asked of the library (ops.attention_plan with the call's own operands: the plan the launchers switch on) and must be the
one the case is listed under (row_cases.intended); tests/test_attention_plan_cpu.py pins template lines, grids and the other routes.

dispatch line                                                                        case (part-graph ... of row_cases.CASES)     knob
---------------------------------------------------------------------------------------------------------------------------------------
route sd_rows (launch_sd_rows), H in {1,2,4,8} x d_k in {4,8,16}: row_attention_sd_kernel<H, DK4, .., MODE, SCATTER> per sweep,
two lane mappings (rows <= 16 entries / 17..512), hub chunks in the first blocks (hub_scores_partial_heads, hub_normalise_body)
  MODE 0 (row softmax), with and without edge_w                                     1-hubs, the 12 pairs, plain and -rw             0
  MODE 2 -> 1 (squareplus), per-wave maxima (gmax_part, no hub rows)                 2-nohubs, the 12 pairs                          0
  MODE 2 -> 1 (squareplus), slots + gmax_fold_kernel (hub rows)                      2-hubs, the 12 pairs                            0
  MODE 0, SCATTER (norm_idx 1: rows of the transposed graph, out_pos)                3-hubs_t -n1, the 12 pairs                      0
  MODE 2 -> 1, SCATTER                                                               3-hubs_t -n1-sqp, the 12 pairs                  0
  MODE 4 (exp kernel)                                                                4-hubs exp_kernel, the 12 pairs                 0
  MODE 3 (GAT through the 4-wide table of gat_terms_kernel, DK4 = 1)                 5-hubs gat h in {1,2,4,8}, d_k 4 and 16         0
  a launch of hub blocks only (n_rows == 0 clamp): no row <= 16 / none of 17..512    8-no16, 8-no64 at (4,4), (8,16), plain / -sqp   0
  other d_k: no such line -> route rows                                              6 scaled_dot d_k 12, 32; 4 exp_kernel d_k 12    0, 1
route rows (launch_rows): row_attention_kernel<TYPE, H, GL, P, VEC4> per row class,
hub rows by launch_hubs (hub_scores_partial_sd_kernel<H> / hub_scores_partial_kernel<TYPE, VEC4>) + hub_normalise_kernel
  SCALED_DOT, H in {1,2,4,8}                                                         1-hubs (12 pairs); 6 d_k 12, 32                 1; 0, 1
  COSINE, PEARSON, H in {1,2,4,8}                                                    6-hubs cosine_sim / pearson, d_k 4, 8           0, 1
  EXP_KERNEL, H in {1,2,4,8}                                                         4-hubs (12 pairs); d_k 12                       1; 0, 1
  GAT (VEC4 false), H in {1,2,4,8}                                                   5-hubs gat; with edge_w (-rw leaves gat_sd)     1; 0, 1
  (the row_attention_sd_kernel form of this route serves a forked solver stream: tests/test_attention_plan_cpu.py pins it)
route general, the three passes: scores_kernel<TYPE, VEC4>, seg_stats_heads_kernel<H> / seg_stats_kernel, seg_stats_long_partial_kernel +
seg_stats_long_combine_kernel (hub rows; long COLUMNS with max_chunks = 3 for norm_idx 1), normalise_kernel
  d_k = 2 / h = 3 / ldqk = 2A + 1 (VEC4 false)                                       7-hubs, 7-hubs_t: dk2, h3, -ld+1                0, 1
  att [E,h] and prods [E,h] requested, H in {1,2,4,8} and 3, softmax and squareplus  7 -all                                          0, 1
  squareplus / norm_idx 1 with the specialised rows switched off                     2, 3, 8 -sqp                                    1
  norm_idx 1 with edge_w (leaves the SCATTER fast path)                              3-hubs_t-h4-dk4-n1-rw                           0, 1
  GAT, h = 3                                                                         5-hubs-gat-h3                                   0, 1
route sd_one (one launch, hub weights deferred to the aggregation), launch_attn_spmm (attention inside the aggregation): reached through
gnpde_rhs_eval only -- tests/test_attention_routes_gpu.py
"""
import ctypes
import functools

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
import row_cases as RC
from helpers import TOL, assert_parity

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graph(name, dev):
  ei, lens, side = RC.graph_edges(name)
  graph = G.CSRGraph(ei.to(dev), lens.numel())
  view = graph.transposed_positions()[0] if side else graph
  # a change of the builder must not quietly move a case off its line
  assert (view.n_bin16, view.n_bin64, view.n_long_rows, view.n_long_chunks) == RC.expected_bins(lens), name
  if side:
    assert graph.n_long_cols == view.n_long_rows and (view.n_long_rows == 0 or (graph.max_col_len + 511) // 512 == 3)
  return graph


def _ws_addr(graph, st):
  """The workspace gnpde_edge_attention will be handed (graph.workspace caches it by tag and size)."""
  return graph.workspace('att', _lib.lib().gnpde_attention_workspace_bytes(graph.ref(), ctypes.byref(st))).data_ptr()


@pytest.mark.parametrize('generic', [0, 1], ids=['specialised', 'generic'])
@pytest.mark.parametrize('c', RC.CASES, ids=RC.case_id)
def test_dispatch_line(dev, c, generic):
  ei, lens, side = RC.graph_edges(c.graph)
  assert side == c.norm_idx
  graph = _graph(c.graph, str(dev))
  table, a, ew = RC.case_inputs(c)
  A = c.h * c.dk
  tab = table.to(dev)
  ld = tab.stride(0)
  gat = c.att_type == 'gat'
  q, k = tab, (tab if gat else tab[:, A:])
  # the preconditions of the case's line
  assert ld == (A if gat else 2 * A) + c.ld_pad and A // c.h == c.dk
  vec4 = c.dk % 4 == 0 and ld % 4 == 0 and q.data_ptr() % 16 == 0 and k.data_ptr() % 16 == 0
  assert vec4 == (c.dk % 4 == 0 and c.ld_pad == 0), 'alignment of q / k'
  view = graph.transposed_positions()[0] if side else graph
  if c.graph in ('hubs', 'hubs_t'):
    assert view.n_long_rows == len(RC.HUBS) and view.n_bin16 > 0 and view.n_bin64 > 0
  elif c.graph == 'nohubs':
    assert view.n_long_rows == 0
  elif c.graph == 'no16':
    assert view.n_bin16 == 0 and view.n_bin64 > 0 and view.n_long_rows == 2
  elif c.graph == 'no64':
    assert view.n_bin64 == 0 and view.n_bin16 > 0 and view.n_long_rows == 2

  ew_csr = ops.edge_to_csr_mean(graph, ew.to(dev)) if c.reweight else None
  st = ops.attention_struct(_lib.ATT_GAT if gat else _lib.ATT_TYPES[c.att_type], c.h, A, c.norm_idx, c.sqp, q=q, k=k, ldqk=ld, leaky_slope=c.slope,
                            gat_a=a.to(dev) if gat else None, output_var=torch.tensor([RC.OUTPUT_VAR], device=dev),
                            lengthscale=torch.tensor([RC.lengthscale(c.dk)], device=dev), edge_w_csr=ew_csr,
                            transposed=graph.transposed_positions() if c.norm_idx == 1 else None)
  want_all = c.outputs == 'all'
  try:
    ops.tune(_lib.TUNE_ATT_GENERIC_ROWS, generic)
    # the library's own answer for the very operands of the call below: the case runs the line it is there for
    plan = ops.attention_plan(graph, st, True, want_all, want_all, ws_addr=_ws_addr(graph, st))
    assert plan.route_name == RC.intended(c, generic) and plan.vec4 == vec4, (RC.case_id(c), plan.route_name)
    if c.sqp and plan.route_name == RC.SD:      # squareplus' maximum sweep: per-wave maxima without hub rows, slots + fold with them
      assert plan.gmax == (_lib.ATT_GMAX_PER_WAVE if c.graph == 'nohubs' else _lib.ATT_GMAX_SLOTS_FOLD)
    w, att, prods = ops.edge_attention(graph, st, True, want_all, want_all, like=tab)
    torch.cuda.synchronize()
  finally:
    ops.tune(_lib.TUNE_ATT_GENERIC_ROWS, 0)

  att64, prods64 = RC.reference64(c)            # computed once per case, shared by both knob values
  perm = graph.perm_long.cpu()
  seg = ei[c.norm_idx]
  what = '%s [%s, %s]' % (RC.case_id(c), 'generic' if generic else 'specialised', RC.intended(c, generic))
  w_ref = att64.mean(dim=1)[perm]
  print('ROWERR %s head-mean %s' % (what, RC.class_errors(RC.per_segment_error(w[:graph.e], w_ref, seg[perm]), lens)))
  RC.assert_rows(w[:graph.e], w_ref, seg[perm], lens, TOL, what + ' head-mean weights (CSR order)')
  if want_all:
    print('ROWERR %s att %s' % (what, RC.class_errors(RC.per_segment_error(att, att64, seg), lens)))
    RC.assert_rows(att, att64, seg, lens, TOL, what + ' att [E,h]')
    assert_parity(prods, prods64, what=what + ' prods [E,h]')
