"""Every launch line of the attention backward (csrc/backward.hip) against a float64 oracle, judged segment by segment
(tests/bwd_cases.py: inputs, references, tolerances, the lists of cases; tests/row_cases.py: the staircase graphs and the metric).  The
kernels are called through entry points that forward every optional operand of the launchers (gnpde_attention_rows_bwd_dq,
gnpde_head_rowsum); every comparison is with float64, never with another device path, and per ROW (column for d k): a hub row's entries are
about 1e-3 of a short row's, so a whole-tensor norm lets a hub row that is 1 % wrong pass.  Every case runs twice and the two results
agree bit for bit (fixed-order reductions); hub_ws is filled with NaN before the call; the graph's bins are asserted as built
(row_cases.expected_bins).  Case ids below are those of bwd_cases.ds_id / dq_id / hr_id / sb_id / hs_id; "12 pairs" = heads in {1,2,4,8} x
d_k in {4,8,16}, "9 pairs" = those with heads * d_k <= 32.

launch line                                                                              case
-------------------------------------------------------------------------------------------------------------------------------------
launch_attention_rows_bwd_dq -> GNPDE_AB(H, DK), 12 lines; per line, DQ off (launch_attention_rows_bwd_v<H, DK, false>):
  attention_rows_bwd_kernel<H, DK, 16, 1, false, false>      rows <= 16 entries              ds-hubs-h*-dk* (12 pairs, plain and -rw)
  attention_rows_bwd_kernel<H, DK, 64, 1, false, false>      rows 17..64, one pass           the same cases
  attention_rows_bwd_kernel<H, DK, 64, 8, false, false>      rows 65..512, eight passes      the same cases
  attention_hub_stats_kernel<H, DK> + attention_hub_ds_kernel<H, DK, false>   (hub_ws set)   ds-hubs-...-chunks
  attention_hub_bwd_kernel<H, DK, false>                     (hub_ws NULL: a block per hub)  ds-hubs-...-block
  a launch class absent: no row <= 16 / none of 17..512                                      ds-no16-*, ds-no64-* at (4,4), (8,16)
  no hub launch at all                                                                       ds-nohubs-h4-dk4-chunks
  edge_w_csr NULL / set                                                                      plain / -rw
  rpos NULL / set (RRef reads r through csr_positions)                                       all others / ds-hubs-...-rpos: (1,4), (2,8),
                                                                                             (4,16), (8,4), both hub forms
  scale NULL / raw scale without sigmoid / sigmoid(scale)                                    -noscale / -raw / all others
the same lines with DQ on (launch_attention_rows_bwd_v<H, DK, true>), the 9 pairs:
  attention_rows_bwd_kernel<H, DK, 16 | 64, 1 | 8, false, true> (LaneTranspose<C, GL / 2>)   dq-hubs-h*-dk*-chunks and -block
  attention_hub_ds_kernel<H, DK, true> + hub_rowpart_fold_kernel                             dq-hubs-...-chunks
  attention_hub_bwd_kernel<H, DK, true>                                                      dq-hubs-...-block
  with edge_w_csr; a launch class absent; no hub rows                                        dq-hubs-h4-dk4-rw-chunks, dq-hubs-h8-dk4-rw-block;
                                                                                             dq-no16-*, dq-no64-*; dq-nohubs-*
  dq set for a pair with heads * d_k > 32 -> GNPDE_ESHAPE                                    test_unsupported_shapes_raise
launch_head_rowsum -> GNPDE_HR(H, DK4), 9 lines; per line:
  head_rowsum_kernel<H, DK4, 16, 1, false> / <.., 64, 1, ..> / <.., 64, 8, ..>               hr-dq-hubs-* (pos NULL),
  (LaneTranspose<C, GL / 2> per (A, GL))                                                     hr-dk-hubs_t-* (pos = t_from_csr), 9 pairs each
  head_rowsum_chunk_kernel<H, DK4> + hub_rowpart_fold_kernel (hub_ws set)                    hr-...-chunks
  head_rowsum_hub_kernel<H, DK4> (hub_ws NULL)                                               hr-...-block
  a launch class absent; no hub rows                                                         hr-dq-no16-*, hr-dq-no64-* at (4,4), (8,4);
                                                                                             hr-dq-nohubs-*, hr-dk-nohubs_t-*
  an unsupported shape -> GNPDE_ESHAPE                                                       test_unsupported_shapes_raise
gnpde_softmax_rows_bwd -> GNPDE_SB(HT): softmax_rows_bwd_kernel<1 | 2 | 4 | 8>                sb-hubs-h{1,2,4,8}-dk4, plain and -rw
  softmax_rows_bwd_kernel<0> (run-time head loop)                                            sb-hubs-h3-dk4, plain and -rw
gnpde_head_spmm -> GNPDE_HS(N4): head_spmm_kernel<N4, 64, true>, N4 = A / 4 in {1, ..., 64}   hs-h1-dk4 (1), h2-dk4 (2), h4-dk4 (4), h4-dk8 (8),
  rows (segpos NULL) and by_column (CSC view)                                                 h8-dk8 (16), h8-dk16 (32), h8-dk32 (64); -rows / -cols
gnpde_head_spmm -> GNPDE_HSA(VW, CPL): head_spmm_any_kernel<VW, CPL>
  (2, 1)   (2, 2)   (1, 1)   (1, 2)            (1, 3)             (1, 4)                     hs-h4-dk2, h8-dk30, h3-dk3, h3-dk25 (A = 75),
  ((1, 2) and (1, 3) are reached by no shape of tests/test_head_shapes_gpu.py)               h5-dk33 (A = 165), h7-dk35 (A = 245); -rows / -cols
unreachable: the in-kernel hub branches of attention_rows_bwd_kernel and head_rowsum_kernel (template parameter HUBS) -- both kernels are
  only ever instantiated with HUBS = false, the hub rows go to the kernels above; head_spmm_kernel with GL = 16 or HUBS = false (the
  launcher instantiates <N4, 64, true> only).

Device class errors measured on the MI355X, worst per length class (<=16 | 17..512 | >512) over the cases of a group (the ROWERR lines).  The
tolerance is max(TOL, 3 x the fp32 oracle's own error for that class of that case): TOL but for the <= 16 class of the cases whose
draw has fp32 within a factor 3 of TOL (dq-hubs-h8-dk4-rw-block, 1.14e-5 against a bound of 1.46e-5, is the one figure above TOL).
  ds, attention backward, chunked hubs          9.1e-6 | 5.8e-7 | 6.4e-7        a block per hub      9.1e-6 | 5.8e-7 | 6.9e-7
  d q of the same launch, chunked hubs          6.8e-6 | 5.7e-7 | 5.4e-7        a block per hub      1.1e-5 | 5.6e-7 | 4.9e-7
  head_rowsum d q, chunked hubs                 2.8e-7 | 3.0e-7 | 3.0e-7        a block per hub      2.8e-7 | 3.0e-7 | 4.0e-7
  head_rowsum d k, chunked hubs                 3.9e-7 | 2.0e-7 | 2.2e-7        a block per hub      3.9e-7 | 2.0e-7 | 2.2e-7
  softmax_rows_bwd                              7.1e-6 | 3.6e-7 | 1.1e-7
  head_spmm float4 lines                        3.9e-7 | 8.0e-7 | 6.5e-7        generic lines        3.0e-7 | 8.0e-7 | 5.0e-7
"""
import functools
import math

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
import bwd_cases as BC
import row_cases as RC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graph(name, dev):
  ei, lens, side = RC.graph_edges(name)
  graph = G.CSRGraph(ei.to(dev), lens.numel())
  view = graph.transposed_positions()[0] if side else graph
  # a change of the builder must not quietly move a case off its line
  assert (view.n_bin16, view.n_bin64, view.n_long_rows, view.n_long_chunks) == RC.expected_bins(lens), name
  assert view.n_bin_le64 == int(((lens > 16) & (lens <= 64)).sum())
  if name in ('hubs', 'hubs_t'):        # all three row classes and the hub rows are there
    assert view.n_bin16 > 0 and view.n_bin_le64 > 0 and view.n_bin64 - view.n_bin_le64 > 0 and view.n_long_rows == len(RC.HUBS)
  elif name in ('nohubs', 'nohubs_t'):
    assert view.n_long_rows == 0 and view.n_bin16 > 0 and view.n_bin64 - view.n_bin_le64 > 0
  elif name == 'no16':
    assert view.n_bin16 == 0 and view.n_bin64 > 0 and view.n_long_rows == 2
  elif name == 'no64':
    assert view.n_bin64 == 0 and view.n_bin16 > 0 and view.n_long_rows == 2
  assert graph.e == ei.shape[1]
  return graph


def _hub_ws(view, h, A, form, like):
  """NaN-filled scratch for the chunked hub rows, or None (a block per hub row; a graph without hub rows)."""
  if form == 'block':
    return None
  ws = ops.hub_bwd_workspace(view, h, A, like)
  assert (ws is None) == (view.n_long_rows == 0)
  return None if ws is None else ws.fill_(float('nan'))


def _operands(c, dev):
  """(graph, attention struct, table, r in CSR order, edge weights in CSR order or None) of a RefCase on the device."""
  graph = _graph(c.graph, str(dev))
  table, r, ew = BC.inputs(c)
  A = c.h * c.dk
  tab = table.to(dev)
  perm = graph.perm_long
  ew_csr = ew.to(dev)[perm].contiguous() if ew is not None else None
  st = ops.attention_struct(_lib.ATT_SCALED_DOT, c.h, A, 0, False, q=tab, k=tab[:, A:], ldqk=2 * A, edge_w_csr=ew_csr)
  assert tab.stride(0) == 2 * A and tab.data_ptr() % 16 == 0 and tab[:, A:].data_ptr() % 16 == 0
  return graph, st, tab, r.to(dev)[perm].contiguous(), ew_csr


def _rowerr(what, name, got, ref, seg, lens, tol):
  err, _ = BC.segment_error(got, ref, seg)
  print('ROWERR %s %s %s' % (what, name, RC.class_errors(err, lens)))
  BC.assert_segments(got, ref, seg, lens, tol, '%s %s' % (what, name))


# ------------------------------------------------------------------------------------------------
# attention backward: ds
# ------------------------------------------------------------------------------------------------
def _run_ds(graph, st, r_csr, c, variant, form, tab, dq=None):
  alpha = torch.tensor([BC.RAW_SCALE if variant == 'raw' else BC.ALPHA], device=tab.device)
  kw = dict(scale=None if variant == 'noscale' else alpha, scale_sigmoid=variant != 'raw', dq=dq)
  ws = _hub_ws(graph, c.h, c.h * c.dk, form, tab)
  if variant == 'rpos':                 # r stored in the transposed graph's order, read through csr_from_t
    gt, t_from_csr = graph.transposed_positions()
    r_t = r_csr[t_from_csr.long()].contiguous()
    assert not torch.equal(r_t, r_csr)
    ds = ops.attention_rows_bwd_dq(graph, st, r_t, rpos=graph.csr_positions(), hub_ws=ws, **kw)
  else:
    ds = ops.attention_rows_bwd_dq(graph, st, r_csr, hub_ws=ws, **kw)
  torch.cuda.synchronize()
  if ws is not None:                    # the chunk kernels ran: per-chunk statistics (and d q partials) were written
    used = graph.n_long_chunks * (3 * c.h + (c.h * c.dk if dq is not None else 0))
    assert bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all())
  return ds[:graph.e]


def _ds_scale(variant):
  s = 1.0 / (1.0 + math.exp(-BC.ALPHA))
  return {'noscale': 1.0 / s, 'raw': BC.RAW_SCALE / s}.get(variant, 1.0)


@pytest.mark.parametrize('case', BC.DS_CASES, ids=BC.ds_id)
def test_attention_bwd_ds(dev, case):
  c = case.ref
  ei, lens, side = RC.graph_edges(c.graph)
  graph, st, tab, r_csr, ew_csr = _operands(c, dev)
  assert side == 0 and (case.hubs == 'chunks' or graph.n_long_rows > 0)
  ds = _run_ds(graph, st, r_csr, c, case.variant, case.hubs, tab)
  perm = graph.perm_long.cpu()
  ref = BC.reference64(c).ds[perm] * _ds_scale(case.variant)
  _rowerr(BC.ds_id(case), 'ds', ds, ref, ei[0][perm], lens, BC.tolerances(c, 'ds'))
  assert torch.equal(_run_ds(graph, st, r_csr, c, case.variant, case.hubs, tab), ds), 'two launches differ'


# ------------------------------------------------------------------------------------------------
# attention backward: d q formed in the same launch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', BC.DQ_CASES, ids=BC.dq_id)
def test_attention_bwd_fused_dq(dev, case):
  c = case.ref
  ei, lens, side = RC.graph_edges(c.graph)
  graph, st, tab, r_csr, ew_csr = _operands(c, dev)
  A = c.h * c.dk
  assert side == 0 and _lib.lib().gnpde_attention_rows_bwd_dq_supported(c.h, c.dk) == 1

  def run():
    big = torch.full((graph.n, 2 * A), float('nan'), device=dev)
    return _run_ds(graph, st, r_csr, c, '', case.hubs, tab, dq=big[:, :A]), big

  ds, big = run()
  has = lens > 0
  assert bool(torch.isnan(big[:, A:]).all()), 'columns [A, 2A) were written'
  assert bool(torch.isnan(big[~has.to(dev), :A]).all()), 'a row without entries was written'
  ref = BC.reference64(c)
  perm = graph.perm_long.cpu()
  got, keep = BC.node_rows(big[:, :A], lens)
  _rowerr(BC.dq_id(case), 'dq', got, ref.dq[keep], keep, lens, BC.tolerances(c, 'dq'))
  _rowerr(BC.dq_id(case), 'ds', ds, ref.ds[perm], ei[0][perm], lens, BC.tolerances(c, 'ds'))
  # the same launch without d q gives the same ds, bit for bit; and two launches agree
  assert torch.equal(_run_ds(graph, st, r_csr, c, '', case.hubs, tab), ds), 'ds differs between DQ on and off'
  ds2, big2 = run()
  assert torch.equal(ds2, ds) and torch.equal(big2[has.to(dev), :A], big[has.to(dev), :A]), 'two launches differ'


# ------------------------------------------------------------------------------------------------
# head_rowsum: d q over the rows, d k over the rows of the transposed graph
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', BC.HR_CASES, ids=BC.hr_id)
def test_head_rowsum(dev, case):
  c = case.ref
  ei, lens, side = RC.graph_edges(c.graph)
  graph = _graph(c.graph, str(dev))
  table, r, ew = BC.inputs(c)
  A = c.h * c.dk
  by_column = case.side == 'dk'
  assert side == int(by_column) and _lib.lib().gnpde_head_rowsum_supported(c.h, c.dk) == 1
  tab = table.to(dev)
  # ds: the float64 reference rounded to fp32, in CSR order -- the kernel is judged alone, not through another kernel's output
  ds_edge = BC.reference64(c).ds.float()
  ds_csr = ds_edge.to(dev)[graph.perm_long].contiguous()
  if by_column:
    view, pos = graph.transposed_positions()
    feat, col0 = tab[:, :A], A
    assert not torch.equal(pos.long(), torch.arange(graph.e, device=dev))
  else:
    view, pos, feat, col0 = graph, None, tab[:, A:], 0
  assert feat.data_ptr() % 16 == 0 and feat.stride(0) % 4 == 0 and ds_csr.data_ptr() % 16 == 0
  assert case.hubs == 'chunks' or view.n_long_rows > 0

  def run():
    big = torch.full((graph.n, 2 * A), float('nan'), device=dev)
    ws = _hub_ws(view, c.h, A, case.hubs, tab)
    ops.head_rowsum(view, ds_csr, feat, c.h, c.dk, 1.0 / math.sqrt(c.dk), big[:, col0:col0 + A], pos=pos, hub_ws=ws)
    torch.cuda.synchronize()
    if ws is not None:
      used = view.n_long_chunks * A
      assert bool(torch.isfinite(ws[:used]).all()) and bool(torch.isnan(ws[used:]).all())
    return big

  big = run()
  has = (lens > 0).to(dev)
  other = slice(A, 2 * A) if col0 == 0 else slice(0, A)
  assert bool(torch.isnan(big[:, other]).all()), 'columns outside the slice were written'
  assert bool(torch.isnan(big[~has, col0:col0 + A]).all()), 'a row without entries was written'
  ref = BC.head_sums(ei, ds_edge.double(), table, c.h, c.dk, by_column)
  got, keep = BC.node_rows(big[:, col0:col0 + A], lens)
  _rowerr(BC.hr_id(case), 'dk' if by_column else 'dq', got, ref[keep], keep, lens, BC.tolerances(c, 'dk' if by_column else 'dq'))
  assert torch.equal(run()[has, col0:col0 + A], big[has, col0:col0 + A]), 'two launches differ'


# ------------------------------------------------------------------------------------------------
# gnpde_softmax_rows_bwd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', BC.SB_CASES, ids=BC.sb_id)
def test_softmax_rows_bwd(dev, c):
  ei, lens, side = RC.graph_edges(c.graph)
  graph, st, tab, r_csr, ew_csr = _operands(c, dev)
  table, r, ew = BC.inputs(c)
  att32 = BC.reference64(c).att.float()          # edge order, from the float64 oracle
  alpha = torch.tensor([BC.ALPHA], device=dev)

  def run():
    ds = ops.softmax_rows_bwd(graph, att32.to(dev), r_csr, edge_w_csr=ew_csr, scale=alpha, scale_sigmoid=True)
    torch.cuda.synchronize()
    return ds[:graph.e]

  ds = run()
  perm = graph.perm_long.cpu()
  ref = BC.ds_from_att(ei, att32.double(), r.double(), None if ew is None else ew.double(), lens.numel())[perm]
  _rowerr(BC.sb_id(c), 'ds', ds, ref, ei[0][perm], lens, BC.tolerances(c, 'ds'))
  assert torch.equal(run(), ds), 'two launches differ'


# ------------------------------------------------------------------------------------------------
# gnpde_head_spmm: the float4 lines and every instantiation of the generic kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', BC.HS_CASES, ids=BC.hs_id)
def test_head_spmm(dev, c):
  name, ds_edge, table = BC.head_spmm_inputs(c)
  ei, lens, side = RC.graph_edges(name)
  graph = _graph(name, str(dev))
  A = c.h * c.dk
  tab = table.to(dev)
  ds_csr = ds_edge.to(dev)[graph.perm_long].contiguous()
  feat, col0 = (tab[:, :A], A) if c.by_column else (tab[:, A:], 0)
  assert (graph.n_long_cols if c.by_column else graph.n_long_rows) == len(RC.HUBS)

  def run():
    big = torch.full((graph.n, 2 * A), float('nan'), device=dev)
    out = big[:, col0:col0 + A]
    # the preconditions of the line the case is listed under (bwd_cases.head_spmm_line restates the launcher's switch)
    line = BC.head_spmm_line(c.h, c.dk)
    aligned16 = feat.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0 and (2 * A) % 4 == 0
    aligned8 = feat.data_ptr() % 8 == 0 and out.data_ptr() % 8 == 0 and (2 * A) % 2 == 0
    assert (line[0] == 'vec4') == (c.dk % 4 == 0 and (A // 4) & (A // 4 - 1) == 0 and aligned16)
    assert line[0] == 'vec4' or (line[1] == 2) == (c.dk % 2 == 0 and aligned8)
    ops.head_spmm(graph, ds_csr, feat, c.h, c.dk, 0.37, by_column=c.by_column, out=out)
    torch.cuda.synchronize()
    return big

  big = run()
  other = slice(A, 2 * A) if col0 == 0 else slice(0, A)
  assert bool(torch.isnan(big[:, other]).all()), 'columns outside the slice were written'
  ref, tol, lens_ = BC.head_spmm_reference(c)
  got = big[:, col0:col0 + A]
  assert float(got[(lens == 0).to(dev)].abs().max()) == 0.0, 'an empty segment is not a zero row'
  _rowerr(BC.hs_id(c), 'out', got, ref * (0.37 * math.sqrt(c.dk)), torch.arange(graph.n), lens, tol)
  assert torch.equal(run()[:, col0:col0 + A], got), 'two launches differ'


def test_unsupported_shapes_raise(dev):
  """d q asked of a pair the fused kernel does not have, and a head shape head_rowsum does not have: GNPDE_ESHAPE, nothing launched."""
  c = BC.RefCase('hubs', 8, 16, False)
  graph, st, tab, r_csr, ew_csr = _operands(c, dev)
  assert _lib.lib().gnpde_attention_rows_bwd_dq_supported(8, 16) == 0 and _lib.lib().gnpde_head_rowsum_supported(8, 8) == 0
  big = torch.full((graph.n, 128), float('nan'), device=dev)
  with pytest.raises(_lib.GnpdeError, match='error -2'):
    ops.attention_rows_bwd_dq(graph, st, r_csr, dq=big)
  ds = torch.zeros(graph.e, 8, device=dev)
  with pytest.raises(_lib.GnpdeError, match='error -2'):
    ops.head_rowsum(graph, ds, tab[:, :64], 8, 8, 1.0, big[:, :64])
  torch.cuda.synchronize()
  assert bool(torch.isnan(big).all())
  assert [(h, dk) for h in (1, 2, 4, 8, 3) for dk in (4, 8, 16, 12) if _lib.lib().gnpde_head_rowsum_supported(h, dk)] == BC.HR_PAIRS
  assert [(h, dk) for h in (1, 2, 4, 8, 3) for dk in (4, 8, 16, 12) if _lib.lib().gnpde_attention_rows_bwd_dq_supported(h, dk)] == BC.DQ_PAIRS
