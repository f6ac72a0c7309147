"""The helpers of tests/bwd_cases.py on the CPU: the inputs of every case of tests/test_bwd_dispatch_gpu.py are valid and the bound that
test applies holds for the reference alone.

* float64 autograd of L = sigmoid(alpha) sum r w through the oracle and index_add of the formula's ds give the same d q (by rows) and
  d k (by columns) to 1e-12: two independent derivations of one reference.
* ds sums to zero over every row, per head, once the edge weight is divided out.
* The oracle evaluated in fp32 stays <= helpers.TOL per segment against float64 on every case (bwd_cases._case turns a draw away
  otherwise: 73 draws for the 44 cases, at most 4 for one), so the device tolerance max(TOL, 3 x that error) lies in [TOL, 3 TOL] and is
  TOL wherever fp32 is not itself within a factor 3 of it.  Measured worst per length class (<=16 | 17..512 | >512) over the cases:
    ds   9.0e-6 | 2.3e-6 | 1.4e-6        d q  6.2e-6 | 4.2e-6 | 5.6e-6        d k  7.8e-6 | 1.3e-6 | 1.1e-6
  (the <= 16 class is the worst because a two-entry row's r - c cancels to a small fraction of r; d q of a hub row is a sequential fp32
  index_add over 1100 terms that cancel).
* The segments judged absolutely (reference below 1e-6 of the tensor's largest entry) are exactly the one-entry rows, where ds = 0 and
  d q = 0 identically; d k has none."""
import pytest
import torch

import bwd_cases as BC
import row_cases as RC
from helpers import TOL


def test_case_lists_cover_every_pair():
  assert {(c.ref.h, c.ref.dk) for c in BC.DS_CASES if c.ref.graph == 'hubs' and not c.variant} == set(BC.AB_PAIRS)
  for hubs in BC.HUB_FORMS:
    assert {(c.ref.h, c.ref.dk) for c in BC.DS_CASES if c.ref.graph == 'hubs' and c.ref.reweight and c.hubs == hubs} == set(BC.AB_PAIRS)
    assert {(c.ref.h, c.ref.dk) for c in BC.DQ_CASES if c.ref.graph == 'hubs' and c.hubs == hubs} == set(BC.DQ_PAIRS)
    for side, graph in (('dq', 'hubs'), ('dk', 'hubs_t')):
      assert {(c.ref.h, c.ref.dk) for c in BC.HR_CASES if c.side == side and c.ref.graph == graph and c.hubs == hubs} == set(BC.HR_PAIRS)
  assert sorted({c.ref.h for c in BC.DS_CASES if c.variant == 'rpos'}) == [1, 2, 4, 8]
  assert {c.variant for c in BC.DS_CASES} == {'', 'rpos', 'noscale', 'raw'}
  # d k never runs on a graph whose columns are short, d q / ds never on a transposed staircase
  assert all(c.ref.graph.endswith('_t') == (c.side == 'dk') for c in BC.HR_CASES)
  assert all(not c.ref.graph.endswith('_t') for c in BC.DS_CASES + BC.DQ_CASES)
  assert int(BC.segment_lens('hubs', True).max()) <= 40 and int(BC.segment_lens('hubs_t', True).max()) == 1100


def test_head_spmm_lines():
  """gnpde_head_spmm's switch, restated: the seven float4 lines and the six generic instantiations each have a shape."""
  assert [BC.head_spmm_line(h, dk) for h, dk in BC.HS_VEC4] == [('vec4', a4) for a4 in (1, 2, 4, 8, 16, 32, 64)]
  for (h, dk), (vw, cpl) in BC.HS_ANY.items():
    assert BC.head_spmm_line(h, dk) == ('any', vw, cpl), (h, dk)
  assert sorted(BC.HS_ANY.values()) == [(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2)]
  assert all(h * dk <= 256 for h, dk in BC.HS_VEC4 + list(BC.HS_ANY))


def test_segment_error_judges_zero_segments_absolutely():
  ref = torch.tensor([[2.0], [1.0], [0.0], [1e-9]], dtype=torch.float64)
  got = ref.clone().float()
  got[2, 0] = 1e-5            # segment 1 is zero in the reference: 1e-5 / 2.0 (the tensor's maximum)
  got[1, 0] += 1e-3           # segment 0: 1e-3 / 2.0
  seg = torch.tensor([0, 0, 1, 3])
  err, degenerate = BC.segment_error(got, ref, seg)
  assert degenerate.tolist() == [False, True, False, True]
  assert abs(float(err[0]) - 5e-4) < 1e-7 and abs(float(err[1]) - 5e-6) < 1e-9 and float(err[2]) == 0.0      # (got is fp32)
  lens = torch.tensor([2, 1, 0, 1])
  BC.assert_segments(got, ref, seg, lens, {'<=16': 1e-3}, 'fine')
  with pytest.raises(AssertionError, match=r'segment 0 \(2 entries\)'):
    BC.assert_segments(got, ref, seg, lens, TOL, 'too tight')


@pytest.mark.parametrize('c', BC.REF_CASES, ids=BC.ref_id)
def test_reference_is_consistent_and_fp32_stays_under_the_tolerance(c):
  ei, lens, side = RC.graph_edges(c.graph)
  table, r, ew = BC.inputs(c)
  ref = BC.reference64(c)
  n, A = lens.numel(), c.h * c.dk
  assert table.dtype == torch.float32 and table.shape == (n, 2 * A) and r.shape == (ei.shape[1],)
  assert ref.ds.dtype == torch.float64 and ref.ds.shape == (ei.shape[1], c.h) and ref.dq.shape == ref.dk.shape == (n, A)
  rows, cols = BC.segment_lens(c.graph, False), BC.segment_lens(c.graph, True)
  assert torch.equal(cols if side else rows, lens)

  # two derivations of d q / d k
  for name, got, by_column in (('dq', ref.dq, False), ('dk', ref.dk, True)):
    formula = BC.head_sums(ei, ref.ds, table, c.h, c.dk, by_column)
    assert float((formula - got).abs().max()) <= 1e-12 * max(1.0, float(got.abs().max())), name
  # ds / edge_w sums to zero over every row, per head
  plain = ref.ds if ew is None else ref.ds / ew.double().unsqueeze(1)
  sums = torch.zeros(n, c.h, dtype=torch.float64).index_add_(0, ei[0], plain)
  assert float(sums.abs().max()) <= 1e-12 * float(ref.ds.abs().max())

  # the fp32 oracle alone, per segment and length class; the zero segments
  errs = BC.oracle_fp32_errors(c)
  for what in ('ds', 'dq', 'dk'):
    err, degenerate, lens_ = errs[what]
    per_class = RC.class_errors(err, lens_)
    print('FP32ERR %s %s %s' % (BC.ref_id(c), what, per_class))
    assert float(err.max()) <= TOL, (what, per_class)
    tol = BC.tolerances(c, what)              # TOL except where fp32 itself is within a factor 3 of it; never more than 3 TOL
    assert set(tol) == set(per_class) and all(TOL <= t <= 3 * TOL and t == max(TOL, 3 * per_class[k]) for k, t in tol.items())
    expect = (rows == 1) if what in ('ds', 'dq') else torch.zeros(n, dtype=torch.bool)
    assert torch.equal(degenerate, expect[:degenerate.numel()]) and not bool(expect[degenerate.numel():].any()), what
  one = (rows == 1).nonzero().flatten()
  if one.numel():
    assert float(ref.ds[torch.isin(ei[0], one)].abs().max()) == 0.0 and float(ref.dq[one].abs().max()) == 0.0


@pytest.mark.parametrize('c', BC.HS_CASES, ids=BC.hs_id)
def test_head_spmm_reference(c):
  graph, ds, table = BC.head_spmm_inputs(c)
  ei, lens, side = RC.graph_edges(graph)
  ref, tol, lens_ = BC.head_spmm_reference(c)
  assert side == int(c.by_column) and torch.equal(lens_, BC.segment_lens(graph, c.by_column))
  assert ref.dtype == torch.float64 and ref.shape == (lens.numel(), c.h * c.dk)
  print('FP32ERR %s %s' % (BC.hs_id(c), tol))
  assert tol == {name: TOL for name in tol}, tol      # well-conditioned sums of standard-normal terms: fp32 is nowhere near TOL / 3
