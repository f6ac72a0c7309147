"""The inputs of tests/test_spmm_dispatch_gpu.py (tests/agg_cases.py), checked on the host library without a device: the graphs have the rows
and bins the cases assume, the pair block is made of pairs under both row deals, every launch is planned on the line it is listed under,
and the float64 reference is far enough from fp32 rounding that helpers.TOL judges the kernels and not the reference."""
import ctypes

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
import agg_cases as AC
import row_cases as RC
from helpers import TOL

BASE = 1 << 20          # operand addresses: only their alignment is read
T = torch.zeros(8)      # every epilogue operand: one aligned host tensor (nothing is dereferenced)


@pytest.fixture(scope='module')
def graphs():
  return {kind: G.CSRGraph(AC.graph_edges(kind)[0], AC.N) for kind in AC.KINDS}


@pytest.mark.parametrize('kind', AC.KINDS)
def test_graph_has_the_rows_the_cases_assume(graphs, kind):
  ei, lens, w = AC.graph_edges(kind)
  g = graphs[kind]
  assert lens.numel() == AC.N and lens[:2 * len(AC.PAIRS)].tolist() == [v for p in AC.PAIRS for v in p]
  have = set(lens.tolist())
  assert set(AC.STAIRS + AC.HUBS + [AC.MULTI]) <= have and int((lens == 0).sum()) >= 5
  assert AC.MULTI > 8 * AC.LONG_ROW and AC.MULTI % (8 * AC.LONG_ROW) > AC.LONG_ROW      # the eight-at-a-time loop once and a remainder of two
  assert (g.n_bin16, g.n_bin64, g.n_long_rows, g.n_long_chunks) == RC.expected_bins(lens)
  hubs = lens[lens > AC.LONG_ROW].tolist()
  assert sorted(hubs) == sorted(AC.HUBS + [AC.MULTI, 513, 600, 513, 513, 1024]) and g.n_long_chunks == sum(-(-v // 512) for v in hubs)
  assert (2 * g.n_bin16 >= AC.N) == (kind == 'short')
  # one row lists a column twice; the MULTI row repeats columns; every other row's columns are distinct
  key = ei[0] * AC.N + ei[1]
  uniq, cnt = torch.unique(key, return_counts=True)
  dup_rows = set((uniq[cnt > 1] // AC.N).tolist())
  multi = int((lens == AC.MULTI).nonzero())
  assert multi in dup_rows and len(dup_rows) == 2 and int(lens[list(dup_rows - {multi})[0]]) == AC.DUP_LEN
  assert float(w.min()) >= 0.01 and float(w.max()) <= 0.31
  # the row range of part (e) begins at an odd row inside the block, behind two hub rows
  b = AC.ROW_RANGE_BEGIN
  assert b % 2 == 1 and b < 2 * len(AC.PAIRS) and int((lens[:b] > AC.LONG_ROW).sum()) == 2 and int((lens[b:] > AC.LONG_ROW).sum()) >= 2


def _row_map(deal_knob):
  """(row_shift, the 8 row lists) of gnpde_xcd_row_map for rows [0, N) with the deal forced"""
  ops.tune(10, deal_knob)
  try:
    shift, per = ctypes.c_int32(), ctypes.c_int32()
    L = _lib.lib()
    assert L.gnpde_xcd_row_map(0, AC.N, 0, ctypes.byref(shift), ctypes.byref(per), None) == 0
    m = torch.zeros(AC.XCDS * per.value, dtype=torch.int32)
    assert L.gnpde_xcd_row_map(0, AC.N, 0, ctypes.byref(shift), ctypes.byref(per), ctypes.c_void_p(m.data_ptr())) == 0
  finally:
    ops.tune(10, 0)
  return shift.value, m.view(AC.XCDS, per.value).tolist()


@pytest.mark.parametrize('knob,shift', [(1, -1), (2, 4)], ids=['contiguous', 'hashed'])
def test_pair_block_is_made_of_pairs_under_both_deals(knob, shift):
  got_shift, lists = _row_map(knob)
  assert got_shift == shift and lists == AC.xcd_lists(AC.N, 0, shift)          # the library's lists are the host restatement's
  seen = sorted(r for rows in lists for r in rows if r >= 0)
  assert seen == list(range(AC.N))                                            # every row exactly once
  where = {r: (x, i) for x, rows in enumerate(lists) for i, r in enumerate(rows) if r >= 0}
  for i in range(len(AC.PAIRS)):
    (x0, r0), (x1, r1) = where[2 * i], where[2 * i + 1]
    assert x0 == x1 and r0 % 2 == 0 and r1 == r0 + 1, (i, AC.PAIRS[i])         # rows (r0, r0 + 1) of one XCD's list: one wave's two halves
  if shift < 0:
    for rows in lists:
      assert len(rows) % 2 == 1 and all(r >= 0 for r in rows)                 # an odd share: the last pair has no second row
    assert all(r < len(lists[0]) for r in range(2 * len(AC.PAIRS)))           # the block lies in XCD 0's share
  # ... and under a row range that begins at an odd row the pairs are (odd, even) ones: every row still exactly once
  b = AC.ROW_RANGE_BEGIN
  sub = AC.xcd_lists(AC.N, b, shift)
  assert sorted(r for rows in sub for r in rows if r >= 0) == list(range(b, AC.N))


def _epilogue(launch):
  stage, with_x0, sigmoid = launch
  kw = {name: T for name in AC.READS[stage] + AC.WRITES[stage] if name not in ('p0', 'p1')}
  if stage == 'LINCOMB':
    kw.update(prev=(T, T), coef=AC.COEF)
  return ops.make_epilogue(T, T if with_x0 else None, T if with_x0 else None, sigmoid, stage=getattr(_lib, 'STAGE_' + stage), dt=AC.DT, **kw)


def _plan(g, d, launch, ld=None, u=BASE, **kw):
  ld = d if ld is None else ld
  if launch[0] == 'plain':
    return ops.spmm_plan(g, u, d, ld, None, plain_out_addr=2 * BASE, ws_addr=3 * BASE, **kw)
  return ops.spmm_plan(g, u, d, ld, _epilogue(launch), ws_addr=3 * BASE, **kw)


@pytest.mark.parametrize('kind', AC.KINDS)
def test_every_launch_is_planned_on_its_line(graphs, kind):
  g = graphs[kind]
  lines = set()
  for d in AC.WIDTHS:
    for launch in AC.launches(d):
      what = (kind, d, AC.launch_id(launch))
      p = _plan(g, d, launch)
      assert AC.plan_line(p) == AC.intended(kind, d), what
      assert p.fold_kind == AC.fold_kind(kind, d, launch) and p.fold_kind == ('reduce4' if d in AC.LANES16 else 'scalar'), what
      assert (p.lo, p.defer, p.forked) == (0, 0, 0) and p.full == int(d in (128, 256)), what
      lines.add(AC.plan_line(p))
      if launch[0] != 'plain' and d in (80, 100, 128):        # part (b): with tickets the row-pair kernel folds the prefetchable stages itself
        p = _plan(g, d, launch, tickets=True)
        want = 'in_kernel' if (kind == 'short' and launch[0] in AC.PREFETCHABLE) else 'reduce4'
        assert p.fold_kind == want == AC.fold_kind(kind, d, launch, tickets=True), what
      if d in AC.LANES16:                                     # part (d): the bf16 operand takes the same line
        p = _plan(g, d, launch, lo=True)
        assert (AC.plan_line(p), p.lo, p.fold_kind) == (AC.intended(kind, d), 1, 'reduce4_lo'), what
  # every line of the table is among the cases: seven rows lines per lane type, and row pairs / wide 32 / wide 64 on 16-byte lanes
  rows16 = {(16, 'rows') + t for t in ((8, 1, 4), (16, 1, 4), (64, 2, 2), (64, 3, 1), (64, 4, 1))}
  narrow = {(b, 'rows') + t for b in (8, 4) for t in AC._SEVEN}
  special = {(16, 'pair', 32, 1, 16)} if kind == 'short' else {(16, 'wide', 32, 1, 8)}
  assert lines == rows16 | narrow | special | {(16, 'wide', 64, 1, 8)}


def test_quad_row_range_and_demoted_lanes_are_planned_as_listed(graphs):
  g = graphs['short']
  rhs, rk3 = ('RHS', True, True), ('RK3', True, True)
  ops.tune(18, 2)
  try:
    for d in (80, 128):
      p = _plan(g, d, ('RK2C', True, True), lo=True)
      assert AC.plan_line(p) == AC.intended('short', d, quad=True) == (16, 'quad_lo', 16, 1, 16) and p.fold_kind == 'reduce4_lo'
  finally:
    ops.tune(18, 0)
  # part (f): a state 4 / 8 bytes past an aligned address, a row stride of 129 / 130 floats
  for launch in (rhs, rk3):
    for lanes, kw in ((4, dict(u=BASE + 4)), (8, dict(u=BASE + 8)), (4, dict(ld=129)), (8, dict(ld=130))):
      p = _plan(g, 128, launch, **kw)
      assert AC.plan_line(p) == AC.intended('short', 128, lanes=lanes) and p.fold_kind == AC.fold_kind('short', 128, launch, lanes=lanes) == 'scalar', kw
  assert AC.intended('short', 128, lanes=4) == (4, 'rows', 64, 2, 2) and AC.intended('short', 128, lanes=8) == (8, 'rows', 32, 2, 4)
  # part (e): a row range keeps the line and never folds in the kernel
  for kind in AC.KINDS:
    sub = G.CSRGraph(AC.graph_edges(kind)[0], AC.N)
    sub.set_row_range(AC.ROW_RANGE_BEGIN, AC.N)
    for d in (128, 50):
      for launch in (rhs, ('RK2C', True, True)):
        p = _plan(sub, d, launch, tickets=True)
        assert AC.plan_line(p) == AC.intended(kind, d) and p.fold_kind == AC.fold_kind(kind, d, launch), (kind, d)


@pytest.mark.parametrize('kind', AC.KINDS)
@pytest.mark.parametrize('d', [6, 128, 800])
def test_reference_alone_stays_within_half_the_tolerance(kind, d):
  """The same formulas in float32 on the CPU (the aggregation in edge order, one running sum per row) against the float64 reference, by
  the metric of the device test: at most TOL / 2 on every row, for the plain aggregation and all eleven stages with and without the
  source term.  What is left of TOL is the kernels'."""
  ei, lens, w = AC.graph_edges(kind)
  worst = {}
  for launch in AC.launches(d, variants=True):
    ref32 = AC.reference(kind, d, launch, torch.float32)
    ref64 = AC.reference(kind, d, launch, torch.float64)
    for name in ref64:
      assert ref32[name].dtype == torch.float32 and ref64[name].dtype == torch.float64
      AC.worst(worst, AC.assert_rows(ref32[name], ref64[name], lens, TOL / 2, '%s d=%d %s %s (fp32 restatement)' % (kind, d, AC.launch_id(launch), name)))
  print('REFERR %s d=%d %s' % (kind, d, worst))
