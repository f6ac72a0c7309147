"""The aggregation's launch plan (gnpde_spmm_plan, plan_spmm in csrc/spmm.hip): which kernel, template line, grid and hub-row fold a call
takes -- the decision launch_spmm_rhs switches on, asked without a device.  tests/test_spmm_dispatch_gpu.py runs every line of the table
against the oracle and cannot see a wrong route that still computes the right numbers; this file pins the routes.

The expected values are literal tables, written from the dispatch code as it stood before the plan existed (dispatch_rows<4|2|1>,
dispatch_rows_lo, the a16 / a8 rules, the fold_in_kernel and defer conditions of launch_spmm_rhs), not taken from the planner.

Two host graphs of 600 rows, two hub rows (513 and 600 entries: two 512-entry chunks each) and one empty row: the other rows have 3
entries (mostly short rows -> row pairs for 17..32 16-byte lanes) or 24 (-> the wide-row kernel)."""
import ctypes

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops

N = 600
BASE = 1 << 20          # operand addresses: only their alignment is read


def _host_graph(m, n=N, hubs=(513, 600, 0)):
  src, dst = [], []
  for i in range(n):
    k = hubs[i] if i < len(hubs) else m
    src.append(torch.full((k,), i))
    dst.append((torch.arange(k) + i) % n)
  return G.CSRGraph(torch.stack([torch.cat(src), torch.cat(dst)]).long(), n)


@pytest.fixture(scope='module')
def graphs():
  out = {'short': _host_graph(3), 'long': _host_graph(24)}
  # the preconditions of the two kinds of line (as tests/test_spmm_dispatch_gpu.py asserts them)
  assert 2 * out['short'].n_bin16 >= N and 2 * out['long'].n_bin16 < N
  for g in out.values():
    assert g.n_long_rows == 2 and g.n_long_chunks == 4
  return out


T = torch.zeros(8)      # every epilogue operand: one aligned host tensor (nothing is dereferenced)
STAGE_OPERANDS = {
  _lib.STAGE_RHS: dict(out_k=T), _lib.STAGE_EULER: dict(y=T, out_y=T),
  _lib.STAGE_RK1: dict(out_k=T, y=T, out_y=T), _lib.STAGE_RK2: dict(out_k=T, y=T, k1=T, out_y=T),
  _lib.STAGE_RK3: dict(out_k=T, y=T, k1=T, k2=T, out_y=T), _lib.STAGE_RK4: dict(y=T, k1=T, k2=T, k3=T, out_y=T),
  _lib.STAGE_RK1C: dict(out_y=T), _lib.STAGE_RK2C: dict(y=T, out_y=T), _lib.STAGE_RK3C: dict(k1=T, out_y=T),
  _lib.STAGE_RK4C: dict(y=T, k1=T, out_y=T), _lib.STAGE_LINCOMB: dict(out_k=T),
}
IN_KERNEL_STAGES = (_lib.STAGE_RHS, _lib.STAGE_EULER, _lib.STAGE_RK1C, _lib.STAGE_RK2C, _lib.STAGE_RK3C, _lib.STAGE_RK4C)
OTHER_STAGES = (_lib.STAGE_RK1, _lib.STAGE_RK2, _lib.STAGE_RK3, _lib.STAGE_RK4, _lib.STAGE_LINCOMB)


def epilogue(stage=_lib.STAGE_RHS, **over):
  kw = dict(STAGE_OPERANDS[stage])
  kw.update(over)
  return ops.make_epilogue(T, None, None, True, stage=stage, **kw)


def plan(g, d, ld=None, u=BASE, stage=_lib.STAGE_RHS, plain=False, **kw):
  ld = d if ld is None else ld
  if plain:
    return ops.spmm_plan(g, u, d, ld, None, plain_out_addr=2 * BASE, ws_addr=3 * BASE, **kw)
  return ops.spmm_plan(g, u, d, ld, epilogue(stage), ws_addr=3 * BASE, **kw)


def line(p):
  return (p.kernel, p.L, p.K, p.U)


# d -> (line on the short-row graph, line on the long-row graph); the widths and lines named in tests/test_spmm_dispatch_gpu.py
ROWS = lambda L, K, U: (('rows', L, K, U),) * 2     # noqa: E731
LANES16 = {24: ROWS(8, 1, 4), 64: ROWS(16, 1, 4),
           80: (('pair', 32, 1, 16), ('wide', 32, 1, 8)), 100: (('pair', 32, 1, 16), ('wide', 32, 1, 8)),
           128: (('pair', 32, 1, 16), ('wide', 32, 1, 8)),
           200: (('wide', 64, 1, 8),) * 2, 256: (('wide', 64, 1, 8),) * 2,
           300: ROWS(64, 2, 2), 520: ROWS(64, 3, 1), 800: ROWS(64, 4, 1)}
SEVEN = [(8, 1, 4), (16, 1, 4), (16, 2, 4), (32, 2, 4), (64, 2, 2), (64, 3, 1), (64, 4, 1)]
LANES8 = dict(zip([6, 30, 50, 90, 162, 302, 402], (ROWS(*t) for t in SEVEN)))
LANES4 = dict(zip([7, 15, 31, 63, 127, 191, 255], (ROWS(*t) for t in SEVEN)))
TABLE = [(16, d, v) for d, v in LANES16.items()] + [(8, d, v) for d, v in LANES8.items()] + [(4, d, v) for d, v in LANES4.items()]
KINDS = ('short', 'long')


def expected_grid(g, p, chunks=4, rows=N, row_begin=0):
  """8 * max(1, ceil((ceil(chunks / 8) + ceil(rows_per_xcd / rows per wave)) / waves per workgroup)), rows_per_xcd from gnpde_xcd_row_map"""
  shift, per = ctypes.c_int32(), ctypes.c_int32()
  assert _lib.lib().gnpde_xcd_row_map(row_begin, row_begin + rows, g.struct.xcd_deal, ctypes.byref(shift), ctypes.byref(per), None) == 0
  rows_per_wave = {'rows': 1, 'wide': 1, 'pair': 2, 'quad_lo': 4}[p.kernel]
  waves_per_block = {'rows': 4, 'wide': 1, 'pair': 1, 'quad_lo': 1}[p.kernel]
  assert p.block == 64 * waves_per_block
  waves = -(-chunks // 8) + -(-per.value // rows_per_wave)
  return 8 * max(1, -(-waves // waves_per_block))


@pytest.fixture(params=[1, 2], ids=['contiguous', 'hashed'])
def deal(request):
  """both ways of dealing the rows to the XCDs, forced (gnpde_tune(10, .)) whatever the graph builder chose"""
  ops.tune(10, request.param)
  try:
    yield request.param
  finally:
    ops.tune(10, 0)


@pytest.mark.parametrize('plain', [False, True], ids=['epilogue', 'plain'])
def test_every_dispatch_line(graphs, deal, plain):
  for lanes, d, want in TABLE:
    for kind, w in zip(KINDS, want):
      g = graphs[kind]
      p = plan(g, d, plain=plain)
      what = (kind, d)
      assert (p.lane_bytes, line(p)) == (lanes, w), what
      assert p.full == int(d in (128, 256)), what
      assert (p.lo, p.defer, p.forked) == (0, 0, 0), what
      assert p.fold_kind == ('reduce4' if lanes == 16 else 'scalar'), what
      assert p.grid == expected_grid(g, p), what


def test_row_shift_differs_between_the_two_deals():
  # (so that the grids above were computed for two different lists: 75 rows per XCD against 5 blocks of 16)
  L = _lib.lib()
  got = []
  for knob in (1, 2):
    ops.tune(10, knob)
    try:
      shift, per = ctypes.c_int32(), ctypes.c_int32()
      assert L.gnpde_xcd_row_map(0, N, 0, ctypes.byref(shift), ctypes.byref(per), None) == 0
      got.append((shift.value, per.value))
    finally:
      ops.tune(10, 0)
  assert got == [(-1, 75), (4, 80)]


def test_bf16_operand_takes_the_same_lines(graphs, deal):
  for d, want in LANES16.items():
    for kind, w in zip(KINDS, want):
      g = graphs[kind]
      for plain in (False, True):
        p = plan(g, d, plain=plain, lo=True)
        assert (p.lane_bytes, line(p), p.lo, p.full) == (16, w, 1, int(d in (128, 256))), (kind, d)
        assert p.fold_kind == 'reduce4_lo' and p.grid == expected_grid(g, p), (kind, d)
  # narrower lanes have no bf16 form
  for d in list(LANES8) + list(LANES4):
    with pytest.raises(_lib.GnpdeError, match='error -2.*16-byte lanes'):
      plan(graphs['short'], d, lo=True)


def test_quad_form_of_the_bf16_operand(graphs, deal):
  """gnpde_tune(18, 2): four rows per wave where d % 8 == 0, on the row-pair route only"""
  ops.tune(18, 2)
  try:
    for d, want in ((80, ('quad_lo', 16, 1, 16)), (128, ('quad_lo', 16, 1, 16)), (100, ('pair', 32, 1, 16))):
      p = plan(graphs['short'], d, lo=True)
      assert (line(p), p.lo, p.full) == (want, 1, int(want[0] == 'pair' and d == 128)), d
      assert p.grid == expected_grid(graphs['short'], p), d
      assert line(plan(graphs['long'], d, lo=True)) == ('wide', 32, 1, 8), d
    assert line(plan(graphs['short'], 128)) == ('pair', 32, 1, 16)       # the fp32 table is not concerned
  finally:
    ops.tune(18, 0)


def test_misaligned_operands_demote_the_lanes(graphs):
  g = graphs['short']
  assert (plan(g, 128, u=BASE + 4).lane_bytes, line(plan(g, 128, u=BASE + 4))) == (4, ('rows', 64, 2, 2))
  assert (plan(g, 128, u=BASE + 8).lane_bytes, line(plan(g, 128, u=BASE + 8))) == (8, ('rows', 32, 2, 4))
  # any operand counts: the workspace, the plain output, an epilogue operand
  assert ops.spmm_plan(g, BASE, 128, 128, epilogue(), ws_addr=3 * BASE + 8).lane_bytes == 8
  assert ops.spmm_plan(g, BASE, 128, 128, None, plain_out_addr=2 * BASE + 4, ws_addr=3 * BASE).lane_bytes == 4
  off = torch.zeros(16)[1:]                              # 4 bytes past an aligned address
  assert off.data_ptr() % 8 == 4
  p = ops.spmm_plan(g, BASE, 128, 128, epilogue(_lib.STAGE_EULER, y=off), ws_addr=3 * BASE)
  assert (p.lane_bytes, p.fold_kind) == (4, 'scalar')
  # the row stride counts
  assert plan(g, 128, ld=130).lane_bytes == 8 and plan(g, 128, ld=129).lane_bytes == 4


def test_padded_rows_keep_16_byte_lanes(graphs):
  for kind, want in zip(KINDS, (('pair', 32, 1, 16), ('wide', 32, 1, 8))):
    p = plan(graphs[kind], 126, ld=128, padded_rows=True)
    assert (p.lane_bytes, line(p), p.full, p.fold_kind) == (16, want, 0, 'reduce4'), kind
    p = plan(graphs[kind], 126, ld=128)                   # without the promise: 8-byte lanes
    assert (p.lane_bytes, line(p)) == (8, ('rows', 32, 2, 4)), kind
  p = plan(graphs['short'], 126, ld=126)
  assert (p.lane_bytes, line(p), p.fold_kind) == (8, ('rows', 32, 2, 4), 'scalar')


def test_fold_choice(graphs):
  g = graphs['short']
  for st in IN_KERNEL_STAGES:
    p = plan(g, 128, stage=st, tickets=True)
    assert (p.kernel, p.fold_kind, p.forked) == ('pair', 'in_kernel', 0), st
    assert plan(g, 128, stage=st).fold_kind == 'reduce4', st                                   # without tickets
    assert plan(graphs['long'], 128, stage=st, tickets=True).fold_kind == 'reduce4', st        # the wide-row kernel does not fold
    assert plan(g, 128, stage=st, tickets=True, lo=True).fold_kind == 'reduce4_lo', st
    assert plan(g, 126, ld=126, stage=st, tickets=True).fold_kind == 'scalar', st
    assert plan(g, 126, ld=128, padded_rows=True, stage=st, tickets=True).fold_kind == 'in_kernel', st
    p = plan(g, 128, stage=st, tickets=True, fork=True)
    assert (p.kernel, p.fold_kind, p.forked) == ('pair', 'reduce4', 1), st
    assert p.grid == expected_grid(g, p, chunks=0), st                                         # the chunks run on the other stream
  for st in OTHER_STAGES:
    assert plan(g, 128, stage=st, tickets=True).fold_kind == 'reduce4', st
  assert plan(g, 128, plain=True, tickets=True).fold_kind == 'reduce4'
  try:
    ops.agg_fold_launch(1)
    for st in IN_KERNEL_STAGES:
      assert plan(g, 128, stage=st, tickets=True).fold_kind == 'reduce4', st
  finally:
    ops.agg_fold_launch(0)
  assert plan(g, 128, tickets=True).fold_kind == 'in_kernel'
  # a graph without hub rows has nothing to fold
  p = plan(_host_graph(3, hubs=()), 128, tickets=True, fork=True)
  assert (p.kernel, p.fold_kind, p.forked) == ('pair', 'none', 0)


def test_row_range_never_folds_in_the_kernel():
  g = _host_graph(3)
  g.set_row_range(300, N)
  p = plan(g, 128, tickets=True)
  assert (p.kernel, p.fold_kind) == ('pair', 'reduce4')
  assert p.grid == expected_grid(g, p, rows=300, row_begin=300)
  with pytest.raises(_lib.GnpdeError, match='error -1.*deferred'):
    plan(g, 128, defer=True)
  with pytest.raises(_lib.GnpdeError, match='error -1.*fork'):
    plan(g, 128, fork=True)


def test_defer_only_where_the_row_pair_kernel_runs_alone(graphs):
  g = graphs['short']
  for kw in (dict(d=128), dict(d=80), dict(d=100), dict(d=126, ld=128, padded_rows=True), dict(d=128, tickets=True)):
    p = plan(g, **kw, defer=True)
    assert (p.kernel, p.defer, p.lo, p.forked) == ('pair', 1, 0, 0), kw
    assert p.fold_kind == ('in_kernel' if kw.get('tickets') else 'reduce4'), kw
  refused = [(g, dict(d=64)), (g, dict(d=256)), (g, dict(d=126, ld=128)), (g, dict(d=128, u=BASE + 8)), (g, dict(d=128, lo=True)),
             (g, dict(d=128, fork=True)), (graphs['long'], dict(d=128)), (graphs['long'], dict(d=80))]
  for gg, kw in refused:
    with pytest.raises(_lib.GnpdeError, match='error -1.*deferred hub weights need the row-pair kernel'):
      plan(gg, **kw, defer=True)
    assert plan(gg, **kw).defer == 0                      # the same call without the request is planned
  # gnpde_tune(9, .) times one kind of work item alone: not a launch to hand the weights to
  ops.tune(9, 2)
  try:
    with pytest.raises(_lib.GnpdeError, match='error -1.*deferred'):
      plan(g, 128, defer=True)
    assert plan(g, 128, tickets=True).fold_kind == 'reduce4'
  finally:
    ops.tune(9, 0)


def test_adjoint_dot_slots_are_the_one_row_per_wave_grid_plus_the_hub_rows(graphs, deal):
  L = _lib.lib()
  for kind in KINDS:
    g = graphs[kind]
    p = plan(graphs['long'], 128)                         # a one-row-per-wave line
    assert p.kernel == 'wide'
    assert L.gnpde_adjoint_rows_dot_slots(g.ref(), 128) == expected_grid(g, p) + 2 == p.grid + 2


def test_refusals_come_before_any_launch(graphs):
  """What the launch refuses, the plan refuses with the same code -- and both without a device: the launchers validate first."""
  L = _lib.lib()
  g = graphs['short']
  with pytest.raises(_lib.GnpdeError, match='too large'):
    plan(g, 1025)
  with pytest.raises(_lib.GnpdeError, match='error -2.*too large'):
    plan(g, 514, u=BASE + 8)
  with pytest.raises(_lib.GnpdeError, match='error -1'):
    ops.spmm_plan(g, BASE, 128, 128, epilogue(), plain_out_addr=2 * BASE)           # both an epilogue and a plain output
  with pytest.raises(_lib.GnpdeError, match='error -1'):
    ops.spmm_plan(g, BASE, 128, 64, epilogue())                                       # ld < d
  # a null operand that the stage reads (every stage, operand by operand), and an output on the gathered table
  for st, operands in STAGE_OPERANDS.items():
    for name in operands:
      if st == _lib.STAGE_LINCOMB:
        continue
      with pytest.raises(_lib.GnpdeError, match='error -1.*%s is null' % name):
        ops.spmm_plan(g, BASE, 128, 128, epilogue(st, **{name: None}))
  with pytest.raises(_lib.GnpdeError, match='error -1.*LINCOMB without output'):
    ops.spmm_plan(g, BASE, 128, 128, epilogue(_lib.STAGE_LINCOMB, out_k=None))
  with pytest.raises(_lib.GnpdeError, match='error -1.*LINCOMB needs y'):
    ops.spmm_plan(g, BASE, 128, 128, epilogue(_lib.STAGE_LINCOMB, out_y=T))
  with pytest.raises(_lib.GnpdeError, match='error -1.*aliases'):
    ops.spmm_plan(g, T.data_ptr(), 128, 128, epilogue())
  with pytest.raises(_lib.GnpdeError, match='error -1.*bad stage'):
    ops.spmm_plan(g, BASE, 128, 128, ops.make_epilogue(T, None, None, True, stage=11, out_k=T))
  with pytest.raises(_lib.GnpdeError, match='error -1.*x0 given without beta'):
    ops.spmm_plan(g, BASE, 128, 128, ops.make_epilogue(T, None, T, True, out_k=T))
  # the launch itself: the same refusal with host tensors, so nothing can have been launched
  d = 128
  u, w = torch.zeros(N, d), torch.zeros(g.e)
  ws = torch.zeros(L.gnpde_spmm_workspace_bytes(g.ref(), d), dtype=torch.uint8)
  vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
  for st, name in ((_lib.STAGE_RK4C, 'k1'), (_lib.STAGE_EULER, 'y'), (_lib.STAGE_RHS, 'out_k')):
    epi = epilogue(st, **{name: None})
    assert L.gnpde_spmm_rhs(g.ref(), vp(w), vp(u), d, d, ctypes.byref(epi), vp(ws), ws.numel(), None) == -1
    assert ('%s is null' % name) in L.gnpde_last_error().decode()
