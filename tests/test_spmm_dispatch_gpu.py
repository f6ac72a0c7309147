"""Every launch line of the aggregation (plan_spmm / launch_spmm_rhs in csrc/spmm.hip) and every stage of its epilogues
against float64, judged row by row (tests/agg_cases.py: the graphs, the operands, the references, the metric; tests/test_agg_cases_cpu.py
checks those inputs on the host).  Two graphs of 1208 rows -- `short` (rows of 1..16 entries: the row-pair line) and `long` (17..40: the
wide-row line) -- both with a staircase of row lengths on either side of every batch and class boundary, nine hub rows of 513..4609
entries (2..10 chunks), empty rows and a block of prescribed row pairs.  Before every launch the library is asked for its plan with the
call's own operand addresses and the graph's cached workspace (ops.spmm_plan) and must name the line below; every output is prefilled with
NaN and must come back finite; every row must be within helpers.TOL of float64 by its OWN scale; every operand that is only read must be
bit-unchanged.  Each launch prints a ROWERR line with the worst row error per length class.

dispatch line                                                                     case                                              part
------------------------------------------------------------------------------------------------------------------------------------------
spmm_rows_kernel<VEC, L, K, U>, 16-byte lanes: (8,1,4) (16,1,4) (64,2,2) (64,3,1) (64,4,1)  d = 24, 64, 300, 520, 800, both graphs     a, c
spmm_rows_kernel, 8-byte lanes, the seven lines (8,1,4) .. (64,4,1)                d = 6, 30, 50, 90, 162, 302, 402, both graphs       a, c, e
spmm_rows_kernel, 4-byte lanes, the same seven lines                               d = 7, 15, 31, 63, 127, 191, 255, both graphs       a, c
spmm_pair_kernel<4, FULL> (17..32 lanes, mostly short rows): own rows, shared-row  short, d = 80, 100 (column predicate), 128 (FULL);  a, b, c, e
  fallback, hub / empty / missing partner, hub chunks as shared-row items          the pair block and the odd shares of the XCDs
spmm_wide_kernel<4, 32, 8, FULL>                                                   long, d = 80, 100, 128                              a, c, e
spmm_wide_kernel<4, 64, 8, FULL>                                                   d = 200, 256 (FULL), both graphs                    a, c
plain aggregation (plain_out, no epilogue) on each of these lines                  the first launch of every case                      a, d
the stage algebra: epilogue_pre (RHS, EULER, RK1C..RK4C) and epilogue<> / stage_store  all eleven stages on every line; at d = 100, 50, a, d
  (RK1..RK4, LINCOMB with two earlier derivatives, out_k and out_y)                31 also without x0 and with alpha taken as it is
hub-row fold, spmm_long_reduce4_kernel<false> -> fold_long_row<false>: fold_stage    every LANES16 width (second column pass at d = 300,  a, c, e
  (prefetchable stages) | epilogue<4> (the others) | plain                         520, 800); 2..10 chunks: both loops of the fold
hub-row fold, scalar spmm_long_reduce_kernel -> epilogue<1>                        every LANES8 / LANES4 width; d = 128 demoted        a, c, e, f
hub-row fold inside the row-pair launch (tickets): fold_long_row<true>              short, d = 80, 100, 128, prefetchable stages,       b
                                                                                   with and without x0, against float64
both row deals to the XCDs forced (gnpde_tune(10, 1 | 2))                          d = 24, 128, 256, 50, 31, RK4C and RK3              c
bf16 gather operand (LO instantiations, spmm_long_reduce4_kernel<true>, the         every LANES16 width, all stages, an exactly          d
  shadow store of out_y); spmm_quad_lo_kernel (gnpde_tune(18, 2))                  representable table; quad: short, d = 80, 128
a row range [b, n) with b odd inside the pair block                                d = 128, 50, RHS and RK2C: rows < b keep their bits  e
lanes demoted by a misaligned state or an odd row stride (raw entry point)          short, d = 128 at +4 / +8 bytes and ld = 129 / 130   f
a width past the table                                                             d = 257 on 4-byte lanes: a shape error               g
not here: the forked route and the deferred hub weights (gnpde_rhs_eval only: tests/test_spmm_plan_cpu.py pins the plans,
tests/test_one_launch_attention_gpu.py and tests/test_in_kernel_fold_gpu.py run them); attn_spmm_kernel (tests/test_attention_routes_gpu.py);
the adjoint row kernels (tests/test_adjoint_native_gpu.py).
"""
import ctypes
import functools

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
import agg_cases as AC
import row_cases as RC
from helpers import TOL, assert_parity

pytestmark = pytest.mark.gpu

N = AC.N
NAN = float('nan')


@functools.lru_cache(maxsize=None)
def _graph(kind, dev):
  ei, lens, w = AC.graph_edges(kind)
  graph = G.CSRGraph(ei.to(dev), N)
  # a change of the generator must not quietly move a case to another line of the table
  assert (graph.n_bin16, graph.n_bin64, graph.n_long_rows, graph.n_long_chunks) == RC.expected_bins(lens), kind
  assert (2 * graph.n_bin16 >= N) == (kind == 'short') and graph.n_long_rows >= 2
  return graph, ops.edge_to_csr_mean(graph, w.to(dev))


@pytest.fixture(scope='module')
def graphs(dev):
  out = {}
  for kind in AC.KINDS:
    ei, lens, w = AC.graph_edges(kind)
    out[kind] = (ei, w) + _graph(kind, str(dev))
  return out


def _workspace(graph, d):
  """the workspace ops.spmm / ops.spmm_rhs will hand the launch (graph.workspace caches it by tag and size)"""
  return graph.workspace('spmm%d' % d, _lib.lib().gnpde_spmm_workspace_bytes(graph.ref(), d))


def _bits(t):
  return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


class Case(object):
  """The device operands of one (graph, d): uploaded once, a pristine copy of each kept to compare the bits after every launch."""

  def __init__(self, dev, kind, d, bf16=False):
    self.dev, self.kind, self.d, self.bf16 = dev, kind, d, bf16
    self.graph, self.w_csr = _graph(kind, str(dev))
    self.lens = AC.graph_edges(kind)[1]
    self.t = {k: v.to(dev) for k, v in AC.operands(kind, d, bf16).items()}
    self.t['w_csr'] = self.w_csr
    self.alpha, self.beta = torch.tensor([AC.ALPHA], device=dev), torch.tensor([AC.BETA], device=dev)
    self.t['alpha'], self.t['beta'] = self.alpha, self.beta
    if bf16:
      self.t['u_lo'] = ops.to_bf16(self.t['u'])
      assert torch.equal(self.t['u_lo'].float(), self.t['u'])        # widen(u_lo) == u: the float64 reference is exact for this route
    self.pristine = {k: v.clone() for k, v in self.t.items()}
    self.worst = {}

  def stage_kw(self, launch, outs):
    stage = launch[0]
    kw = dict(stage=getattr(_lib, 'STAGE_' + stage), dt=AC.DT)
    kw.update({name: self.t[name] for name in AC.READS[stage] if name not in ('p0', 'p1')})
    if stage == 'LINCOMB':
      kw.update(prev=(self.t['p0'], self.t['p1']), coef=AC.COEF)
    kw.update(outs)
    return kw

  def check_inputs_unchanged(self, what):
    for k, v in self.t.items():
      assert torch.equal(_bits(v), _bits(self.pristine[k])), '%s: the launch wrote to its operand %s' % (what, k)

  def compare(self, launch, outs, what, rows=slice(None)):
    ref = AC.reference(self.kind, self.d, launch, bf16=self.bf16)
    assert set(ref) == set(outs)
    for name, got in outs.items():
      got = got.cpu()
      per_class = AC.assert_rows(got, ref[name], self.lens, TOL, '%s %s' % (what, name), rows)
      assert_parity(got[rows], ref[name][rows], what='%s %s (whole tensor)' % (what, name))
      print('ROWERR %s %s %s' % (what, name, per_class))
      AC.worst(self.worst, per_class)

  def run(self, launch, line, fold, *, tickets=None, lo=False, what=''):
    """One launch through ops.spmm / ops.spmm_rhs: the plan for these very operands, NaN-prefilled outputs, every row against float64."""
    stage, with_x0, sigmoid = launch
    t, graph, d = self.t, self.graph, self.d
    what = '%s %s d=%d %s' % (what, self.kind, d, AC.launch_id(launch))
    ws = _workspace(graph, d)
    lo_out = None
    if stage == 'plain':
      outs = {'out': torch.full((N, d), NAN, device=self.dev)}
      plan = ops.spmm_plan(graph, t['u'].data_ptr(), d, d, None, plain_out_addr=outs['out'].data_ptr(), ws_addr=ws.data_ptr(), lo=lo)
    else:
      outs = {name: torch.full((N, d), NAN, device=self.dev) for name in AC.WRITES[stage]}
      kw = self.stage_kw(launch, outs)
      x0 = t['x0'] if with_x0 else None
      epi = ops.make_epilogue(self.alpha, self.beta if with_x0 else None, x0, sigmoid, **kw)
      plan = ops.spmm_plan(graph, t['u'].data_ptr(), d, d, epi, ws_addr=ws.data_ptr(), tickets=tickets is not None, lo=lo)
    assert AC.plan_line(plan) == line and plan.fold_kind == fold and plan.lo == int(lo), (what, AC.plan_line(plan), plan.fold_kind)
    assert plan.full == int(d in (128, 256) and plan.kernel != 'quad_lo'), what
    if stage == 'plain':
      if lo:
        ops.spmm_lo(graph, self.w_csr, t['u_lo'], out=outs['out'])
      else:
        ops.spmm(graph, self.w_csr, t['u'], out=outs['out'])
    else:
      gather_lo = None
      if lo:
        lo_out = torch.full((N, d), NAN, device=self.dev).to(torch.bfloat16) if 'out_y' in outs else None
        gather_lo = (t['u_lo'], lo_out)
      ops.spmm_rhs(graph, self.w_csr, t['u'], self.alpha, self.beta if with_x0 else None, x0, sigmoid, gather_lo=gather_lo, tickets=tickets, **kw)
    torch.cuda.synchronize()
    assert _workspace(graph, d).data_ptr() == ws.data_ptr(), what            # the plan was asked about the workspace the launch got
    self.check_inputs_unchanged(what)
    self.compare(launch, outs, what)
    if lo_out is not None:     # the shadow is the bf16 rounding of the very out_y that was stored
      assert torch.equal(_bits(lo_out), _bits(outs['out_y'].to(torch.bfloat16))), '%s: shadow of out_y' % what
    return outs


# ---- (a) every width, both graphs, the plain aggregation and all eleven stages ----------------------------------------------------------

@pytest.mark.parametrize('kind', AC.KINDS)
@pytest.mark.parametrize('d', AC.WIDTHS)
def test_dispatch_line(dev, kind, d):
  c = Case(dev, kind, d)
  assert c.t['u'].stride(0) == d
  for launch in AC.launches(d):
    c.run(launch, AC.intended(kind, d), AC.fold_kind(kind, d, launch), what='(a)')
  print('ROWERR (a) %s d=%d worst of %d launches %s' % (kind, d, len(AC.launches(d)), c.worst))


# ---- (b) the hub rows folded inside the row-pair launch, against float64 ------------------------------------------------------------------

def _folds():
  return int(_lib.lib().gnpde_in_kernel_fold_launches())


@pytest.mark.parametrize('d', [80, 100, 128])
def test_in_kernel_fold_against_float64(dev, d):
  c = Case(dev, 'short', d)
  nbytes = int(_lib.lib().gnpde_spmm_ticket_bytes(c.graph.ref()))
  assert nbytes == 4 * c.graph.n_long_rows
  tickets = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
  for stage in AC.PREFETCHABLE:
    for with_x0 in (True, False):
      launch = (stage, with_x0, True)
      c0 = _folds()
      c.run(launch, (16, 'pair', 32, 1, 16), 'in_kernel', tickets=tickets, what='(b)')
      assert _folds() == c0 + 1, AC.launch_id(launch)
      assert int(tickets.abs().sum()) == 0, AC.launch_id(launch)           # every last arriver put its ticket back
  # a stage that fold_stage does not state keeps the fold launch, tickets or not
  c0 = _folds()
  c.run(('RK3', True, True), (16, 'pair', 32, 1, 16), 'reduce4', tickets=tickets, what='(b)')
  assert _folds() == c0 and int(tickets.abs().sum()) == 0
  print('ROWERR (b) short d=%d worst %s' % (d, c.worst))


# ---- (c) both row deals forced --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', AC.KINDS)
@pytest.mark.parametrize('knob', [1, 2], ids=['contiguous', 'hashed'])
def test_both_row_deals(dev, kind, knob):
  worst = {}
  ops.tune(10, knob)
  try:
    for d in (24, 128, 256, 50, 31):        # rows on 16-byte lanes, row pairs | wide 32, wide 64, rows on 8- and on 4-byte lanes
      c = Case(dev, kind, d)
      for stage in ('RK4C', 'RK3'):
        launch = (stage, True, True)
        c.run(launch, AC.intended(kind, d), AC.fold_kind(kind, d, launch), what='(c) deal %d' % knob)
      AC.worst(worst, c.worst)
  finally:
    ops.tune(10, 0)
  print('ROWERR (c) %s deal %d worst %s' % (kind, knob, worst))


# ---- (d) the bf16 gather operand with an exactly representable table ------------------------------------------------------------------------

@pytest.mark.parametrize('kind', AC.KINDS)
@pytest.mark.parametrize('d', AC.LANES16)
def test_bf16_gather_operand(dev, kind, d):
  c = Case(dev, kind, d, bf16=True)
  for launch in AC.launches(d, variants=False):
    c.run(launch, AC.intended(kind, d), AC.fold_kind(kind, d, launch, lo=True), lo=True, what='(d)')
  print('ROWERR (d) %s d=%d worst %s' % (kind, d, c.worst))


@pytest.mark.parametrize('d', [80, 128])
def test_bf16_quad_mapping(dev, d):
  c = Case(dev, 'short', d, bf16=True)
  ops.tune(_lib.TUNE_LO_MAPPING, 2)
  try:
    for launch in AC.launches(d, variants=False):
      c.run(launch, AC.intended('short', d, quad=True), 'reduce4_lo', lo=True, what='(d) quad')
  finally:
    ops.tune(_lib.TUNE_LO_MAPPING, 0)
  print('ROWERR (d) quad short d=%d worst %s' % (d, c.worst))


# ---- (e) a row range ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', AC.KINDS)
@pytest.mark.parametrize('d', [128, 50])
def test_row_range_leaves_the_other_rows_alone(dev, kind, d):
  """Rows [b, n) with b odd and inside the pair block: the pairs of the row-pair kernel are then (odd, even) rows.  Rows below b keep
  their prefill bit for bit -- the two hub rows among them too, whose chunk items still run but whose fold must not store."""
  b = AC.ROW_RANGE_BEGIN
  c = Case(dev, kind, d)
  graph = c.graph
  assert int((c.lens[:b] > AC.LONG_ROW).sum()) == 2
  prefill = _bits(torch.full((b, d), NAN, device=dev))
  try:
    graph.set_row_range(b, N)
    for stage in ('RHS', 'RK2C'):
      launch = (stage, True, True)
      what = '(e) %s d=%d %s rows [%d, n)' % (kind, d, stage, b)
      (name,) = AC.WRITES[stage]
      out = torch.full((N, d), NAN, device=dev)
      kw = c.stage_kw(launch, {name: out})
      epi = ops.make_epilogue(c.alpha, c.beta, c.t['x0'], True, **kw)
      plan = ops.spmm_plan(graph, c.t['u'].data_ptr(), d, d, epi, ws_addr=_workspace(graph, d).data_ptr())
      assert AC.plan_line(plan) == AC.intended(kind, d) and plan.fold_kind == AC.fold_kind(kind, d, launch), what
      ops.spmm_rhs(graph, c.w_csr, c.t['u'], c.alpha, c.beta, c.t['x0'], True, **kw)
      torch.cuda.synchronize()
      c.check_inputs_unchanged(what)
      untouched = (_bits(out[:b]) == prefill).all(dim=1).cpu()
      assert bool(untouched.all()), '%s: rows %s below the range were written' % (what, (~untouched).nonzero().flatten().tolist())
      c.compare(launch, {name: out}, what, rows=slice(b, N))
  finally:
    graph.set_row_range(0, N)
  print('ROWERR (e) %s d=%d worst %s' % (kind, d, c.worst))


# ---- (f) lanes demoted by a misaligned state or an odd row stride, through the raw entry point ----------------------------------------------

@pytest.mark.parametrize('how', ['u+4', 'u+8', 'ld129', 'ld130'])
def test_demoted_lanes(dev, how):
  """d = 128 on 4- and 8-byte lanes: rows (64,2,2) / (32,2,4) and the scalar fold, with a prefetchable and a classic stage.  With a
  padded row stride every operand shares it, and columns [d, ld) of every output keep their prefill."""
  d, kind = 128, 'short'
  c = Case(dev, kind, d)
  graph = c.graph
  lanes = 4 if how in ('u+4', 'ld129') else 8
  ld = {'ld129': 129, 'ld130': 130}.get(how, d)
  shift = {'u+4': 1, 'u+8': 2}.get(how, 0)

  def place(x):      # [n, d] -> a view with row stride ld whose padding columns are zero
    buf = torch.zeros(N, ld, device=dev)
    buf[:, :d] = x
    return buf[:, :d]
  t = dict(c.t)
  if shift:
    flat = torch.zeros(N * d + 4, device=dev)
    flat[shift:shift + N * d] = c.t['u'].flatten()
    t['u'] = flat[shift:shift + N * d].view(N, d)
    assert t['u'].data_ptr() % 16 == 4 * shift
  else:
    t = {k: (place(v) if v.dim() == 2 else v) for k, v in t.items()}
  pristine = {k: v.clone() for k, v in t.items()}
  L = _lib.lib()
  ws = _workspace(graph, d)
  for stage in ('RHS', 'RK3'):
    launch = (stage, True, True)
    what = '(f) %s %s' % (how, stage)
    full = {name: torch.full((N, ld), NAN, device=dev) for name in AC.WRITES[stage]}
    kw = dict(stage=getattr(_lib, 'STAGE_' + stage), dt=AC.DT)
    kw.update({name: t[name] for name in AC.READS[stage]})
    kw.update({name: v[:, :d] for name, v in full.items()})
    epi = ops.make_epilogue(c.alpha, c.beta, t['x0'], True, **kw)
    plan = ops.spmm_plan(graph, t['u'].data_ptr(), d, ld, epi, ws_addr=ws.data_ptr())
    assert AC.plan_line(plan) == AC.intended(kind, d, lanes=lanes) and plan.fold_kind == 'scalar', (what, AC.plan_line(plan))
    _lib.check(L.gnpde_spmm_rhs(graph.ref(), _lib.ptr(c.w_csr), _lib.ptr(t['u']), d, ld, ctypes.byref(epi), _lib.ptr(ws), ws.numel(),
                                _lib.stream_of(t['u'])))
    torch.cuda.synchronize()
    for k, v in t.items():
      assert torch.equal(_bits(v), _bits(pristine[k])), '%s: the launch wrote to its operand %s' % (what, k)
    for name, v in full.items():
      assert bool(torch.isnan(v[:, d:]).all()), '%s: columns [d, ld) of %s were written' % (what, name)
    c.compare(launch, {name: v[:, :d].contiguous() for name, v in full.items()}, what)
  print('ROWERR (f) %s worst %s' % (how, c.worst))


# ---- (g) ------------------------------------------------------------------------------------------------------------------------------------

def test_width_past_the_table_is_a_shape_error(dev, graphs):
  ei, w, graph, w_csr = graphs['short']
  x = torch.zeros(N, 257, device=dev)      # 257 4-byte lanes: one more than the widest line
  with pytest.raises(G.GnpdeError, match='too large'):
    ops.spmm(graph, w_csr, x)
  with pytest.raises(G.GnpdeError, match='too large'):
    ops.spmm_rhs(graph, w_csr, x, torch.tensor(0.3).to(dev), torch.tensor(-0.7).to(dev), x, True)
