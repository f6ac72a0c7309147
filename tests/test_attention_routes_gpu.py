"""One GRAND-nl evaluation (gnpde_rhs_eval), three routes of its row attention, each against the float64 oracle and judged per OUTPUT
ROW (largest error in the row over the row's largest |reference|, helpers.TOL for every row -- hub rows and one-entry rows alike):

  route (enqueue_rhs, csrc/solver.hip)                                         case
  ----------------------------------------------------------------------------------------------------------------------------------
  attention inside the aggregation: launch_attn_spmm -> attn_spmm_kernel       staircase without hubs, gnpde_tune(TUNE_ROW_FUSION, .) 0
    <4, 32 | 64, 8, H, DK4, exact width?>, (H, d_k) in (4,4) (8,16) (4,16)     (small graph: chosen) and 1 (forced); d = 68 (17 slots,
    (2,16)                                                                     column predicate), 128 (32, none), 256 (64, none)
  one launch: launch_sd_one -> row_attention_sd_one_kernel<H, DK4>, hub        staircase with hubs, d in {96, 128}, H in {1, 2, 4} at
    weights formed by the aggregation's chunk items (HubDefer)                 A = 16 (d_k 16, 8, 4); the counter advances
  two launches: launch_sd_with_hubs, hub rows normalised by the second         the same with gnpde_tune(TUNE_ATT_ONE_LAUNCH, 1), and
                                                                               H = 8 (never one launch); the counter stands still
    cosine_sim / pearson: scaled_dot over rows the evaluation normalised,      the same staircase, H in {2, 4} at A = 16, d = 128: the
    and NOT the one launch (the condition names the caller's score type)       counter stands still, same bits with the key at 1

The float64 reference (oracle/restate.py, dtype-generic) takes the DEVICE's own fp32 projection output, read back from the evaluation's
workspace and upcast, as its q||k: the projection's rounding is not part of the comparison.  The fp32 oracle's own per-row error on the
same inputs is printed next to each figure."""
import ctypes
import functools

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
import row_cases as RC
from helpers import TOL

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.2, 0.1


@functools.lru_cache(maxsize=None)
def _graph(name, dev):
  ei, lens, side = RC.graph_edges(name)
  assert side == 0
  graph = G.CSRGraph(ei.to(dev), lens.numel())
  assert (graph.n_bin16, graph.n_bin64, graph.n_long_rows, graph.n_long_chunks) == RC.expected_bins(lens)
  assert 2 * graph.n_bin16 >= graph.n              # mostly short rows: the row-pair aggregation kernel at d = 68..128
  return graph


def _count():
  return int(_lib.lib().gnpde_one_launch_evaluations())


def _evaluate(name, d, h, A, dev, tunes=(), att_type=_lib.ATT_SCALED_DOT):
  """(f [n, d], q||k [n, 2A] as the evaluation's projection wrote it, one-launch evaluations counted, inputs on the CPU)."""
  graph = _graph(name, str(dev))
  n = graph.n
  g = torch.Generator().manual_seed(7 * d + 3 * h + A)
  x, x0 = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
  W = torch.randn(2 * A, d, generator=g) / d ** 0.5           # q, k of unit variance: scores as in the dispatch cases
  b = torch.randn(2 * A, generator=g) * 0.1
  xd, x0d, Wd, bd = x.to(dev), x0.to(dev), W.to(dev), b.to(dev)
  alpha, beta = torch.tensor(ALPHA, device=dev), torch.tensor(BETA, device=dev)
  st = ops.attention_struct(att_type, h, A, 0, False)
  desc = ops.RhsDescriptor(_lib.RHS_TRANSFORMER, graph, d, xd.stride(0), alpha, beta, x0d, True, proj_w=Wd, proj_b=bd, att=st)
  desc.keep += [st]
  L = _lib.lib()
  try:
    for key, value in tunes:
      ops.tune(key, value)
    ws = graph.workspace('rhs%d_%d' % (desc.struct.kind, d), L.gnpde_rhs_workspace_bytes(desc.ref()))
    c0 = _count()
    f = ops.rhs_eval(desc, xd).clone()
    torch.cuda.synchronize()
    taken = _count() - c0
    flat = ws[:n * 2 * A * 4].view(torch.float32).clone()
  finally:
    for key, _ in tunes:
      ops.tune(key, 0)
  # the projection lies first in the workspace: two tables [n, A] where the solver writes them so, else interleaved rows [n, 2A]
  if L.gnpde_linear_split_supported(_lib.ptr(xd), n, d, xd.stride(0), _lib.ptr(Wd), 2 * A, Wd.stride(0), A):
    qk = torch.cat([flat[:n * A].view(n, A), flat[n * A:].view(n, A)], dim=1)
  else:
    qk = flat.view(n, 2 * A)
  # it IS the projection (a wrong guess of the layout would hand the oracle another table)
  lin = torch.nn.functional.linear(x.double(), W.double(), b.double())
  if att_type != _lib.ATT_SCALED_DOT:        # (cosine_sim / pearson: the evaluation normalised the projected rows in place)
    return f, qk.cpu(), taken, (x, x0)
  assert float((qk.cpu().double() - lin).abs().max()) <= 1e-5 * float(lin.abs().max()), 'projection read back from the workspace'
  return f, qk.cpu(), taken, (x, x0)


def _reference(name, qk, h, A, x, x0, dtype):
  ei, lens, _ = RC.graph_edges(name)
  eye, zero = torch.eye(A, dtype=dtype), torch.zeros(A, A, dtype=dtype)
  att, _ = RC.R.transformer_attention(qk.to(dtype), ei, torch.cat([eye, zero], dim=1), None, torch.cat([zero, eye], dim=1), None, h)
  return RC.R.rhs_from_attention(x.to(dtype), ei, att, torch.tensor(ALPHA, dtype=dtype), torch.tensor(BETA, dtype=dtype), x0.to(dtype),
                                 no_alpha_sigmoid=False, add_source=True)


def _check(name, runs, h, A, what):
  """runs: [(label, f, qk, (x, x0))] of ONE shape -- the same projection bits in each, so one float64 reference serves them all."""
  ei, lens, _ = RC.graph_edges(name)
  rows = torch.arange(lens.numel())
  qk, (x, x0) = runs[0][2], runs[0][3]
  ref = _reference(name, qk, h, A, x, x0, torch.float64)
  own = RC.class_errors(RC.per_segment_error(_reference(name, qk, h, A, x, x0, torch.float32), ref, rows), lens.clamp_min(1))
  for label, f, qk_i, _ in runs:
    assert torch.equal(qk_i, qk), '%s %s: the routes share one projection' % (what, label)
    # (rows without entries are judged too: f = -alpha x + beta x0; counted with the <= 16 class)
    print('ROWERR %s %s per output row %s (fp32 oracle %s)' % (what, label, RC.class_errors(RC.per_segment_error(f, ref, rows), lens.clamp_min(1)), own))
    RC.assert_rows(f, ref, rows, lens.clamp_min(1), TOL, '%s %s' % (what, label))


@pytest.mark.parametrize('h,dk', [(4, 4), (8, 16), (4, 16), (2, 16)])
@pytest.mark.parametrize('d', [68, 128, 256])
def test_attention_inside_the_aggregation(dev, d, h, dk):
  graph = _graph('nohubs', str(dev))
  # the route's conditions (attn_spmm_supported): a state that fits one XCD's L2 and no hub rows -> chosen with the key at 0 as well
  assert graph.n_long_rows == 0 and graph.n * d * 4 <= (4 << 20) and d % 4 == 0 and 16 < (d + 3) // 4 <= 64
  runs = []
  for fusion in (0, 1):
    f, qk, taken, inputs = _evaluate('nohubs', d, h, h * dk, dev, tunes=[(_lib.TUNE_ROW_FUSION, fusion)] if fusion else [])
    assert taken == 0
    runs.append(('TUNE_ROW_FUSION=%d' % fusion, f, qk, inputs))
  _check('nohubs', runs, h, h * dk, 'attn_spmm d=%d h=%d d_k=%d' % (d, h, dk))


@pytest.mark.parametrize('h', [1, 2, 4, 8])
@pytest.mark.parametrize('d', [96, 128])
def test_one_launch_and_two_launches(dev, d, h):
  A = 16 if h < 8 else 64
  graph = _graph('hubs', str(dev))
  assert graph.n_long_rows == len(RC.HUBS) and d % 4 == 0 and 16 < d // 4 <= 32
  runs = []
  f, qk, taken, inputs = _evaluate('hubs', d, h, A, dev)
  assert taken == (1 if h < 8 else 0), 'h=%d: %d evaluations in the one-launch form' % (h, taken)
  runs.append(('one launch' if h < 8 else 'two launches (8 heads)', f, qk, inputs))
  if h < 8:
    f, qk, taken, inputs = _evaluate('hubs', d, h, A, dev, tunes=[(_lib.TUNE_ATT_ONE_LAUNCH, 1)])
    assert taken == 0
    runs.append(('two launches', f, qk, inputs))
  _check('hubs', runs, h, A, 'rhs_eval d=%d h=%d d_k=%d' % (d, h, A // h))


@pytest.mark.parametrize('h', [2, 4])
@pytest.mark.parametrize('att_type', ['cosine_sim', 'pearson'])
def test_cosine_and_pearson_keep_their_two_launches(dev, att_type, h):
  """enqueue_rhs hands these to the attention as scaled_dot over normalised head vectors, a shape the one-launch form would accept; its
  condition names the score type the caller asked for, so the counter stands still and gnpde_tune(TUNE_ATT_ONE_LAUNCH, 1) changes
  nothing.  (Their numbers: tests/test_golden_gpu.py and the dispatch cases of part 6.)"""
  d, A = 128, 16
  graph = _graph('hubs', str(dev))
  assert graph.n_long_rows == len(RC.HUBS)
  f, qk, taken, _ = _evaluate('hubs', d, h, A, dev, att_type=_lib.ATT_TYPES[att_type])
  assert taken == 0, '%s h=%d: %d evaluations in the one-launch form' % (att_type, h, taken)
  f1, qk1, taken1, _ = _evaluate('hubs', d, h, A, dev, tunes=[(_lib.TUNE_ATT_ONE_LAUNCH, 1)], att_type=_lib.ATT_TYPES[att_type])
  assert taken1 == 0 and bool(torch.isfinite(f).all()) and torch.equal(f, f1) and torch.equal(qk, qk1)
