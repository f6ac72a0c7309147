"""Approximate forward push of graph diffusion rewiring, everything that needs no device: the float64 yardstick (gdc_push_oracle.py)
against the three relations on every shape of the GPU tests, the share of entries the pipeline bound leaves open, the symbols and
the ABI number in header / library / bindings / INTEGRATION.md, argument errors of the C entry points and of the Python surface, the
option plumbing of `GDCWrapper` / `apply_gdc` and the drop-in flag."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, dropin, ops
import gdc_push_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_gdc_push_workspace_bytes', 'gnpde_gdc_push_count', 'gnpde_gdc_push_fill', 'gnpde_gdc_push_residuals',
           'gnpde_rank_select_begin', 'gnpde_rank_select_hist', 'gnpde_rank_select_pick', 'gnpde_rank_select_values')
PIPELINE_SHAPE, PIPELINE_THRESHOLD = O.PIPELINE_SHAPE, O.PIPELINE_THRESHOLD


@pytest.mark.parametrize('name', sorted(O.SHAPES))
def test_oracle_pushes_satisfy_the_three_relations(name):
  """0 <= Pi - p < eps deg, mass 1, r < alpha eps deg for the synchronous push (every source) and the LIFO push (a few sources),
  in float64 with no slack but the inverse's rounding: this pins the yardstick of the GPU tests."""
  c = O.SHAPES[name]
  _, A, deg, Pi = O.shape(name)
  assert (A == A.T).all() and (np.diag(A) == 1).all()
  P, R = O.push_all(name)
  ratio = O.check_relations(P, R, Pi, deg, c['alpha'], c['eps'], label=name + ' synchronous')
  assert ratio > 0.5, 'the bound is not close to tight on this shape'
  rows = O.rows_of(A)
  src = [0] if name == 'fine600' else [0, 1, c['n'] // 2, c['n'] - 1]
  out = [O.push_lifo(rows, deg, s, c['alpha'], c['eps']) for s in src]
  O.check_relations(np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), Pi[src], deg, c['alpha'], c['eps'], label=name + ' LIFO')


def test_local_shape_is_local_and_hub_shape_has_a_hub():
  P, _ = O.push_all('local300')
  assert 30 < (P > 0).sum(1).mean() < 100
  assert O.shape('hub600')[2].max() == 531


def test_pipeline_bound_leaves_few_entries_open():
  b = O.pipeline_band(PIPELINE_SHAPE, PIPELINE_THRESHOLD)
  print('%s at %g: %d kept, %d open (%.4f)' % (PIPELINE_SHAPE, PIPELINE_THRESHOLD, int(b['kept'].sum()), int(b['open'].sum()), b['share']))
  assert b['share'] <= O.OPEN_CAP and int(b['kept'].sum()) > 1000
  assert not (b['inside'] & ~b['kept']).any() and not (b['outside'] & b['kept']).any()
  sums = b['out'].sum(0)
  np.testing.assert_allclose(sums[b['kept'].any(0)], 1.0, rtol=1e-12)


def test_symbols_and_abi_number_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  declared = set(re.findall(r'\b(gnpde_[a-z_0-9]+)\s*\(', header))
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  L = G.lib()
  for name in SYMBOLS:
    assert name in declared, name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name), name + ' is not exported by the library'
    assert name in doc, name + ' is not in INTEGRATION.md'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 14 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION


def test_entry_points_reject_bad_arguments_before_any_launch():
  """Outside 0 < alpha < 1, eps > 0 finite, alpha eps >= 2^-60, sources inside [0, n), capacity >= -1, 1 <= slow_groups <= 1024, the
  residual read-out's n <= 4096 and the workspace size the entry points return an error code and a message; nothing touches a
  device (this test runs without one)."""
  L = G.lib()
  g = G.CSRGraph(torch.tensor([[0, 1, 2, 0, 1, 2], [1, 2, 0, 0, 1, 2]]), 3)
  p = _lib.ptr
  need = L.gnpde_gdc_push_workspace_bytes(3, 3, 2)
  assert need > 0 and L.gnpde_gdc_push_workspace_bytes(3, 3, 3) > need
  for bad in ((0, 1, 1), (3, 0, 1), (3, 4, 1), (3, 3, 0), (3, 3, 1025), (2 ** 31, 1, 1)):
    assert L.gnpde_gdc_push_workspace_bytes(*bad) == 0
  buf = torch.zeros(need, dtype=torch.uint8)
  i64 = torch.zeros(16, dtype=torch.int64)
  f = torch.zeros(16)

  def count(s0=0, ns=3, alpha=0.15, eps=1e-3, cap=-1, groups=2, counts=i64, info=i64, graph=g.ref(), ws=need):
    return L.gnpde_gdc_push_count(graph, s0, ns, alpha, eps, cap, groups, p(counts), p(info), p(buf), ws, None)
  assert count(alpha=0.0) == -1 and b'gdc_push_count' in L.gnpde_last_error() and b'alpha' in L.gnpde_last_error()
  assert count(alpha=1.0) == -1 and count(eps=0.0) == -1 and count(eps=float('inf')) == -1 and count(eps=float('nan')) == -1
  assert count(eps=1e-19) == -1 and b'quantum' in L.gnpde_last_error()
  assert count(s0=-1) == -1 and count(s0=1, ns=3) == -1 and count(ns=0) == -1
  assert count(cap=-2) == -1 and count(groups=0) == -2 and count(groups=1025) == -2
  assert count(counts=None) == -1 and count(info=None) == -1 and count(graph=None) == -1
  assert count(ws=need - 1) == -3 and b'workspace' in L.gnpde_last_error()
  fill = lambda offsets=i64, out=i64, w=f, ld=8: L.gnpde_gdc_push_fill(g.ref(), 0, 3, 0.15, 1e-3, -1, 2, p(offsets), p(out), ld, p(w), p(i64),
                                                                      p(buf), need, None)
  assert fill(offsets=None) == -1 and fill(out=None) == -1 and fill(w=None) == -1 and fill(ld=-1) == -1
  assert L.gnpde_gdc_push_residuals(g.ref(), 0, 3, 0.15, 1e-3, -1, 2, None, p(i64), p(buf), need, None) == -1
  big = G.CSRGraph(torch.tensor([[0], [1]]), 4097)
  ws_big = torch.zeros(L.gnpde_gdc_push_workspace_bytes(4097, 1, 1), dtype=torch.uint8)
  assert L.gnpde_gdc_push_residuals(big.ref(), 0, 1, 0.15, 1e-3, -1, 1, p(f), p(i64), p(ws_big), ws_big.numel(), None) == -2
  assert b'4096' in L.gnpde_last_error()
  ws = torch.zeros(int(L.gnpde_quantile_workspace_bytes()), dtype=torch.uint8)
  assert L.gnpde_rank_select_begin(-1, 0, p(ws), ws.numel(), None) == -1 and L.gnpde_rank_select_begin(0, 1, p(ws), 8, None) == -3
  assert L.gnpde_rank_select_hist(None, 4, 0, p(ws), ws.numel(), None) == -1 and L.gnpde_rank_select_hist(p(f), 4, 4, p(ws), ws.numel(), None) == -1
  assert L.gnpde_rank_select_pick(4, p(ws), ws.numel(), None) == -1 and L.gnpde_rank_select_values(None, p(ws), ws.numel(), None) == -1


def test_python_surface_argument_errors():
  ei = torch.tensor([[0, 1], [1, 0]])
  for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(eps=0.0), dict(eps=float('inf')), dict(normalization_in='max'), dict(batch=0)):
    with pytest.raises(ValueError):
      ops.gdc_push(ei, 2, **dict(dict(alpha=0.15, eps=1e-3), **kw))
  with pytest.raises(ValueError):
    ops.gdc_push(ei, 0, 0.15, 1e-3)
  with pytest.raises(ValueError):
    ops.gdc_push(torch.zeros(3, 2, dtype=torch.long), 2, 0.15, 1e-3)
  with pytest.raises(NotImplementedError, match='weighted'):
    ops.gdc_push(ei, 2, 0.15, 1e-3, edge_weight=torch.ones(2))
  with pytest.raises(NotImplementedError, match='self_loop_weight'):
    ops.gdc_push(ei, 2, 0.15, 1e-3, self_loop_weight=0.5)
  with pytest.raises(G.GnpdeError, match='4096'):
    ops.gdc_push(ei, 5000, 0.15, 1e-3, return_residuals=True)
  with pytest.raises(G.GnpdeError, match='HIP'):       # no CPU fallback
    ops.gdc_push(ei, 2, 0.15, 1e-3)
  with pytest.raises(ValueError):
    ops.gdc_sparse_threshold(ei, torch.ones(2), 2)
  with pytest.raises(ValueError):
    ops.gdc_sparse_threshold(ei, torch.ones(2), 2, eps=0.1, avg_degree=2)
  with pytest.raises(ValueError):
    ops.gdc_sparse_threshold(ei, torch.ones(2), 2, eps=0.0)
  # the exact path's avg_degree: one selection only, 1 <= avg_degree < n
  for kw in (dict(k=2, avg_degree=1), dict(eps=0.1, avg_degree=1), dict(avg_degree=0), dict(avg_degree=2)):
    with pytest.raises(ValueError):
      ops.gdc(ei, None, 2, method='ppr', alpha=0.1, **kw)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.gdc(ei, None, 2, method='ppr', alpha=0.1, avg_degree=1)


class _Data(object):
  def __init__(self, n, ei, w=None):
    self.num_nodes, self.edge_index, self.edge_attr = n, ei, w


EI = torch.tensor([[0, 1], [1, 2]])


def test_wrapper_refusals_on_the_push_path():
  W = G.graph_rewiring.GDCWrapper
  push = dict(approx='push', exact=False)
  with pytest.raises(ValueError, match='approx'):
    W(approx='pull')
  with pytest.raises(NotImplementedError, match='no top-k'):
    W(diffusion_kwargs=dict(method='ppr', alpha=0.15, eps=1e-4), sparsification_kwargs=dict(method='topk', k=4, dim=0), **push)(_Data(3, EI))
  thr = dict(method='threshold', eps=0.01)
  for diff in (dict(method='heat', t=3.0, eps=1e-4), dict(method='coeff', coeffs=[0.5, 0.5], eps=1e-4)):
    with pytest.raises(NotImplementedError, match='ppr only'):
      W(diffusion_kwargs=diff, sparsification_kwargs=thr, **push)(_Data(3, EI))
    with pytest.raises(NotImplementedError, match='ppr only'):
      W(diffusion_kwargs=diff, sparsification_kwargs=thr, **push).position_encoding(_Data(3, EI))
  ppr = dict(method='ppr', alpha=0.15, eps=1e-4)
  with pytest.raises(NotImplementedError, match='weighted'):
    W(diffusion_kwargs=ppr, sparsification_kwargs=thr, **push)(_Data(3, EI, torch.ones(2)))
  with pytest.raises(NotImplementedError, match='self_loop_weight'):
    W(0.5, diffusion_kwargs=ppr, sparsification_kwargs=thr, **push)(_Data(3, EI))
  with pytest.raises(ValueError, match='eps'):
    W(diffusion_kwargs=dict(method='ppr', alpha=0.15), sparsification_kwargs=thr, **push)(_Data(3, EI))
  with pytest.raises(G.GnpdeError, match='HIP'):                     # a valid call reaches the device check: no CPU fallback
    W(diffusion_kwargs=ppr, sparsification_kwargs=thr, **push)(_Data(3, EI))


def test_wrapper_takes_the_push_only_with_the_option_and_exact_false(monkeypatch):
  calls = []

  def fake_push(edge_index, n, alpha, eps, **kw):
    calls.append(('push', n, alpha, eps, kw))
    return torch.tensor([[0, 1, 2], [0, 0, 1]]), torch.tensor([0.5, 0.25, 1.0])

  def fake_sparse(ei, w, n, **kw):
    calls.append(('sparse', n, kw))
    return ei[:, :2], w[:2]

  def fake_gdc(edge_index, edge_weight, n, **kw):
    calls.append(('exact', n, kw))
    return torch.tensor([[2, 0], [0, 1]]), torch.tensor([0.25, 1.0])
  monkeypatch.setattr(ops, 'gdc_push', fake_push)
  monkeypatch.setattr(ops, 'gdc_sparse_threshold', fake_sparse)
  monkeypatch.setattr(ops, 'gdc', fake_gdc)
  W = G.graph_rewiring.GDCWrapper
  kw = dict(diffusion_kwargs=dict(method='ppr', alpha=0.1, eps=1e-4), sparsification_kwargs=dict(method='threshold', eps=0.01))
  data = W(**kw, approx='push', exact=False)(_Data(3, EI))
  assert [c[0] for c in calls] == ['push', 'sparse']
  assert calls[0][1:4] == (3, 0.1, 1e-4) and calls[0][4] == dict(self_loop_weight=1, normalization_in='sym', edge_weight=None)
  assert calls[1][2] == dict(normalization_out='col', eps=0.01)
  assert data.edge_index.tolist() == [[0, 1], [0, 0]] and data.edge_attr.tolist() == [0.5, 0.25]
  del calls[:]
  W(diffusion_kwargs=kw['diffusion_kwargs'], sparsification_kwargs=dict(method='threshold', avg_degree=2), approx='push', exact=False)(_Data(3, EI))
  assert calls[1][2] == dict(normalization_out='col', avg_degree=2)
  for other in (dict(approx='push', exact=True), dict(approx=None, exact=False), dict()):
    del calls[:]
    W(**kw, **other)(_Data(3, EI))
    assert [c[0] for c in calls] == ['exact'], other
  # avg_degree on the exact path: handed on when it is below n, refused at and above n (the whole dense matrix)
  del calls[:]
  W(sparsification_kwargs=dict(method='threshold', avg_degree=2))(_Data(3, EI))
  assert calls[0][2]['avg_degree'] == 2 and 'eps' not in calls[0][2]
  with pytest.raises(NotImplementedError, match='avg_degree'):
    W(sparsification_kwargs=dict(method='threshold', avg_degree=3))(_Data(3, EI))


OPT = dict(gdc_method='ppr', ppr_alpha=0.07, heat_time=2.5, gdc_sparsification='threshold', gdc_k=24, gdc_threshold=0.003, self_loop_weight=1,
           exact=False, pos_enc_orientation='row')


def test_apply_gdc_reads_the_option(monkeypatch):
  made = []
  real = G.graph_rewiring.GDCWrapper

  class Spy(real):
    def __init__(self, *a, **kw):
      made.append(kw)
      real.__init__(self, *a, **kw)

    def __call__(self, data):
      return data
  monkeypatch.setattr(G.graph_rewiring, 'GDCWrapper', Spy)
  G.graph_rewiring.apply_gdc(_Data(3, EI), dict(OPT))
  assert made.pop()['approx'] is None
  G.graph_rewiring.apply_gdc(_Data(3, EI), dict(OPT, gnpde_gdc_approx='push'))
  kw = made.pop()
  assert kw['approx'] == 'push' and kw['exact'] is False and kw['diffusion_kwargs'] == dict(method='ppr', alpha=0.07, eps=0.003)
  assert kw['sparsification_kwargs'] == dict(method='threshold', eps=0.003)
  monkeypatch.setattr(G.graph_rewiring, 'GDC_APPROX_DEFAULT', 'push')          # what the drop-in's --native-gdc-push sets
  G.graph_rewiring.apply_gdc(_Data(3, EI), dict(OPT))
  assert made.pop()['approx'] == 'push'
  G.graph_rewiring.apply_gdc(_Data(3, EI), dict(OPT, gnpde_gdc_approx=None))
  assert made.pop()['approx'] is None


@pytest.fixture
def clean_dropin():
  dropin.uninstall()
  saved = list(sys.path)
  yield
  dropin.uninstall()
  sys.path[:] = saved
  sys.modules.pop('graph_rewiring', None)


def test_dropin_flag_sets_the_option_and_uninstall_clears_it(clean_dropin):
  import gnpde_amd.graph_rewiring as ours
  assert ours.GDC_APPROX_DEFAULT is None
  dropin.install(native_gdc=True)
  assert ours.GDC_APPROX_DEFAULT is None
  dropin.uninstall()
  served = dropin.install(native_gdc_push=True)
  assert 'graph_rewiring' in served and ours.GDC_APPROX_DEFAULT == 'push'
  import graph_rewiring
  assert graph_rewiring.apply_gdc is ours.apply_gdc and graph_rewiring.GDCWrapper is ours.GDCWrapper
  dropin.uninstall()
  assert ours.GDC_APPROX_DEFAULT is None
  with pytest.raises(SystemExit, match='--native-gdc-push'):
    dropin.main([])
