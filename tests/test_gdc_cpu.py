"""Graph diffusion rewiring, everything that needs no device: the series truncation (`gdc_terms`), known answers of the in-test
oracle (gdc_oracle.py), the option mapping of `apply_gdc`, argument errors, the symbols and the ABI number in header / library /
bindings / INTEGRATION.md, the drop-in's `graph_rewiring`, and the cap on the entries the derived bound leaves undetermined."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, dropin, ops
import gdc_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_gdc_workspace_bytes', 'gnpde_gdc_block', 'gnpde_gdc_topk', 'gnpde_gdc_emit', 'gnpde_gdc_threshold_count',
           'gnpde_gdc_threshold_fill', 'gnpde_gdc_segment_sums', 'gnpde_gdc_dense')


@pytest.mark.parametrize('method,param,tol', [('ppr', 0.05, 1e-6), ('ppr', 0.15, 1e-6), ('ppr', 0.3, 1e-4), ('heat', 3.0, 1e-6),
                                              ('heat', 5.0, 1e-8), ('heat', 0.5, 1e-6)])
def test_terms_tail_is_under_tol_and_minimal(method, param, tol):
  theta = ops.gdc_terms(method, param, tol)
  exact = (lambda m: param * (1.0 - param) ** m) if method == 'ppr' else (lambda m: math.exp(-param) * param ** m / math.factorial(m))
  assert len(theta) - 1 <= ops.GDC_MAX_TERMS
  np.testing.assert_allclose(theta, [exact(m) for m in range(len(theta))], rtol=1e-12)
  assert 1.0 - math.fsum(exact(m) for m in range(len(theta))) <= tol
  assert 1.0 - math.fsum(exact(m) for m in range(len(theta) - 1)) > tol, 'M - 1 terms would have been enough'
  assert theta == pytest.approx(O.terms(method, param, tol), rel=1e-12)


@pytest.mark.parametrize('alpha', [0.05, 0.15, 0.3])
def test_terms_ppr_closed_form(alpha):
  M = len(ops.gdc_terms('ppr', alpha, 1e-6)) - 1
  assert M == math.ceil(math.log(1e-6) / math.log(1.0 - alpha)) - 1


def test_terms_coeff_is_the_list_and_bad_arguments_raise():
  assert ops.gdc_terms('coeff', [0, 1]) == [0.0, 1.0]
  assert ops.gdc_terms('ppr', 1.0) == [1.0]
  assert ops.gdc_terms('heat', 0.0) == [1.0]
  for method, param, tol in (('ppr', 0.0, 1e-6), ('ppr', 1.5, 1e-6), ('heat', -1.0, 1e-6), ('walk', 0.1, 1e-6), ('ppr', 0.1, 0.0),
                             ('coeff', [], 1e-6), ('coeff', [0.5, -0.1], 1e-6), ('ppr', 1e-4, 1e-9), ('coeff', [0.0] * 4098, 1e-6)):
    with pytest.raises(ValueError):
      ops.gdc_terms(method, param, tol)


def test_oracle_two_nodes_closed_form():
  """0 - 1 with unit loops: T = P = [[1, 1], [1, 1]] / 2 is a projector, so ppr S = alpha I + (1 - alpha) P and heat
  S = P + e^-t (I - P); both columns already sum to 1."""
  ei = np.array([[0, 1], [1, 0]])
  for method, param, diag in (('ppr', 0.15, (1 + 0.15) / 2), ('heat', 3.0, 0.5 + 0.5 * math.exp(-3.0))):
    out_ei, w = O.gdc_oracle(ei, None, 2, method, param, k=2)
    assert out_ei.tolist() == [[0, 1, 1, 0], [0, 0, 1, 1]]
    np.testing.assert_allclose(w, [diag, 1 - diag, diag, 1 - diag], rtol=1e-13)
    _, w1 = O.gdc_oracle(ei, None, 2, method, param, k=1)          # top-1 keeps the diagonal, which normalises to 1
    assert w1.tolist() == [1.0, 1.0]


@pytest.mark.parametrize('name', ['plain_k16', 'directed', 'weighted_dups', 'threshold', 'isolated'])
def test_oracle_columns_sum_to_one(name):
  ei, w, n, c = O.case_inputs(name)
  kw = {a: c[a] for a in ('k', 'eps', 'self_loop_weight', 'normalization_in') if a in c}
  out_ei, out_w = O.gdc_oracle(ei, w, n, c['method'], c['param'], **kw)
  sums = np.bincount(out_ei[1], weights=out_w, minlength=n)
  kept = np.bincount(out_ei[1], minlength=n) > 0
  np.testing.assert_allclose(sums[kept], 1.0, rtol=1e-12)
  assert (sums[~kept] == 0).all() and np.isfinite(out_w).all() and (out_w > 0).all()
  if name == 'threshold':
    assert 0 < int((~kept).sum()) < n, 'the threshold case is meant to leave SOME columns empty'


def test_oracle_isolated_node_keeps_its_diagonal():
  """A node without edges and without loop: T e_j = 0, so column j of S is theta_0 e_j, which normalises to 1."""
  ei = np.array([[0, 1], [1, 0]])
  A, _ = O.adjacency(ei, None, 3, 0.0)
  S = O.diffusion(O.normalise(A, 'sym'), 'ppr', 0.15)
  assert S[2, 2] == pytest.approx(0.15, rel=1e-15) and (S[:2, 2] == 0).all() and (S[2, :2] == 0).all()
  out_ei, w = O.gdc_oracle(ei, None, 3, 'ppr', 0.15, k=4, self_loop_weight=0.0)
  assert out_ei[:, out_ei[1] == 2].tolist() == [[2], [2]] and w[out_ei[1] == 2].tolist() == [1.0]


@pytest.mark.parametrize('method,param', [('ppr', 0.15), ('heat', 3.0)])
def test_oracle_closed_forms_agree_with_their_series(method, param):
  ei, w, n, _ = O.case_inputs('weighted_dups')
  A, _ = O.adjacency(ei, w, n, 1.0)
  T = O.normalise(A, 'sym')
  assert np.abs(O.diffusion(T, method, param) - O.series(T, O.terms(method, param, 1e-15))).max() <= 1e-12


def test_oracle_orders_by_value_then_row():
  assert O.column_order(np.array([0.25, 0.5, 0.25, 0.0, 0.5])).tolist() == [1, 4, 0, 2, 3]


@pytest.mark.parametrize('name', sorted(O.CASES))
def test_band_leaves_few_entries_undetermined(name):
  """The membership rule of the GPU tests decides all but <= 2 % of the entries (counted on the oracle alone)."""
  band = O.case_band(name)
  print('%s: gamma %.3e, %d undetermined entries (%.4f %%)' % (name, band.gamma, band.undetermined(), 100.0 * band.share()))
  assert band.share() <= O.CAP_SHARE
  # the oracle's own answer passes the rule
  ei, w, n, c = O.case_inputs(name)
  kw = {a: c[a] for a in ('k', 'eps', 'self_loop_weight', 'normalization_in') if a in c}
  out_ei, out_w = O.gdc_oracle(ei, w, n, c['method'], c['param'], normalization_out=None, **kw)
  band.check(out_ei, out_w)


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
  assert in_header >= 11 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION


def _tiny_graph():
  return G.CSRGraph(torch.tensor([[0, 1, 2], [1, 2, 0]]), 3)


def test_entry_points_reject_bad_arguments_before_any_launch():
  """Outside block % 4 == 0 in 4 .. 256, 1 <= k <= 128, 1 <= terms <= 4097, eps > 0 and the dense cap the C entry points return an
  error code and a message; nothing touches a device (this test runs without one)."""
  L = G.lib()
  g = _tiny_graph()
  buf = torch.zeros(1 << 16, dtype=torch.uint8)
  f = torch.zeros(4096)
  i64 = torch.zeros(4096, dtype=torch.int64)
  p = _lib.ptr
  assert L.gnpde_gdc_workspace_bytes(g.ref(), 6, 4) == 0 and L.gnpde_gdc_workspace_bytes(g.ref(), 260, 4) == 0
  assert L.gnpde_gdc_workspace_bytes(g.ref(), 8, 129) == 0 and L.gnpde_gdc_workspace_bytes(None, 8, 4) == 0
  need = L.gnpde_gdc_workspace_bytes(g.ref(), 8, 4)
  assert 2 * 3 * 8 * 4 <= need <= buf.numel()
  block = lambda terms, j0, B, ws=buf.numel(): L.gnpde_gdc_block(g.ref(), p(f), p(f), terms, j0, B, p(f), p(buf), ws, None)
  assert block(0, 0, 8) == -2 and b'gdc_block' in L.gnpde_last_error()
  assert block(4098, 0, 8) == -2
  assert block(3, 0, 6) == -2 and block(3, 0, 512) == -2
  assert block(3, 3, 8) == -1 and block(3, -1, 8) == -1
  assert block(3, 0, 8, ws=16) == -3
  assert L.gnpde_gdc_block(g.ref(), p(f), None, 3, 0, 8, p(f), p(buf), buf.numel(), None) == -1
  topk = lambda k: L.gnpde_gdc_topk(g.ref(), p(f), 0, 8, k, p(i64), p(i64), p(buf), buf.numel(), None)
  assert topk(0) == -2 and topk(129) == -2 and b'gdc_topk' in L.gnpde_last_error()
  assert L.gnpde_gdc_emit(p(i64), p(i64), 3, 0, 1, p(i64), 0, p(f), None) == -2
  assert L.gnpde_gdc_emit(None, p(i64), 3, 4, 1, p(i64), 0, p(f), None) == -1
  assert L.gnpde_gdc_threshold_count(g.ref(), p(f), 0, 8, 0.0, p(i64), p(buf), buf.numel(), None) == -1
  assert L.gnpde_gdc_threshold_fill(g.ref(), 0, 8, -1.0, p(i64), p(i64), 0, p(f), p(buf), buf.numel(), None) == -1
  assert L.gnpde_gdc_segment_sums(None, p(i64), 1, p(f), 0, None) == -1
  assert L.gnpde_gdc_dense(g.ref(), p(f), 0, 8, 1, p(f), 35, p(buf), buf.numel(), None) == -2 and b'cap' in L.gnpde_last_error()


def test_python_surface_argument_errors():
  ei = torch.tensor([[0, 1], [1, 0]])
  bad = [dict(method='ppr'), dict(method='walk', alpha=0.1, k=2), dict(method='ppr', alpha=0.1), dict(method='ppr', alpha=0.1, k=2, eps=0.1),
         dict(method='ppr', alpha=0.1, k=0), dict(method='ppr', alpha=0.1, k=129), dict(method='ppr', alpha=0.1, eps=0.0),
         dict(method='ppr', alpha=0.1, k=2, block=6), dict(method='ppr', alpha=0.1, k=2, block=512), dict(method='ppr', alpha=2.0, k=2),
         dict(method='heat', t=1.0, k=2, normalization_in='max'), dict(method='ppr', alpha=0.1, k=2, normalization_out='max'),
         dict(method='coeff', coeffs=[], k=2)]
  for kw in bad:
    with pytest.raises(ValueError):
      ops.gdc(ei, None, 2, **kw)
  with pytest.raises(ValueError):
    ops.gdc(ei, None, 0, method='ppr', alpha=0.1, k=2)
  with pytest.raises(ValueError):
    ops.gdc(torch.zeros(3, 2, dtype=torch.long), None, 2, method='ppr', alpha=0.1, k=2)
  with pytest.raises(G.GnpdeError, match='cap'):
    ops.gdc(ei, None, 2, method='ppr', alpha=0.1, dense_out=True, dense_cap_bytes=15)
  with pytest.raises(G.GnpdeError, match='HIP'):       # no CPU fallback
    ops.gdc(ei, None, 2, method='ppr', alpha=0.1, k=2)


class _Data(object):
  def __init__(self, n, ei, w=None):
    self.num_nodes, self.edge_index, self.edge_attr = n, ei, w


OPT = dict(gdc_method='ppr', ppr_alpha=0.07, heat_time=2.5, gdc_sparsification='topk', gdc_k=24, gdc_threshold=0.003, self_loop_weight=1,
           exact=True, pos_enc_orientation='row')


def test_apply_gdc_maps_the_options(monkeypatch):
  seen = []

  def fake(edge_index, edge_weight, n, **kw):
    seen.append((n, kw))
    if kw.get('dense_out'):
      return torch.arange(9.0).reshape(3, 3)
    return torch.tensor([[2, 0, 1], [0, 1, 0]]), torch.tensor([0.25, 1.0, 0.75])
  monkeypatch.setattr(ops, 'gdc', fake)
  ei = torch.tensor([[0, 1], [1, 2]])
  data = G.graph_rewiring.apply_gdc(_Data([3], ei), dict(OPT))
  n, kw = seen.pop()
  assert n == 3 and data.num_nodes == 3
  assert kw == dict(method='ppr', alpha=0.07, k=24, self_loop_weight=1.0, normalization_in='sym', normalization_out='col', tol=1e-6, block=256)
  # (row, col) order, as coalesce returns it
  assert data.edge_index.tolist() == [[0, 1, 2], [1, 0, 0]] and data.edge_attr.tolist() == [1.0, 0.75, 0.25]
  G.graph_rewiring.apply_gdc(_Data(3, ei), dict(OPT, gdc_method='heat', gdc_sparsification='threshold', self_loop_weight=0, exact=False,
                                                gnpde_gdc_tol=1e-4))
  n, kw = seen.pop()
  assert kw == dict(method='heat', t=2.5, eps=0.003, self_loop_weight=0.0, normalization_in='sym', normalization_out='col', tol=1e-4, block=256)
  enc = G.graph_rewiring.apply_gdc(_Data(3, ei), dict(OPT), type='pos_encoding')
  assert seen.pop()[1]['dense_out'] is True and enc.tolist() == torch.arange(9.0).reshape(3, 3).tolist()
  enc = G.graph_rewiring.apply_gdc(_Data(3, ei), dict(OPT, pos_enc_orientation='col'), type='pos_encoding')
  assert enc.tolist() == torch.arange(9.0).reshape(3, 3).T.tolist()


def test_wrapper_refuses_what_is_not_built_and_needs_no_torch_geometric():
  W = G.graph_rewiring.GDCWrapper
  with pytest.raises(NotImplementedError, match='avg_degree'):
    W()(_Data(2, torch.tensor([[0], [1]])))
  with pytest.raises(NotImplementedError, match='dim'):
    W(sparsification_kwargs=dict(method='topk', k=4, dim=1))(_Data(2, torch.tensor([[0], [1]])))
  src = open(os.path.join(ROOT, 'graph-neural-pde_amd', 'graph_rewiring.py')).read()
  assert not re.search(r'^\s*(import|from)\s+torch_geometric', src, re.M)
  assert hasattr(W, 'position_encoding') and callable(W)


STUB = '''
MARK = 'from the stub'
def KNN(x, opt):
  return 'stub KNN'
def apply_gdc(data, opt, type="combined"):
  return 'stub gdc'
class GDCWrapper(object):
  pass
def unrelated():
  return MARK
'''


@pytest.fixture
def clean_dropin():
  dropin.uninstall()
  saved = list(sys.path)
  yield
  dropin.uninstall()
  sys.path[:] = saved
  sys.modules.pop('graph_rewiring', None)


def test_dropin_serves_the_native_gdc_names(tmp_path, clean_dropin):
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  served = dropin.install(native_gdc=True)
  assert 'graph_rewiring' in served
  from graph_rewiring import apply_gdc, GDCWrapper, KNN, unrelated       # what the reference's data.py does
  ours = sys.modules['gnpde_amd.graph_rewiring']
  assert apply_gdc is ours.apply_gdc and GDCWrapper is ours.GDCWrapper
  assert KNN(None, None) == 'stub KNN' and unrelated() == 'from the stub'
  dropin.uninstall()
  assert 'graph_rewiring' not in sys.modules and not dropin.installed()
  # both flags: all three names
  dropin.install(native_knn=True, native_gdc=True)
  import graph_rewiring
  assert graph_rewiring.KNN is ours.KNN and graph_rewiring.apply_gdc is ours.apply_gdc and graph_rewiring.GDCWrapper is ours.GDCWrapper
  assert graph_rewiring.unrelated() == 'from the stub'


def test_dropin_gdc_without_a_reference_file_is_ours(clean_dropin):
  dropin.install(native_gdc=True)
  import graph_rewiring
  ours = sys.modules['gnpde_amd.graph_rewiring']
  assert graph_rewiring.apply_gdc is ours.apply_gdc and graph_rewiring.__gnpde_reference__ is None


def test_dropin_knn_flag_alone_leaves_gdc_to_the_reference(tmp_path, clean_dropin):
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  dropin.install(native_knn=True)
  import graph_rewiring
  assert graph_rewiring.apply_gdc(None, None) == 'stub gdc'


def test_dropin_usage_names_the_flag():
  with pytest.raises(SystemExit, match='--native-gdc'):
    dropin.main([])
  with pytest.raises(SystemExit, match='--native-gdc'):
    dropin.main(['--no-such-flag'])
