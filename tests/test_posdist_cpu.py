"""Positional-distance rewiring, everything that needs no device: the float64 oracle (posdist_oracle.py) against the libraries the
reference itself calls, the rank rule against np.quantile, the symbols and the ABI number in header / library / bindings /
INTEGRATION.md, argument checks of the C entry points and of the Python surface, the drop-in flag and the branch table of
`apply_pos_dist_rewire`."""
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, dropin
import posdist_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_knn_metric', 'gnpde_radius_workspace_bytes', 'gnpde_radius_quantile', 'gnpde_radius_count', 'gnpde_radius_fill')


def test_symbols_in_header_library_bindings_and_docs():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  L = G.lib()
  for name in SYMBOLS:
    assert re.search(r'\b' + name + r'\s*\(', header), name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name)
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 12 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION
  assert re.search(r'#define\s+GNPDE_METRIC_SQEUCLIDEAN\s+0', header) and re.search(r'#define\s+GNPDE_METRIC_POINCARE\s+1', header)
  assert (_lib.METRIC_SQEUCLIDEAN, _lib.METRIC_POINCARE) == (0, 1)
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for name in SYMBOLS:
    assert name in doc
  # the header states the two arguments the issue asks for: key symmetry and the rank rule against np.quantile
  assert 'bit-identical to key_ji' in header and 'lower\n * order statistic' in header.replace('\r', '')


def test_entry_points_reject_bad_arguments_before_any_launch():
  L = G.lib()
  x = torch.zeros(10, 4)
  tau = torch.zeros(2)
  rowptr = torch.zeros(11, dtype=torch.int64)
  ei = torch.zeros(2, 100, dtype=torch.int64)
  ws = torch.zeros(int(L.gnpde_radius_workspace_bytes(10, 4)), dtype=torch.uint8)
  p = _lib.ptr
  quant = lambda n, metric, q: L.gnpde_radius_quantile(p(x), n, 4, 4, metric, q, p(tau), p(ws), ws.numel(), None)
  for q in (-0.001, 1.5, float('nan')):
    assert quant(10, 0, q) == -2 and b'radius_quantile' in L.gnpde_last_error()
  assert quant(10, 2, 0.5) == -2 and quant(10, -1, 0.5) == -2
  assert quant(2 ** 31, 0, 0.5) == -2
  assert quant(0, 0, 0.5) == -1
  assert L.gnpde_radius_quantile(p(x), 10, 4, 3, 0, 0.5, p(tau), p(ws), ws.numel(), None) == -1       # row stride under the width
  assert L.gnpde_radius_quantile(p(x), 10, 4, 4, 0, 0.5, p(tau), p(ws), 8, None) == -3
  assert L.gnpde_radius_count(p(x), 10, 4, 4, 7, None, 1.0, p(rowptr), p(ws), ws.numel(), None) == -2
  assert L.gnpde_radius_count(p(x), 10, 4, 4, 0, None, -1.0, p(rowptr), p(ws), ws.numel(), None) == -1
  assert L.gnpde_radius_count(p(x), 2 ** 31, 4, 4, 0, None, 1.0, p(rowptr), p(ws), ws.numel(), None) == -2
  assert L.gnpde_radius_fill(p(x), 10, 4, 4, 3, None, 1.0, p(ei), 100, p(ws), ws.numel(), None) == -2
  assert L.gnpde_radius_fill(p(x), 10, 4, 4, 0, None, 1.0, None, 100, p(ws), ws.numel(), None) == -1
  assert L.gnpde_radius_workspace_bytes(0, 4) == 0 and L.gnpde_radius_workspace_bytes(2 ** 31, 4) == 0
  assert L.gnpde_radius_workspace_bytes(10, 4) >= 2 * 40 + 3 * 2048 * 8
  idx = torch.zeros(10, 2, dtype=torch.int64)
  kws = torch.zeros(int(L.gnpde_knn_workspace_bytes(10, 4, 2)), dtype=torch.uint8)
  assert L.gnpde_knn_metric(p(x), 10, 4, 4, 2, 2, p(idx), None, p(kws), kws.numel(), None) == -2
  assert b'metric' in L.gnpde_last_error()
  assert L.gnpde_knn_metric(p(x), 10, 4, 4, 11, 1, p(idx), None, p(kws), kws.numel(), None) == -2


def test_python_surface_checks_arguments_without_a_device():
  x = torch.zeros(8, 3)
  with pytest.raises(G.GnpdeError, match='metric'):
    G.ops.knn(x, 2, metric='cosine')
  with pytest.raises(G.GnpdeError):
    G.ops.knn(x, 2, metric='poincare')                 # a host tensor
  with pytest.raises(G.GnpdeError, match='exactly one'):
    G.ops.radius_graph(x)
  with pytest.raises(G.GnpdeError, match='exactly one'):
    G.ops.radius_graph(x, quantile=0.1, threshold=1.0)
  for q in (-0.1, 1.0001, float('nan')):
    with pytest.raises(G.GnpdeError, match='quantile'):
      G.ops.radius_graph(x, quantile=q)
  with pytest.raises(G.GnpdeError, match='metric'):
    G.ops.radius_graph(x, quantile=0.1, metric='cosine')
  with pytest.raises(G.GnpdeError, match='threshold'):
    G.ops.radius_graph(x, threshold=-1.0)
  with pytest.raises(G.GnpdeError):
    G.ops.radius_graph(x, quantile=0.1)                # a host tensor
  with pytest.raises(G.GnpdeError):
    G.ops.radius_graph(torch.zeros(8), quantile=0.1)
  with pytest.raises(TypeError):
    G.ops.radius_graph(x, 0.1)                         # quantile / threshold are keyword-only


@pytest.mark.parametrize('metric', P.METRICS)
def test_threshold_to_key_inverts_key_to_distance(metric):
  """distance_to_key(key_to_distance(k)) == k for float32 keys over many binades: `threshold=` given a returned tau distance
  selects the same key, hence the same set."""
  rng = np.random.default_rng(3)
  keys = np.concatenate([np.float32(2.0) ** rng.integers(-60, 40, 200) * rng.uniform(1, 2, 200).astype(np.float32),
                         np.array([0.0, 1.0, 0.25, 3.0e38], dtype=np.float32)]).astype(np.float32)
  for k in keys:
    t = G.ops.key_to_distance(k, metric)
    assert G.ops.distance_to_key(t, metric) == float(k)
    below = np.nextafter(np.float64(t), -np.inf)
    if k > 0:
      assert G.ops.distance_to_key(below, metric) < float(k)
  assert G.ops.distance_to_key(float('inf'), metric) == float('inf')
  assert G.ops.distance_to_key(0.0, metric) == 0.0


def tie_free(n, d, seed, scale=1.0):
  return torch.rand(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def test_oracle_agrees_with_scipy_and_the_reference_formula():
  """hyperbolic_distances.hyperbolize restated line by line on scipy's pdist / squareform (with the argument handling it
  lacks) against posdist_oracle.distances64."""
  sd = pytest.importorskip('scipy.spatial.distance')
  x = (tie_free(60, 5, 1) - 0.5) * 0.8                       # inside the unit ball
  m = sd.squareform(sd.pdist(x.numpy(), 'sqeuclidean'))
  qsqr = np.sum(x.numpy() ** 2, axis=1)
  eps = np.finfo(np.double).eps
  divisor = np.maximum(1 - qsqr[:, np.newaxis], eps) * np.maximum(1 - qsqr[np.newaxis, :], eps)
  ref = np.arccosh(1 + 2 * m / divisor)
  ours = P.distances64(x, 'poincare').numpy()
  assert np.allclose(ours, ref, rtol=1e-9, atol=1e-12)
  assert np.allclose(P.distances64(x, 'sqeuclidean').numpy(), sd.squareform(sd.pdist(x.numpy(), 'euclidean')), rtol=1e-12, atol=1e-12)
  # a row on the unit sphere gets the clamp, not an error
  y = x.clone()
  y[0] = 0
  y[0, 0] = 1.0
  assert bool(torch.isfinite(P.distances64(y, 'poincare')).all())


@pytest.mark.parametrize('metric', P.METRICS)
def test_oracle_order_agrees_with_sklearn_on_tie_free_input(metric):
  nb = pytest.importorskip('sklearn.neighbors')
  x = (tie_free(80, 4, 2) - 0.5) * 0.9
  dist = P.distances64(x, metric).numpy()
  k = 9
  _, indices = nb.NearestNeighbors(n_neighbors=k, metric='precomputed').fit(dist).kneighbors(dist)
  assert np.array_equal(indices, P.knn_order(P.keys64(x, metric).numpy())[:, :k].numpy())


def tied_keys(n, levels, seed):
  """A symmetric [n, n] key matrix with zero diagonal and only `levels` distinct off-diagonal values."""
  g = torch.Generator().manual_seed(seed)
  v = torch.randint(1, levels + 1, (n, n), generator=g).double()
  v = torch.triu(v, 1)
  return (v + v.T).numpy()


@pytest.mark.parametrize('q', [0.0, 1e-3, 0.01, 0.5, 1.0])
@pytest.mark.parametrize('source', ['ties3', 'ties40', 'integers', 'real'])
def test_rank_rule_selects_what_numpy_quantile_selects(source, q):
  """The set {key <= key of rank floor((n^2 - 1) q)} equals np.where(dist <= np.quantile(dist, q)): on heavily tied matrices, on
  the exact integer case and on a tie-free one; for the distance as for the key (the map is monotone)."""
  if source == 'ties3':
    keys = tied_keys(57, 3, 1)
  elif source == 'ties40':
    keys = tied_keys(120, 40, 2)
  elif source == 'integers':
    keys = P.exact_case('sqeuclidean', 65, 3)[1].astype(np.float64)
  else:
    keys = P.keys64((tie_free(90, 6, 5) - 0.5) * 0.9, 'poincare').numpy()
  ours = P.radius_edges(keys, P.quantile_key(keys, q))
  assert torch.equal(ours, P.numpy_quantile_edges(keys, q))
  dist = np.arccosh(1 + 2 * keys)
  assert torch.equal(ours, P.numpy_quantile_edges(dist, q))
  if q == 0.0:
    assert ours.shape[1] == int((keys == 0).sum())
  if q == 1.0:
    assert ours.shape[1] == keys.size


def test_exact_poincare_inputs_are_exact_in_fp32():
  """The claim behind the bit-for-bit device tests: for the dyadic inputs s, a, a_i a_j and D survive the cast to fp32 unchanged,
  so keys32 differs from the float64 key by one rounding of the division only; the key matrix is symmetric bit for bit."""
  for d in (1, 2, 3, 16, 22, 162):
    x = P.dyadic_input(257, d, 1000 * 257 + d)
    s = P.sq_norms64(x)
    assert float(s.max()) < 1
    a = 1.0 - s
    prod = a[:, None] * a[None, :]
    D = P.K.dist64(x)
    for t in (s, a, prod, D):
      assert torch.equal(t.float().double(), t)
    k32 = P.keys32(x, 'poincare')
    exact = (D / prod).numpy()
    assert np.all(np.abs(k32.astype(np.float64) - exact) <= 2.0 ** -24 * exact)
    assert np.array_equal(k32, k32.T) and np.all(np.diag(k32) == 0)


@pytest.mark.parametrize('metric', P.METRICS)
@pytest.mark.parametrize('case', range(3))
def test_the_band_leaves_few_pairs_undetermined(metric, case):
  """On the oracle alone: the derived band decides all but 1 % of the radius graph's edges and of the k-NN entries."""
  band = P.real_radius_band(metric, case)
  open_ = band.undetermined()
  print('%s %s: tau %.6g, b* %.3g, %d of E = %d pairs undetermined' % (metric, P.real_shape(metric, case), band.tau, band.bstar,
                                                                      open_, band.E))
  assert open_ <= P.CAP_SHARE * band.E
  n, _, _, k = P.real_shape(metric, case)
  assert P.real_knn_band(metric, case).undetermined() <= P.CAP_SHARE * n * k


STUB = '''
MARK = 'from the stub'
def apply_pos_dist_rewire(data, opt, data_dir='../data'):
  return 'stub rewire'
def apply_beltrami(data, opt, data_dir='../data'):
  return 'stub beltrami'
def KNN(x, opt):
  return 'stub KNN'
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


def test_dropin_serves_the_native_pos_dist_rewire(tmp_path, clean_dropin):
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  served = dropin.install(native_posdist=True)
  assert 'graph_rewiring' in served
  import graph_rewiring
  ours = sys.modules['gnpde_amd.graph_rewiring']
  for name in ('apply_pos_dist_rewire', 'apply_beltrami', 'hyperbolize', 'apply_feat_KNN', 'apply_dist_KNN', 'apply_dist_threshold'):
    assert getattr(graph_rewiring, name) is getattr(ours, name)
  assert graph_rewiring.KNN(None, None) == 'stub KNN' and graph_rewiring.unrelated() == 'from the stub'
  dropin.uninstall()
  assert 'graph_rewiring' not in sys.modules and '_reference_graph_rewiring' not in sys.modules and not dropin.installed()
  # the flags combine, and without this one the stub's function is served
  dropin.install(native_knn=True, native_posdist=True)
  import graph_rewiring as both
  assert both.KNN is ours.KNN and both.apply_pos_dist_rewire is ours.apply_pos_dist_rewire
  dropin.uninstall()
  dropin.install(native_knn=True)
  import graph_rewiring as knn_only
  assert knn_only.apply_pos_dist_rewire(None, None) == 'stub rewire'


def test_dropin_command_line_knows_the_flag():
  with pytest.raises(SystemExit, match='--native-posdist'):
    dropin.main(['--no-such-flag'])
  with pytest.raises(SystemExit, match='no such script'):
    dropin.main(['--native-posdist', '/nonexistent/script.py'])


def fake_ops(monkeypatch, calls):
  """ops.knn / ops.radius_graph answered by the oracle on the host."""
  def knn(x, k, return_dist=False, metric='sqeuclidean'):
    calls.append(('knn', metric, int(k)))
    return P.knn_order(P.keys64(x, metric).numpy())[:, :k]

  def radius_graph(x, *, quantile=None, threshold=None, metric='sqeuclidean', **kw):
    calls.append(('radius', metric, quantile))
    keys = P.keys64(x, metric).numpy()
    return P.radius_edges(keys, P.quantile_key(keys, quantile))
  monkeypatch.setattr(G.ops, 'knn', knn)
  monkeypatch.setattr(G.ops, 'radius_graph', radius_graph)
  monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)


@pytest.mark.parametrize('kind,sparse,expect', [
  ('HYPS16', 'topk', ('knn', 'poincare', 5)),
  ('HYPS16', 'threshold', ('radius', 'poincare', 0.03)),
  ('DW64', 'topk', ('knn', 'sqeuclidean', 5)),
  ('DW64', 'threshold', ('radius', 'sqeuclidean', 1 / 1000)),
])
def test_branch_table_of_apply_pos_dist_rewire(monkeypatch, kind, sparse, expect):
  calls = []
  fake_ops(monkeypatch, calls)
  n = 40
  enc = (tie_free(n, 4, 7) - 0.5).float() * 0.9
  data = types.SimpleNamespace(x=torch.zeros(n, 3), edge_index=torch.zeros(2, 7, dtype=torch.int64), edge_attr=torch.ones(7),
                               num_nodes=n)
  opt = {'pos_enc_type': kind, 'gdc_sparsification': sparse, 'gdc_k': 5, 'pos_dist_quantile': 0.03, 'dataset': 'Synthetic'}
  out = G.graph_rewiring.apply_pos_dist_rewire(data, opt, pos_encoding=enc)
  assert out is data and calls == [expect]
  metric = expect[1]
  keys = P.keys64(enc, metric).numpy()
  if sparse == 'topk':
    want = torch.stack([torch.arange(n).repeat_interleave(5), P.knn_order(keys)[:, :5].reshape(-1)])
  else:
    want = P.radius_edges(keys, P.quantile_key(keys, expect[2]))
  assert data.edge_index.dtype == torch.int64 and torch.equal(data.edge_index, want)
  assert data.edge_attr is None                      # a stale attribute of the old edge set is dropped


def test_apply_pos_dist_rewire_loads_the_cached_pickle_and_writes_none(monkeypatch, tmp_path):
  import pickle
  calls = []
  fake_ops(monkeypatch, calls)
  n = 30
  enc = (tie_free(n, 3, 9) - 0.5).float()
  (tmp_path / 'pos_encodings').mkdir()
  with open(tmp_path / 'pos_encodings' / 'Synthetic_DW64.pkl', 'wb') as f:
    pickle.dump({'data': enc}, f)
  with open(tmp_path / 'pos_encodings' / 'Synthetic_HYPS03.pkl', 'wb') as f:
    pickle.dump(enc * 0.9, f)
  for kind in ('DW64', 'HYPS03'):
    data = types.SimpleNamespace(edge_index=torch.zeros(2, 0, dtype=torch.int64), edge_attr=None, num_nodes=n)
    opt = {'pos_enc_type': kind, 'gdc_sparsification': 'topk', 'gdc_k': 4, 'pos_dist_quantile': 0.1, 'dataset': 'Synthetic'}
    G.graph_rewiring.apply_pos_dist_rewire(data, opt, data_dir=str(tmp_path))
    assert data.edge_index.shape == (2, 4 * n)
  assert sorted(os.listdir(tmp_path / 'pos_encodings')) == ['Synthetic_DW64.pkl', 'Synthetic_HYPS03.pkl']   # no _dists.pkl
  with pytest.raises(FileNotFoundError):
    G.graph_rewiring.apply_beltrami(None, {'pos_enc_type': 'HYPS99', 'dataset': 'Synthetic'}, data_dir=str(tmp_path))
  with pytest.raises(ValueError):
    G.graph_rewiring.apply_pos_dist_rewire(None, {'pos_enc_type': 'GDC', 'gdc_sparsification': 'topk'}, pos_encoding=enc)


def test_hyperbolize_refuses_large_inputs():
  with pytest.raises(G.GnpdeError, match='refused'):
    G.graph_rewiring.hyperbolize(torch.zeros(129, 2))
