"""ops.knn(metric='poincare') and ops.radius_graph on the device against the float64 oracle of posdist_oracle.py: exact inputs
bit for bit across every tile edge and every column split, real-valued inputs under the derived rounding band, determinism,
strided rows, the edge cap, argument errors and `apply_pos_dist_rewire` end to end."""
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib
import posdist_oracle as P

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 65, 257, 1000)                 # below / across the 64-row and 64-column tiles, several workgroups
DS = {'sqeuclidean': (1, 3, 4, 22, 162), 'poincare': (1, 2, 3, 16, 22, 162)}   # K chunks of 16: partial, one, several
QS = (0.0, 1 / 1000, 0.01, 0.25, 1.0)
SPLITS = (0, 1, 3)
EXACT = [(m, n, d) for m in P.METRICS for n in NS for d in DS[m]]


@pytest.fixture
def splits():
  def force(s):
    G.ops.tune(_lib.TUNE_KNN_SPLITS, s)
  yield force
  G.ops.tune(_lib.TUNE_KNN_SPLITS, 0)


def on_device(x, dev):
  """The input as the model holds it: d = 162 on 164-float rows whose padding (poisoned) must not be read."""
  if x.shape[1] == 162:
    full = torch.full((x.shape[0], 164), 777.0, device=dev)
    full[:, :162] = x.to(dev)
    return full[:, :162]
  return x.to(dev)


def f32_bits(v):
  return int(np.float32(v).view(np.uint32))


@pytest.mark.parametrize('metric,n,d', EXACT)
def test_exact_radius_graphs(dev, splits, metric, n, d):
  """Edge sets equal np.where of the oracle's fp32 keys exactly and in (row, col) order; tau equals the oracle's rank-lo key bit
  for bit; threshold= given tau's distance returns the same set; every forced column split returns the same bytes.  At d = 1
  most keys tie at the threshold (E far above q n^2); q = 0 keeps exactly the zero-distance pairs; q = 1 all n^2 pairs."""
  x, keys = P.exact_case(metric, n, d)
  xd = on_device(x, dev)
  for q in QS:
    if q == 1.0 and n > 257:
      continue
    tau = P.quantile_key(keys, q)
    want = P.radius_edges(keys, tau)
    if q == 0.0:
      assert want.shape[1] == int((keys == 0).sum())
    if q == 1.0:
      assert want.shape[1] == n * n
    first = None
    for s in SPLITS:
      splits(s)
      ei, tau_key, tau_dist = G.ops.radius_graph(xd, quantile=q, metric=metric, return_threshold=True)
      assert ei.dtype == torch.int64 and ei.dim() == 2 and ei.shape[0] == 2
      assert f32_bits(tau_key) == f32_bits(tau), 'q = %g, S = %d: tau %r is not the rank-lo key %r' % (q, s, tau_key, float(tau))
      assert torch.equal(ei.cpu(), want), 'q = %g, S = %d: the edge set differs from np.where of the oracle' % (q, s)
      again = G.ops.radius_graph(xd, threshold=tau_dist, metric=metric)
      assert torch.equal(again, ei), 'q = %g, S = %d: threshold= at tau\'s distance selects another set' % (q, s)
      if first is None:
        first = ei
      assert torch.equal(ei, first)


@pytest.mark.parametrize('n,d', [(n, d) for n in NS for d in DS['poincare']])
def test_exact_poincare_knn(dev, splits, n, d):
  """Indices equal the oracle's (key, index) order, ties at the k-th place included; a row is its own first neighbour at
  distance exactly 0; the key of (i, j) equals that of (j, i), so mutual distances agree bit for bit."""
  x, keys = P.exact_case('poincare', n, d)
  order = P.knn_order(keys)
  xd = on_device(x, dev)
  ks = sorted({k for k in (1, 2, 16, 33, 64, 128, n) if k <= min(n, 128)})
  for s in SPLITS:
    splits(s)
    for k in ks:
      idx, dist = G.ops.knn(xd, k, return_dist=True, metric='poincare')
      assert idx.shape == (n, k) and idx.dtype == torch.int64 and dist.dtype == torch.float32
      assert torch.equal(idx.cpu(), order[:, :k]), 'k = %d, S = %d: indices differ from the (key, index) order' % (k, s)
      assert bool((dist[:, 0] == 0).all())
      want = P.distance_of(np.take_along_axis(keys, order[:, :k].numpy(), axis=1).astype(np.float64), 'poincare')
      assert torch.allclose(dist.cpu().double(), want, rtol=16 * P.U, atol=0)
  if n >= 2:
    k = min(n, 128)
    idx, dist = G.ops.knn(xd, k, return_dist=True, metric='poincare')
    full = torch.full((n, n), -1.0)
    full.scatter_(1, idx.cpu(), dist.cpu())
    both = (full >= 0) & (full.T >= 0)
    assert torch.equal(full[both], full.T[both]), 'distance(i, j) and distance(j, i) differ'


def test_exact_duplicated_rows(dev):
  """40 copies of one row: zero keys off the diagonal, ties in index order; q = 0 keeps exactly those pairs."""
  for metric in P.METRICS:
    x, keys = P.exact_case(metric, 257, 4, 40)
    xd = x.to(dev)
    assert int((keys == 0).sum()) > 257 + 40 * 40
    assert torch.equal(G.ops.radius_graph(xd, quantile=0.0, metric=metric).cpu(), P.radius_edges(keys, 0.0))
    order = P.knn_order(keys)
    for k in (16, 41, 64):
      assert torch.equal(G.ops.knn(xd, k, metric=metric).cpu(), order[:, :k])


def test_exact_key_symmetry(dev):
  """key(i, j) is bit-identical to key(j, i) on real-valued input: the radius graph at any threshold is symmetric, and so is
  what count / fill see on either side of the diagonal."""
  x = P.poincare_input(0).to(dev)
  for thr in (0.3, 1.0, 2.5):
    ei = G.ops.radius_graph(x, threshold=thr, metric='poincare').cpu()
    n = x.shape[0]
    got = torch.zeros(n, n, dtype=torch.bool)
    got[ei[0], ei[1]] = True
    assert torch.equal(got, got.T) and bool(got.diagonal().all())


@pytest.mark.parametrize('metric', P.METRICS)
@pytest.mark.parametrize('case', range(3))
@pytest.mark.parametrize('s', SPLITS)
def test_real_valued_radius_graphs(dev, splits, metric, case, s):
  """Every pair with R < tau - BR - b* is present, every pair with R > tau + BR + b* absent, the output sorted, duplicate free
  and symmetric, tau within b* of the exact one -- after the oracle alone has shown that at most 1 % of E is left open."""
  n, d, q, _ = P.real_shape(metric, case)
  band = P.real_radius_band(metric, case)
  open_ = band.undetermined()
  print('%s %s: %d of E = %d pairs undetermined' % (metric, (n, d, q), open_, band.E))
  assert open_ <= P.CAP_SHARE * band.E
  splits(s)
  xd = on_device(P.real_input(metric, case), dev)
  ei, tau_key, tau_dist = G.ops.radius_graph(xd, quantile=q, metric=metric, return_threshold=True)
  print('tau %.9g (exact %.9g, b* %.3g), E = %d' % (tau_key, band.tau, band.bstar, ei.shape[1]))
  band.check(ei, tau_key)
  assert torch.equal(G.ops.radius_graph(xd, threshold=tau_dist, metric=metric), ei)


@pytest.mark.parametrize('case', range(3))
@pytest.mark.parametrize('s', SPLITS)
def test_real_valued_poincare_knn(dev, splits, case, s):
  """The inclusion rule of knn_oracle.Band on the Poincare keys with the band BR; returned distances within the image of
  [R - BR, R + BR] under arccosh plus 16 u."""
  n, d, _, k = P.real_shape('poincare', case)
  band = P.real_knn_band('poincare', case)
  open_ = band.undetermined()
  print('poincare %s: %d of %d entries undetermined' % ((n, d, k), open_, n * k))
  assert open_ <= P.CAP_SHARE * n * k
  splits(s)
  idx, dist = G.ops.knn(P.real_input('poincare', case).to(dev), k, return_dist=True, metric='poincare')
  band.check(idx)
  P.check_distances(dist, idx, band, 'poincare')
  d_ = dist.cpu()
  assert bool((d_[:, 1:] >= d_[:, :-1]).all()), 'distances decrease along a row'


def test_determinism(dev, splits):
  x = (torch.rand(3000, 16, generator=torch.Generator().manual_seed(11)) - 0.5).mul(0.4).to(dev)
  runs = []
  for s in (0, 0, 1, 3, 7):
    splits(s)
    runs.append(G.ops.radius_graph(x, quantile=0.002, metric='poincare', return_threshold=True))
  for ei, tau_key, _ in runs[1:]:
    assert torch.equal(ei, runs[0][0]) and tau_key == runs[0][1]
  a = G.ops.knn(x, 40, return_dist=True, metric='poincare')
  b = G.ops.knn(x, 40, return_dist=True, metric='poincare')
  assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_strided_rows_and_column_slices(dev):
  """Padded rows are read in place (test_exact_* at d = 162 poison the padding); a column slice with a foreign row stride gives
  what its contiguous copy gives."""
  big = (torch.rand(300, 40, generator=torch.Generator().manual_seed(3)) - 0.5).mul(0.3).to(dev)
  view = big[:, 3:25]
  for metric in P.METRICS:
    assert torch.equal(G.ops.radius_graph(view, quantile=0.01, metric=metric), G.ops.radius_graph(view.contiguous(), quantile=0.01, metric=metric))
    assert torch.equal(G.ops.knn(view, 9, metric=metric), G.ops.knn(view.contiguous(), 9, metric=metric))


def test_max_edges_is_checked_before_anything_of_size_e_is_allocated(dev):
  x, _ = P.exact_case('sqeuclidean', 1000, 4)
  xd = x.to(dev)
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  with pytest.raises(G.GnpdeError, match='max_edges'):
    G.ops.radius_graph(xd, quantile=1.0, max_edges=1000)          # E = 10^6: edge_index would take 16 MB
  assert torch.cuda.max_memory_allocated() - base < (1 << 20)
  assert G.ops.radius_graph(xd, quantile=0.0, max_edges=100000).shape[1] >= 1000


def test_errors(dev):
  x = torch.zeros(200, 8, device=dev)
  with pytest.raises(G.GnpdeError):
    G.ops.radius_graph(x.cpu(), quantile=0.1)
  with pytest.raises(G.GnpdeError):
    G.ops.radius_graph(x.double(), quantile=0.1)
  with pytest.raises(G.GnpdeError):
    G.ops.radius_graph(torch.zeros(200, device=dev), quantile=0.1)
  with pytest.raises(G.GnpdeError):
    G.ops.knn(x.double(), 4, metric='poincare')
  with pytest.raises(G.GnpdeError):
    G.ops.knn(x, 201, metric='poincare')
  with pytest.raises(G.GnpdeError):
    G.ops.radius_graph(x, quantile=2.0)
  torch.cuda.synchronize()


def test_hyperbolize_is_the_dense_matrix(dev):
  x, keys = P.exact_case('poincare', 65, 3)
  got = G.graph_rewiring.hyperbolize(x.to(dev)).cpu().double()
  want = P.distance_of(keys.astype(np.float64), 'poincare')
  assert torch.allclose(got, want, rtol=16 * P.U, atol=0) and bool((got.diagonal() == 0).all())


@pytest.mark.parametrize('kind,sparse', [('HYPS16', 'topk'), ('HYPS16', 'threshold'), ('DW64', 'topk'), ('DW64', 'threshold')])
def test_apply_pos_dist_rewire_end_to_end(dev, kind, sparse):
  """The four branches on a 300-node synthetic `data` with given (exact) encodings: edge_index int64 [2, E] equal to the oracle's."""
  n, k, q = 300, 7, 0.02
  metric = 'poincare' if kind.startswith('HYP') else 'sqeuclidean'
  x, keys = P.exact_case(metric, n, 16)
  data = types.SimpleNamespace(x=torch.zeros(n, 3, device=dev), edge_index=torch.zeros(2, 5, dtype=torch.int64, device=dev),
                               edge_attr=torch.ones(5, device=dev), num_nodes=n)
  opt = {'pos_enc_type': kind, 'gdc_sparsification': sparse, 'gdc_k': k, 'pos_dist_quantile': q, 'dataset': 'Synthetic'}
  out = G.graph_rewiring.apply_pos_dist_rewire(data, opt, pos_encoding=x)       # a host tensor, as the reference's pickles hold
  assert out is data and data.edge_attr is None
  ei = data.edge_index
  assert ei.dtype == torch.int64 and ei.dim() == 2 and ei.shape[0] == 2
  if sparse == 'topk':
    want = torch.stack([torch.arange(n).repeat_interleave(k), P.knn_order(keys)[:, :k].reshape(-1)])
  else:
    want = P.radius_edges(keys, P.quantile_key(keys, q if metric == 'poincare' else 1 / 1000))
  assert torch.equal(ei.cpu(), want)
