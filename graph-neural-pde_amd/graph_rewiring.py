"""Graph rewiring under the reference's names and signatures (src/graph_rewiring.py).

k-nearest-neighbour rewiring in feature space (BLEND's `--rewire_KNN`; reference src/graph_rewiring.py:116-147): `KNN` and
`apply_KNN` under the reference's names and signatures.  The search is the native kernel behind `ops.knn` (the reference uses a
pykeops LazyTensor.argKmin); making the edge set undirected is torch device ops (once per rewiring).

Tie order is a definition of this package (KeOps leaves it unspecified): a node's neighbours are ascending by the computed
distance, equal distances by ascending node index; a node is its own first neighbour (distance exactly 0).

Graph diffusion rewiring (`--rewiring gdc`, and `--beltrami --pos_enc_type GDC`; reference graph_rewiring.py:51-90, 345-401):
`apply_gdc` and `GDCWrapper`.  The reference's class subclasses torch_geometric.transforms.GDC and inverts a dense [n, n] matrix;
here the diffusion matrix is formed column block by column block with the aggregation kernel and sparsified on the device
(`ops.gdc`; the definition is in include/gnpde.h).  torch_geometric is not imported.  One deliberate difference: zero entries are
never emitted (PyG's dense top-k also emits zero-weight edges, in arbitrary order).

Positional-distance rewiring (`--rewiring pos_enc_knn`; reference graph_rewiring.py:285-342, hyperbolic_distances.py:7-14,
distances_kNN.py): `apply_pos_dist_rewire` with `hyperbolize`, `apply_feat_KNN`, `apply_dist_KNN`, `apply_dist_threshold` and
`apply_beltrami`.  The reference builds a dense float64 [n, n] distance matrix (scipy pdist + squareform), takes np.quantile over
it or hands it to sklearn's NearestNeighbors(metric='precomputed'); here the edge set comes straight from the encodings
(`ops.knn(metric=...)`, `ops.radius_graph`), so the helpers take ENCODINGS where the reference's take a distance matrix.
Deliberate differences: no [n, n] distance pickle is written; the edge set is computed whether or not a cache file existed (the
reference's HYP branch leaves `ei` unbound on a cache hit); a stale `data.edge_attr` is dropped; scipy, sklearn and
torch_geometric are not imported."""
import os
import pickle

import torch

from . import ops


def to_undirected(edge_index, num_nodes):
  """Both directions of every edge, duplicates removed, sorted by (row, col): what torch_geometric.utils.to_undirected returns for
  an index without edge attributes."""
  row = torch.cat([edge_index[0], edge_index[1]])
  col = torch.cat([edge_index[1], edge_index[0]])
  key = torch.unique(row * int(num_nodes) + col)     # sorted
  return torch.stack([torch.div(key, int(num_nodes), rounding_mode='floor'), key % int(num_nodes)], dim=0)


def KNN(x, opt):
  """edge_index [2, n k] int64: row 0 is every node repeated k times, row 1 its k nearest neighbours in squared Euclidean
  distance (the reference's layout, graph_rewiring.py:127-129); with opt['rewire_KNN_sym'] the undirected edge set."""
  k = opt['rewire_KNN_k']
  print(f"Rewiring with KNN: t={opt['rewire_KNN_T']}, k={opt['rewire_KNN_k']}")
  ind = ops.knn(x, k)
  n = ind.shape[0]
  src = torch.arange(n, dtype=torch.int64, device=ind.device).repeat_interleave(k)
  ei = torch.stack([src, ind.reshape(-1)], dim=0)
  if opt['rewire_KNN_sym']:
    ei = to_undirected(ei, n)
  return ei


@torch.no_grad()
def apply_KNN(data, pos_encoding, model, opt):
  if opt['rewire_KNN_T'] == "raw":
    ei = KNN(data.x, opt)  # rewiring on raw features here
  elif opt['rewire_KNN_T'] == "T0":
    ei = KNN(model.forward_encoder(data.x, pos_encoding), opt)
  elif opt['rewire_KNN_T'] == 'TN':
    ei = KNN(model.forward_ODE(data.x, pos_encoding), opt)
  else:
    raise Exception("Need to set rewire_KNN_T")
  return ei


class GDCWrapper(object):
  """The reference's GDCWrapper (graph_rewiring.py:345-401) without torch_geometric: same constructor, `__call__(data)` and
  `position_encoding(data)`.  diffusion_kwargs: method 'ppr' (alpha), 'heat' (t) or 'coeff' (coeffs); sparsification_kwargs: method
  'topk' (k; dim = 0, per column, is the only orientation the reference uses) or 'threshold' (eps).  `exact` and the approximate
  push's `eps` in diffusion_kwargs are accepted and ignored: this path computes the exact object up to `tol` (the truncated tail
  of the series, 1e-6 by default), for every size.  Sparsification by avg_degree is not built."""

  def __init__(self, self_loop_weight=1, normalization_in='sym', normalization_out='col',
               diffusion_kwargs=dict(method='ppr', alpha=0.15), sparsification_kwargs=dict(method='threshold', avg_degree=64),
               exact=True, tol=1e-6, block=256):
    self.self_loop_weight = self_loop_weight
    self.normalization_in = normalization_in
    self.normalization_out = normalization_out
    self.diffusion_kwargs = diffusion_kwargs
    self.sparsification_kwargs = sparsification_kwargs
    self.exact = exact
    self.tol = tol
    self.block = block

  def _diffusion(self):
    kw = self.diffusion_kwargs
    method = kw.get('method')
    if method == 'ppr':
      return dict(method='ppr', alpha=kw['alpha'])
    if method == 'heat':
      return dict(method='heat', t=kw['t'])
    if method == 'coeff':
      return dict(method='coeff', coeffs=kw['coeffs'])
    raise ValueError('GDCWrapper: unknown diffusion method %r' % (method,))

  def _sparsification(self):
    kw = self.sparsification_kwargs
    method = kw.get('method')
    if method == 'topk':
      if kw.get('dim', 0) != 0:
        raise NotImplementedError('GDCWrapper: top-k along dim = %r is not built (the reference uses dim = 0, per column)' % kw.get('dim'))
      return dict(k=kw['k'])
    if method == 'threshold':
      if 'eps' not in kw:
        raise NotImplementedError('GDCWrapper: threshold sparsification by avg_degree is not built; give eps')
      return dict(eps=kw['eps'])
    raise ValueError('GDCWrapper: unknown sparsification method %r' % (method,))

  def _common(self, data):
    n = data.num_nodes[0] if isinstance(data.num_nodes, list) else data.num_nodes
    kw = dict(self_loop_weight=float(self.self_loop_weight) if self.self_loop_weight else 0.0, normalization_in=self.normalization_in,
              normalization_out=self.normalization_out, tol=self.tol, block=self.block)
    kw.update(self._diffusion())
    return int(n), kw

  @torch.no_grad()
  def __call__(self, data):
    """data.edge_index / data.edge_attr replaced by the diffused, sparsified, normalised graph, sorted by (row, col) as
    torch_sparse.coalesce returns it."""
    n, kw = self._common(data)
    kw.update(self._sparsification())
    ei, ew = ops.gdc(data.edge_index, data.edge_attr, n, **kw)
    order = torch.sort(ei[0] * n + ei[1]).indices       # (row, col) pairs are unique
    data.edge_index, data.edge_attr = ei[:, order].contiguous(), ew[order].contiguous()
    return data

  @torch.no_grad()
  def position_encoding(self, data):
    """The dense [n, n] diffusion matrix, normalised, entry [i, j] = S[i, j] (no sparsification, reference :363-401)."""
    n, kw = self._common(data)
    return ops.gdc(data.edge_index, data.edge_attr, n, dense_out=True, **kw)


def apply_gdc(data, opt, type="combined"):
  """The reference's apply_gdc (graph_rewiring.py:51-90) with the same option mapping: gdc_method with ppr_alpha / heat_time,
  gdc_sparsification with gdc_k (per-column top-k) or gdc_threshold, self_loop_weight, 'sym' in and 'col' out, pos_enc_orientation.
  opt['exact'] and the push tolerance are accepted and ignored (see GDCWrapper); opt['gnpde_gdc_tol'] (1e-6) truncates the series."""
  num_edges = lambda d: int(d.edge_index.shape[1])
  print('raw data contains {} edges and {} nodes'.format(num_edges(data), data.num_nodes))
  print('performing gdc transformation with method {}, sparsification {}'.format(opt['gdc_method'], opt['gdc_sparsification']))
  if opt['gdc_method'] == 'ppr':
    diff_args = dict(method='ppr', alpha=opt['ppr_alpha'])
  else:
    diff_args = dict(method='heat', t=opt['heat_time'])
  if opt['gdc_sparsification'] == 'topk':
    sparse_args = dict(method='topk', k=opt['gdc_k'], dim=0)
  else:
    sparse_args = dict(method='threshold', eps=opt['gdc_threshold'])
  diff_args['eps'] = opt.get('gdc_threshold')
  print('gdc sparse args: {}'.format(sparse_args))
  gdc = GDCWrapper(float(opt['self_loop_weight']) if opt['self_loop_weight'] != 0 else None, normalization_in='sym',
                   normalization_out='col', diffusion_kwargs=diff_args, sparsification_kwargs=sparse_args,
                   exact=opt.get('exact', True), tol=opt.get('gnpde_gdc_tol', 1e-6))
  if isinstance(data.num_nodes, list):
    data.num_nodes = data.num_nodes[0]
  if type == 'combined':
    data = gdc(data)
  elif type == 'pos_encoding':
    if opt['pos_enc_orientation'] == "row":  # encode row of S_hat
      return gdc.position_encoding(data)
    elif opt['pos_enc_orientation'] == "col":  # encode col of S_hat
      return gdc.position_encoding(data).T
  print('following rewiring data contains {} edges and {} nodes'.format(num_edges(data), data.num_nodes))
  return data


HYPERBOLIZE_CAP = 2 << 30     # bytes of the dense [n, n] float32 matrix `hyperbolize` agrees to write
POS_DIST_QUANTILE = 1 / 1000  # the reference's default of apply_dist_threshold / threshold_mat (distances_kNN.py:21, 31)


def _encodings(x):
  """Positional encodings as a float32 matrix on the device the native ops run on (the reference's pickles hold CPU tensors or
  ndarrays)."""
  x = torch.as_tensor(x)
  if x.dtype != torch.float32:
    x = x.to(torch.float32)
  if not x.is_cuda and torch.cuda.is_available():
    x = x.cuda()
  return x


def hyperbolize(x):
  """Dense [n, n] float32 matrix of Poincare-ball distances arccosh(1 + 2 |x_i - x_j|^2 / ((1 - |x_i|^2)(1 - |x_j|^2))) between the
  rows of x (reference hyperbolic_distances.py:7-14): every row of the native search with k = n, scattered into place.  For small
  n and for tests only: it refuses above HYPERBOLIZE_CAP bytes, as `ops.gdc(dense_out=True)` does, and above the largest k of
  the search (n <= 128).  Nothing else in this module needs this matrix."""
  x = _encodings(x)
  n = x.shape[0]
  if 4 * n * n > HYPERBOLIZE_CAP or n > ops.KNN_MAX_K:
    raise ops._lib.GnpdeError('hyperbolize: a dense [%d, %d] matrix is refused (n <= %d, %d bytes); use ops.knn(metric='
                              "'poincare') or ops.radius_graph" % (n, n, ops.KNN_MAX_K, HYPERBOLIZE_CAP))
  idx, dist = ops.knn(x, n, return_dist=True, metric='poincare')
  out = torch.empty(n, n, dtype=torch.float32, device=dist.device)
  out.scatter_(1, idx, dist)
  return out


def _knn_edges(x, k, metric):
  ind = ops.knn(_encodings(x), int(k), metric=metric)
  n = ind.shape[0]
  src = torch.arange(n, dtype=torch.int64, device=ind.device).repeat_interleave(int(k))
  return torch.stack([src, ind.reshape(-1)], dim=0)


def apply_feat_KNN(x, k):
  """edge_index [2, n k] int64 (row 0: every node k times, row 1: its k nearest rows of x in Euclidean distance, itself first):
  the reference's distances_kNN.apply_feat_KNN (:5-11, sklearn NearestNeighbors) on the native search.  x: ENCODINGS [n, d]."""
  return _knn_edges(x, k, 'sqeuclidean')


def apply_dist_KNN(x, k):
  """The reference's distances_kNN.apply_dist_KNN (:13-19) for hyperbolic distances -- but x is the ENCODINGS [n, d] (points of the
  Poincare ball), not the precomputed [n, n] distance matrix: the distances are formed tile by tile inside the search."""
  return _knn_edges(x, k, 'poincare')


def apply_dist_threshold(x, quant=POS_DIST_QUANTILE, metric='sqeuclidean'):
  """edge_index [2, E] int64 of every pair, self loops included, whose distance is <= the quant-quantile of all n^2 distances,
  sorted by (row, col): the reference's distances_kNN.apply_dist_threshold (:21-32, np.quantile + np.where) -- but x is the
  ENCODINGS [n, d], not a distance matrix; metric 'sqeuclidean' (Euclidean distances) or 'poincare' (hyperbolic)."""
  return ops.radius_graph(_encodings(x), quantile=quant, metric=metric)


def apply_beltrami(data, opt, data_dir='../data'):
  """Positional encodings (reference graph_rewiring.py:244-282): the cached pickle `<data_dir>/pos_encodings/<dataset>_<type>.pkl`
  the reference loads (the 'data' entry for DW* types); otherwise, for pos_enc_type 'GDC', the native
  `apply_gdc(type='pos_encoding')`, cached as the reference caches it.  Generating DeepWalk or hyperbolic embeddings is not
  built: a missing pickle of such a type is an error."""
  pos_enc_dir = os.path.join(data_dir, 'pos_encodings')
  fname = os.path.join(pos_enc_dir, '%s_%s.pkl' % (opt['dataset'], opt['pos_enc_type']))
  print('[i] Looking for positional encodings in %s...' % fname)
  if os.path.exists(fname):
    print('    Found them! Loading cached version')
    with open(fname, 'rb') as f:
      pos_encoding = pickle.load(f)
    if opt['pos_enc_type'].startswith('DW'):
      pos_encoding = pos_encoding['data']
    return pos_encoding
  if opt['pos_enc_type'] != 'GDC':
    raise FileNotFoundError('apply_beltrami: no cached positional encodings %s, and type %r cannot be generated here'
                            % (fname, opt['pos_enc_type']))
  print('    Encodings not found! Calculating and caching them')
  pos_encoding = apply_gdc(data, opt, type='pos_encoding')
  os.makedirs(pos_enc_dir, exist_ok=True)
  with open(fname, 'wb') as f:
    pickle.dump(pos_encoding, f)
  return pos_encoding


def apply_pos_dist_rewire(data, opt, data_dir='../data', pos_encoding=None):
  """data.edge_index replaced by the graph of positional-encoding distances (reference graph_rewiring.py:285-342), same branch table:
    pos_enc_type HYP* + gdc_sparsification 'topk'       Poincare k-NN with k = opt['gdc_k']
    pos_enc_type HYP* + 'threshold'                     Poincare radius graph at the quantile opt['pos_dist_quantile']
    pos_enc_type DW*  + 'topk'                          Euclidean k-NN with k = opt['gdc_k']
    pos_enc_type DW*  + 'threshold'                     Euclidean radius graph at the reference's default quantile 1/1000
  pos_encoding: the encodings [n, d], when the caller has them; otherwise apply_beltrami(data, opt, data_dir) loads them.
  Differences from the reference (module docstring): no [n, n] distance pickle, the edge set is always computed, edge_attr is
  dropped.  edge_index is int64 [2, E] on the device of the search."""
  kind, sparse = opt['pos_enc_type'], opt['gdc_sparsification']
  if kind.startswith('HYP'):
    metric = 'poincare'
  elif kind.startswith('DW'):
    metric = 'sqeuclidean'
  else:
    raise ValueError('apply_pos_dist_rewire: positional encoding type %r is neither HYP* nor DW*' % (kind,))
  if sparse not in ('topk', 'threshold'):
    raise ValueError('apply_pos_dist_rewire: gdc_sparsification %r is neither topk nor threshold' % (sparse,))
  if pos_encoding is None:
    pos_encoding = apply_beltrami(data, opt, data_dir)
  if sparse == 'topk':
    ei = apply_dist_KNN(pos_encoding, opt['gdc_k']) if metric == 'poincare' else apply_feat_KNN(pos_encoding, opt['gdc_k'])
  else:
    quant = opt['pos_dist_quantile'] if metric == 'poincare' else POS_DIST_QUANTILE
    ei = apply_dist_threshold(pos_encoding, quant, metric=metric)
  data.edge_index = ei.to(torch.int64)
  if getattr(data, 'edge_attr', None) is not None:
    data.edge_attr = None
  return data
