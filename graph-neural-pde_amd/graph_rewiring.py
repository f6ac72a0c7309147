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
never emitted (PyG's dense top-k also emits zero-weight edges, in arbitrary order).  With opt['gnpde_gdc_approx'] = 'push' and a false
opt['exact'] the reference's approximate branch runs instead: a forward push per source (`ops.gdc_push`), nothing dense.

Positional-distance rewiring (`--rewiring pos_enc_knn`; reference graph_rewiring.py:285-342, hyperbolic_distances.py:7-14,
distances_kNN.py): `apply_pos_dist_rewire` with `hyperbolize`, `apply_feat_KNN`, `apply_dist_KNN`, `apply_dist_threshold` and
`apply_beltrami` (which, with opt['gnpde_generate_pos_enc'], trains a missing DW<d> pickle natively: deepwalk_embeddings.py; with
opt['gnpde_generate_hyp_enc'], a missing HYPS<dd> pickle: hyperbolic_embeddings.py; and, with opt['gnpde_pos_enc_nmf_dim'], compresses a missing GDC encoding by NMF: pos_enc_factorisation.py).  The reference builds a dense float64 [n, n] distance matrix (scipy pdist + squareform), takes np.quantile over
it or hands it to sklearn's NearestNeighbors(metric='precomputed'); here the edge set comes straight from the encodings
(`ops.knn(metric=...)`, `ops.radius_graph`), so the helpers take ENCODINGS where the reference's take a distance matrix.
Deliberate differences: no [n, n] distance pickle is written; the edge set is computed whether or not a cache file existed (the
reference's HYP branch leaves `ei` unbound on a cache hit); a stale `data.edge_attr` is dropped; scipy, sklearn and
torch_geometric are not imported.

Edge-sampling rewiring (`--fa_layer` of GNN_KNN, and `apply_edge_sampling`; reference graph_rewiring.py:150-241): `add_edges`,
`add_outgoing_attention_edges`, `edge_sampling` and `apply_edge_sampling` under the reference's names and signatures, on the native
generator, multinomial, union and `>=` selection of `ops` (csrc/edge_sampling.hip; include/gnpde.h defines them).  The random
stream is this package's own Philox4x32-10 stream, keyed by opt['edge_sampling_seed'] (default torch.initial_seed(), read once
per model) and a per-model call counter: equal seeds give equal edge sets call by call.  Refused, because they cannot work in
the reference either: the add types 'anchored' and 'degree' (its `cat` is unbound), the four `*_distance*` sampling spaces (they
name an attention type the attention layer does not have), removal on a block whose `get_attention_weights` does not read
`odefunc.edge_index`, and three configurations whose per-edge arrays keep the OLD length (reweight_attention, the Laplacian
function on the constant block, the mixed block).  `GNN_FA` (GNN_FA.py) is the model that runs the layer."""
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


GDC_APPROX_DEFAULT = None     # apply_gdc's opt['gnpde_gdc_approx'] when the opt does not set it (the drop-in's --native-gdc-push: 'push')


class GDCWrapper(object):
  """The reference's GDCWrapper (graph_rewiring.py:345-401) without torch_geometric: same constructor, `__call__(data)` and
  `position_encoding(data)`.  diffusion_kwargs: method 'ppr' (alpha), 'heat' (t) or 'coeff' (coeffs); sparsification_kwargs: method
  'topk' (k; dim = 0, per column, is the only orientation the reference uses) or 'threshold' (eps, or avg_degree: the threshold
  that keeps avg_degree n entries, torch_geometric's __calculate_eps__; on the exact path 1 <= avg_degree < n).
  approx=None (the default): `exact` and the approximate push's `eps` in diffusion_kwargs are accepted and ignored; the exact object
  up to `tol` (the truncated tail of the series, 1e-6 by default) is computed for every size.
  approx='push' AND exact false: torch_geometric's approximate branch -- the forward push of `ops.gdc_push` with tolerance
  diffusion_kwargs['eps'], then the sparse threshold and the output normalisation; nothing dense, cost ~ n / (alpha eps).  As in
  torch_geometric that branch has ppr only (heat / coeff: NotImplementedError), no top-k, the unweighted graph and
  self_loop_weight None or 1."""

  def __init__(self, self_loop_weight=1, normalization_in='sym', normalization_out='col',
               diffusion_kwargs=dict(method='ppr', alpha=0.15), sparsification_kwargs=dict(method='threshold', avg_degree=64),
               exact=True, tol=1e-6, block=256, approx=None):
    if approx not in (None, 'push'):
      raise ValueError("GDCWrapper: approx = %r is neither None nor 'push'" % (approx,))
    self.approx = approx
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

  def _sparsification(self, n):
    kw = self.sparsification_kwargs
    method = kw.get('method')
    if method == 'topk':
      if kw.get('dim', 0) != 0:
        raise NotImplementedError('GDCWrapper: top-k along dim = %r is not built (the reference uses dim = 0, per column)' % kw.get('dim'))
      return dict(k=kw['k'])
    if method == 'threshold':
      if 'eps' not in kw:
        if int(kw['avg_degree']) >= n:
          raise NotImplementedError('GDCWrapper: threshold sparsification by avg_degree = %d >= n = %d on the exact path is not built: '
                                    'it keeps every entry of the dense [n, n] matrix; give eps or a smaller avg_degree'
                                    % (int(kw['avg_degree']), n))
        return dict(avg_degree=int(kw['avg_degree']))
      return dict(eps=kw['eps'])
    raise ValueError('GDCWrapper: unknown sparsification method %r' % (method,))

  def _takes_push(self):
    return self.approx == 'push' and not self.exact

  def _push(self, data, n):
    """(edge_index, values) of the approximate diffusion matrix, sorted by (row, col), before sparsification."""
    kw = self.diffusion_kwargs
    if kw.get('method') != 'ppr':
      raise NotImplementedError("GDCWrapper: approx = 'push' has no %r diffusion: the forward push approximates ppr only "
                                "(torch_geometric's approximate branch raises for heat as well)" % (kw.get('method'),))
    if kw.get('eps') is None:
      raise ValueError("GDCWrapper: approx = 'push' needs the push tolerance diffusion_kwargs['eps']")
    return ops.gdc_push(data.edge_index, n, kw['alpha'], kw['eps'], self_loop_weight=self.self_loop_weight,
                        normalization_in=self.normalization_in, edge_weight=data.edge_attr)

  def _push_sparsification(self):
    kw = self.sparsification_kwargs
    method = kw.get('method')
    if method == 'topk':
      raise NotImplementedError("GDCWrapper: approx = 'push' has no top-k sparsification: torch_geometric's sparse path "
                                "(sparsify_sparse) has no top-k either; use method 'threshold'")
    if method == 'threshold':
      return dict(eps=kw['eps']) if 'eps' in kw else dict(avg_degree=int(kw['avg_degree']))
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
    if self._takes_push():
      sparse = self._push_sparsification()
      ei, ew = self._push(data, n)
      data.edge_index, data.edge_attr = ops.gdc_sparse_threshold(ei, ew, n, normalization_out=self.normalization_out, **sparse)
      return data
    kw.update(self._sparsification(n))
    ei, ew = ops.gdc(data.edge_index, data.edge_attr, n, **kw)
    order = torch.sort(ei[0] * n + ei[1]).indices       # (row, col) pairs are unique
    data.edge_index, data.edge_attr = ei[:, order].contiguous(), ew[order].contiguous()
    return data

  @torch.no_grad()
  def position_encoding(self, data):
    """The dense [n, n] diffusion matrix, normalised, entry [i, j] = S[i, j] (no sparsification, reference :363-401)."""
    n, kw = self._common(data)
    if self._takes_push():
      if 4 * n * n > ops.GDC_DENSE_CAP:
        raise ops._lib.GnpdeError('GDCWrapper.position_encoding: the dense %d x %d matrix exceeds the cap of %d bytes' % (n, n, ops.GDC_DENSE_CAP))
      ei, ew = self._push(data, n)
      if self.normalization_out is not None and ew.numel():
        ew = ops._gdc_normalise(ei[0], ei[1], ew, n, self.normalization_out)
      dense = torch.zeros(n, n, dtype=torch.float32, device=ew.device)
      dense[ei[0], ei[1]] = ew                            # (row, col) pairs are unique
      return dense
    return ops.gdc(data.edge_index, data.edge_attr, n, dense_out=True, **kw)


def apply_gdc(data, opt, type="combined"):
  """The reference's apply_gdc (graph_rewiring.py:51-90) with the same option mapping: gdc_method with ppr_alpha / heat_time,
  gdc_sparsification with gdc_k (per-column top-k) or gdc_threshold, self_loop_weight, 'sym' in and 'col' out, pos_enc_orientation.
  opt['gnpde_gdc_tol'] (1e-6) truncates the series.  opt['gnpde_gdc_approx'] = 'push' together with a false opt['exact'] takes the
  approximate forward push with tolerance opt['gdc_threshold'], as the reference does for exact = False; without that option
  opt['exact'] and the push tolerance are accepted and ignored (see GDCWrapper)."""
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
                   exact=opt.get('exact', True), tol=opt.get('gnpde_gdc_tol', 1e-6), approx=opt.get('gnpde_gdc_approx', GDC_APPROX_DEFAULT))
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


DW_DEFAULTS = dict(walk_length=20, context_size=16, walks_per_node=16, num_negative_samples=1)   # the reference script's defaults


def _generate_deepwalk(data, opt, fname):
  """Train DW<d> encodings natively (deepwalk_embeddings.DeepWalk) and cache them in the layout of the reference's pickles."""
  from . import deepwalk_embeddings
  kind = opt['pos_enc_type']
  if not kind[2:].isdigit():
    raise ValueError('apply_beltrami: cannot read the embedding width from pos_enc_type %r (expected DW<d>)' % (kind,))
  model = deepwalk_embeddings.DeepWalk(data.edge_index, data.num_nodes, embedding_dim=int(kind[2:]), seed=opt.get('seed', 0), **DW_DEFAULTS)
  model.fit(opt.get('gnpde_dw_epochs', 100), batch_size=128)
  z = model.embedding.detach().to(torch.device('cpu'))
  os.makedirs(os.path.dirname(fname), exist_ok=True)
  with open(fname, 'wb') as f:
    pickle.dump({'data': z, 'acc': deepwalk_embeddings.node_classification_accuracy(z, data)}, f)
  return z


def _generate_hyperbolic(data, opt, fname):
  """Train HYPS<dd> encodings natively (hyperbolic_embeddings.PoincareEmbedding with its defaults) and cache them as the CPU tensor
  [n, dd] that the reference's pickles of this type hold."""
  from . import hyperbolic_embeddings
  try:
    d = hyperbolic_embeddings.embedding_dim_of(opt['pos_enc_type'])
  except ValueError as err:
    raise ValueError('apply_beltrami: %s' % err)
  n = data.num_nodes[0] if isinstance(data.num_nodes, list) else data.num_nodes
  model = hyperbolic_embeddings.PoincareEmbedding(data.edge_index, n, embedding_dim=d, seed=opt.get('seed', 0))
  model.fit(opt.get('gnpde_hyp_epochs', 100), batch_size=128)
  z = model.embedding.detach().to(torch.device('cpu'))
  os.makedirs(os.path.dirname(fname), exist_ok=True)
  with open(fname, 'wb') as f:
    pickle.dump(z, f)
  return z


NMF_DEFAULTS = dict(max_iter=100, tol=0.002)     # the reference script's defaults (pos_enc_factorisation.py --max_iter, --tol)


def _generate_compressed_gdc(data, opt, fname):
  """GDC encodings compressed to opt['gnpde_pos_enc_nmf_dim'] columns (pos_enc_factorisation.NMF) and cached as a CPU tensor where the
  reference's script leaves its W.  While the dense [n, n] matrix fits ops.GDC_DENSE_CAP the input is apply_gdc(type='pos_encoding'),
  the reference's literal input; above it the sparse GDC graph of apply_gdc(type='combined') (transposed for orientation 'col')."""
  import copy
  from . import pos_enc_factorisation
  n = data.num_nodes[0] if isinstance(data.num_nodes, list) else data.num_nodes
  if 4 * int(n) * int(n) <= ops.GDC_DENSE_CAP:
    print('    NMF input: the dense %d x %d GDC matrix' % (n, n))
    x = apply_gdc(data, opt, type='pos_encoding').contiguous()
  else:
    print('    NMF input: the sparse GDC graph (the dense %d x %d matrix exceeds %d bytes)' % (n, n, ops.GDC_DENSE_CAP))
    sparse = apply_gdc(copy.copy(data), opt, type='combined')
    ei = sparse.edge_index if opt['pos_enc_orientation'] == 'row' else sparse.edge_index.flip(0)
    x = (ei.contiguous(), sparse.edge_attr, (int(n), int(n)))
  model = pos_enc_factorisation.NMF(n_components=int(opt['gnpde_pos_enc_nmf_dim']), init='random', random_state=0,
                                    max_iter=opt.get('gnpde_pos_enc_nmf_iters', NMF_DEFAULTS['max_iter']),
                                    tol=opt.get('gnpde_pos_enc_nmf_tol', NMF_DEFAULTS['tol']), verbose=1)
  w = model.fit_transform(x).to(torch.device('cpu'))
  os.makedirs(os.path.dirname(fname), exist_ok=True)
  with open(fname, 'wb') as f:
    pickle.dump(w, f)
  return w


def apply_beltrami(data, opt, data_dir='../data'):
  """Positional encodings (reference graph_rewiring.py:244-282): the cached pickle `<data_dir>/pos_encodings/<dataset>_<type>.pkl`
  the reference loads (the 'data' entry for DW* types); otherwise, for pos_enc_type 'GDC', the native
  `apply_gdc(type='pos_encoding')`, cached as the reference caches it.  With a truthy opt['gnpde_generate_pos_enc'] a missing DW<d>
  pickle is trained natively (deepwalk_embeddings.DeepWalk with the reference script's defaults, opt['gnpde_dw_epochs'] epochs,
  default 100, seed opt['seed']) and cached in that layout.  With a truthy opt['gnpde_generate_hyp_enc'] a missing HYPS<dd> pickle is
  trained natively (hyperbolic_embeddings.PoincareEmbedding with its defaults, opt['gnpde_hyp_epochs'] epochs, default 100, seed
  opt['seed']) and cached as a CPU tensor [n, dd]; each key covers its own type only.  Without its option a missing DW* or HYP*
  pickle is an error, and HYP* types other than HYPS<dd> are never generated.  With opt['gnpde_pos_enc_nmf_dim'] = r a missing GDC pickle is
  generated AND compressed to [n, r] by the native NMF (the reference's pos_enc_factorisation.py; opt['gnpde_pos_enc_nmf_iters'],
  default 100, and opt['gnpde_pos_enc_nmf_tol'], default 0.002), from the sparse GDC graph once the dense matrix exceeds
  ops.GDC_DENSE_CAP, and W is cached as a CPU tensor at the same path."""
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
  if opt['pos_enc_type'].startswith('DW') and opt.get('gnpde_generate_pos_enc'):
    print('    Encodings not found! Training DeepWalk embeddings and caching them')
    return _generate_deepwalk(data, opt, fname)
  if opt['pos_enc_type'].startswith('HYP') and opt.get('gnpde_generate_hyp_enc'):
    print('    Encodings not found! Training Poincare embeddings and caching them')
    return _generate_hyperbolic(data, opt, fname)
  if opt['pos_enc_type'] != 'GDC':
    hint = ''
    if opt['pos_enc_type'].startswith('DW'):
      hint = " (set opt['gnpde_generate_pos_enc'] to train them)"
    elif opt['pos_enc_type'].startswith('HYPS'):
      hint = " (set opt['gnpde_generate_hyp_enc'] to train them)"
    raise FileNotFoundError('apply_beltrami: no cached positional encodings %s, and type %r cannot be generated here%s'
                            % (fname, opt['pos_enc_type'], hint))
  if opt.get('gnpde_pos_enc_nmf_dim'):
    print('    Encodings not found! Calculating, compressing and caching them')
    return _generate_compressed_gdc(data, opt, fname)
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


ADD_TYPES = ('random', 'importance', 'n2_radius')
ADD_TYPES_BROKEN = ('anchored', 'degree')
SAMPLING_SPACES_BROKEN = ('pos_distance', 'z_distance', 'pos_distance_QK', 'z_distance_QK')
SAMPLING_BLOCKS = ('attention',)      # blocks whose get_attention_weights reads odefunc.edge_index and nothing of the old length


def _sampling_stream(model):
  """(seed, call) of the next drawing call of this model; the call counter advances."""
  st = getattr(model, '_edge_sampling_state', None)
  if st is None:
    seed = model.opt.get('edge_sampling_seed')
    st = model._edge_sampling_state = {'seed': int(torch.initial_seed() if seed is None else seed), 'call': 0}
  call = st['call']
  st['call'] = call + 1
  return st['seed'], call


def check_edge_sampling_supported(model, opt, removal=None):
  """Raise for the option combinations that cannot run on a changed edge set (module docstring).  removal: whether edges are
  removed as well (default: opt['edge_sampling_rmv'] != 0)."""
  mopt = model.opt
  add_type = opt.get('edge_sampling_add_type')
  if add_type in ADD_TYPES_BROKEN:
    raise NotImplementedError("edge_sampling_add_type %r is not implemented: the reference's add_edges crashes on it (its `cat` is "
                              "never assigned, graph_rewiring.py:211-220)" % (add_type,))
  if add_type is not None and add_type not in ADD_TYPES:
    raise ValueError('edge_sampling_add_type %r is none of %s' % (add_type, ', '.join(ADD_TYPES)))
  if mopt.get('reweight_attention'):
    raise NotImplementedError("opt['reweight_attention'] cannot be combined with edge sampling: the attention layer's stored "
                              "edge_weights keep the length of the original edge set")
  if mopt.get('block') == 'constant' and mopt.get('function') == 'laplacian':
    raise NotImplementedError("edge sampling with function 'laplacian' on block 'constant' is not possible: odefunc.edge_weight "
                              "keeps the length of the original edge set")
  if mopt.get('block') == 'mixed':
    raise NotImplementedError("edge sampling on block 'mixed' is not possible: its mixing term odefunc.edge_weight keeps the "
                              "length of the original edge set")
  if removal is None:
    removal = opt.get('edge_sampling_rmv', 0) != 0
  if removal:
    space = opt.get('edge_sampling_space', 'attention')
    if space in SAMPLING_SPACES_BROKEN:
      raise NotImplementedError("edge_sampling_space %r is not implemented: the reference sets it as an attention_type that "
                                "SpGraphTransAttentionLayer does not have" % (space,))
    if space != 'attention':
      raise ValueError("edge_sampling_space %r is not 'attention'" % (space,))
    if mopt.get('block') not in SAMPLING_BLOCKS:
      raise NotImplementedError("edge removal (edge_sampling_rmv != 0) needs a block whose get_attention_weights reads "
                                "odefunc.edge_index: block %r has none that fits the changed edge set (supported: %s)"
                                % (mopt.get('block'), ', '.join(SAMPLING_BLOCKS)))


def set_edge_index(model, edge_index):
  """odefunc.edge_index <- edge_index, the regularised twin kept in step (as ODEblock._share_graph does)."""
  if edge_index.shape[1] > ops.INT32_MAX:
    raise ops._lib.GnpdeError('an edge set of %d columns is refused: positions of an edge set are int32' % edge_index.shape[1])
  block = model.odeblock
  block.odefunc.edge_index = edge_index
  block.reg_odefunc.odefunc.edge_index = edge_index
  return edge_index


def _both_directions(a, b):
  return torch.cat([torch.stack([a, b], dim=0), torch.stack([b, a], dim=0)], dim=1)


@torch.no_grad()
def add_outgoing_attention_edges(model, M):
  """[2, 2 M] new edges (M pairs, both directions) whose first endpoint is drawn from softmax(importance), importance_j = the
  mean over node j's incoming edges of the head-mean attention, and whose second endpoint is uniform (reference :177-197)."""
  f = model.odeblock.odefunc
  if f.attention_weights is None:
    raise ops._lib.GnpdeError("add_outgoing_attention_edges: odefunc.attention_weights has not been set (edge_sampling_add_type "
                              "'importance' needs a block that stores its attention)")
  atts = f.attention_weights.detach()
  if atts.dim() == 2:
    atts = atts.mean(dim=1)
  M = int(M)
  seed, call = _sampling_stream(model)
  importance = ops.node_importance(f.edge_index, atts, model.num_nodes)
  anchors = ops.sample_nodes(importance, M, seed, 0, call)
  partners = ops.random_nodes(model.num_nodes, M, seed, 1, call, device=importance.device)
  return _both_directions(anchors, partners)


@torch.no_grad()
def add_edges(model, opt):
  """The edge set of the extra diffusion (reference :200-224): odefunc.edge_index joined with M = int(E * edge_sampling_add) new
  pairs in both directions, unique columns ascending by (row, col); 'n2_radius': all n^2 pairs.  'importance' with M == 0 returns
  edge_index as it is, not uniqued, as the reference does."""
  check_edge_sampling_supported(model, opt, removal=False)
  n = model.num_nodes
  ei = model.odeblock.odefunc.edge_index
  M = int(ei.shape[1] * opt['edge_sampling_add'])
  kind = opt['edge_sampling_add_type']
  if kind == 'n2_radius':
    ops.require_hip(ei)
    return ops.full_adjacency(n, device=ei.device)
  if kind == 'random':
    ops.require_hip(ei)
    seed, call = _sampling_stream(model)
    new_edges = _both_directions(ops.random_nodes(n, M, seed, 0, call, device=ei.device), ops.random_nodes(n, M, seed, 1, call, device=ei.device))
  elif M > 0:
    new_edges = add_outgoing_attention_edges(model, M)
  else:
    return ei
  return ops.edge_union(ei, new_edges, n)


@torch.no_grad()
def edge_sampling(model, z, opt):
  """Keep the columns of odefunc.edge_index whose head-mean attention at state z is >= its edge_sampling_rmv quantile, in their
  order; with edge_sampling_sym the undirected set.  Written to odefunc.edge_index and returned (reference :150-174)."""
  check_edge_sampling_supported(model, opt, removal=True)
  mean_att = model.odeblock.get_attention_weights(z).detach()
  if mean_att.dim() == 2:
    mean_att = mean_att.mean(dim=1)
  threshold = ops.quantile(mean_att, opt['edge_sampling_rmv'])
  ei = ops.select_edges(model.odeblock.odefunc.edge_index, mean_att, threshold)
  if opt['edge_sampling_sym']:
    ei = to_undirected(ei, model.num_nodes)
  return set_edge_index(model, ei)


@torch.no_grad()
def apply_edge_sampling(x, pos_encoding, model, opt):
  """add_edges, then edge_sampling at the encoder output ('T0') or the diffused state ('TN') (reference :227-241)."""
  print("Rewiring with edge sampling")
  set_edge_index(model, add_edges(model, opt))
  if opt['edge_sampling_T'] == "T0":
    z = model.forward_encoder(x, pos_encoding)
  elif opt['edge_sampling_T'] == 'TN':
    z = model.forward_ODE(x, pos_encoding)
  else:
    raise Exception("Need to set edge_sampling_T")
  edge_sampling(model, z, opt)
