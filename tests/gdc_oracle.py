"""Dense float64 yardstick of the graph diffusion rewiring (shared by test_gdc_*.py; torch_geometric is not installed, so the
definition of include/gnpde.h is restated here with numpy.linalg.inv / scipy.linalg.expm and a stable sort on (-value, row)).

Error bound of the fp32 path.  Every term of S = sum_m theta_m T^m is non-negative, so rounding errors are
RELATIVE: with u = 2^-24 and L the longest row or column of the coalesced A, one Horner step X <- T X + theta_m E costs an entry at
most  (L - 1) [the row's sum: the depth of ANY summation tree over L terms, so whatever kernel the aggregation dispatch picks]
+ 1 [product] + 1 [diagonal add] + c_T  roundings.  An entry of T = w r_i r_j carries c_T <= D + 4 + (dup - 1): the two degree
sums at half weight each (r = deg^-1/2), D = ceil(L / 64) - 1 + 6 being the depth of the fixed-order segment sum (a lane adds
every 64th entry in turn, then a 6-level butterfly), the two roundings of r to fp32, two products, and the sum of `dup` duplicate
edges ('row' / 'col': one degree sum and a division, fewer).  Over the M steps, the rounding of theta and the final store:
    N = M ((L - 1) + 2 + D + 4 + dup - 1) + 2 ,   gamma = N u / (1 - N u) .
The truncated tail lowers an entry by at most  tail * max_m (T^m)_ij  with tail = 1 - sum_{m <= M} theta_m;  'sym':
T = D^1/2 P D^-1/2 with P = D^-1 A (sub)stochastic, so (T^m)_ij <= sqrt(deg_i / deg_j); 'row' / 'col': T^m is (sub)stochastic, <= 1.
    | S_native - S | <= gamma S + tail_ij .
Membership of an entry in a column's selection is decided by the bound alone (`Band`): clearly inside, clearly outside, or open."""
import functools
import math

import numpy as np
import scipy.linalg

U = 2.0 ** -24
CAP_SHARE = 0.02       # open entries allowed, as a share of n k (top-k) or of n n (threshold)
ZERO = 1e-15           # |entries| under this in the float64 inverse / exponential are structural zeros (rounding noise of the solve)


def terms(method, param, tol=1e-6):
  """theta_0 .. theta_M, M the smallest with 1 - sum <= tol (float64, fsum)."""
  if method == 'coeff':
    return [float(c) for c in param]
  theta = []
  while True:
    m = len(theta)
    theta.append(param * (1.0 - param) ** m if method == 'ppr' else math.exp(-param) * param ** m / math.factorial(m))
    if 1.0 - math.fsum(theta) <= tol:
      return theta


def adjacency(ei, w, n, self_loop_weight=1.0):
  """Step 1: dense float64 A (duplicates summed) and the multiplicity pattern."""
  ei = np.asarray(ei)
  w = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
  A = np.zeros((n, n))
  C = np.zeros((n, n), dtype=np.int64)
  np.add.at(A, (ei[0], ei[1]), w)
  np.add.at(C, (ei[0], ei[1]), 1)
  if self_loop_weight:
    A[np.arange(n), np.arange(n)] += self_loop_weight
    C[np.arange(n), np.arange(n)] += 1
  return A, C


def inv0(x, p=-1.0):
  out = np.zeros_like(x)
  np.power(x, p, out=out, where=x > 0)
  return out


def normalise(A, kind):
  """Steps 2 / 5 on a dense matrix; the reciprocal of zero is 0."""
  if kind is None:
    return A
  if kind == 'sym':
    r = inv0(A.sum(1), -0.5)
    return r[:, None] * A * r[None, :]
  if kind == 'col':
    return A * inv0(A.sum(0))[None, :]
  if kind == 'row':
    return A * inv0(A.sum(1))[:, None]
  raise ValueError(kind)


def series(T, theta):
  S = np.zeros_like(T)
  P = np.eye(T.shape[0])
  for c in theta:
    S += c * P
    P = P @ T
  return S


def diffusion(T, method, param):
  """Step 3, the exact object."""
  n = T.shape[0]
  if method == 'ppr':
    S = param * np.linalg.inv(np.eye(n) - (1.0 - param) * T)
  elif method == 'heat':
    S = scipy.linalg.expm(param * (T - np.eye(n)))
  else:
    return series(T, param)
  S[np.abs(S) < ZERO] = 0.0
  return S


def column_order(v):
  """Rows of a column by (value descending, row ascending)."""
  return np.lexsort((np.arange(v.shape[0]), -v))


def sparsify(S, k=None, eps=None):
  """Step 4: the kept mask and, per column, the kept rows in order."""
  n = S.shape[0]
  keep = np.zeros((n, n), dtype=bool)
  cols = []
  for j in range(n):
    order = column_order(S[:, j])
    order = order[S[order, j] > 0][:k] if k is not None else order[S[order, j] >= eps]
    keep[order, j] = True
    cols.append(order)
  return keep, cols


def gdc_oracle(ei, w, n, method, param, k=None, eps=None, self_loop_weight=1.0, normalization_in='sym', normalization_out='col'):
  """(edge_index [2, E'] int64, weight [E'] float64) in the native order: ascending column, within a column by (-value, row)."""
  A, _ = adjacency(ei, w, n, self_loop_weight)
  S = diffusion(normalise(A, normalization_in), method, param)
  keep, cols = sparsify(S, k, eps)
  W = normalise(np.where(keep, S, 0.0), normalization_out)
  rows = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
  cc = np.concatenate([np.full(len(c), j, dtype=np.int64) for j, c in enumerate(cols)])
  return np.stack([rows.astype(np.int64), cc]), W[rows, cc]


def dense_oracle(ei, w, n, method, param, self_loop_weight=1.0, normalization_in='sym', normalization_out='col'):
  A, _ = adjacency(ei, w, n, self_loop_weight)
  return normalise(diffusion(normalise(A, normalization_in), method, param), normalization_out)


class Band(object):
  """Exact S of one case, the derived bound, and the membership rule."""

  def __init__(self, ei, w, n, method, param, k=None, eps=None, self_loop_weight=1.0, normalization_in='sym', tol=1e-6):
    A, C = adjacency(ei, w, n, self_loop_weight)
    self.n, self.k, self.eps = n, k, eps
    self.S = diffusion(normalise(A, normalization_in), method, param)
    theta = terms(method, param, tol)
    tail = 0.0 if method == 'coeff' else max(1.0 - math.fsum(theta), 0.0)
    L = int(max((A > 0).sum(1).max(), (A > 0).sum(0).max(), 1))
    D = (L + 63) // 64 - 1 + 6
    N = (len(theta) - 1) * ((L - 1) + 2 + D + 4 + int(C.max()) - 1) + 2
    self.gamma = N * U / (1.0 - N * U)
    if normalization_in == 'sym':
      deg = A.sum(1)
      entry = np.sqrt(deg)[:, None] * inv0(deg, -0.5)[None, :]
    else:
      entry = np.ones((n, n))
    self.tail = tail * entry
    self.lo = self.S * (1.0 - self.gamma) - self.tail
    self.hi = self.S * (1.0 + self.gamma)
    if k is not None:
      inside = np.zeros((n, n), dtype=bool)
      outside = np.zeros((n, n), dtype=bool)
      for j in range(n):
        lo, hi = self.lo[:, j], self.hi[:, j]
        hi_sorted = np.sort(hi)
        could_beat = n - np.searchsorted(hi_sorted, lo, side='left') - 1          # others with hi >= lo_i (hi_i >= lo_i itself)
        lo_sorted = np.sort(lo[lo > 0])
        surely_above = lo_sorted.shape[0] - np.searchsorted(lo_sorted, hi, side='right')   # others with lo > hi_i, lo > 0
        inside[:, j] = (lo > 0) & (could_beat <= k - 1)
        outside[:, j] = (surely_above >= k) | (hi <= 0)
      self.inside, self.outside = inside, outside
    else:
      self.inside, self.outside = self.lo >= eps, self.hi < eps

  def undetermined(self):
    return int((~self.inside & ~self.outside).sum())

  def share(self):
    return self.undetermined() / float(self.n * (self.k if self.k is not None else self.n))

  def check(self, out_ei, out_w):
    """Native result with normalization_out = None (numpy arrays): order, membership and values."""
    n = self.n
    row, col, w = out_ei[0], out_ei[1], out_w.astype(np.float64)
    assert np.isfinite(w).all() and (w > 0).all()
    assert row.min() >= 0 and row.max() < n and (np.diff(col) >= 0).all(), 'columns are not ascending'
    same = np.diff(col) == 0
    assert (np.diff(w)[same] <= 0).all(), 'values increase inside a column'
    tie = same & (np.diff(w) == 0)
    assert (np.diff(row)[tie] > 0).all(), 'equal values are not in ascending row order'
    got = np.zeros((n, n), dtype=bool)
    got[row, col] = True
    assert int(got.sum()) == row.shape[0], 'an entry is returned twice'
    if self.k is not None:
      assert np.bincount(col, minlength=n).max() <= self.k
    assert not (got & self.outside).any(), '%d returned entries are clearly outside' % int((got & self.outside).sum())
    assert not (self.inside & ~got).any(), '%d entries clearly inside were not returned' % int((self.inside & ~got).sum())
    err = np.abs(w - self.S[row, col])
    bound = self.gamma * self.S[row, col] + self.tail[row, col]
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print('value error: max %.3e, worst error / bound %.3f (gamma %.3e)' % (float(err.max()), worst, self.gamma))
    assert (err <= bound).all(), 'value off by %.3e beyond the bound' % float((err - bound).max())


def random_graph(n, deg, seed, directed=False, hub=0, isolated=0, dup=0):
  """[2, E] int64: n * deg / 2 random pairs (both directions unless directed); `hub` extra neighbours of node 0 (both directions);
  the last `isolated` nodes get no edge; `dup` edges are repeated."""
  r = np.random.RandomState(seed)
  m = n - isolated
  a, b = r.randint(0, m, n * deg // 2), r.randint(0, m, n * deg // 2)
  a, b = a[a != b], b[a != b]
  ei = np.stack([a, b])
  if not directed:
    ei = np.concatenate([ei, ei[::-1]], axis=1)
  if hub:
    other = 1 + r.permutation(m - 1)[:hub]
    z = np.zeros(hub, dtype=np.int64)
    ei = np.concatenate([ei, np.stack([z, other]), np.stack([other, z])], axis=1)
  if dup:
    ei = np.concatenate([ei, ei[:, r.randint(0, ei.shape[1], dup)]], axis=1)
  return ei.astype(np.int64)


def random_weights(e, seed):
  """fp32-representable weights in [0.5, 1.5)."""
  return (0.5 + np.random.RandomState(seed).rand(e)).astype(np.float32)


# name -> keyword arguments of a GPU-test case (graph + gdc arguments); `block` is the native path's column block
def _cases():
  c = {}
  c['second_block'] = dict(graph=dict(n=257, deg=6, seed=1), method='ppr', param=0.15, k=16, block=256)
  for k in (1, 16, 128):
    c['plain_k%d' % k] = dict(graph=dict(n=300, deg=6, seed=2), method='ppr', param=0.05, k=k, block=256)
  c['few_positive'] = dict(graph=dict(n=40, deg=4, seed=3), method='ppr', param=0.15, k=64, block=256)
  c['block64'] = dict(graph=dict(n=300, deg=6, seed=2), method='ppr', param=0.05, k=16, block=64)
  # the hub row (> 512 entries) makes L, and with it gamma, large: ppr alpha = 0.15 (85 steps) leaves 2.9 % of the entries open on
  # the unweighted graph, over the cap, and the unweighted alpha = 0.3 sits exactly on it (192 of 9600: the many leaves that hang on
  # the hub alone are exactly tied).  Random weights break those ties: alpha = 0.3 with weights leaves 0.8 % open
  c['hub_ppr'] = dict(graph=dict(n=600, deg=4, seed=4, hub=530), weights=12, method='ppr', param=0.3, k=16, block=256)
  c['hub_heat'] = dict(graph=dict(n=600, deg=4, seed=4, hub=530), method='heat', param=3.0, k=16, block=256)
  # two row splits (n > 512) merged with k > 64: the merge's strided loop over k and its ballot count
  c['split_k128'] = dict(graph=dict(n=600, deg=6, seed=12), method='heat', param=3.0, k=128, block=256)
  c['directed'] = dict(graph=dict(n=300, deg=8, seed=5, directed=True), method='ppr', param=0.15, k=16, block=256)
  c['weighted_dups'] = dict(graph=dict(n=120, deg=6, seed=6, dup=60), weights=7, method='heat', param=3.0, k=16, block=64)
  c['isolated'] = dict(graph=dict(n=100, deg=4, seed=8, isolated=5), method='ppr', param=0.15, k=8, block=256, self_loop_weight=0.0)
  c['threshold'] = dict(graph=dict(n=300, deg=6, seed=9), method='ppr', param=0.15, eps=0.2, block=256)
  c['threshold_heat'] = dict(graph=dict(n=300, deg=6, seed=9), method='heat', param=3.0, eps=0.02, block=64)
  c['coeff'] = dict(graph=dict(n=300, deg=6, seed=10), weights=11, method='coeff', param=(0.5, 0.3, 0.2), k=16, block=256)
  c['col_in'] = dict(graph=dict(n=300, deg=8, seed=5, directed=True), method='ppr', param=0.15, k=16, block=256, normalization_in='col')
  return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case_inputs(name):
  """(edge_index [2, E] int64 numpy, weights fp32 numpy or None, n, keyword arguments shared by oracle and native path)."""
  c = dict(CASES[name])
  g = c.pop('graph')
  ei = random_graph(**g)
  seed_w = c.pop('weights', None)
  w = random_weights(ei.shape[1], seed_w) if seed_w is not None else None
  return ei, w, g['n'], c


@functools.lru_cache(maxsize=None)
def case_band(name):
  ei, w, n, c = case_inputs(name)
  return Band(ei, w, n, c['method'], c['param'], k=c.get('k'), eps=c.get('eps'), self_loop_weight=c.get('self_loop_weight', 1.0),
              normalization_in=c.get('normalization_in', 'sym'))
