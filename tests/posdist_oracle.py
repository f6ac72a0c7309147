"""Brute-force yardstick of the positional-distance rewiring (shared by test_posdist_*.py).  No reference-recorded fixture is
possible: the reference's helpers do not run on current libraries (hyperbolize takes neither a tensor nor an ndarray, and
distances_kNN imports a name that has left sklearn.neighbors).  This file restates them in float64, dense, on the CPU:

  D_ij          sum_c (x_ic - x_jc)^2, direct form                     scipy pdist(x, 'sqeuclidean') + squareform,
                                                                       reference src/hyperbolic_distances.py:8-10
  R_ij          D_ij / (a_i a_j), a_i = max(1 - |x_i|^2, eps_float64)  hyperbolic_distances.py:9-12
  distance      arccosh(1 + 2 R) (hyperbolic) or sqrt(D) (Euclidean)   hyperbolic_distances.py:13; distances_kNN.py:35-37
  k-NN          stable sort of every row by (value, index)             distances_kNN.py:5-19 (sklearn NearestNeighbors)
  threshold     np.quantile(dist, q), np.where(dist <= thresh)         distances_kNN.py:21-32
  rank rule     the key of rank lo = floor((n^2 - 1) q) among all n^2 keys selects the same set (include/gnpde.h has the argument)

Exact inputs.  Euclidean: the integers of knn_oracle.integer_input (every product and sum exact in fp32).  Poincare: dyadic
entries m / 16 with |m| <= 2 (|m| <= 1 at d = 162): s_i = sum m^2 / 256 < 1, a_i = 1 - s_i (multiples of 2^-8), a_i a_j (multiples of
2^-16 below 1) and D_ij (multiples of 2^-8) are all exact in fp32, so the kernel's key is ONE correctly rounded fp32 division,
which np.float32 division reproduces bit for bit (`keys32`).

Real-valued inputs: the rounding band.  u = 2^-24.  The computed D is within B_ij = (d + 4) u (|x_i| + |x_j|)^2 of the true one
(knn_oracle.py).  The computed norm s_i carries at most (d + 1) u s_i (d products and the partial sums), the subtraction
1 - s_i one more rounding u a_i, so the computed a_i has the relative error e_i = ((d + 1) u s_i + u) / a_i.  The product a_i a_j
adds u, the division u, and 2 u cover the second-order terms: the computed key is within
    BR_ij = (B_ij + (e_i + e_j + 4 u) D_ij) / (a_i a_j)
of R_ij.  (Euclidean: BR = B.)

The quantile key under rounding (an order-statistic argument).  Let tau be the exact key of rank lo and M = max BR.  lo + 1 pairs
have an exact key <= tau.  Such a pair's computed key is <= R + BR: either that is <= tau, or R > tau - BR >= tau - M, the pair lies
within 2 M of tau and its computed key is <= tau + b*, b* = the largest band among the pairs within 2 M of tau.  So lo + 1 computed
keys are <= tau + b*, and the computed order statistic of rank lo is <= tau + b*.  The n^2 - lo pairs with an exact key >= tau give
>= tau - b* in the same way.  The computed tau is therefore within b* of the exact one, and a pair can be on the wrong side of it
only inside |R_ij - tau| <= BR_ij + b*.
The band formula changes only with a written derivation, never by fitting it to what a device returned."""
import functools
import math

import numpy as np
import torch

import knn_oracle as K

U = 2.0 ** -24
EPS64 = float(np.finfo(np.double).eps)
METRICS = ('sqeuclidean', 'poincare')
CAP_SHARE = 0.01                     # undetermined pairs allowed, as a share of E (radius) or n k (k-NN)


def sq_norms64(x):
  return (x.detach().cpu().double() ** 2).sum(1)


def keys64(x, metric):
  """[n, n] float64 keys: D (sqeuclidean) or R = D / (a_i a_j) (poincare, float64-epsilon clamp as in the reference)."""
  D = K.dist64(x)
  if metric == 'sqeuclidean':
    return D
  a = torch.clamp(1.0 - sq_norms64(x), min=EPS64)
  return D / (a[:, None] * a[None, :])


def distance_of(keys, metric):
  """The distance a key stands for (float64 tensor or array in, the same out)."""
  k = torch.as_tensor(keys, dtype=torch.float64)
  return torch.sqrt(k) if metric == 'sqeuclidean' else torch.acosh(1.0 + 2.0 * k)


def distances64(x, metric):
  return distance_of(keys64(x, metric), metric)


def keys32(x, metric):
  """The kernel's fp32 keys of an EXACT input as a float32 ndarray [n, n] (module docstring): D exact, one fp32 division."""
  D = K.dist64(x).numpy().astype(np.float32)
  if metric == 'sqeuclidean':
    return D
  s = sq_norms64(x).numpy().astype(np.float32)
  a = np.maximum(np.float32(1.0) - s, np.float32(U))
  return (D / (a[:, None] * a[None, :])).astype(np.float32)


def rank_lo(n, q):
  """floor((n^2 - 1) q) in double, as numpy forms the lower neighbour of its virtual index."""
  last = n * n - 1
  return min(int(math.floor(float(last) * float(q))), last)


def quantile_key(keys, q):
  """The key of rank lo among all n^2 keys (ndarray or tensor [n, n])."""
  flat = np.sort(np.asarray(keys).reshape(-1), kind='stable')
  n = int(round(math.sqrt(flat.size)))
  return flat[rank_lo(n, q)]


def radius_edges(keys, tau):
  """np.where(keys <= tau) as an int64 tensor [2, E]: sorted by (row, col)."""
  r, c = np.where(np.asarray(keys) <= tau)
  return torch.from_numpy(np.vstack((r, c)).astype(np.int64))


def numpy_quantile_edges(dist, q):
  """The reference's apply_dist_threshold (distances_kNN.py:21-32) on a dense distance matrix."""
  dist = np.asarray(dist)
  thresh = np.quantile(dist, q, axis=None)
  return torch.from_numpy(np.vstack(np.where(dist <= thresh)).astype(np.int64))


def knn_order(keys):
  """Indices of every row by (key, index)."""
  return torch.from_numpy(np.argsort(np.asarray(keys), axis=1, kind='stable').astype(np.int64))


def dyadic_input(n, d, seed):
  """Entries m / 16 with m in {-2 .. 2} (d = 162: {-1, 0, 1}): points well inside the unit ball, every fp32 step but the division
  exact."""
  top = 1 if d == 162 else 2
  return torch.randint(-top, top + 1, (n, d), generator=torch.Generator().manual_seed(seed)).float() / 16.0


@functools.lru_cache(maxsize=None)
def exact_case(metric, n, d, dup=0):
  """(input, fp32 keys [n, n] ndarray) of an exact case; dup: rows 100 .. 100 + dup are copies of row 7."""
  seed = 1000 * n + d
  x = K.integer_input(n, d, seed) if metric == 'sqeuclidean' else dyadic_input(n, d, seed)
  if dup:
    x = x.clone()
    x[100:100 + dup] = x[7]
  return x, keys32(x, metric)


# (n, d, q, k) of the real-valued Poincare cases; the Euclidean ones are knn_oracle.REAL_SHAPES with the same q
POINCARE_SHAPES = [(1000, 16, 0.01, 16), (777, 2, 0.02, 64), (257, 8, 0.05, 16)]
REAL_Q = (0.01, 0.02, 0.05)


def poincare_input(case):
  """z / |z| * U^(1/d) * 0.95 with z normal and U uniform: uniform in the ball of radius 0.95."""
  n, d, _, _ = POINCARE_SHAPES[case]
  g = torch.Generator().manual_seed(100 + case)
  z = torch.randn(n, d, generator=g, dtype=torch.float64)
  r = torch.rand(n, generator=g, dtype=torch.float64) ** (1.0 / d) * 0.95
  return (z / z.norm(dim=1, keepdim=True) * r[:, None]).float()


def real_input(metric, case):
  return K.real_input(case) if metric == 'sqeuclidean' else poincare_input(case)


def real_shape(metric, case):
  """(n, d, q, k)"""
  if metric == 'sqeuclidean':
    n, d, k = K.REAL_SHAPES[case]
    return n, d, REAL_Q[case], k
  return POINCARE_SHAPES[case]


def key_band(x, metric):
  """BR_ij of the module docstring ([n, n] float64); B_ij for the Euclidean key."""
  B = K.band(x)
  if metric == 'sqeuclidean':
    return B
  d = x.shape[1]
  s = sq_norms64(x)
  a = torch.clamp(1.0 - s, min=EPS64)
  e = ((d + 1) * U * s + U) / a
  return (B + (e[:, None] + e[None, :] + 4 * U) * K.dist64(x)) / (a[:, None] * a[None, :])


class RadiusBand(object):
  """Oracle of the quantile radius graph of one real-valued input: exact keys, exact tau, the bands BR and b*."""

  def __init__(self, x, metric, q):
    self.n, self.metric, self.q = x.shape[0], metric, q
    self.R = keys64(x, metric)
    self.BR = key_band(x, metric)
    self.tau = float(quantile_key(self.R.numpy(), q))
    M = float(self.BR.max())
    near = (self.R - self.tau).abs() <= 2 * M
    self.bstar = float(self.BR[near].max())
    self.must = self.R < self.tau - self.BR - self.bstar
    self.never = self.R > self.tau + self.BR + self.bstar
    self.E = int((self.R <= self.tau).sum())

  def undetermined(self):
    return int((~self.must & ~self.never).sum())

  def check(self, ei, tau_key=None):
    n = self.n
    ei = ei.detach().cpu()
    assert ei.dtype == torch.int64 and ei.dim() == 2 and ei.shape[0] == 2
    assert int(ei.min()) >= 0 and int(ei.max()) < n
    flat = ei[0] * n + ei[1]
    assert bool((flat[1:] > flat[:-1]).all()), 'edges are not strictly ascending by (row, col): unsorted or duplicated'
    got = torch.zeros(n, n, dtype=torch.bool)
    got[ei[0], ei[1]] = True
    assert torch.equal(got, got.T), 'the edge set is not symmetric'
    missed = self.must & ~got
    assert not bool(missed.any()), '%d pairs clearly under the threshold are absent' % int(missed.sum())
    extra = self.never & got
    assert not bool(extra.any()), '%d pairs clearly over the threshold are present' % int(extra.sum())
    if tau_key is not None:
      assert abs(float(tau_key) - self.tau) <= self.bstar, \
        'tau %.9g is off the exact %.9g by more than b* = %.3g' % (tau_key, self.tau, self.bstar)


@functools.lru_cache(maxsize=None)
def real_radius_band(metric, case):
  return RadiusBand(real_input(metric, case), metric, real_shape(metric, case)[2])


@functools.lru_cache(maxsize=None)
def real_knn_band(metric, case):
  """knn_oracle.Band (its inclusion rule, `check` and `undetermined`) on the keys of `metric` with the band BR."""
  x = real_input(metric, case)
  k = real_shape(metric, case)[3]
  band = object.__new__(K.Band)
  band.n, band.k = x.shape[0], k
  band.D = keys64(x, metric)
  band.B = key_band(x, metric)
  Ds, order = K.order_of(band.D)
  band.tau = Ds[:, k - 1]
  band.kth = order[:, k - 1]
  band.b = band.B.gather(1, band.kth[:, None])[:, 0]
  return band


def check_distances(dist, idx, band, metric):
  """Returned distances lie within the image of [R - BR, R + BR] under the key -> distance map, plus 16 u relative for the fp32
  sqrt / log1p; a row's own distance is exactly 0."""
  idx = idx.detach().cpu()
  dist = dist.detach().cpu().double()
  rows = torch.arange(band.n)[:, None]
  R, BR = band.D[rows, idx], band.B[rows, idx]
  lo = distance_of(torch.clamp(R - BR, min=0.0), metric) * (1 - 16 * U)
  hi = distance_of(R + BR, metric) * (1 + 16 * U)
  bad = (dist < lo) | (dist > hi)
  assert not bool(bad.any()), '%d returned distances lie outside the band' % int(bad.sum())
  assert bool((dist[:, 0] == 0).all()), 'a node is not at distance exactly 0 from itself'
