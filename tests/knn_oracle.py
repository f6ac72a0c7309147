"""Brute-force yardstick of the k-nearest-neighbour search (shared by test_knn_*.py; there is no reference-recorded fixture:
the reference's KNN needs pykeops).  float64 D_ij = sum_c (x_ic - x_jc)^2 on the CPU in the direct form, then a STABLE sort
of every row, i.e. ascending by (distance, index): equal distances keep ascending column order.

Real-valued inputs: the kernel forms D in fp32 as |x_i|^2 + |x_j|^2 - 2 x_i.x_j.  With u = 2^-24, the two norms carry at most
d u |x|^2 each, the dot product d u |x_i| |x_j| (Cauchy-Schwarz on sum |a b|) and the two additions 2 u more, together under
    B_ij = (d + 4) * 2^-24 * (|x_i| + |x_j|)^2 .
An entry can therefore be on the wrong side of the k-th distance tau_i only inside the band |D_ij - tau_i| < B_ij + b_i
(b_i: the bound of the k-th pair itself); `undetermined` counts those entries on the oracle alone."""
import functools

import torch


def dist64(x):
  """[n, n] float64 squared distances, direct form, by row blocks."""
  X = x.detach().cpu().double()
  n, d = X.shape
  step = max(1, int(2e7) // max(1, n * d))
  return torch.cat([((X[a:a + step, None, :] - X[None, :, :]) ** 2).sum(-1) for a in range(0, n, step)], dim=0)


def order_of(D):
  """(sorted distances, indices) of every row by (distance, index)."""
  return torch.sort(D, dim=1, stable=True)


def knn_oracle(x, k):
  Ds, order = order_of(dist64(x))
  return order[:, :k], Ds[:, :k]


def band(x):
  """B_ij of the module docstring, [n, n] float64."""
  X = x.detach().cpu().double()
  nrm = X.norm(dim=1)
  return (X.shape[1] + 4) * 2.0 ** -24 * (nrm[:, None] + nrm[None, :]) ** 2


class Band(object):
  """Oracle of one real-valued input: distances, the k-th distance of every row and the rounding band around it."""

  def __init__(self, x, k):
    self.n, self.k = x.shape[0], k
    self.D = dist64(x)
    self.B = band(x)
    Ds, order = order_of(self.D)
    self.tau = Ds[:, k - 1]
    self.kth = order[:, k - 1]
    self.b = self.B.gather(1, self.kth[:, None])[:, 0]

  def undetermined(self):
    """Entries other than the k-th itself that the band leaves open."""
    open_ = (self.D - self.tau[:, None]).abs() < self.B + self.b[:, None]
    open_[torch.arange(self.n), self.kth] = False
    return int(open_.sum())

  def check(self, idx, dist=None, self_first=True):
    """The inclusion rule: every returned entry is allowed, every entry clearly under the k-th distance is returned, returned
    distances are within the band of the true ones, ascending, ties by ascending index."""
    n, k = self.n, self.k
    idx = idx.detach().cpu()
    assert idx.shape == (n, k) and idx.dtype == torch.int64
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    rows = torch.arange(n)[:, None]
    Dr, Br = self.D[rows, idx], self.B[rows, idx]
    bad = Dr > self.tau[:, None] + Br + self.b[:, None]
    assert not bool(bad.any()), '%d returned entries lie beyond the band' % int(bad.sum())
    must = self.D < self.tau[:, None] - self.B - self.b[:, None]
    got = torch.zeros(n, n, dtype=torch.bool)
    got[rows.expand(n, k), idx] = True
    assert int(got.sum()) == n * k, 'a row returns an index twice'
    missed = must & ~got
    assert not bool(missed.any()), '%d entries clearly under the k-th distance were not returned' % int(missed.sum())
    if self_first:
      assert torch.equal(idx[:, 0], torch.arange(n)), 'column 0 is not the node itself'
    if dist is not None:
      dist = dist.detach().cpu()
      assert dist.shape == (n, k) and dist.dtype == torch.float32
      err = (dist.double() - Dr).abs()
      assert bool((err <= Br).all()), 'returned distance off by %.3e (band %.3e)' % (float(err.max()), float(Br.max()))
      assert bool((dist[:, 1:] >= dist[:, :-1]).all()), 'distances decrease along a row'
      tie = dist[:, 1:] == dist[:, :-1]
      assert bool((idx[:, 1:] > idx[:, :-1])[tie].all()), 'equal distances are not in ascending index order'
      if self_first:
        assert bool((dist[:, 0] == 0).all()), 'a node is not at distance exactly 0 from itself'


REAL_SHAPES = [(1000, 32, 16), (777, 162, 64), (257, 22, 16)]     # (n, d, k), standard normal, seed = index
CAP_SHARE = 0.01                                                  # undetermined entries allowed, as a share of n k


def real_input(case):
  n, d, _ = REAL_SHAPES[case]
  return torch.randn(n, d, generator=torch.Generator().manual_seed(case))


@functools.lru_cache(maxsize=None)
def real_band(case):
  return Band(real_input(case), REAL_SHAPES[case][2])


def integer_input(n, d, seed, ld=None):
  """Integers in [-8, 8] as fp32 (every product and sum of either distance form is exact for d <= 162); with ld the rows
  are a view of an [n, ld] allocation whose padding holds a value that would wreck the result if it were read."""
  x = torch.randint(-8, 9, (n, d), generator=torch.Generator().manual_seed(seed)).float()
  if ld is None:
    return x
  full = torch.full((n, ld), 777.0)
  full[:, :d] = x
  return full[:, :d]


@functools.lru_cache(maxsize=None)
def integer_order(n, d, seed, dup=0):
  """(input, sorted float64 distances, order) of an exact case; dup: rows 100 .. 100+dup are copies of row 7."""
  x = integer_input(n, d, seed)
  if dup:
    x[100:100 + dup] = x[7]
  Ds, order = order_of(dist64(x))
  return x, Ds, order
