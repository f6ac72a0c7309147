"""ops.knn / gnpde_knn on the device against the brute-force float64 oracle of knn_oracle.py: exact (integer) inputs across
every tile edge, with and without the column split, real-valued inputs under the derived rounding band, argument errors,
run-to-run identity."""
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib
import knn_oracle as O

pytestmark = pytest.mark.gpu

NS = (1, 2, 63, 65, 257, 1000)                 # below / across the 64-row and 64-column tiles, several workgroups
DS = (1, 3, 4, 22, 162)                        # K chunks of 16: partial, one, several; 162 lives on 164-float rows
KS = (1, 2, 16, 63, 64, 65, 128)               # both row-buffer sizes (k <= 32, k > 32) and the 64-column step; plus k = n
EXACT = [(n, d) for n in NS for d in DS]


def ks_of(n):
  return sorted({k for k in KS + (n,) if k <= min(n, 128)})


def on_device(x, d, dev):
  """The input as the model holds it: d = 162 on 164-float rows whose padding must not be read."""
  if d == 162:
    full = torch.full((x.shape[0], 164), 777.0, device=dev)
    full[:, :d] = x.to(dev)
    return full[:, :d]
  return x.to(dev)


def check_exact(x, Ds, order, xd, ks):
  for k in ks:
    idx, dist = G.ops.knn(xd, k, return_dist=True)
    assert idx.shape == (x.shape[0], k) and idx.dtype == torch.int64 and dist.dtype == torch.float32
    assert torch.equal(idx.cpu(), order[:, :k]), 'k = %d: indices differ from the (distance, index) order' % k
    assert torch.equal(dist.cpu().double(), Ds[:, :k]), 'k = %d: distances are not the integers' % k
    assert torch.equal(G.ops.knn(xd, k), idx)


@pytest.mark.parametrize('n,d', EXACT)
def test_exact_cases(dev, n, d):
  """Integers in [-8, 8]: every product and sum is exact in fp32, so indices (tie rule included) and distances must equal
  the oracle's.  n = 1000 with d = 1 or 3 leaves most rows tied at the k-th place."""
  x, Ds, order = O.integer_order(n, d, 1000 * n + d)
  check_exact(x, Ds, order, on_device(x, d, dev), ks_of(n))


def test_exact_duplicated_rows(dev):
  """40 copies of one row: many distances tie at 0 (the copies come in index order, a copy's own index not first unless it
  is the smallest) and at equal positive values."""
  x, Ds, order = O.integer_order(257, 4, 5, dup=40)
  assert int((Ds[7, :41] == 0).sum()) == 41
  check_exact(x, Ds, order, x.to(dev), (1, 16, 41, 64, 128))


def test_exact_ties_at_the_kth_place(dev):
  x, Ds, order = O.integer_order(1000, 3, 1000 * 1000 + 3)
  k = 16
  assert float((Ds[:, k - 1] == Ds[:, k]).double().mean()) > 0.5, 'the case was meant to tie at the k-th place'
  check_exact(x, Ds, order, x.to(dev), (k,))


@pytest.fixture
def splits():
  def force(s):
    G.ops.tune(_lib.TUNE_KNN_SPLITS, s)
  yield force
  G.ops.tune(_lib.TUNE_KNN_SPLITS, 0)


@pytest.mark.parametrize('n,d', EXACT + [(5000, 16)])
def test_exact_cases_with_the_column_split_forced(dev, splits, n, d):
  """S = 1 (no merge pass) and S = 3 (partial lists + merge kernel; at n = 5000 a row tile has several column workgroups of
  several tiles each): identical to each other and to the oracle."""
  x, Ds, order = O.integer_order(n, d, 1000 * n + d)
  xd = on_device(x, d, dev)
  ks = (32,) if n == 5000 else ks_of(n)
  got = {}
  for s in (1, 3):
    splits(s)
    check_exact(x, Ds, order, xd, ks)
    got[s] = [G.ops.knn(xd, k, return_dist=True) for k in ks]
  for (i1, d1), (i3, d3) in zip(got[1], got[3]):
    assert torch.equal(i1, i3) and torch.equal(d1, d3)


@pytest.mark.parametrize('case', range(len(O.REAL_SHAPES)))
@pytest.mark.parametrize('s', [0, 1, 3])
def test_real_valued_cases(dev, splits, case, s):
  """Standard normal inputs: inclusion under the derived band B_ij = (d + 4) 2^-24 (|x_i| + |x_j|)^2 (knn_oracle.py), after
  the oracle alone has shown that the band leaves at most 1 % of the n k entries undetermined."""
  n, d, k = O.REAL_SHAPES[case]
  band = O.real_band(case)
  open_ = band.undetermined()
  print('case %s: %d of %d entries undetermined' % ((n, d, k), open_, n * k))
  assert open_ <= O.CAP_SHARE * n * k
  splits(s)
  idx, dist = G.ops.knn(on_device(O.real_input(case), d, dev), k, return_dist=True)
  band.check(idx, dist)


def test_errors(dev):
  x = torch.zeros(200, 8, device=dev)
  for k in (0, -1, 201, 129):
    with pytest.raises(G.GnpdeError):
      G.ops.knn(x, k)
  with pytest.raises(G.GnpdeError):
    G.ops.knn(torch.zeros(100, 8, device=dev), 101)
  with pytest.raises(G.GnpdeError):
    G.ops.knn(x.cpu(), 4)
  with pytest.raises(G.GnpdeError):
    G.ops.knn(x.double(), 4)
  with pytest.raises(G.GnpdeError):
    G.ops.knn(torch.zeros(200, device=dev), 4)
  torch.cuda.synchronize()


def test_determinism(dev):
  x = torch.randn(3000, 48, generator=torch.Generator().manual_seed(11)).to(dev)
  a = G.ops.knn(x, 40, return_dist=True)
  b = G.ops.knn(x, 40, return_dist=True)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
  assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_strided_rows_and_column_slices(dev):
  """Padded rows are read in place; a column slice with a foreign row stride gives what its contiguous copy gives."""
  big = torch.randn(300, 40, generator=torch.Generator().manual_seed(3)).to(dev)
  view = big[:, 3:25]
  assert torch.equal(G.ops.knn(view, 9), G.ops.knn(view.contiguous(), 9))
