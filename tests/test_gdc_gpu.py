"""Graph diffusion rewiring on the device against the float64 oracle (gdc_oracle.py): values inside the derived bound
|S_native - S| <= gamma S + tail_ij, membership by the bound alone, exact cases entry for entry, determinism, column sums, block
widths, the dense mode and the reference-named wrappers.  Shapes: a second block of one column (n = 257), k in {1, 16, 128}, fewer
than k positive entries, a row of more than 512 entries, directed / weighted / duplicate edges, isolated nodes, empty columns."""

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
import gdc_oracle as O

pytestmark = pytest.mark.gpu


def native_kwargs(c):
  kw = {a: c[a] for a in ('k', 'eps', 'self_loop_weight', 'normalization_in', 'block') if a in c}
  kw[{'ppr': 'alpha', 'heat': 't', 'coeff': 'coeffs'}[c['method']]] = c['param']
  return dict(kw, method=c['method'])


_RESULTS = {}


def native(name, dev, normalization_out=None, **over):
  """(edge_index, weight) of a case as device tensors; the plain runs are computed once and shared."""
  key = (name, normalization_out, tuple(sorted(over.items())))
  if key not in _RESULTS:
    ei, w, n, c = O.case_inputs(name)
    kw = dict(native_kwargs(c), normalization_out=normalization_out, **over)
    _RESULTS[key] = ops.gdc(torch.from_numpy(ei).to(dev), None if w is None else torch.from_numpy(w).to(dev), n, **kw)
  return _RESULTS[key]


def to_numpy(res):
  return res[0].cpu().numpy(), res[1].cpu().numpy()


@pytest.mark.parametrize('name', sorted(O.CASES))
def test_values_and_membership_inside_the_derived_bound(name, dev):
  out_ei, out_w = native(name, dev)
  assert out_ei.dtype == torch.int64 and out_w.dtype == torch.float32 and out_ei.shape == (2, out_w.numel())
  O.case_band(name).check(*to_numpy((out_ei, out_w)))


def test_hub_case_has_a_long_row_and_few_positive_case_returns_fewer(dev):
  ei, _, n, _ = O.case_inputs('hub_heat')
  assert np.bincount(ei[0], minlength=n).max() > 512
  out_ei, _ = to_numpy(native('few_positive', dev))
  counts = np.bincount(out_ei[1], minlength=40)
  assert counts.max() <= 40 < 64 and (counts == (O.case_band('few_positive').S > 0).sum(0)).all()


@pytest.mark.parametrize('name', ['second_block', 'plain_k128', 'hub_heat', 'threshold', 'isolated', 'weighted_dups'])
def test_column_normalised_weights_sum_to_one(name, dev):
  """'col': the same entries in the same order as the unnormalised run, each value divided by its column's sum."""
  raw_ei, raw_w = to_numpy(native(name, dev))
  out_ei, out_w = to_numpy(native(name, dev, normalization_out='col'))
  assert np.array_equal(raw_ei, out_ei)
  assert np.isfinite(out_w).all() and (out_w > 0).all()
  n = O.case_inputs(name)[2]
  counts = np.bincount(out_ei[1], minlength=n)
  sums = np.bincount(out_ei[1], weights=out_w.astype(np.float64), minlength=n)
  kept = counts > 0
  # every weight is one division: k roundings of 2^-24 each in a sum close to 1
  assert (np.abs(sums[kept] - 1.0) <= counts[kept] * 2.0 ** -23).all(), float(np.abs(sums[kept] - 1.0).max())
  assert (sums[~kept] == 0).all()
  colsum = np.bincount(raw_ei[1], weights=raw_w.astype(np.float64), minlength=n)
  want = raw_w.astype(np.float64) / colsum[raw_ei[1]]
  depth = (counts.max() + 63) // 64 + 6 + 1          # the column sum's fixed-order tree and the division
  assert (np.abs(out_w - want) <= depth * 2.0 ** -24 * want).all()
  if name == 'threshold':
    assert 0 < int((~kept).sum()) < n


@pytest.mark.parametrize('name', ['plain_k16', 'hub_ppr', 'threshold', 'weighted_dups'])
def test_two_runs_are_bit_identical(name, dev):
  ei, w, n, c = O.case_inputs(name)
  run = lambda: ops.gdc(torch.from_numpy(ei).to(dev), None if w is None else torch.from_numpy(w).to(dev), n, **native_kwargs(c))
  a, b = run(), run()
  assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_block_widths_agree_within_the_value_bound(dev):
  """block = 64 and block = 256 on the same graph: both lie within the bound of the exact S, so entries both return differ by at
  most twice the bound; which entries are returned is checked per run by the membership rule."""
  band = O.case_band('plain_k16')
  dense = []
  for name in ('plain_k16', 'block64'):
    out_ei, out_w = to_numpy(native(name, dev))
    d = np.zeros((band.n, band.n))
    d[out_ei[0], out_ei[1]] = out_w
    dense.append(d)
  both = (dense[0] > 0) & (dense[1] > 0)
  assert both.sum() >= 0.98 * (dense[0] > 0).sum()
  assert (np.abs(dense[0] - dense[1])[both] <= 2.0 * (band.gamma * band.S + band.tail)[both]).all()


def path_graph(n):
  a = np.arange(n - 1)
  return np.stack([np.concatenate([a, a + 1]), np.concatenate([a + 1, a])])


def star_graph(leaves):
  a = np.arange(1, leaves + 1)
  z = np.zeros(leaves, dtype=np.int64)
  return np.stack([np.concatenate([z, a]), np.concatenate([a, z])])


DYADIC = (0.5, 0.25, 0.125, 0.125)
# (edges, n, arguments): every entry of T and of S is a dyadic fraction, exact in fp32 and float64 alike, with many exact ties
# (star_threshold: the leaf-to-leaf entries are exactly eps = 2^-9 and are kept); 'transition' is exact in its order only
EXACT = {
  'path': (path_graph(37), 37, dict(method='coeff', param=DYADIC, k=3, self_loop_weight=0.0, normalization_in='row')),
  'star': (star_graph(64), 65, dict(method='coeff', param=DYADIC, k=5, self_loop_weight=0.0, normalization_in='row')),
  'star_threshold': (star_graph(64), 65, dict(method='coeff', param=DYADIC, eps=2.0 ** -9, self_loop_weight=0.0, normalization_in='row')),
  'identity': (O.random_graph(70, 4, 21), 70, dict(method='coeff', param=(1.0,), k=4)),
  'transition': (O.random_graph(70, 4, 21, directed=True), 70, dict(method='coeff', param=(0.0, 1.0), k=128, normalization_in='row')),
}


@pytest.mark.parametrize('name', sorted(EXACT))
def test_exact_cases_match_the_oracle_entry_for_entry(name, dev):
  ei, n, c = EXACT[name]
  kw = {a: c[a] for a in ('k', 'eps', 'self_loop_weight', 'normalization_in') if a in c}
  want_ei, want_w = O.gdc_oracle(ei, None, n, c['method'], c['param'], normalization_out=None, **kw)
  got_ei, got_w = to_numpy(ops.gdc(torch.from_numpy(ei).to(dev), None, n, normalization_out=None, **native_kwargs(dict(c, block=64))))
  assert np.array_equal(got_ei, want_ei), 'edge set or order differs (ties go to the smaller row)'
  if name == 'transition':      # S = T = 1 / deg_i: one fp32 division; the ORDER is exact (equal degrees give equal values in both)
    assert (np.abs(got_w - want_w) <= 2.0 ** -24 * want_w).all()
  else:
    assert np.array_equal(got_w.astype(np.float64), want_w)
  if name == 'identity':
    assert got_ei.tolist() == [list(range(n)), list(range(n))] and (got_w == 1).all()
  if name in ('star', 'path'):
    assert (np.diff(got_w)[np.diff(got_ei[1]) == 0] == 0).any(), 'the case is meant to contain ties'


@pytest.mark.parametrize('kind', ['row', 'sym'])
def test_row_and_sym_output_normalisation(kind, dev):
  raw_ei, raw_w = to_numpy(native('second_block', dev))
  out_ei, out_w = to_numpy(native('second_block', dev, normalization_out=kind))
  assert np.array_equal(raw_ei, out_ei)
  d = np.zeros((257, 257))
  d[raw_ei[0], raw_ei[1]] = raw_w
  want = O.normalise(d, kind)[raw_ei[0], raw_ei[1]]
  assert np.isfinite(out_w).all() and (np.abs(out_w - want) <= 16 * 2.0 ** -24 * want).all()


def dense_bound(band, S_norm, n):
  """|d - D| for D_ij = S_ij / sum_i S_ij: the entry's own bound over the sum, plus D times the relative error of the sum (its
  entries' bounds and the depth of the fixed-order column sum) and of the division."""
  colsum = band.S.sum(0)
  entry = (band.gamma * band.S + band.tail) / colsum[None, :]
  rel_sum = ((band.gamma * band.S + band.tail).sum(0) / colsum)[None, :] + ((n + 63) // 64 + 6 + 1) * O.U
  return entry + S_norm * rel_sum * 1.01


@pytest.mark.parametrize('orientation', ['row', 'col'])
def test_dense_position_encoding(orientation, dev):
  ei, w, n, c = O.case_inputs('plain_k16')
  data = type('D', (), {})()
  data.num_nodes, data.edge_index, data.edge_attr = n, torch.from_numpy(ei).to(dev), None
  opt = dict(gdc_method='ppr', ppr_alpha=c['param'], gdc_sparsification='topk', gdc_k=16, gdc_threshold=0.01, self_loop_weight=1, exact=True,
             pos_enc_orientation=orientation)
  enc = G.graph_rewiring.apply_gdc(data, opt, type='pos_encoding')
  assert enc.shape == (n, n) and enc.dtype == torch.float32 and bool(torch.isfinite(enc).all())
  got = enc.cpu().numpy().astype(np.float64)
  want = O.dense_oracle(ei, w, n, 'ppr', c['param'])
  bound = dense_bound(O.case_band('plain_k16'), want, n)
  if orientation == 'col':
    want, bound = want.T, bound.T
  assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) - bound).max())
  assert not np.allclose(got, got.T, rtol=1e-3, atol=0), 'S must not be symmetric here: the orientations would be indistinguishable'


def test_apply_gdc_combined_is_the_native_result_in_row_col_order(dev):
  ei, w, n, c = O.case_inputs('directed')
  data = type('D', (), {})()
  data.num_nodes, data.edge_index, data.edge_attr = [n], torch.from_numpy(ei).to(dev), None
  opt = dict(gdc_method='ppr', ppr_alpha=c['param'], gdc_sparsification='topk', gdc_k=c['k'], gdc_threshold=0.01, self_loop_weight=1, exact=True)
  out = G.graph_rewiring.apply_gdc(data, opt)
  want_ei, want_w = native('directed', dev, normalization_out='col')
  order = torch.sort(want_ei[0] * n + want_ei[1]).indices
  assert out is data and data.num_nodes == n
  assert torch.equal(data.edge_index, want_ei[:, order]) and torch.equal(data.edge_attr, want_w[order])
  key = data.edge_index[0] * n + data.edge_index[1]
  assert bool((key[1:] > key[:-1]).all())


def test_out_of_range_arguments_raise(dev):
  ei = torch.tensor([[0, 1], [1, 0]], device=dev)
  for kw in (dict(k=0), dict(k=129), dict(k=4, block=6), dict(eps=-0.5), dict(k=4, tol=2.0)):
    with pytest.raises((ValueError, G.GnpdeError)):
      ops.gdc(ei, None, 2, method='ppr', alpha=0.15, **kw)
  with pytest.raises(ValueError, match='more than'):
    ops.gdc(ei, None, 2, method='ppr', alpha=1e-4, k=2, tol=1e-9)           # M would exceed 4096
  with pytest.raises(G.GnpdeError, match='cap'):
    ops.gdc(ei, None, 2, method='ppr', alpha=0.15, dense_out=True, dense_cap_bytes=8)
  for w in ([1.0, -0.5], [1.0, float('nan')], [float('inf'), 1.0]):          # the bound and the key order need non-negative terms
    with pytest.raises(ValueError, match='non-negative'):
      ops.gdc(ei, torch.tensor(w, device=dev), 2, method='ppr', alpha=0.15, k=2)
  with pytest.raises(ValueError, match='self_loop_weight'):
    ops.gdc(ei, None, 2, method='ppr', alpha=0.15, k=2, self_loop_weight=-1.0)
  with pytest.raises(ValueError, match='outside'):
    ops.gdc(torch.tensor([[0, 5], [1, 0]], device=dev), None, 2, method='ppr', alpha=0.15, k=2)
