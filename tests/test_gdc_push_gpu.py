"""Approximate forward push on the device against the float64 yardstick (gdc_push_oracle.py; its docstring derives the slack):
the three relations 0 <= Pi - p < eps deg, mass 1, r < alpha eps deg with gamma = u / (1 - u) and the fixed-point quantum, bitwise
determinism over runs, batches and stores, the forced slow path, the wrapper's pipeline against the same pipeline in numpy,
threshold by avg_degree on the push and on the exact path, and the surface.  Shapes: the five of gdc_push_oracle.SHAPES, none
larger (n <= 600; the hub row has 531 entries, more than the 16 lanes of a row group and more than one round of a wave)."""
import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
import gdc_oracle as E
import gdc_push_oracle as O

PIPELINE_SHAPE, PIPELINE_THRESHOLD = O.PIPELINE_SHAPE, O.PIPELINE_THRESHOLD

pytestmark = pytest.mark.gpu

_RUNS = {}


def native(name, dev, normalization_in='row', **kw):
  """(edge_index, values, info) of ops.gdc_push on a shape, computed once per argument set and shared."""
  key = (name, normalization_in, tuple(sorted(kw.items())))
  if key not in _RUNS:
    c = O.SHAPES[name]
    ei = torch.from_numpy(O.shape(name)[0]).to(dev)
    _RUNS[key] = ops.gdc_push(ei, c['n'], c['alpha'], c['eps'], normalization_in=normalization_in, return_info=True, **kw)
  return _RUNS[key]


def dense(ei, w, n):
  out = np.zeros((n, n))
  out[ei[0].cpu().numpy(), ei[1].cpu().numpy()] = w.cpu().numpy().astype(np.float64)
  return out


def col_slack(m):
  """A column of m kept values: its fixed-order fp32 sum (at most m - 1 roundings), the division, and the float64 check's own
  sum of the rounded quotients: (m + 1) roundings, relative because every term is positive."""
  return (m + 1) * O.U / (1.0 - (m + 1) * O.U)


def same_bits(a, b):
  return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize('name', ['local300', 'hub600'])
def test_bound_mass_and_residuals(name, dev):
  """-gamma p <= Pi - p < eps deg + gamma Pi + LOST / alpha, |mass - 1| <= gamma + (LOST + q) / alpha, r < alpha eps deg (1 + gamma):
  N = 1 rounding (the conversion of a fixed-point value to fp32), quantum 2^-60 (gdc_push_oracle's docstring)."""
  c = O.SHAPES[name]
  _, _, deg, Pi = O.shape(name)
  ei, w, info = native(name, dev, return_residuals=True)
  assert ei.dtype == torch.int64 and w.dtype == torch.float32 and ei.shape == (2, w.numel()) and bool((w > 0).all())
  key = ei[0] * c['n'] + ei[1]
  assert bool((key[1:] > key[:-1]).all()), 'not sorted by (s, u), or an entry twice'
  R = info['residuals'].cpu().numpy()
  assert R.shape == (c['n'], c['n'])
  O.check_relations(dense(ei, w, c['n']), R, Pi, deg, c['alpha'], c['eps'], gamma=O.GAMMA,
                    lost=O.lost_mass(c['alpha'], c['eps'], deg.max()), label=name + ' native')
  assert info['slow_sources'] == 0


def test_local_shape_stays_local(dev):
  ei, _, _ = native('local300', dev)
  assert 30 * 300 < ei.shape[1] < 100 * 300


@pytest.mark.parametrize('name', ['local300', 'hub600'])
def test_bitwise_determinism_over_runs_and_batches(name, dev):
  c = O.SHAPES[name]
  base = native(name, dev)
  ei = torch.from_numpy(O.shape(name)[0]).to(dev)
  again = ops.gdc_push(ei, c['n'], c['alpha'], c['eps'], normalization_in='row')
  assert same_bits(base, again), 'two runs differ'
  for kw in (dict(batch=37), dict(batch=256, slow_groups=3)):
    assert same_bits(base, native(name, dev, **kw)), 'the result depends on %r' % (kw,)


def test_slow_path_is_bit_identical_and_counted(dev):
  """capacity = 0 sends every source of the hub shape through the global-memory store: the fixed-point design gives the same bits
  (values AND residuals) as the LDS hash."""
  n = O.SHAPES['hub600']['n']
  fast = native('hub600', dev, return_residuals=True)
  slow = native('hub600', dev, return_residuals=True, capacity=0, slow_groups=5)
  assert slow[2]['slow_sources'] == n and fast[2]['slow_sources'] == 0
  assert same_bits(fast, slow)
  assert torch.equal(fast[2]['residuals'].view(torch.int32), slow[2]['residuals'].view(torch.int32))


def test_sources_split_between_the_stores_by_their_support(dev):
  """capacity = 149 distinct nodes (the median support of the local shape): exactly the sources that touch more nodes take the
  slow path, and the result keeps its bits."""
  n = O.SHAPES['local300']['n']
  fast = native('local300', dev, return_residuals=True)
  mixed = native('local300', dev, capacity=149, batch=100)
  touched = (dense(fast[0], fast[1], n) > 0) | (fast[2]['residuals'].cpu().numpy() > 0)
  print('touched nodes per source %d .. %d, %d sources on the slow path' % (touched.sum(1).min(), touched.sum(1).max(), mixed[2]['slow_sources']))
  assert 0 < mixed[2]['slow_sources'] < n and mixed[2]['slow_sources'] == int((touched.sum(1) > 149).sum())
  assert same_bits(fast, mixed)


class _Data(object):
  def __init__(self, n, ei, w=None):
    self.num_nodes, self.edge_index, self.edge_attr = n, ei, w


def test_wrapper_pipeline_against_numpy(dev):
  """GDCWrapper(approx='push', exact=False): 'sym' in, threshold, 'col' out against the same steps in numpy on the float64 push.
  Entries farther from the threshold than the bound agree in membership; at most 2 % of the oracle's kept entries are open."""
  c = O.SHAPES[PIPELINE_SHAPE]
  n = c['n']
  band = O.pipeline_band(PIPELINE_SHAPE, PIPELINE_THRESHOLD)
  assert band['share'] <= O.OPEN_CAP
  W = G.graph_rewiring.GDCWrapper(1, 'sym', 'col', dict(method='ppr', alpha=c['alpha'], eps=c['eps']),
                                  dict(method='threshold', eps=PIPELINE_THRESHOLD), exact=False, approx='push')
  data = W(_Data(n, torch.from_numpy(O.shape(PIPELINE_SHAPE)[0]).to(dev)))
  ei, w = data.edge_index, data.edge_attr
  assert ei.dtype == torch.int64 and w.dtype == torch.float32 and ei.shape == (2, w.numel())
  key = ei[0] * n + ei[1]
  assert bool((key[1:] > key[:-1]).all()), 'not in (row, col) order'
  got = dense(ei, torch.ones_like(w), n) > 0
  print('%d native entries, %d in the oracle, %d open' % (int(got.sum()), int(band['kept'].sum()), int(band['open'].sum())))
  assert not (got & band['outside']).any(), '%d returned entries are clearly outside' % int((got & band['outside']).sum())
  assert not (band['inside'] & ~got).any(), '%d entries clearly inside are missing' % int((band['inside'] & ~got).sum())
  out = dense(ei, w, n)
  slack = col_slack(int(got.sum(0).max()))
  sums = out.sum(0)
  assert np.abs(sums[got.any(0)] - 1.0).max() <= slack and (sums[~got.any(0)] == 0).all()
  # where the two kept sets agree in a column, the normalised values agree to the width of the bound over the column's sum
  agree = (got == band['kept']).all(0) & got.any(0)
  colsum = np.where(band['kept'], band['S'], 0.0).sum(0)
  wsum = np.where(band['kept'], band['width'], 0.0).sum(0)
  agree &= wsum < 0.5 * colsum
  # |a / A - b / B| <= |a - b| / A + (b / B) |A - B| / A <= 2 sum(width) / (B - sum(width)), plus the native column's own rounding
  err = np.abs(out - band['out'])[:, agree]
  lim = (2.0 * wsum / np.maximum(colsum - wsum, 1e-300) + 2.0 * slack)[None, agree]
  print('%d columns with equal kept sets, worst error / limit %.3f' % (int(agree.sum()), float((err / lim).max())))
  assert int(agree.sum()) > n // 2 and (err <= lim).all()


def test_position_encoding_is_the_dense_form_of_the_list(dev):
  c = O.SHAPES['local300']
  n = c['n']
  ei = torch.from_numpy(O.shape('local300')[0]).to(dev)
  W = G.graph_rewiring.GDCWrapper(1, 'sym', 'col', dict(method='ppr', alpha=c['alpha'], eps=c['eps']),
                                  dict(method='threshold', eps=0.01), exact=False, approx='push')
  enc = W.position_encoding(_Data(n, ei))
  sei, sw, _ = native('local300', dev, normalization_in='sym')
  assert enc.shape == (n, n) and int((enc > 0).sum()) == sw.numel()
  assert np.abs(enc.sum(0).double().cpu().numpy() - 1.0).max() <= col_slack(int((enc > 0).sum(0).max()))     # the diagonal is always kept
  raw = torch.zeros(n, n, device=dev)
  raw[sei[0], sei[1]] = sw
  assert torch.equal(enc > 0, raw > 0)


AVG_DEGREE = 8


def test_avg_degree_on_the_push_path(dev):
  """The threshold is the fp32 mean of the K-th and (K + 1)-th largest NATIVE values (bitwise), the kept set is exactly the
  values >= it (so the edge count is K plus the ties at the cut), and it matches the midpoint of the float64 pipeline's own values
  to the bound (order statistics are 1-Lipschitz in the entrywise bound)."""
  c = O.SHAPES['local300']
  n, K = c['n'], AVG_DEGREE * c['n']
  sei, sw, _ = native('local300', dev, normalization_in='sym')
  assert sw.numel() > K + 1
  ei, w, eps = ops.gdc_sparse_threshold(sei, sw, n, avg_degree=AVG_DEGREE, normalization_out=None, return_eps=True)
  top = torch.sort(sw, descending=True).values
  assert eps == float((top[K - 1] + top[K]) * 0.5)
  keep = sw >= eps
  assert torch.equal(ei, sei[:, keep]) and torch.equal(w, sw[keep])
  ties = int((sw == top[K - 1]).sum()) + int((sw == top[K]).sum())
  assert 0 <= ei.shape[1] - K <= ties
  # every native value lies within its own entry's width of the float64 pipeline's value, so the K-th largest native value lies
  # between the K-th largest of (S - width) and of (S + width); the fp32 midpoint adds one rounding
  band = O.pipeline_band('local300', 0.01)
  lo, hi = np.sort((band['S'] - band['width']).ravel())[::-1], np.sort((band['S'] + band['width']).ravel())[::-1]
  lo_mid, hi_mid = 0.5 * (lo[K - 1] + lo[K]), 0.5 * (hi[K - 1] + hi[K])
  print('eps native %.6e in [%.6e, %.6e]' % (eps, lo_mid, hi_mid))
  assert lo_mid - O.GAMMA * abs(lo_mid) <= eps <= hi_mid * (1.0 + O.GAMMA)
  # the wrapper: same entries, 'col' normalised, (row, col) order; fewer entries than avg_degree n keeps them all
  W = G.graph_rewiring.GDCWrapper(1, 'sym', 'col', dict(method='ppr', alpha=c['alpha'], eps=c['eps']),
                                  dict(method='threshold', avg_degree=AVG_DEGREE), exact=False, approx='push')
  data = W(_Data(n, torch.from_numpy(O.shape('local300')[0]).to(dev)))
  assert torch.equal(data.edge_index, ei)
  cols = data.edge_index[1].cpu().numpy()
  sums = np.bincount(cols, weights=data.edge_attr.double().cpu().numpy(), minlength=n)
  assert np.abs(sums[np.unique(cols)] - 1.0).max() <= col_slack(int(np.bincount(cols).max()))
  all_ei, all_w, none = ops.gdc_sparse_threshold(sei, sw, n, avg_degree=n, normalization_out=None, return_eps=True)
  assert none is None and torch.equal(all_ei, sei) and torch.equal(all_w, sw)


def test_avg_degree_on_the_exact_path(dev):
  """ops.gdc(avg_degree=) equals ops.gdc(eps=) at the threshold it reports; that threshold lies between the midpoints of the
  K-th / (K + 1)-th largest lower and upper bounds of the exact entries (gdc_oracle.Band), and the count is K up to the ties."""
  c = O.SHAPES['local300']
  n, K = c['n'], AVG_DEGREE * c['n']
  ei_np = O.shape('local300')[0]
  ei = torch.from_numpy(ei_np).to(dev)
  kw = dict(method='ppr', alpha=c['alpha'], normalization_out=None, block=64)
  out_ei, out_w, eps = ops.gdc(ei, None, n, avg_degree=AVG_DEGREE, return_eps=True, **kw)
  ref_ei, ref_w = ops.gdc(ei, None, n, eps=eps, **kw)
  assert torch.equal(out_ei, ref_ei) and torch.equal(out_w, ref_w)
  band = E.Band(ei_np, None, n, 'ppr', c['alpha'], eps=1.0)
  lo, hi = np.sort(band.lo.ravel())[::-1], np.sort(band.hi.ravel())[::-1]
  lo_mid, hi_mid = 0.5 * (lo[K - 1] + lo[K]), 0.5 * (hi[K - 1] + hi[K])
  print('eps native %.6e in [%.6e, %.6e], %d entries for K = %d' % (eps, lo_mid, hi_mid, out_w.numel(), K))
  assert lo_mid - O.GAMMA * abs(lo_mid) <= eps <= hi_mid * (1.0 + O.GAMMA)
  ties = int(((band.lo <= eps) & (band.hi >= eps)).sum())        # kept beyond the first K: values equal to eps
  assert 0 <= out_w.numel() - K <= ties and bool((out_w >= eps).all())
  data = G.graph_rewiring.GDCWrapper(1, 'sym', 'col', dict(method='ppr', alpha=c['alpha']), dict(method='threshold', avg_degree=AVG_DEGREE),
                                     block=64)(_Data(n, ei))
  assert data.edge_index.shape[1] == out_w.numel()


OPT = dict(gdc_method='ppr', ppr_alpha=0.15, heat_time=3.0, gdc_sparsification='threshold', gdc_k=16, gdc_threshold=1e-3, self_loop_weight=1,
           exact=False, pos_enc_orientation='row')


def test_apply_gdc_takes_the_push_only_with_the_option(dev, monkeypatch):
  n = O.SHAPES['local300']['n']
  ei = torch.from_numpy(O.shape('local300')[0]).to(dev)
  pushed = []
  real = ops.gdc_push
  monkeypatch.setattr(ops, 'gdc_push', lambda *a, **kw: pushed.append(1) or real(*a, **kw))
  apply_gdc = G.graph_rewiring.apply_gdc
  # option absent (and exact = False): bitwise the exact path, as before -- ops.gdc and the (row, col) sort
  plain = apply_gdc(_Data(n, ei), dict(OPT))
  assert not pushed
  ref_ei, ref_w = ops.gdc(ei, None, n, method='ppr', alpha=0.15, eps=1e-3, self_loop_weight=1.0, normalization_in='sym',
                          normalization_out='col', tol=1e-6, block=256)
  order = torch.sort(ref_ei[0] * n + ref_ei[1]).indices
  assert torch.equal(plain.edge_index, ref_ei[:, order]) and torch.equal(plain.edge_attr.view(torch.int32), ref_w[order].view(torch.int32))
  apply_gdc(_Data(n, ei), dict(OPT, gnpde_gdc_approx='push', exact=True))
  assert not pushed
  data = apply_gdc(_Data(n, ei), dict(OPT, gnpde_gdc_approx='push'))
  assert pushed == [1]
  sei, sw, _ = native('local300', dev, normalization_in='sym')           # the shape's eps is the option's 1e-3
  keep = sw >= 1e-3
  assert torch.equal(data.edge_index, sei[:, keep])
  for bad, text in ((dict(gdc_sparsification='topk'), 'no top-k'), (dict(gdc_method='heat'), 'ppr only'), (dict(self_loop_weight=0.5), 'self_loop_weight')):
    with pytest.raises(NotImplementedError, match=text):
      apply_gdc(_Data(n, ei), dict(OPT, gnpde_gdc_approx='push', **bad))
  with pytest.raises(NotImplementedError, match='weighted'):
    apply_gdc(_Data(n, ei, torch.ones(ei.shape[1], device=dev)), dict(OPT, gnpde_gdc_approx='push'))
