"""Native NMF (csrc/nmf.hip, ops.nmf, pos_enc_factorisation.NMF) on the device against the CPU oracle (nmf_oracle.py) and the
sklearn-recorded fixtures (tests/golden/nmf_fit_*.npz, tools/record_nmf_fixtures.py): one half-sweep within 8 x the float32 oracle's
own distance from the float64 oracle, bit identity, whole fits, invariants, the apply_beltrami opt-in.

With GNPDE_NMF_PARITY_OUT=<path> the sweep test writes its yardstick and the native deviations there (profiles/nmf_parity.txt)."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
from gnpde_amd import pos_enc_factorisation as PF
import nmf_oracle as O

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
BOUND = 8                  # times the float32 oracle's own deviation
PARITY = []                # (n, k, kind, dW, dv) of the sweep cases, for the parity file


def _padded(a, dev, extra, fill):
  """The float32 matrix `a` on the device as a column slice of a wider buffer filled with `fill`."""
  buf = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.float32, device=dev)
  view = buf[:, 3:3 + a.shape[1]] if extra > 3 else buf[:, :a.shape[1]]
  view.copy_(torch.from_numpy(a))
  return buf, view


# ---- 1. one half-sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', O.SWEEP_K)
@pytest.mark.parametrize('n', O.SWEEP_N)
def test_half_sweep_against_the_float64_oracle(dev, n, k):
  cases, delta_w, delta_v = O.sweep_family()
  for kind in ('mixed', 'clip'):
    W, Gm, P, W64, v64 = cases[(n, k, kind)]
    wbuf, w = _padded(W, dev, 5, 7.0)             # W and P as column slices of wider buffers: padded row strides, odd offsets
    pbuf, p = _padded(P, dev, 2, -3.0)
    v = ops.nmf_cd_sweep(w, torch.from_numpy(Gm).to(dev), p)
    assert v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda
    got = w.cpu().numpy().astype(np.float64)
    d_w, d_v = float(np.abs(got - W64).max()), abs(float(v) - v64)
    PARITY.append((n, k, kind, d_w, d_v))
    print('n %3d k %3d %-5s dW %.3e (delta %.3e)  dv %.3e (delta %.3e)' % (n, k, kind, d_w, delta_w, d_v, delta_v))
    assert d_w <= BOUND * delta_w, (kind, d_w, delta_w)
    assert d_v <= BOUND * delta_v, (kind, d_v, delta_v)
    assert (got[W64 == 0] == 0).all(), kind                                     # exact zeros stay exact
    if k >= 2:
      assert np.array_equal(got[:, k // 2], W[:, k // 2].astype(np.float64))     # G[t, t] == 0: untouched
    if kind == 'clip':
      assert np.count_nonzero(np.delete(got, k // 2, axis=1) if k >= 2 else got) == 0
    # nothing outside the slices is written, P is not written
    assert bool((wbuf[:, :3] == 7.0).all()) and bool((wbuf[:, 3 + k:] == 7.0).all())
    assert bool((pbuf[:, k:] == -3.0).all()) and np.array_equal(p.cpu().numpy(), P)


def test_write_parity_file():
  """Not a check of the kernel: with GNPDE_NMF_PARITY_OUT set, the figures of the sweep test above go to that file."""
  path = os.environ.get('GNPDE_NMF_PARITY_OUT')
  if not path or not PARITY:
    return
  _, delta_w, delta_v = O.sweep_family()
  with open(path, 'w') as f:
    f.write('NMF half-sweep (gnpde_nmf_cd_sweep) against the float64 oracle, tests/test_nmf_gpu.py on an MI355X\n')
    f.write('yardstick: float32 oracle (fresh form) vs float64 oracle, largest over the family: delta_W %.3e  delta_v %.3e; bound %d x\n'
            % (delta_w, delta_v, BOUND))
    f.write('%4s %4s %-6s %12s %8s %12s %8s\n' % ('n', 'k', 'kind', 'max |dW|', '/delta', '|dv|', '/delta'))
    for n, k, kind, d_w, d_v in PARITY:
      f.write('%4d %4d %-6s %12.3e %8.2f %12.3e %8.2f\n' % (n, k, kind, d_w, d_w / delta_w, d_v, d_v / delta_v))
    f.write('largest: dW %.2f delta_W, dv %.2f delta_v\n' % (max(r[3] for r in PARITY) / delta_w, max(r[4] for r in PARITY) / delta_v))


# ---- 2. bit identity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (17, 128, 129))
def test_bit_identical_from_run_to_run_and_inside_a_larger_n(dev, k):
  W, Gm, P = O.sweep_case(130, k, 'mixed')
  g = torch.from_numpy(Gm).to(dev)
  runs = []
  for _ in range(2):
    w = torch.from_numpy(W).to(dev)
    runs.append((w, ops.nmf_cd_sweep(w, g, torch.from_numpy(P).to(dev))))
  assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
  # the same 130 rows as the rows 9000 .. 9129 of a larger problem (more than one pass of the persistent grid, several chunks of the
  # violation sum): the same bits
  big_n = 9500
  reps = (big_n + 129) // 130
  wb = torch.from_numpy(np.tile(W, (reps, 1))[:big_n].copy()).to(dev)
  pb = torch.from_numpy(np.tile(P, (reps, 1))[:big_n].copy()).to(dev)
  wb[9000:9130].copy_(torch.from_numpy(W))
  pb[9000:9130].copy_(torch.from_numpy(P))
  ops.nmf_cd_sweep(wb, g, pb)
  assert torch.equal(wb[9000:9130], runs[0][0])


# ---- 3. whole fits against sklearn's -----------------------------------------------------------------------------------------------
def _fixture_x(fx, dev):
  if 'X' in fx:
    return torch.from_numpy(fx['X']).to(dev)
  ei = torch.from_numpy(np.stack([fx['row'], fx['col']])).to(dev)
  return ei, torch.from_numpy(fx['value']).to(dev), tuple(int(s) for s in fx['shape'])


@pytest.mark.parametrize('name', ('sparse', 'dense', 'rect'))
def test_fit_against_the_sklearn_fixture(dev, name):
  fx = np.load(os.path.join(GOLDEN, 'nmf_fit_%s.npz' % name))
  model = PF.NMF(4, init='custom', max_iter=300, tol=float(fx['tol']))
  W = model.fit_transform(_fixture_x(fx, dev), W=torch.from_numpy(fx['W0']).to(dev), H=torch.from_numpy(fx['H0']).to(dev))
  d_w = float(np.abs(W.cpu().numpy().astype(np.float64) - fx['W']).max())
  d_h = float(np.abs(model.components_.cpu().numpy().astype(np.float64) - fx['H']).max())
  d_e = abs(model.reconstruction_err_ - float(fx['reconstruction_err']))
  print('%s: n_iter %d (fixture %d)  dW %.3e (oracle %.3e)  dH %.3e (oracle %.3e)  derr %.3e (oracle %.3e)'
        % (name, model.n_iter_, int(fx['n_iter']), d_w, float(fx['dev_W']), d_h, float(fx['dev_H']), d_e, float(fx['dev_err'])))
  assert model.n_iter_ == int(fx['n_iter']) >= 20
  assert W.shape == fx['W'].shape and model.components_.shape == fx['H'].shape
  assert d_w <= BOUND * float(fx['dev_W'])
  assert d_h <= BOUND * float(fx['dev_H'])
  assert d_e <= BOUND * float(fx['dev_err'])


# ---- 4. invariants ---------------------------------------------------------------------------------------------------------------
def test_invariants_and_sparse_route_equals_dense_route(dev):
  n, k = 300, 32
  rng = np.random.RandomState(11)
  dense = (rng.rand(n, n) * (rng.rand(n, n) < 0.05)).astype(np.float32)
  avg = np.sqrt(dense.mean() / k)
  W0, H0 = (avg * np.abs(rng.randn(n, k))).astype(np.float32), (avg * np.abs(rng.randn(k, n))).astype(np.float32)
  row, col = np.nonzero(dense)
  order = rng.permutation(row.size)                                             # the edge list in no particular order
  ei = torch.from_numpy(np.stack([row[order], col[order]])).to(dev)
  sparse = (ei, torch.from_numpy(dense[row[order], col[order]]).to(dev), (n, n))
  xd, w0, h0 = torch.from_numpy(dense).to(dev), torch.from_numpy(W0).to(dev), torch.from_numpy(H0).to(dev)
  _, delta_w, _ = O.sweep_family()
  W, H, last = w0, h0, None
  for it in range(1, 11):
    W, H, n_iter, err = ops.nmf(sparse, k, W=W, H=H, max_iter=1, tol=0.0)
    err = float(err)
    print('iteration %2d: reconstruction_err %.8f' % (it, err))
    assert n_iter == 1 and bool((W >= 0).all()) and bool((H >= 0).all()) and bool(torch.isfinite(W).all()) and bool(torch.isfinite(H).all())
    assert last is None or err <= last * (1 + 1e-6), (it, err, last)
    last = err
  assert torch.equal(w0, torch.from_numpy(W0).to(dev)) and torch.equal(h0, torch.from_numpy(H0).to(dev))       # the init is not written
  a = ops.nmf(sparse, k, W=w0, H=h0, max_iter=10, tol=0.0)
  d = ops.nmf(xd, k, W=w0, H=h0, max_iter=10, tol=0.0)
  assert a[2] == d[2] == 10 and torch.equal(a[0], W) and torch.equal(a[1], H) and float(a[3]) == last
  d_w, d_h = float((a[0] - d[0]).abs().max()), float((a[1] - d[1]).abs().max())
  print('sparse route vs dense route after 10 iterations: dW %.3e dH %.3e (bound %.3e), err %.8f / %.8f' % (d_w, d_h, BOUND * delta_w, float(a[3]), float(d[3])))
  assert d_w <= BOUND * delta_w and d_h <= BOUND * delta_w
  assert abs(float(a[3]) - float(d[3])) <= 1e-6 * last
  assert abs(last - O.reconstruction_err(dense, a[0].cpu().numpy(), a[1].cpu().numpy())) <= 1e-5 * last
  # the stop: tol in the middle of the step of the ratio sequence between the iterations 5 and 6 (float64 oracle); check_every = 4
  # only delays it to the next multiple of 4; the random init is the same for the same seed
  ratios = O.fit(dense, W0, H0, 8, 0.0)[3]
  tol = float(np.sqrt(ratios[4] * ratios[5]))
  assert ratios[5] * 1.02 <= tol <= min(ratios[:5]) / 1.02, ratios
  assert ops.nmf(sparse, k, W=w0, H=h0, max_iter=10, tol=tol)[2] == 6
  assert ops.nmf(sparse, k, W=w0, H=h0, max_iter=10, tol=tol, check_every=4)[2] == 8
  r1, r2 = ops.nmf(sparse, k, max_iter=2, tol=0.0, seed=5), ops.nmf(sparse, k, max_iter=2, tol=0.0, seed=5)
  assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and not torch.equal(r1[0], ops.nmf(sparse, k, max_iter=2, tol=0.0, seed=6)[0])


def test_refusals_on_the_device(dev):
  x = torch.rand(12, 12, device=dev)
  for bad, text in ((-1.0, 'X has a negative entry'), (float('nan'), 'X has a non-finite entry'), (float('inf'), 'non-finite')):
    y = x.clone()
    y[3, 4] = bad
    with pytest.raises(G.GnpdeError, match=text):
      ops.nmf(y, 3)
  w, h = torch.rand(12, 3, device=dev), torch.rand(3, 12, device=dev)
  h[1, 1] = -0.5
  with pytest.raises(G.GnpdeError, match='initial W or H has a negative entry'):
    ops.nmf(x, 3, W=w, H=h)
  ei = torch.tensor([[0, 1, 1], [2, 3, 3]], device=dev)
  with pytest.raises(G.GnpdeError, match='repeats 1'):
    ops.nmf((ei, torch.ones(3, device=dev), (12, 12)), 2)
  with pytest.raises(G.GnpdeError, match='must be square'):
    ops.nmf((ei[:, :2], torch.ones(2, device=dev), (12, 13)), 2)
  with pytest.raises(G.GnpdeError, match='outside \\[0, n\\)'):
    ops.nmf((torch.tensor([[0, 1], [2, 12]], device=dev), torch.ones(2, device=dev), (12, 12)), 2)
  with pytest.raises(G.GnpdeError, match='float32'):
    ops.nmf(x.double(), 2)
  with pytest.raises(G.GnpdeError, match='unit column stride'):
    ops.nmf_cd_sweep(torch.rand(3, 12, device=dev).t(), torch.eye(3, device=dev), torch.rand(12, 3, device=dev))
  buf = torch.rand(12, 8, device=dev)
  with pytest.raises(G.GnpdeError, match='W and P alias'):
    ops.nmf_cd_sweep(buf[:, :3], torch.eye(3, device=dev), buf[:, 4:7])


# ---- 5. apply_beltrami -----------------------------------------------------------------------------------------------------------
def test_apply_beltrami_compresses_caches_and_reloads(dev, tmp_path, monkeypatch, capsys):
  n = 200
  ei = G.synthetic.uniform_graph(n, 600, seed=1)
  opt = {'pos_enc_type': 'GDC', 'dataset': 'Synthetic', 'gdc_method': 'ppr', 'ppr_alpha': 0.05, 'gdc_sparsification': 'topk', 'gdc_k': 16,
         'gdc_threshold': 0.01, 'self_loop_weight': 1, 'exact': True, 'pos_enc_orientation': 'row', 'gnpde_pos_enc_nmf_dim': 16}

  def data():
    return types.SimpleNamespace(edge_index=ei.to(dev), edge_attr=None, num_nodes=n)

  fname = tmp_path / 'pos_encodings' / 'Synthetic_GDC.pkl'
  enc = G.graph_rewiring.apply_beltrami(data(), opt, data_dir=str(tmp_path))
  out = capsys.readouterr().out
  assert 'NMF input: the dense 200 x 200 GDC matrix' in out
  assert enc.shape == (n, 16) and enc.dtype == torch.float32 and not enc.is_cuda and bool(torch.isfinite(enc).all()) and bool((enc >= 0).all())
  assert float(enc.max()) > 0
  with open(fname, 'rb') as f:
    stored = pickle.load(f)
  assert isinstance(stored, torch.Tensor) and torch.equal(stored, enc)

  def no_fit(*a, **kw):
    raise AssertionError('a cached pickle must not be factorised again')
  with monkeypatch.context() as mp:
    mp.setattr(PF.NMF, 'fit_transform', no_fit)
    mp.setattr(ops, 'nmf', no_fit)
    assert torch.equal(G.graph_rewiring.apply_beltrami(data(), opt, data_dir=str(tmp_path)), enc)
  assert 'Found them! Loading cached version' in capsys.readouterr().out

  # without the option: the dense encoding, cached, with the message as before
  plain = {key: v for key, v in opt.items() if not key.startswith('gnpde_pos_enc_nmf')}
  other = tmp_path / 'plain'
  full = G.graph_rewiring.apply_beltrami(data(), plain, data_dir=str(other))
  out = capsys.readouterr().out
  assert 'Encodings not found! Calculating and caching them' in out and 'NMF' not in out
  assert full.shape == (n, n) and torch.equal(full, G.graph_rewiring.apply_gdc(data(), plain, type='pos_encoding'))
  capsys.readouterr()

  # the dense matrix over the cap: the sparse GDC graph is factorised, and that is announced; the data object keeps its edges
  for orientation in ('row', 'col'):
    where = tmp_path / ('sparse_' + orientation)
    d = data()
    with monkeypatch.context() as mp:
      mp.setattr(ops, 'GDC_DENSE_CAP', 4 * n * n - 1)
      got = G.graph_rewiring.apply_beltrami(d, dict(opt, pos_enc_orientation=orientation), data_dir=str(where))
    out = capsys.readouterr().out
    assert 'NMF input: the sparse GDC graph (the dense 200 x 200 matrix exceeds %d bytes)' % (4 * n * n - 1) in out
    assert got.shape == (n, 16) and not got.is_cuda and bool((got >= 0).all()) and float(got.max()) > 0
    assert torch.equal(d.edge_index, ei.to(dev)) and d.edge_attr is None
    assert os.path.exists(where / 'pos_encodings' / 'Synthetic_GDC.pkl')
    # it factorises the graph apply_gdc(type='combined') returns (transposed for 'col'): the same call by hand gives the same bits
    sp = G.graph_rewiring.apply_gdc(data(), opt, type='combined')
    e2 = sp.edge_index if orientation == 'row' else sp.edge_index.flip(0)
    want = PF.NMF(16, init='random', random_state=0, max_iter=100, tol=0.002).fit_transform((e2.contiguous(), sp.edge_attr, (n, n)))
    assert torch.equal(got, want.cpu())


def test_compress_pos_encodings_writes_w_over_the_pickle(dev, tmp_path):
  n = 200
  data = types.SimpleNamespace(edge_index=G.synthetic.uniform_graph(n, 600, seed=1).to(dev), edge_attr=None, num_nodes=n)
  opt = {'pos_enc_type': 'GDC', 'dataset': 'Synthetic', 'gdc_method': 'ppr', 'ppr_alpha': 0.05, 'gdc_sparsification': 'topk', 'gdc_k': 16,
         'gdc_threshold': 0.01, 'self_loop_weight': 1, 'exact': True, 'pos_enc_orientation': 'row', 'embedding_dim': 8, 'max_iter': 30, 'tol': 0.01}
  full = G.graph_rewiring.apply_gdc(data, opt, type='pos_encoding')
  W = PF.compress_pos_encodings(data, opt, data_dir=str(tmp_path))
  with open(tmp_path / 'pos_encodings' / 'Synthetic_GDC.pkl', 'rb') as f:
    stored = pickle.load(f)
  assert torch.equal(stored, W) and W.shape == (n, 8) and W.dtype == torch.float32 and not W.is_cuda and bool((W >= 0).all())
  want = PF.NMF(8, init='random', random_state=0, max_iter=30, tol=0.01).fit_transform(full)
  assert torch.equal(W, want.cpu())
  assert torch.equal(G.graph_rewiring.apply_beltrami(data, opt, data_dir=str(tmp_path)), W)      # the model now loads the width-8 encoding
  with pytest.raises(ValueError, match='is not GDC'):
    PF.compress_pos_encodings(data, dict(opt, pos_enc_type='DW64'), data_dir=str(tmp_path))
