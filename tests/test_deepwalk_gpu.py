"""Native DeepWalk positional encodings on the device against the CPU oracle (deepwalk_oracle.py): walks, negative walks and the epoch
order for integer equality; the step and the trainer against the float64 oracle within 8 x (the fp32 oracle's own distance from it);
run-to-run bit identity; the use condition; the apply_beltrami opt-in; refusals."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
from gnpde_amd.deepwalk_embeddings import DeepWalk
import deepwalk_oracle as O

pytestmark = pytest.mark.gpu

SEED = 20260
WALK_R = (0, 1, 63, 65, 257, 70001)              # wave, workgroup and multi-block boundaries
WALK_L = (1, 3, 4, 5, 20, 80)                    # the word-to-block mapping crosses a Philox block at 4
FIRST_WALK = (0, 2 ** 32 - 3)                    # the block counter crosses its low word


@pytest.fixture(scope='module')
def graphs(dev):
  out = {}
  for name, (ei, n) in (('ring', O.ring()), ('odd', O.odd_graph()), ('star', O.star())):
    out[name] = (O.csr(ei, n), ops.walk_csr(torch.from_numpy(ei).to(dev), n), n)
  return out


def _starts(n, R, seed):
  s = np.random.default_rng(seed).integers(0, n, size=R)
  s[::2] = s[::2] % 9 % n                        # small ids often: the star's hub, the odd graph's sink and isolated node
  return s


@pytest.mark.parametrize('L', WALK_L)
def test_walks_equal_the_oracle(dev, graphs, L):
  for R in WALK_R:
    for fw in FIRST_WALK:
      W = O.walk_words(R, L, SEED, 16, 3, fw) if R else None
      for name, ((rowptr, col), wg, n) in graphs.items():
        starts = _starts(n, R, R + L)
        want = O.random_walks(rowptr, col, starts, L, SEED, 16, 3, fw, W=W)
        got = ops.random_walks(wg, n, torch.from_numpy(starts).to(dev), L, SEED, 16, 3, first_walk=fw)
        assert got.dtype == torch.int64 and got.shape == (R, L + 1)
        assert np.array_equal(got.cpu().numpy(), want), (name, R, L, fw)


def test_walks_from_an_edge_list_repeats_and_stays(dev, graphs):
  ei, n = O.odd_graph()
  rowptr, col = O.csr(ei, n)
  starts = np.arange(n)
  got = ops.random_walks(torch.from_numpy(ei).to(dev), n, torch.from_numpy(starts).to(dev), 6, 1, 16, 0, repeats=3).cpu().numpy()
  assert np.array_equal(got, O.random_walks(rowptr, col, np.tile(starts, 3), 6, 1, 16, 0))
  assert (got[got[:, 0] == 7] == 7).all() and (got[got[:, 0] == 5] == 5).all()      # the isolated node and the sink stay
  with pytest.raises(G.GnpdeError, match='start node'):
    ops.random_walks(graphs['ring'][1], 5, torch.tensor([0, 5], device=dev), 3, 0, 16, 0)


@pytest.mark.parametrize('n', (1, 2, 1000, 2 ** 31 - 1))
def test_negative_walks_equal_the_oracle(dev, n):
  for L in WALK_L:
    for R in WALK_R:
      for fw in FIRST_WALK:
        starts = np.random.default_rng(R + L).integers(0, n, size=R)
        want = O.negative_walks(n, starts, L, SEED, 17, 5, fw)
        got = ops.negative_walks(n, torch.from_numpy(starts).to(dev), L, SEED, 17, 5, first_walk=fw)
        assert got.shape == (R, L + 1) and np.array_equal(got.cpu().numpy(), want), (n, R, L, fw)


@pytest.mark.parametrize('n', (1, 2, 255, 257, 70001))
def test_permutation(dev, n):
  got = ops.random_permutation(n, SEED, 18, 2, device=dev)
  assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), O.random_permutation(n, SEED, 18, 2))
  assert np.array_equal(np.sort(got.cpu().numpy()), np.arange(n))
  assert torch.equal(got, ops.random_permutation(n, SEED, 18, 2, device=dev))
  if n > 2:
    for other in ((SEED + 1, 18, 2), (SEED, 19, 2), (SEED, 18, 3)):
      assert not torch.equal(got, ops.random_permutation(n, *other, device=dev)), other


# ---- the step --------------------------------------------------------------------------------------------------------------------
def _device_steps(name, dev, pad=0):
  c = O.CASES[name]
  w, batches = O.case_inputs(name)
  n, d = w.shape
  emb = torch.zeros(n, d + pad, device=dev)[:, :d]
  emb.copy_(w)
  m, v = torch.zeros(n, d, device=dev), torch.zeros(n, d, device=dev)
  losses = [ops.deepwalk_step(emb, m, v, t, p.to(dev), q.to(dev), c['C']) for t, (p, q) in enumerate(batches, 1)]
  return emb, m, v, [float(x) for x in losses]


def _compare(label, got, ref):
  emb, m, v, losses = got
  figures = dict(weight=float((emb.cpu().double() - ref.weight).abs().max()), exp_avg=float((m.cpu().double() - ref.exp_avg).abs().max()),
                 exp_avg_sq=float((v.cpu().double() - ref.exp_avg_sq).abs().max()),
                 loss=max(abs(a - b) for a, b in zip(losses, ref.losses)))
  print('%s: d32 %.3e tol %.3e  ' % (label, ref.d32, ref.tol) + '  '.join('%s %.3e' % kv for kv in figures.items()))
  assert all(np.isfinite(x) for x in losses) and bool(torch.isfinite(emb).all())
  for key, err in figures.items():
    assert err <= ref.tol, (label, key, err, ref.tol)


@pytest.mark.parametrize('name', sorted(O.CASES))
def test_step_against_the_float64_oracle(dev, name):
  if O.case_refused(name):                       # (80, 2) at d = 256: 81 rows of 256 floats do not fit 64 KiB of LDS -- the documented limit
    w, batches = O.case_inputs(name)
    z = torch.zeros_like(w, device=dev)
    with pytest.raises(G.GnpdeError, match='64 KiB of LDS'):
      ops.deepwalk_step(w.to(dev), z, z.clone(), 1, batches[0][0].to(dev), batches[0][1].to(dev), O.CASES[name]['C'])
    return
  _compare(name, _device_steps(name, dev), O.case_result(name))


def test_untouched_rows_keep_their_bits(dev):
  w, batches = O.case_inputs('sparse-n300')
  emb, m, v, _ = _device_steps('sparse-n300', dev)
  touched = torch.zeros(w.shape[0], dtype=torch.bool)
  for p, q in batches:
    touched[p.reshape(-1)] = True
    touched[q.reshape(-1)] = True
  assert 0 < int(touched.sum()) < w.shape[0] // 2
  assert torch.equal(emb.cpu()[~touched], w[~touched])
  assert not m.cpu()[~touched].any() and not v.cpu()[~touched].any()
  assert (emb.cpu()[touched] != w[touched]).any(dim=1).all()


def test_padded_rows_and_repeats_are_bit_identical(dev):
  a = _device_steps('collide-n7', dev)
  b = _device_steps('collide-n7', dev)
  c = _device_steps('collide-n7', dev, pad=4)
  assert c[0].stride(0) == 68
  for x, y, z in zip(a[:3], b[:3], c[:3]):
    assert torch.equal(x, y) and torch.equal(x, z)
  assert a[3] == b[3] == c[3]
  _compare('collide-n7 padded', c, O.case_result('collide-n7'))


def test_int32_walks_and_a_given_loss_slot(dev):
  c = O.CASES['steps8-n300']
  w, batches = O.case_inputs('steps8-n300')
  p, q = batches[0]
  outs = []
  for cast in (torch.int64, torch.int32):
    emb, m, v = w.to(dev), torch.zeros_like(w, device=dev), torch.zeros_like(w, device=dev)
    slot = torch.zeros(3, device=dev)
    loss = ops.deepwalk_step(emb, m, v, 1, p.to(dev).to(cast), q.to(dev).to(cast), c['C'], loss_out=slot[1:2])
    assert loss.dim() == 0 and loss.is_cuda and float(slot[1]) == float(loss) and float(slot[0]) == 0 == float(slot[2])
    outs.append((emb, float(loss)))
  assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
  bad = p.clone()
  bad[0, 1] = w.shape[0]
  with pytest.raises(G.GnpdeError, match='walk entry'):
    ops.deepwalk_step(w.to(dev), torch.zeros_like(w, device=dev), torch.zeros_like(w, device=dev), 1, bad.to(dev), q.to(dev), c['C'])


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def _train(dev, seed):
  t = O.TRAINER
  ei, n = O.trainer_graph()
  model = DeepWalk(torch.from_numpy(ei).to(dev), n, embedding_dim=t['d'], walk_length=t['L'], context_size=t['C'],
                   walks_per_node=t['walks_per_node'], num_negative_samples=t['k'], lr=t['lr'], seed=seed)
  return model, model.fit(t['epochs'], batch_size=t['batch_size'])


def test_trainer_equals_the_oracle_trainer(dev):
  ref = O.trainer_result(0)
  model, means = _train(dev, 0)
  assert model.embedding.shape == (300, 64) and model.embedding.dtype == torch.float32 and model.embedding.is_cuda
  assert model.step_count == 6 and len(means) == 2
  figures = dict(weight=float((model.embedding.cpu().double() - ref.weight).abs().max()),
                 exp_avg=float((model.exp_avg.cpu().double() - ref.exp_avg).abs().max()),
                 exp_avg_sq=float((model.exp_avg_sq.cpu().double() - ref.exp_avg_sq).abs().max()),
                 epoch_loss=max(abs(a - b) for a, b in zip(means, ref.epoch_means)))
  print('trainer: d32 %.3e tol %.3e  ' % (ref.d32, ref.tol) + '  '.join('%s %.3e' % kv for kv in figures.items()))
  for key, err in figures.items():
    assert err <= ref.tol, (key, err, ref.tol)
  again, means2 = _train(dev, 0)
  assert torch.equal(model.embedding, again.embedding) and torch.equal(model.exp_avg_sq, again.exp_avg_sq) and means == means2
  other, means3 = _train(dev, 1)
  assert not torch.equal(model.embedding, other.embedding) and means != means3


def test_use_embeddings_separate_two_planted_communities(dev):
  u = O.USE
  ei, n = O.two_communities(u['n'])
  model = DeepWalk(torch.from_numpy(ei).to(dev), n, embedding_dim=u['d'], walk_length=u['L'], context_size=u['C'],
                   walks_per_node=u['walks_per_node'], num_negative_samples=u['k'], lr=u['lr'], seed=0)
  before = O.community_cosines(model.embedding, n)
  losses = model.fit(u['epochs'], batch_size=u['batch_size'])
  same, different = O.community_cosines(model.embedding, n)
  print('cosines before %+.3f / %+.3f, after %+.3f / %+.3f; loss %.3f -> %.3f' % (before + (same, different, losses[0], losses[-1])))
  assert same > 0 and different < 0
  assert losses[-1] < losses[0]


# ---- apply_beltrami --------------------------------------------------------------------------------------------------------------
def test_apply_beltrami_generates_caches_and_reloads(dev, tmp_path, monkeypatch):
  ei, n = O.trainer_graph()
  data = types.SimpleNamespace(edge_index=torch.from_numpy(ei).to(dev), edge_attr=None, num_nodes=n)
  opt = {'pos_enc_type': 'DW64', 'dataset': 'Synthetic', 'gnpde_generate_pos_enc': True, 'gnpde_dw_epochs': 1, 'seed': 3,
         'gdc_sparsification': 'topk', 'gdc_k': 4}
  with pytest.raises(FileNotFoundError):
    G.graph_rewiring.apply_beltrami(data, dict(opt, gnpde_generate_pos_enc=False), data_dir=str(tmp_path))
  enc = G.graph_rewiring.apply_beltrami(data, opt, data_dir=str(tmp_path))
  fname = tmp_path / 'pos_encodings' / 'Synthetic_DW64.pkl'
  with open(fname, 'rb') as f:
    stored = pickle.load(f)
  assert sorted(stored) == ['acc', 'data'] and isinstance(stored['acc'], float)
  assert stored['data'].shape == (n, 64) and stored['data'].dtype == torch.float32 and not stored['data'].is_cuda
  assert torch.equal(enc, stored['data']) and bool(torch.isfinite(enc).all())

  def no_training(*a, **kw):
    raise AssertionError('a cached pickle must not train')
  monkeypatch.setattr(DeepWalk, 'fit', no_training)
  assert torch.equal(G.graph_rewiring.apply_beltrami(data, opt, data_dir=str(tmp_path)), enc)
  G.graph_rewiring.apply_pos_dist_rewire(data, opt, data_dir=str(tmp_path))
  assert data.edge_index.shape == (2, 4 * n) and os.listdir(tmp_path / 'pos_encodings') == ['Synthetic_DW64.pkl']


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
  ei = torch.from_numpy(O.ring()[0]).to(dev)
  with pytest.raises(NotImplementedError, match='p = q = 1'):
    DeepWalk(ei, 5, p=2)
  with pytest.raises(NotImplementedError, match='p = q = 1'):
    DeepWalk(ei, 5, q=0.5)
  for kw, text in ((dict(embedding_dim=6), 'multiple of 4'), (dict(embedding_dim=260), 'multiple of 4'), (dict(walk_length=128), 'walk_length'),
                   (dict(walk_length=8, context_size=9), 'context_size'), (dict(walk_length=8, context_size=1), 'context_size')):
    with pytest.raises(G.GnpdeError, match=text):
      DeepWalk(ei, 5, **kw)

  def step(d=8, L=4, C=3, host=False):
    z = lambda: torch.zeros(5, d, device='cpu' if host else dev)
    rw = torch.zeros(2, L + 1, dtype=torch.int64, device='cpu' if host else dev)
    return ops.deepwalk_step(z(), z(), z(), 1, rw, rw, C)
  assert float(step()) > 0
  for kw, text in ((dict(d=6), 'multiple of 4'), (dict(d=260), 'multiple of 4'), (dict(L=128), 'walk_length'), (dict(L=4, C=5), 'context_size'),
                   (dict(host=True), 'HIP')):
    with pytest.raises(G.GnpdeError, match=text):
      step(**kw)
  host = torch.zeros(2, dtype=torch.int64)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.random_walks(ei, 5, host, 3, 0, 16, 0)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.negative_walks(5, host, 3, 0, 17, 0)
  with pytest.raises(G.GnpdeError, match='walk_length'):
    ops.negative_walks(5, host.to(dev), 128, 0, 17, 0)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.random_permutation(5, 0, 18, 0, device='cpu')
