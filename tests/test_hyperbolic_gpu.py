"""Native hyperbolic positional encodings on the device against the CPU oracle (hyp_oracle.py): the step and the trainer against the
float64 oracle within 8 x (the fp32 oracle's own distance from it), entry by entry; the projection; bit identity of untouched rows,
padded rows, repeated runs and int32 walks; the functional condition on a tree; apply_beltrami's opt-in and the Poincare k-NN
rewiring on the generated file; refusals."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
from gnpde_amd.hyperbolic_embeddings import PoincareEmbedding
import hyp_oracle as O

pytestmark = pytest.mark.gpu


# ---- the step --------------------------------------------------------------------------------------------------------------------
def _device_steps(name, dev, pad=0, cast=torch.int64, lr=1.0):
  c = O.CASES[name]
  w, batches = O.case_inputs(name)
  n, d = w.shape
  emb = torch.zeros(n, d + pad, device=dev)[:, :d]
  emb.copy_(w)
  losses = [ops.poincare_step(emb, p.to(dev).to(cast), q.to(dev).to(cast), c['C'], lr=lr) for p, q in batches]
  return emb, [float(x) for x in losses]


def _compare(label, got, ref):
  emb, losses = got
  figures = dict(emb=float((emb.cpu().double() - ref.emb).abs().max()), loss=max(abs(a - b) for a, b in zip(losses, ref.losses)))
  print('%s: d32 %.3e tol %.3e  ' % (label, ref.d32, ref.tol) + '  '.join('%s %.3e' % kv for kv in figures.items()))
  assert all(np.isfinite(x) for x in losses) and bool(torch.isfinite(emb).all())
  assert float(emb.double().norm(dim=1).max()) < 1
  for key, err in figures.items():
    assert err <= ref.tol, (label, key, err, ref.tol)


@pytest.mark.parametrize('name', sorted(O.CASES))
def test_step_against_the_float64_oracle(dev, name):
  _compare(name, _device_steps(name, dev), O.case_result(name))


def test_a_row_driven_at_the_boundary_is_projected(dev):
  e = torch.zeros(3, 2, device=dev)
  e[0, 0], e[1, 0] = 0.5, -0.5
  ref = e.cpu().double()
  pos, neg = torch.tensor([[2, 2, 2]]), torch.tensor([[0, 1, 0]])           # the negative walk pushes rows 0 and 1 apart
  for _ in range(40):
    ops.poincare_step(e, pos.to(dev), neg.to(dev), 2, lr=50.0)
    ref = O.Step(ref, pos, neg, 2, lr=50.0).emb
  norms = e.cpu().double().norm(dim=1)
  assert float(ref[0].norm()) >= 1 - 2e-5                                    # the oracle's row is at the edge as well
  assert 1 - 2e-5 <= float(norms[0]) < 1 and 1 - 2e-5 <= float(norms[1]) < 1
  assert float(e[0, 0]) > 0 > float(e[1, 0]) and not e[2].any()


def test_untouched_rows_keep_their_bits(dev):
  w, batches = O.case_inputs('sparse-n300')
  emb, _ = _device_steps('sparse-n300', dev)
  touched = torch.zeros(w.shape[0], dtype=torch.bool)
  for p, q in batches:
    touched[p.reshape(-1)] = True
    touched[q.reshape(-1)] = True
  assert 0 < int(touched.sum()) < w.shape[0] // 2
  assert torch.equal(emb.cpu()[~touched], w[~touched])
  assert (emb.cpu()[touched] != w[touched]).any(dim=1).all()


@pytest.mark.parametrize('name,pad', (('collide-n7', 4), ('grid-L5C5-d2-k1', 2), ('grid-L5C5-d2-k1', 3), ('grid-L3C2-d100-k2', 28)))
def test_padded_rows_and_repeats_are_bit_identical(dev, name, pad):
  if (O.CASES[name]['d'] + pad) % (2 if O.CASES[name]['d'] == 2 else 4):
    with pytest.raises(G.GnpdeError, match='row stride'):                    # a width of 2 takes even strides only
      _device_steps(name, dev, pad=pad)
    return
  a = _device_steps(name, dev)
  b = _device_steps(name, dev)
  c = _device_steps(name, dev, pad=pad)
  assert c[0].stride(0) == O.CASES[name]['d'] + pad
  assert torch.equal(a[0], b[0]) and torch.equal(a[0], c[0]) and a[1] == b[1] == c[1]
  _compare(name + ' padded', c, O.case_result(name))


def test_int32_walks_a_given_loss_slot_and_a_bad_walk_entry(dev):
  c = O.CASES['steps8-n300']
  w, batches = O.case_inputs('steps8-n300')
  p, q = batches[0]
  outs = []
  for cast in (torch.int64, torch.int32):
    emb = w.to(dev)
    slot = torch.zeros(3, device=dev)
    loss = ops.poincare_step(emb, p.to(dev).to(cast), q.to(dev).to(cast), c['C'], loss_out=slot[1:2])
    assert loss.dim() == 0 and loss.is_cuda and float(slot[1]) == float(loss) and float(slot[0]) == 0 == float(slot[2])
    outs.append((emb, float(loss)))
  assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
  bad = p.clone()
  bad[0, 1] = w.shape[0]
  with pytest.raises(G.GnpdeError, match='walk entry'):
    ops.poincare_step(w.to(dev), bad.to(dev), q.to(dev), c['C'])


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def _train(dev, seed):
  t = O.TRAINER
  ei, n = O.trainer_graph()
  model = PoincareEmbedding(torch.from_numpy(ei).to(dev), n, t['d'], walk_length=t['L'], context_size=t['C'],
                            walks_per_node=t['walks_per_node'], num_negative_samples=t['k'], lr=t['lr'], seed=seed)
  return model, model.fit(t['epochs'], batch_size=t['batch_size'])


def test_trainer_equals_the_oracle_trainer(dev):
  ref = O.trainer_result(0)
  model, means = _train(dev, 0)
  assert model.embedding.shape == (300, 16) and model.embedding.dtype == torch.float32 and model.embedding.is_cuda
  assert model.step_count == 6 and model.epoch == 2 and len(means) == 2
  figures = dict(emb=float((model.embedding.cpu().double() - ref.emb).abs().max()),
                 epoch_loss=max(abs(a - b) for a, b in zip(means, ref.epoch_means)))
  print('trainer: d32 %.3e tol %.3e  ' % (ref.d32, ref.tol) + '  '.join('%s %.3e' % kv for kv in figures.items()))
  for key, err in figures.items():
    assert err <= ref.tol, (key, err, ref.tol)
  again, means2 = _train(dev, 0)
  assert torch.equal(model.embedding, again.embedding) and means == means2
  other, means3 = _train(dev, 1)
  assert not torch.equal(model.embedding, other.embedding) and means != means3


def test_native_training_ranks_a_trees_neighbours_as_the_oracle_does(dev):
  u = O.USE
  ei, n = O.tree(u['branching'], u['depth'])
  before, oracle = O.use_result(0)
  model = PoincareEmbedding(torch.from_numpy(ei).to(dev), n, u['d'], walk_length=u['L'], context_size=u['C'],
                            walks_per_node=u['walks_per_node'], num_negative_samples=u['k'], lr=u['lr'], seed=0)
  losses = model.fit(u['epochs'], batch_size=u['batch_size'])
  native = O.neighbour_map(model.embedding, ei, n)
  print('MAP of true neighbours: %.3f at initialisation, float64 oracle %.3f, native %.3f; loss %.3f -> %.3f'
        % (before, oracle, native, losses[0], losses[-1]))
  assert oracle >= O.USE_MAP_FACTOR * before
  assert native >= O.USE_NATIVE_SHARE * oracle
  assert float(model.embedding.double().norm(dim=1).max()) < 1 and losses[-1] < losses[0]


# ---- apply_beltrami --------------------------------------------------------------------------------------------------------------
def test_apply_beltrami_generates_caches_reloads_and_rewires(dev, tmp_path, monkeypatch):
  ei, n = O.trainer_graph()
  data = types.SimpleNamespace(edge_index=torch.from_numpy(ei).to(dev), edge_attr=None, num_nodes=n)
  opt = {'pos_enc_type': 'HYPS16', 'dataset': 'Synthetic', 'gnpde_generate_hyp_enc': True, 'gnpde_hyp_epochs': 2, 'seed': 3,
         'gdc_sparsification': 'topk', 'gdc_k': 4}
  with pytest.raises(FileNotFoundError):
    G.graph_rewiring.apply_beltrami(data, dict(opt, gnpde_generate_hyp_enc=False, gnpde_generate_pos_enc=True), data_dir=str(tmp_path))
  encs = {}
  for kind, d in (('HYPS16', 16), ('HYPS02', 2)):
    enc = G.graph_rewiring.apply_beltrami(data, dict(opt, pos_enc_type=kind), data_dir=str(tmp_path))
    with open(tmp_path / 'pos_encodings' / ('Synthetic_%s.pkl' % kind), 'rb') as f:
      stored = pickle.load(f)
    assert isinstance(stored, torch.Tensor) and stored.shape == (n, d) and stored.dtype == torch.float32 and not stored.is_cuda
    assert torch.equal(enc, stored) and bool(torch.isfinite(enc).all()) and float(enc.double().norm(dim=1).max()) < 1
    assert float(enc.abs().max()) > 10 * O.INIT_RANGE                        # trained, not the initialisation
    encs[kind] = enc

  def no_training(*a, **kw):
    raise AssertionError('a cached pickle must not train')
  monkeypatch.setattr(PoincareEmbedding, 'fit', no_training)
  for kind, enc in encs.items():
    assert torch.equal(G.graph_rewiring.apply_beltrami(data, dict(opt, pos_enc_type=kind), data_dir=str(tmp_path)), enc)
  G.graph_rewiring.apply_pos_dist_rewire(data, opt, data_dir=str(tmp_path))
  assert data.edge_index.shape == (2, 4 * n) and data.edge_index.dtype == torch.int64
  first = data.edge_index.cpu().reshape(2, n, 4)[:, :, 0]
  assert torch.equal(first[0], torch.arange(n)) and torch.equal(first[1], torch.arange(n))     # every node its own first neighbour
  assert sorted(os.listdir(tmp_path / 'pos_encodings')) == ['Synthetic_HYPS02.pkl', 'Synthetic_HYPS16.pkl']


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
  ei = torch.from_numpy(np.array([[0, 1, 2], [1, 2, 0]])).to(dev)
  for kw, text in ((dict(embedding_dim=3), 'multiple of 4'), (dict(embedding_dim=132), 'multiple of 4'), (dict(walk_length=128), 'walk_length'),
                   (dict(walk_length=8, context_size=9), 'context_size'), (dict(walk_length=8, context_size=1), 'context_size'),
                   (dict(embedding_dim=128, walk_length=127), '64 KiB of LDS')):
    with pytest.raises(G.GnpdeError, match=text):
      PoincareEmbedding(ei, 3, **dict(dict(embedding_dim=8), **kw))

  def step(d=8, L=4, C=3, host=False):
    e = torch.zeros(5, d, device='cpu' if host else dev)
    rw = torch.zeros(2, L + 1, dtype=torch.int64, device='cpu' if host else dev)
    return ops.poincare_step(e, rw, rw, C)
  assert float(step()) > 0 and float(step(d=2)) > 0 and float(step(d=128, L=100, C=2)) > 0
  for kw, text in ((dict(d=3), 'multiple of 4'), (dict(d=132), 'multiple of 4'), (dict(L=128), 'walk_length'), (dict(L=4, C=5), 'context_size'),
                   (dict(d=128, L=127, C=2), '64 KiB of LDS'), (dict(d=124, L=127, C=16), '64 KiB of LDS'), (dict(host=True), 'HIP')):
    with pytest.raises(G.GnpdeError, match=text):
      step(**kw)
  with pytest.raises(G.GnpdeError, match='temperature'):
    ops.poincare_step(torch.zeros(5, 8, device=dev), torch.zeros(2, 5, dtype=torch.int64, device=dev), torch.zeros(2, 5, dtype=torch.int64, device=dev),
                      3, temperature=0.0)
