"""Hyperbolic positional encodings, everything that needs no device: the header's closed-form gradient against float64 autograd, the
properties of the step on the oracle (hyp_oracle.py: rows stay in the ball, the bound on a row's move, coincident pairs), the
functional condition on the oracle trainer, the symbols and the ABI number, the refusals of the Python surface and of the C entry
points, and the option table of `apply_beltrami`."""
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
from gnpde_amd import hyperbolic_embeddings as HE
import deepwalk_oracle as DO
import hyp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_poincare_step_workspace_bytes', 'gnpde_poincare_step')
EINVAL, ESHAPE, EWS, ESTATE = -1, -2, -3, -4          # GNPDE_E* of include/gnpde.h


# ---- the definition --------------------------------------------------------------------------------------------------------------
def _random_pairs(m, d, seed, hi=0.999):
  g = torch.Generator().manual_seed(seed)
  rows = lambda: (lambda x: x / x.norm(dim=1, keepdim=True) * (hi * torch.rand(m, 1, generator=g, dtype=torch.float64)))(
    torch.randn(m, d, generator=g, dtype=torch.float64))
  return rows(), rows()


@pytest.mark.parametrize('d', (2, 4, 16, 100))
def test_closed_form_gradient_equals_float64_autograd(d):
  """d dist / d e_u of include/gnpde.h against autograd of dist, relative to the gradient's Euclidean length 2 / alpha."""
  eu, ev = _random_pairs(4000, d, d)
  assert 0.99 < float(eu.norm(dim=1).max()) < 0.999 + 1e-12
  eu.requires_grad_(True)
  ev.requires_grad_(True)
  dist = O.distance(eu, ev)
  gu, gv = torch.autograd.grad(dist.sum(), (eu, ev))
  with torch.no_grad():
    cu, cv = O.distance_gradient(eu, ev), O.distance_gradient(ev, eu)
    alpha, beta = 1 - (eu * eu).sum(1), 1 - (ev * ev).sum(1)
    err_u = float(((cu - gu).norm(dim=1) * alpha / 2).max())
    err_v = float(((cv - gv).norm(dim=1) * beta / 2).max())
    print('d = %d: closed form against autograd, relative to 2 / alpha: %.2e / %.2e' % (d, err_u, err_v))
    assert err_u <= 1e-10 and err_v <= 1e-10
    # the Euclidean length of the gradient is 2 / alpha: what bounds a row's move
    assert float(((cu.norm(dim=1) * alpha / 2) - 1).abs().max()) < 1e-9
    # and dist is arccosh(1 + 2 r)
    r = O.pair_key(eu, ev)[0]
    assert float((dist - torch.acosh(1 + 2 * r)).abs().max()) < 1e-6          # acosh's own cancellation at small r
    big = r > 1
    assert float((dist[big] - torch.acosh(1 + 2 * r[big])).abs().max()) < 1e-12


def test_coincident_pairs_have_no_gradient_and_count_with_dist_zero():
  e = O.spread_rows(4, 4, 1, 0.2, 0.8).double()
  e[1] = e[0]                                                                # identical coordinates, different nodes
  for rw in (torch.tensor([[0, 0, 0]]), torch.tensor([[0, 1, 0]])):         # the same node; the twins
    leaf = e.clone().requires_grad_(True)
    terms = O.loss_terms(leaf, rw, 2, 2.0, 1.0, True)
    terms.sum().backward()
    assert not leaf.grad.any() and bool(torch.isfinite(leaf.grad).all())
    want = -np.log(1 / (1 + np.exp(-2.0)) + O.EPS)                           # x = (R - 0) / T = 2
    assert torch.allclose(terms, torch.full_like(terms, want), atol=1e-15, rtol=0)
    s = O.Step(e, rw, rw, 2)
    assert torch.equal(s.emb, e) and abs(s.loss - (want - np.log(1 / (1 + np.exp(2.0)) + O.EPS))) < 1e-14
    assert s.counts.tolist() == ([8, 0, 0, 0] if int(rw[0, 1]) == 0 else [4, 4, 0, 0])      # a same-node pair counts twice
  assert not O.distance_gradient(e[:1], e[1:2]).any()


@pytest.mark.parametrize('name', ('grid-L5C5-d4-k2', 'collide-n7', 'boundary', 'twins', 'steps8-n300'))
def test_rows_stay_in_the_ball_and_no_row_moves_further_than_the_bound(name):
  c = O.CASES[name]
  w, batches = O.case_inputs(name)
  for lr, T in ((1.0, 1.0), (8.0, 0.5)):
    e = w.double()
    for p, q in batches:
      s = O.Step(e, p, q, c['C'], lr=lr, temperature=T)
      bound = lr * s.alpha / (2 * T)
      assert bool((s.move <= bound * (1 + 1e-12)).all()), (name, lr, float((s.move / bound).max()))
      assert not s.move[~s.touched].any() and torch.equal(s.emb[~s.touched], e[~s.touched])
      norms = s.emb.norm(dim=1)
      assert float(norms.max()) <= O.BALL_EDGE * (1 + 1e-15) < 1
      ends = torch.cat(O.pair_ends(p, c['C']) + O.pair_ends(q, c['C']))
      assert int(s.counts.sum()) == ends.numel() == 2 * (p.shape[0] + q.shape[0]) * len(DO.window_pairs(c['L'], c['C']))
      e = s.emb
  assert float(O.case_result(name).emb.norm(dim=1).max()) < 1


def test_a_row_driven_at_the_boundary_is_projected():
  e = torch.zeros(3, 2, dtype=torch.float64)
  e[0, 0], e[1, 0] = 0.5, -0.5
  pos = torch.tensor([[2, 2, 2]])                                            # touches neither row
  neg = torch.tensor([[0, 1, 0]])                                            # pushes rows 0 and 1 apart
  for _ in range(40):
    e = O.Step(e, pos, neg, 2, lr=50.0).emb
  n0 = float(e[0].norm())
  assert 1 - 2e-5 <= n0 < 1 and float(e[0, 0]) > 0 and float(e[1, 0]) < 0


def test_tolerances_come_from_the_oracle_alone():
  for name in ('grid-L20C16-d16-k1', 'collide-n7', 'boundary'):
    r = O.case_result(name)
    assert 0 < r.d32 < 1e-4 and r.tol == 8 * r.d32 and np.isfinite(r.losses).all()
  assert sorted(O.CASES)[:1] == ['boundary'] and len(O.CASES) == 4 * 4 * 2 + 5
  w, _ = O.case_inputs('boundary')
  norms = w.double().norm(dim=1)
  assert 0.9 <= float(norms.min()) and 0.99 < float(norms.max()) <= 0.999 + 1e-7
  w, batches = O.case_inputs('twins')
  assert torch.equal(w[0], w[1])
  u, v = O.pair_ends(batches[0][1], O.CASES['twins']['C'])
  assert int(((u == 0) & (v == 1)).sum()) > 0 and int((u == v).sum()) > 0    # the twins meet, and so does a node itself


def test_functional_condition_on_the_oracle_trainer():
  """The tree of branching 3 and depth 4: the float64 oracle's MAP of true neighbours is at least 4 x its value at initialisation."""
  ei, n = O.tree(O.USE['branching'], O.USE['depth'])
  assert n == 121 and ei.shape == (2, 240)
  before, after = O.use_result(0)
  print('MAP of true neighbours: %.3f at initialisation, %.3f after %d epochs (float64 oracle)' % (before, after, O.USE['epochs']))
  assert after >= O.USE_MAP_FACTOR * before
  # the measure itself: a perfect ranking scores 1
  line = np.array([[0, 1, 1, 2], [1, 0, 2, 1]])
  assert O.neighbour_map(torch.tensor([[-0.5, 0.0], [0.0, 0.0], [0.5, 0.0]]), line, 3) == 1.0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_number_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  declared = set(re.findall(r'\b(gnpde_[a-z_0-9]+)\s*\(', header))
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  L = G.lib()
  for name in SYMBOLS:
    assert name in declared, name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name), name + ' is not exported by the library'
    assert name in doc, name + ' is not in INTEGRATION.md'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 19 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION
  # a DeepWalk run and a hyperbolic run of one seed share no random numbers
  mine = {ops.STREAM_HYP_POS_WALKS, ops.STREAM_HYP_NEG_WALKS, ops.STREAM_HYP_EPOCH_ORDER}
  assert mine == {O.STREAM_POS, O.STREAM_NEG, O.STREAM_ORDER} == {19, 20, 21}
  assert not mine & {0, 1, ops.STREAM_POS_WALKS, ops.STREAM_NEG_WALKS, ops.STREAM_EPOCH_ORDER}


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSED = ((dict(d=3), 'multiple of 4'), (dict(d=6), 'multiple of 4'), (dict(d=132), 'multiple of 4'), (dict(d=0), 'multiple of 4'),
           (dict(L=128, C=2), 'walk_length'), (dict(L=0, C=2), 'walk_length'), (dict(L=4, C=5), 'context_size'),
           (dict(L=4, C=1), 'context_size'), (dict(L=127, C=2, d=128), '64 KiB of LDS'), (dict(L=127, C=16, d=124), '64 KiB of LDS'))
ACCEPTED = (dict(d=2), dict(d=4), dict(d=128, L=100, C=2), dict(L=127, C=127, d=2), dict(L=127, C=2, d=124), dict(L=2, C=2, d=100))


def test_check_shape_refuses_what_the_kernel_refuses():
  L = G.lib()
  for kw, text in REFUSED:
    a = dict(dict(L=8, C=3, d=8), **kw)
    with pytest.raises(G.GnpdeError, match=text):
      ops.poincare_check_shape(a['L'], a['C'], a['d'])
    assert L.gnpde_poincare_step_workspace_bytes(4, 4, a['L'], a['C'], a['d']) == 0
    assert L.gnpde_poincare_step(None, a['d'], 5, a['d'], None, 4, None, 4, a['L'], a['C'], 1.0, 2.0, 1.0, None, None, None, 0, None) == ESHAPE
    assert text.replace('multiple of 4', 'multiple of 4 in 4 .. 128') in L.gnpde_last_error().decode()
  for kw in ACCEPTED:
    a = dict(dict(L=8, C=3, d=8), **kw)
    ops.poincare_check_shape(a['L'], a['C'], a['d'])
    # past the shape checks the null pointers are what is refused: the two sides agree on the limits
    assert L.gnpde_poincare_step(None, a['d'], 5, a['d'], None, 4, None, 4, a['L'], a['C'], 1.0, 2.0, 1.0, None, None, None, 0, None) == EINVAL


def test_entry_point_rejects_bad_arguments_before_any_launch():
  L = G.lib()
  p = _lib.ptr
  f, i32 = torch.zeros(8, 8), torch.zeros(4, 9, dtype=torch.int32)
  out, flag = torch.zeros(1), torch.zeros(1, dtype=torch.int32)
  call = lambda emb=f, ld=8, n=8, d=8, r_pos=4, r_neg=4, lr=1.0, T=1.0: L.gnpde_poincare_step(
    p(emb), ld, n, d, p(i32), r_pos, p(i32), r_neg, 8, 3, lr, 2.0, T, p(out), p(flag), None, 0, None)
  # everything but the workspace is in order; without a device the sort's temporary-storage query fails first (as deepwalk_step's)
  past = EWS if L.gnpde_poincare_step_workspace_bytes(4, 4, 8, 3, 8) else ESTATE
  assert call() == past and ('workspace' if past == EWS else 'query failed') in L.gnpde_last_error().decode()
  for kw in (dict(ld=4), dict(ld=10), dict(n=0), dict(r_pos=0), dict(r_neg=0), dict(lr=-1.0), dict(T=0.0), dict(lr=float('nan')),
             dict(emb=f[:, 1:], d=4)):
    assert call(**kw) == EINVAL, kw
  assert call(d=2, ld=6) == past and call(d=2, ld=3) == EINVAL
  assert call(r_pos=2 ** 31 // 9, r_neg=1) == ESHAPE and 'INT32_MAX' in L.gnpde_last_error().decode()
  assert float(f.abs().sum()) == 0 and int(flag) == 0


def test_python_surface_refuses_before_any_launch():
  rw = torch.zeros(2, 5, dtype=torch.int64)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.poincare_step(torch.zeros(4, 8), rw, rw, 3)
  with pytest.raises(G.GnpdeError, match='float32 matrix'):
    ops.poincare_step(torch.zeros(4, 8, dtype=torch.float64), rw, rw, 3)
  ei = torch.tensor([[0, 1], [1, 0]])
  for kw, text in ((dict(embedding_dim=3), 'multiple of 4'), (dict(embedding_dim=132), 'multiple of 4'), (dict(walk_length=128), 'walk_length'),
                   (dict(walk_length=8, context_size=9), 'context_size'), (dict(walks_per_node=0), 'at least 1'), (dict(lr=-1.0), 'lr >= 0'),
                   (dict(temperature=0.0), 'temperature > 0')):
    with pytest.raises(G.GnpdeError, match=text):
      HE.PoincareEmbedding(ei, 2, **dict(dict(embedding_dim=8), **kw))
  if not torch.cuda.is_available():
    with pytest.raises(G.GnpdeError, match='HIP'):
      HE.PoincareEmbedding(ei, 2, 8)


def test_initialisation_and_names():
  w = HE.initial_embedding(300, 16, 5)
  assert w.dtype == torch.float32 and torch.equal(w, O.initial_embedding(300, 16, 5)) and not torch.equal(w, HE.initial_embedding(300, 16, 6))
  assert float(w.abs().max()) <= 1e-3 and float(w.min()) < -9e-4 and float(w.max()) > 9e-4
  assert HE.pickle_name(dict(dataset='Cora', embedding_dim=2)) == 'Cora_HYPS02.pkl'
  assert HE.pickle_name(dict(dataset='Cora', embedding_dim=16)) == 'Cora_HYPS16.pkl'
  assert [HE.embedding_dim_of(k) for k in ('HYPS16', 'HYPS08', 'HYPS04', 'HYPS02')] == [16, 8, 4, 2]
  for kind in ('HYPx', 'HYPSx', 'HYP16', 'HYPS', 'HYPS00', 'DW64'):
    with pytest.raises(ValueError, match='HYPS<dd>'):
      HE.embedding_dim_of(kind)


# ---- apply_beltrami --------------------------------------------------------------------------------------------------------------
class _FakeTrainer(object):
  made = []

  def __init__(self, edge_index, num_nodes, **kw):
    self.kw = dict(kw, num_nodes=num_nodes)
    self.embedding = torch.full((num_nodes, kw['embedding_dim']), 0.25)
    _FakeTrainer.made.append(self)

  def fit(self, epochs, batch_size=128):
    self.kw.update(epochs=epochs, batch_size=batch_size)
    return [0.0] * epochs


def test_apply_beltrami_option_table(tmp_path, monkeypatch):
  monkeypatch.setattr(HE, 'PoincareEmbedding', _FakeTrainer)
  del _FakeTrainer.made[:]
  data = types.SimpleNamespace(edge_index=torch.tensor([[0, 1], [1, 0]]), num_nodes=2)
  base = {'dataset': 'Synthetic', 'pos_enc_type': 'HYPS16'}
  beltrami = lambda opt: G.graph_rewiring.apply_beltrami(data, opt, data_dir=str(tmp_path))
  # nothing changes without the opt-in; the DeepWalk key alone does not cover HYP*, and the new key does not cover DW*
  for opt in (base, dict(base, gnpde_generate_hyp_enc=False), dict(base, gnpde_generate_hyp_enc=0), dict(base, gnpde_generate_pos_enc=True),
              dict(base, pos_enc_type='DW64', gnpde_generate_hyp_enc=True)):
    with pytest.raises(FileNotFoundError):
      beltrami(opt)
  with pytest.raises(FileNotFoundError, match='gnpde_generate_hyp_enc'):
    beltrami(base)
  assert not _FakeTrainer.made and not os.path.exists(tmp_path / 'pos_encodings')
  for kind in ('HYPx', 'HYPSx', 'HYP16'):
    with pytest.raises(ValueError, match='HYPS<dd>'):
      beltrami(dict(base, pos_enc_type=kind, gnpde_generate_hyp_enc=True))
  assert not _FakeTrainer.made and not os.path.exists(tmp_path / 'pos_encodings')
  # the opt-in: the trainer's defaults, 100 epochs and seed 0 unless the options say otherwise
  enc = beltrami(dict(base, gnpde_generate_hyp_enc=True))
  assert _FakeTrainer.made.pop().kw == dict(num_nodes=2, embedding_dim=16, seed=0, epochs=100, batch_size=128)
  with open(tmp_path / 'pos_encodings' / 'Synthetic_HYPS16.pkl', 'rb') as f:
    stored = pickle.load(f)
  assert isinstance(stored, torch.Tensor) and not stored.is_cuda and torch.equal(stored, enc) and enc.shape == (2, 16)
  assert torch.equal(beltrami(base), enc) and not _FakeTrainer.made            # a cached pickle is loaded, option or not
  assert torch.equal(beltrami(dict(base, gnpde_generate_hyp_enc=True)), enc) and not _FakeTrainer.made
  beltrami(dict(base, pos_enc_type='HYPS02', gnpde_generate_hyp_enc=1, gnpde_hyp_epochs=3, seed=7, gnpde_dw_epochs=9))
  kw = _FakeTrainer.made.pop().kw
  assert (kw['embedding_dim'], kw['epochs'], kw['seed']) == (2, 3, 7)
  assert sorted(os.listdir(tmp_path / 'pos_encodings')) == ['Synthetic_HYPS02.pkl', 'Synthetic_HYPS16.pkl']


def test_documents_no_longer_say_not_built():
  for name in ('README.md', 'INTEGRATION.md', os.path.join('graph-neural-pde_amd', 'graph_rewiring.py')):
    text = open(os.path.join(ROOT, name)).read()
    assert 'loaded, not generated' not in text and 'generating hyperbolic embeddings is not built' not in text, name
    assert 'gnpde_generate_hyp_enc' in text, name
