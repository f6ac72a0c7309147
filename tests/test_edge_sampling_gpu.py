"""Edge-sampling rewiring on the device: the generator, the node draws, the fixed-point multinomial, the importance, the union, the
`>=` selection and the full adjacency against the CPU oracle (edge_sampling_oracle.py), then graph_rewiring.add_edges /
edge_sampling on a model and GNN_FA end to end.  Shapes are the smallest that cross a 64-lane wave, a 256-thread workgroup, the
4 096-element tile of the compaction and a multi-block scan."""
import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import graph_rewiring as GR
from helpers import assert_parity
import edge_sampling_oracle as O

pytestmark = pytest.mark.gpu

WORD_COUNTS = (0, 1, 3, 4, 5, 257, 70001)


# ---- generator ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(3))
def test_philox_known_answers(dev, case):
  counter, key, want = O.KNOWN_ANSWERS[case]
  got = G.ops.philox_words(key[0] | (key[1] << 32), counter[2], counter[3], counter[0] | (counter[1] << 32), 4, device=dev)
  assert tuple(got.tolist()) == want


@pytest.mark.parametrize('count', WORD_COUNTS)
def test_philox_words_equal_the_oracle(dev, count):
  seed, stream, call, first = 0x123456789abcdef, 1, 7, 2 ** 32 - 3        # the block counter crosses its low word
  got = G.ops.philox_words(seed, stream, call, first, count, device=dev)
  assert got.dtype == torch.int64 and got.shape == (count,)
  assert np.array_equal(got.cpu().numpy().astype(np.uint64), O.words(seed, stream, call, first, count))


def test_streams_and_calls_differ(dev):
  base = G.ops.philox_words(5, 0, 0, 0, 256, device=dev)
  assert not torch.equal(base, G.ops.philox_words(5, 1, 0, 0, 256, device=dev))
  assert not torch.equal(base, G.ops.philox_words(5, 0, 1, 0, 256, device=dev))
  assert not torch.equal(base, G.ops.philox_words(6, 0, 0, 0, 256, device=dev))
  assert torch.equal(base, G.ops.philox_words(5, 0, 0, 0, 256, device=dev))


@pytest.mark.parametrize('n', [1, 2, 3, 1000, 2 ** 31 - 1])
def test_random_nodes_equal_the_oracle(dev, n):
  for count in (0, 1, 255, 256, 257, 70001):
    got = G.ops.random_nodes(n, count, 99, 1, 4, device=dev)
    assert got.dtype == torch.int64 and got.shape == (count,)
    assert torch.equal(got.cpu(), O.random_nodes(n, count, 99, 1, 4)), (n, count)


# ---- multinomial ----------------------------------------------------------------------------------------------------------------
def exact_logits(n, pattern):
  s = torch.full((n,), -200.0)
  if pattern == 'one_hot':
    s[n // 2] = 0.0
  elif pattern == 'alternating':
    s[::2] = 0.0
  else:
    s[:] = 0.0
  return s


@pytest.mark.parametrize('n', [1, 2, 63, 65, 1025, 70001])
@pytest.mark.parametrize('pattern', ['one_hot', 'alternating', 'all_equal'])
def test_sample_nodes_exact_weights(dev, n, pattern):
  """Weights exactly 2^32 or 0: the draws equal the oracle's, and a node of weight 0 is never drawn."""
  s = exact_logits(n, pattern)
  got = G.ops.sample_nodes(s.to(dev), 10000, 31, 0, 2).cpu()
  assert torch.equal(got, O.sample_nodes(s.numpy(), 10000, 31, 0, 2))
  assert bool((s[got] == 0.0).all())


@pytest.mark.parametrize('case', range(len(O.REAL_CASES)))
def test_sample_nodes_real_logits_under_the_band(dev, case):
  s = O.real_logits(case)
  got = G.ops.sample_nodes(s.to(dev), O.REAL_DRAWS, *O.REAL_STREAM)
  band = O.real_band(case)
  print('case %s: %d draws differ from the oracle, %d undetermined' % (O.REAL_CASES[case], int((got.cpu().numpy() != band.draws).sum()),
                                                                         band.undetermined()))
  band.check(got)
  again = G.ops.sample_nodes(s.to(dev), O.REAL_DRAWS, *O.REAL_STREAM)
  assert torch.equal(got, again)
  assert G.ops.sample_nodes(s.to(dev), 0, 1, 0, 0).shape == (0,)


def test_sample_nodes_refuses_nan(dev):
  s = torch.zeros(300)
  s[17] = float('nan')
  with pytest.raises(G.GnpdeError, match='not finite'):
    G.ops.sample_nodes(s.to(dev), 10, 1, 0, 0)
  s[17] = float('inf')
  with pytest.raises(G.GnpdeError, match='not finite'):
    G.ops.sample_nodes(s.to(dev), 10, 1, 0, 0)


# ---- importance -----------------------------------------------------------------------------------------------------------------
def importance_case():
  """65 nodes, a self loop each; node 3 has 3 000 more incoming edges (a long column), node 64 keeps its loop alone."""
  g = torch.Generator().manual_seed(3)
  loops = torch.arange(65)
  src = torch.randint(0, 64, (3000,), generator=g)
  rest_src, rest_dst = torch.randint(0, 65, (400,), generator=g), torch.randint(0, 64, (400,), generator=g)
  ei = torch.cat([torch.stack([loops, loops]), torch.stack([src, torch.full((3000,), 3)]), torch.stack([rest_src, rest_dst])], dim=1)
  ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
  return ei, torch.rand(ei.shape[1], generator=g)


def test_node_importance(dev):
  ei, att = importance_case()
  want, deg = O.node_importance(ei, att, 65)
  assert int(deg[3]) >= 3001 and int(deg[64]) == 1
  got = G.ops.node_importance(ei.to(dev), att.to(dev), 65).cpu().double()
  bound = (deg + 1) * 2.0 ** -24 * want                       # deg additions and one division of non-negative terms
  err = (got - want).abs()
  print('largest error / bound: %.3f' % float((err / bound).max()))
  assert bool((err <= bound).all())
  assert float(got[64]) == float(att[(ei[1] == 64).nonzero()[0, 0]])
  assert torch.equal(G.ops.node_importance(ei.to(dev), att.to(dev), 65).cpu().double(), got)


def test_node_importance_refuses_a_node_without_incoming_edges(dev):
  ei, att = importance_case()
  keep = ei[1] != 64
  with pytest.raises(G.GnpdeError, match='no incoming edge'):
    G.ops.node_importance(ei[:, keep].contiguous().to(dev), att[keep].to(dev), 65)


# ---- union ----------------------------------------------------------------------------------------------------------------------
A5 = torch.tensor([[0, 4, 0, 2, 1], [1, 0, 1, 2, 3]])
B5 = torch.tensor([[3, 2, 3, 0, 4], [4, 2, 4, 1, 4]])
EMPTY = torch.zeros(2, 0, dtype=torch.int64)


@pytest.mark.parametrize('a,b', [(A5, B5), (EMPTY, B5), (A5, EMPTY), (EMPTY, EMPTY)])
def test_edge_union_small(dev, a, b):
  got = G.ops.edge_union(a.to(dev), b.to(dev), 5)
  assert got.dtype == torch.int64 and got.is_contiguous()
  assert torch.equal(got.cpu(), O.edge_union(a, b))


def test_edge_union_keys_beyond_32_bits(dev):
  n = 70001
  g = torch.Generator().manual_seed(8)
  a = torch.randint(0, n, (2, 300000), generator=g)
  b = torch.cat([torch.randint(0, n, (2, 90000), generator=g), a[:, :10000]], dim=1)     # 10 000 columns of b repeat a's
  got = G.ops.edge_union(a.to(dev), b.to(dev), n)
  want = O.edge_union(a, b)
  assert int((want[0] * n + want[1]).max()) > 2 ** 32 and want.shape[1] <= 390000
  assert torch.equal(got.cpu(), want)


def test_edge_union_refuses_an_index_out_of_range(dev):
  bad = B5.clone()
  bad[1, 2] = 5
  with pytest.raises(G.GnpdeError, match=r'outside \[0, n\)'):
    G.ops.edge_union(A5.to(dev), bad.to(dev), 5)
  bad[1, 2] = -1
  with pytest.raises(G.GnpdeError, match=r'outside \[0, n\)'):
    G.ops.edge_union(bad.to(dev), A5.to(dev), 5)


# ---- selection ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 255, 257, 100000, 1048577])   # the last: 257 blocks of 4096, the scan's carry into a second chunk
@pytest.mark.parametrize('rmv', [0.0, 0.32, 0.8, 1.0])
def test_select_edges_with_ties(dev, E, rmv):
  """Scores from eight dyadic values: many tie with the quantile, and `>=` keeps them all, in order."""
  g = torch.Generator().manual_seed(E)
  score = torch.randint(1, 9, (E,), generator=g).float() / 8
  ei = torch.randint(0, 1000, (2, E), generator=g)
  thr = G.ops.quantile(score.to(dev), rmv)
  want, want_thr = O.select_edges(ei, score, rmv)
  assert abs(float(thr) - float(want_thr)) <= 2.0 ** -23      # scores are in (0, 1]: one unit in the last place of the interpolation
  got = G.ops.select_edges(ei.to(dev), score.to(dev), thr)
  assert torch.equal(got.cpu(), want)
  assert torch.equal(G.ops.select_edges(ei.to(dev), score.to(dev), float(want_thr)).cpu(), want)
  if E > 1 and bool((score == want_thr).any()):
    strict, _ = G.ops.threshold_edges(ei.to(dev), score.to(dev), thr, 0, 1000)
    assert strict.shape[1] < got.shape[1] and torch.equal(strict.cpu(), ei[:, score > want_thr])


def test_select_edges_empty(dev):
  assert G.ops.select_edges(EMPTY.to(dev), torch.zeros(0, device=dev), 0.5).shape == (2, 0)


# ---- full adjacency -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 65, 300])
def test_full_adjacency(dev, n):
  assert torch.equal(G.ops.full_adjacency(n, device=dev).cpu(), O.full_adjacency(n))


# ---- add_edges / edge_sampling on a model ---------------------------------------------------------------------------------------
def ready_model(dev, **over):
  """Model in eval mode after one plain solve, so that odefunc.attention_weights belongs to odefunc.edge_index."""
  model, data, opt = O.make_model(dev, **over)
  model.eval()
  with torch.no_grad():
    model.odeblock.set_x0(model.forward_encoder(data.x, None))
    model.odeblock(model.forward_encoder(data.x, None))
  return model, data, opt


def test_add_edges_random(dev):
  model, data, opt = ready_model(dev)
  first = model.odeblock.odefunc.edge_index
  M = int(first.shape[1] * 0.64)
  got = GR.add_edges(model, opt)
  want = O.edge_union(first.cpu(), O.random_pairs(O.N, M, O.SAMPLING_SEED, 0))
  assert torch.equal(got.cpu(), want)
  # the second call of the same model takes call number 1
  assert torch.equal(GR.add_edges(model, opt).cpu(), O.edge_union(first.cpu(), O.random_pairs(O.N, M, O.SAMPLING_SEED, 1)))
  assert model.odeblock.odefunc.edge_index is first


def test_add_edges_importance(dev):
  model, data, opt = ready_model(dev, edge_sampling_add_type='importance')
  f = model.odeblock.odefunc
  first = f.edge_index
  M = int(first.shape[1] * 0.64)
  got = GR.add_edges(model, opt)
  # the same pairs, drawn again through the primitives: M anchors from softmax(importance), M uniform partners
  att_mean = f.attention_weights.mean(dim=1)
  importance = G.ops.node_importance(first, att_mean, O.N)
  anchors = G.ops.sample_nodes(importance, M, O.SAMPLING_SEED, 0, 0)
  partners = G.ops.random_nodes(O.N, M, O.SAMPLING_SEED, 1, 0, device=dev)
  assert anchors.shape == (M,) and torch.equal(partners.cpu(), O.random_nodes(O.N, M, O.SAMPLING_SEED, 1, 0))
  assert torch.equal(got.cpu(), O.edge_union(first.cpu(), O.both_directions(anchors.cpu(), partners.cpu())))
  # the anchors against the oracle's importance (float64) under the band widened by the importance's own fp32 error
  want_imp, deg = O.node_importance(first.cpu(), att_mean.cpu(), O.N)
  imp_err = ((deg + 1) * 2.0 ** -24 * want_imp).numpy()
  assert bool(((importance.cpu().double() - want_imp).abs().numpy() <= imp_err).all())
  band = O.Band(want_imp.float().numpy(), M, O.SAMPLING_SEED, 0, 0, logit_err=imp_err + 2.0 ** -24 * want_imp.numpy())
  band.check(anchors)


def test_add_edges_importance_without_new_edges_and_n2_radius(dev):
  model, data, opt = ready_model(dev, edge_sampling_add_type='importance', edge_sampling_add=0.0)
  assert GR.add_edges(model, opt) is model.odeblock.odefunc.edge_index
  opt['edge_sampling_add_type'] = 'n2_radius'
  full = GR.add_edges(model, opt)
  assert full.shape == (2, 9216) and torch.equal(full.cpu(), O.full_adjacency(O.N))


@pytest.mark.parametrize('sym', [False, True])
def test_edge_sampling_keeps_the_oracles_set(dev, sym):
  model, data, opt = ready_model(dev, edge_sampling_rmv=0.32, edge_sampling_sym=sym)
  first = model.odeblock.odefunc.edge_index
  added = GR.add_edges(model, opt)
  with torch.no_grad():
    z = model.odeblock(model.forward_encoder(data.x, None))
  res = O.restated_forward(model, data.x, first, added)
  assert_parity(z, res['z'], what='first solve')
  GR.set_edge_index(model, added)
  kept = GR.edge_sampling(model, z, opt)
  assert model.odeblock.odefunc.edge_index is kept and model.odeblock.reg_odefunc.odefunc.edge_index is kept
  assert torch.equal(kept.cpu(), res['edge'])
  assert kept.shape[1] < added.shape[1] or sym


# ---- GNN_FA end to end ----------------------------------------------------------------------------------------------------------
def forward_with_added_edges(model, x):
  """(output, the edge set add_edges returned during this forward)."""
  seen = []
  real = GR.add_edges

  def spy(m, opt):
    seen.append(real(m, opt))
    return seen[-1]
  GR.add_edges = spy
  try:
    with torch.no_grad():
      out = model(x, None)
  finally:
    GR.add_edges = real
  return out, seen[0]


@pytest.mark.parametrize('function', ['laplacian', 'transformer'])
@pytest.mark.parametrize('rmv', [0.0, 0.32])
def test_gnn_fa_matches_the_restated_model(dev, function, rmv):
  seed = O.E2E_SEEDS[function]        # (the CPU file asserts the threshold's clearance for exactly this configuration)
  model, data, opt = O.make_model(dev, function=function, edge_sampling_rmv=rmv, edge_sampling_seed=seed, **O.E2E_FIRST_SOLVE)
  model.eval()
  first = model.odeblock.odefunc.edge_index
  out, added = forward_with_added_edges(model, data.x)
  M = int(first.shape[1] * 0.64)
  assert torch.equal(added.cpu(), O.edge_union(first.cpu(), O.random_pairs(O.N, M, seed, 0)))
  res = O.restated_forward(model, data.x, first, added)
  assert_parity(out, res['out'], what='GNN_FA output')
  # the function is back in the state of the first solve, whatever the mode
  assert model.odeblock.odefunc.attention_weights.shape[0] == first.shape[1]
  # the second solve really ran rk4 with step 1 on the other edge set: the plain model gives something else
  opt['fa_layer'] = False
  with torch.no_grad():
    plain = model(data.x, None)
  opt['fa_layer'] = True
  assert not torch.allclose(plain, out, rtol=1e-3, atol=1e-3)
  assert model.odeblock.odefunc.edge_index is model.data_edge_index
  assert model.odeblock.reg_odefunc.odefunc.edge_index is model.data_edge_index
  assert (opt['time'], opt['method'], opt['step_size']) == (2.0, 'euler', 0.5)


def test_gnn_fa_restores_after_a_failure(dev):
  model, data, opt = O.make_model(dev, time=2.0, step_size=0.5, method='euler')
  model.eval()
  opt['edge_sampling_rmv'] = 0.32
  opt['edge_sampling_space'] = 'z_distance'
  with pytest.raises(NotImplementedError, match='z_distance'):
    with torch.no_grad():
      model(data.x, None)
  assert (opt['time'], opt['method'], opt['step_size']) == (2.0, 'euler', 0.5)
  opt['edge_sampling_space'] = 'attention'
  opt['edge_sampling_add_type'] = 'degree'
  with pytest.raises(NotImplementedError, match='degree'):
    with torch.no_grad():
      model.forward_ODE(data.x, None)
  assert model.odeblock.odefunc.edge_index is model.data_edge_index
  assert (opt['time'], opt['method'], opt['step_size']) == (2.0, 'euler', 0.5)


def test_gnn_fa_is_reproducible_call_by_call(dev):
  a, data, _ = O.make_model(dev, edge_sampling_rmv=0.32)
  b, _, _ = O.make_model(dev, edge_sampling_rmv=0.32)
  a.eval(), b.eval()
  out_a1, added_a1 = forward_with_added_edges(a, data.x)
  out_b1, added_b1 = forward_with_added_edges(b, data.x)
  assert torch.equal(out_a1, out_b1) and torch.equal(added_a1, added_b1)
  out_a2, added_a2 = forward_with_added_edges(a, data.x)
  assert added_a2.shape != added_a1.shape or not torch.equal(added_a2, added_a1)
  a._edge_sampling_state['call'] = 1
  out_a3, added_a3 = forward_with_added_edges(a, data.x)
  assert torch.equal(added_a3, added_a2) and torch.equal(out_a3, out_a2)


def test_gnn_fa_n2_radius_with_removal(dev):
  model, data, opt = O.make_model(dev, edge_sampling_add_type='n2_radius', edge_sampling_rmv=0.8)
  model.eval()
  out, added = forward_with_added_edges(model, data.x)
  assert added.shape == (2, O.N * O.N) and out.shape == (O.N, O.CLASSES) and bool(torch.isfinite(out).all())
  assert model.odeblock.odefunc.edge_index is model.data_edge_index


def test_gnn_fa_training_step(dev):
  model, data, opt = O.make_model(dev, edge_sampling_rmv=0.32, edge_sampling_add_type='importance')
  model.train()
  out = model(data.x, None)
  y = torch.randint(0, O.CLASSES, (O.N,), generator=torch.Generator().manual_seed(1)).to(dev)
  torch.nn.CrossEntropyLoss()(out, y).backward()
  for name, p in model.named_parameters():
    if p.grad is not None:
      assert bool(torch.isfinite(p.grad).all()), name + ': non-finite gradient'
  q = model.odeblock.multihead_att_layer.Q.weight
  assert q.grad is not None and float(q.grad.abs().max()) > 0
  assert model.m1.weight.grad is not None and float(model.m1.weight.grad.abs().max()) > 0
  assert model.odeblock.odefunc.edge_index is model.data_edge_index


@pytest.mark.parametrize('function', ['laplacian', 'transformer'])
def test_without_fa_layer_gnn_fa_is_gnn_knn(dev, function):
  fa, data, _ = O.make_model(dev, function=function, fa_layer=False)
  knn, _, _ = O.make_model(dev, cls=G.GNN_KNN, function=function, fa_layer=False)
  fa.eval(), knn.eval()
  with torch.no_grad():
    assert torch.equal(fa(data.x, None), knn(data.x, None))
    assert torch.equal(fa.forward_ODE(data.x, None), knn.forward_ODE(data.x, None))
