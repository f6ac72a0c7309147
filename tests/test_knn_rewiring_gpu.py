"""BLEND's k-nearest-neighbour rewiring on the device: graph_rewiring.KNN / apply_KNN over GNN_KNN, and the rewiring step end to
end -- the solve that follows `odefunc.edge_index = apply_KNN(...)` against the oracle on that same edge set."""
import pytest
import torch

import gnpde_amd as G
from gnpde_amd.graph_rewiring import KNN, apply_KNN
from oracle import restate as R
from helpers import Data, Fixture, assert_parity, random_graph
import knn_oracle as O

pytestmark = pytest.mark.gpu

N, FEAT, HIDDEN, CLASSES, K = 200, 24, 16, 5, 8


def knn_opt(T='raw', sym=False, k=K):
  return {'rewire_KNN_k': k, 'rewire_KNN_T': T, 'rewire_KNN_sym': sym}


def test_knn_layout(dev):
  x, _, order = O.integer_order(257, 4, 77)
  k = 16
  ei = KNN(x.to(dev), knn_opt(k=k))
  assert ei.shape == (2, 257 * k) and ei.dtype == torch.int64
  assert torch.equal(ei[0].cpu(), torch.arange(257).repeat_interleave(k))
  assert torch.equal(ei[1], G.ops.knn(x.to(dev), k).reshape(-1))
  assert torch.equal(ei[1].cpu().reshape(257, k), order[:, :k])


def test_knn_symmetrised(dev):
  """rewire_KNN_sym: both directions, no duplicates, sorted by (row, col) -- the set PyG's to_undirected returns."""
  x, _, order = O.integer_order(257, 4, 77)
  k = 16
  ei = KNN(x.to(dev), knn_opt(k=k, sym=True)).cpu()
  pairs = {(i, int(j)) for i in range(257) for j in order[i, :k]}
  want = sorted(pairs | {(j, i) for i, j in pairs})
  assert [tuple(c) for c in ei.t().tolist()] == want


def make_model(dev, **over):
  opt = dict(Fixture('gnn_constant_transformer_rk4').opt)
  opt.update(hidden_dim=HIDDEN, attention_dim=16, heads=4, function='transformer', block='constant', method='rk4',
             step_size=1.0, time=2.0, input_dropout=0.5, dropout=0.5)
  opt.update(over)
  g = torch.Generator().manual_seed(5)
  x = torch.randn(N, FEAT, generator=g)
  data = Data(x.to(dev), random_graph(N, 4, seed=5).to(dev))
  model = G.GNN_KNN(opt, G.DummyDataset(data, CLASSES), dev).to(dev)
  with torch.no_grad():
    for p in model.parameters():
      if p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
  return model, data, opt


@pytest.mark.parametrize('T', ['raw', 'T0', 'TN'])
def test_apply_knn_searches_the_matching_tensor(dev, T):
  model, data, opt = make_model(dev)
  model.eval()
  with torch.no_grad():
    searched = {'raw': lambda: data.x, 'T0': lambda: model.forward_encoder(data.x, None),
                'TN': lambda: model.forward_ODE(data.x, None)}[T]()
  assert searched.shape == (N, FEAT if T == 'raw' else HIDDEN)
  ei = apply_KNN(data, None, model, knn_opt(T))
  assert ei.shape == (2, N * K) and torch.equal(ei[0].cpu(), torch.arange(N).repeat_interleave(K))
  band = O.Band(searched.cpu(), K)
  assert band.undetermined() <= O.CAP_SHARE * N * K
  band.check(ei[1].reshape(N, K))
  with pytest.raises(Exception, match='rewire_KNN_T'):
    apply_KNN(data, None, model, knn_opt('elsewhere'))


def test_forward_encoder_has_no_dropout(dev):
  model, data, opt = make_model(dev, use_mlp=True)
  with torch.no_grad():
    model.train()
    a, b = model.forward_encoder(data.x, None), model.forward_encoder(data.x, None)
    model.eval()
    c = model.forward_encoder(data.x, None)
  assert torch.equal(a, b) and torch.equal(a, c)
  # the parent's encoder does drop in training mode: the two are different functions there
  model.train()
  with torch.no_grad():
    assert not torch.equal(model.encode(data.x, None), a)


def test_forward_ode_splits_the_augmented_state(dev):
  model, data, opt = make_model(dev, augment=True)
  model.eval()
  with torch.no_grad():
    assert model.forward_encoder(data.x, None).shape == (N, 2 * HIDDEN)
    assert model.forward_ODE(data.x, None).shape == (N, HIDDEN)


def test_rewiring_step_end_to_end(dev):
  """`odefunc.edge_index = apply_KNN(...)`: the next solve runs on the new edge set (oracle rk4 over the oracle right-hand
  side on that edge set, the block tests' tolerance), and a training step afterwards has finite gradients."""
  model, data, opt = make_model(dev)
  model.eval()
  with torch.no_grad():
    z_before = model.forward_ODE(data.x, None)
  ei = apply_KNN(data, None, model, knn_opt('T0'))
  model.odeblock.odefunc.edge_index = ei
  with torch.no_grad():
    x0 = model.forward_encoder(data.x, None)
    z = model.forward_ODE(data.x, None)
  assert not torch.equal(z, z_before)
  f = model.odeblock.odefunc
  lay = f.multihead_att_layer
  cpu = lambda t: t.detach().cpu()
  assert torch.equal(cpu(f.edge_index), cpu(ei))
  x0c = cpu(x0)
  rhs = lambda t, y: R.rhs_transformer(y, cpu(ei), cpu(lay.Q.weight), cpu(lay.Q.bias), cpu(lay.K.weight), cpu(lay.K.bias),
                                       opt['heads'], cpu(f.alpha_train), cpu(f.beta_train), x0c, False, True)
  ref = R.odeint_fixed(rhs, x0c, opt['time'], opt['step_size'], 'rk4')
  assert_parity(z, ref, what='solve on the rewired edge set')

  model.train()
  out = model(data.x, None)
  y = torch.randint(0, CLASSES, (N,), generator=torch.Generator().manual_seed(1)).to(dev)
  torch.nn.CrossEntropyLoss()(out, y).backward()
  with_grad = {name for name, p in model.named_parameters() if p.grad is not None}
  for name in ('m1.weight', 'm2.weight', 'odeblock.odefunc.multihead_att_layer.Q.weight',
               'odeblock.odefunc.multihead_att_layer.K.weight', 'odeblock.odefunc.alpha_train', 'odeblock.odefunc.beta_train'):
    assert name in with_grad, name + ' got no gradient'
  for name, p in model.named_parameters():
    if p.grad is not None:
      assert bool(torch.isfinite(p.grad).all()), name + ': non-finite gradient'
  assert float(model.odeblock.odefunc.multihead_att_layer.Q.weight.grad.abs().max()) > 0


def test_fa_layer_is_refused(dev):
  with pytest.raises(NotImplementedError, match='fa_layer'):
    make_model(dev, fa_layer=True)
  model, data, opt = make_model(dev)
  model.opt['fa_layer'] = True
  with pytest.raises(NotImplementedError, match='fa_layer'):
    model.forward_ODE(data.x, None)
  with pytest.raises(NotImplementedError, match='fa_layer'):
    model(data.x, None)
