"""Native attention backward for every head width and head count: the generic head-SpMM (gnpde_head_spmm for d_k not a multiple
of 4, attention_dim / 4 not a power of two, unaligned operands) and the training paths it opens -- the attention a block computes
once per forward pass, one evaluation of GRAND-nl, GAT with any head count (mix_features included) and the native VJP stage of
scaled-dot GRAND-nl.  References: float64 index_add_ / autograd through the oracle."""
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import autograd as AG
from gnpde_amd import ops
from gnpde_amd.graph import graph_of
from oracle import restate as R
from helpers import Data, assert_parity, random_graph
import test_adjoint_gpu as TA

pytestmark = pytest.mark.gpu

OPT = dict(heads=4, attention_dim=16, attention_type='scaled_dot', attention_norm_idx=0, square_plus=False,
           reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9,
           add_source=True, no_alpha_sigmoid=False, mix_features=False, hidden_dim=20, augment=False, adjoint=False,
           tol_scale=1.0, data_norm='rw', method='rk4', step_size=1.0, max_iters=100, block='constant',
           function='transformer', time=2.0)


def _rand_params(mod, seed, dev):
  g = torch.Generator().manual_seed(seed)
  with torch.no_grad():
    for p in mod.parameters():
      if p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      else:
        p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(dev))


def _grad_close(name, got, ref64, ref32, scale=None):
  """Within 3x the CPU fp32 error of the same op sequence, or 3e-5 relative (the rule of test_autograd_gpu.py)."""
  scale = float(ref64.abs().max()) if scale is None else scale
  e_gpu = float((got.detach().cpu().double().reshape(ref64.shape) - ref64).abs().max()) / scale
  e_cpu = float((ref32.double() - ref64).abs().max()) / scale
  assert e_gpu <= max(3 * e_cpu, 3e-5), '%s: GPU error %.2e vs float64, CPU fp32 error %.2e' % (name, e_gpu, e_cpu)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 2), (8, 1), (3, 3), (2, 5), (1, 6), (3, 4), (5, 8), (1, 24), (8, 30), (1, 1)]


@pytest.mark.parametrize('unaligned', [False, True])
@pytest.mark.parametrize('by_column', [False, True])
@pytest.mark.parametrize('h,dk', SHAPES)
def test_head_spmm_any_head_shape(dev, h, dk, by_column, unaligned):
  """out[i, c] = scale sum_{p in segment i} ds[p, c // d_k] feat[other end of p, c] against float64 index_add_, on a graph with
  hub rows and columns (> GNPDE_LONG_ROW entries), duplicates and isolated nodes; feat as the k half of a q||k table (unaligned
  when A is odd) and out as a column slice; empty segments come out as zero rows; two launches agree bit for bit."""
  n, A = 900, h * dk
  ei = random_graph(n, 5, seed=61, hubs=2, hub_deg=1300, isolated=7, dup=30).to(dev)
  graph = graph_of(ei, n, dev)
  g = torch.Generator().manual_seed(62)
  ds = torch.randn(graph.e, h, generator=g).to(dev)
  if unaligned:      # the k half of q||k at an odd offset, out one column into a wider table
    qk = torch.randn(n, 2 * A + 1, generator=g).to(dev)
    feat = qk[:, A + 1:]
    big = torch.full((n, A + 3), float('nan'), device=dev)
    out = big[:, 1:A + 1]
  else:
    qk = torch.randn(n, 2 * A, generator=g).to(dev)
    feat = qk[:, A:]
    big = torch.full((n, A), float('nan'), device=dev)
    out = big
  scale = 0.37
  ops.head_spmm(graph, ds, feat, h, dk, scale, by_column=by_column, out=out)
  torch.cuda.synchronize()
  # float64 reference in CSR order
  rowptr = graph.t['rowptr'][:n + 1].long().cpu()
  col = graph.t['colidx'][:graph.e].long().cpu()
  row = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
  seg, other = (col, row) if by_column else (row, col)
  head = torch.arange(A) // dk
  contrib = ds.cpu().double()[:, head] * feat.cpu().double()[other]
  ref = scale * torch.zeros(n, A, dtype=torch.float64).index_add_(0, seg, contrib)
  got = out.cpu().double()
  assert torch.isfinite(got).all(), 'a row was not written'
  err = float((got - ref).abs().max()) / float(ref.abs().max())
  assert err <= 1e-5, 'h=%d d_k=%d: relative error %.2e' % (h, dk, err)
  empty = torch.bincount(seg, minlength=n) == 0
  assert int(empty.sum()) >= 7 and float(got[empty].abs().max()) == 0.0
  if unaligned:      # the columns around the slice are untouched
    assert torch.isnan(big[:, 0]).all() and torch.isnan(big[:, A + 1:]).all()
  again = torch.empty_like(out)
  ops.head_spmm(graph, ds, feat, h, dk, scale, by_column=by_column, out=again)
  assert torch.equal(again, out), 'two launches differ'


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the best_params CoauthorCS block (attention block, A = 8, 4 heads: d_k = 2)
# ------------------------------------------------------------------------------------------------------------------------------
def test_coauthorcs_fixture_without_composite(dev):
  """The assertions of test_adjoint_gpu.py for the CoauthorCS fixture (output, every parameter gradient against the reference,
  evaluations, the native adaptive adjoint ran), and no composite backward announced itself."""
  AG._warned.clear()
  TA.test_block_adjoint_training(dev, 'adjoint_attention_laplacian_dopri5_dopri5_coauthorcs')
  assert not AG._warned, 'a composite backward announced itself: %s' % AG._warned


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the attention a block computes once per forward pass
# ------------------------------------------------------------------------------------------------------------------------------
COAUTHOR = dict(OPT, function='laplacian', block='attention', method='euler', time=2.0, square_plus=True, attention_norm_idx=1,
                self_loop_weight=0, add_source=False, hidden_dim=24)


@pytest.mark.parametrize('att_type', ['scaled_dot', 'cosine_sim', 'pearson', 'exp_kernel', 'blend'])
@pytest.mark.parametrize('h,A', [(4, 8), (3, 9)])
def test_layer_attention_any_head_shape(dev, h, A, att_type):
  """AttODEblock + Laplacian function at the CoauthorCS options (squareplus over columns): the attention carries gradients into the
  layer's parameters through the native per-edge VJP (no composite), against float64 autograd through the oracle."""
  n = 400
  split = att_type == 'blend'
  opt = dict(COAUTHOR, heads=h, attention_dim=A, attention_type='exp_kernel' if split else att_type)
  if split:
    f0, p0 = 16, 8
    opt.update(beltrami=True, feat_hidden_dim=f0, pos_enc_hidden_dim=p0)
  d = opt['hidden_dim']
  ei = random_graph(n, 6, seed=71, hubs=1, hub_deg=600, isolated=3)
  g = torch.Generator().manual_seed(72)
  x, c = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
  block = G.AttODEblock(G.LaplacianODEFunc, [], opt, Data(x.to(dev), ei.to(dev)), dev, t=torch.tensor([0, 2.0])).to(dev)
  _rand_params(block, 73, dev)
  lay = block.multihead_att_layer
  with torch.no_grad():
    for nm, v in (('lengthscale', 1.3), ('output_var', 0.8), ('lengthscale_x', 1.2), ('lengthscale_p', 0.9), ('output_var_x', 1.1),
                  ('output_var_p', 0.7)):
      if hasattr(lay, nm):
        getattr(lay, nm).fill_(v)
  assert AG._native_layer_vjp_ok(lay)
  block.train()
  AG._warned.clear()
  xd = x.to(dev).requires_grad_(True)
  block.set_x0(xd)
  z = block(xd)
  (z * c.to(dev)).sum().backward()
  assert not AG._warned, 'a composite backward announced itself: %s' % AG._warned
  f = block.odefunc
  e_n = f.edge_index.cpu()
  ew = f.edge_weight.cpu() if f.edge_weight is not None else None
  if split:
    names = [k for k, _ in lay.named_parameters() if k.split('.')[0] in ('Qx', 'Kx', 'Qp', 'Kp') or 'lengthscale' in k or 'output_var' in k]
  else:
    names = ['Q.weight', 'Q.bias', 'K.weight', 'K.bias'] + (['output_var', 'lengthscale'] if att_type == 'exp_kernel' else [])
  ours = [dict(lay.named_parameters())[k] for k in names]

  def reference(dtype):
    cast = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)   # noqa: E731
    xc = cast(x)
    P = {k: cast(p) for k, p in zip(names, ours)}
    al, be = cast(f.alpha_train), cast(f.beta_train)
    kw = dict(norm_idx=1, square_plus=True, edge_weights=ew.to(dtype) if ew is not None else None, reweight=False)
    if split:
      att, _ = R.transformer_attention_split(xc, e_n, P, h, f0, p0, **kw)
    else:
      if att_type == 'exp_kernel':
        kw.update(output_var=P['output_var'], lengthscale=P['lengthscale'])
      att, _ = R.transformer_attention(xc, e_n, P['Q.weight'], P['Q.bias'], P['K.weight'], P['K.bias'], h, attention_type=att_type, **kw)
    rhs = lambda t, y: R.rhs_from_attention(y, e_n, att, al, be, None, False, False)   # noqa: E731
    zr = R.odeint_fixed(rhs, xc, 2.0, 1.0, 'euler')
    (zr * c.to(dtype)).sum().backward()
    return zr.detach(), [xc.grad] + [P[k].grad for k in names]

  z64, g64 = reference(torch.float64)
  z32, g32 = reference(torch.float32)
  assert_parity(z, z64.float(), what='z')
  dxscale = float(g64[0].abs().max())
  wscale = max(float(t.abs().max()) for t in g64[1:] if t.dim() >= 2)
  for name, a, b32, b64 in zip(['dx'] + names, [xd.grad] + [p.grad for p in ours], g32, g64):
    assert a is not None, name
    if name != 'dx' and wscale < 1e-10 * dxscale:
      # pearson at d_k = 2: a centred pair is +-(a, -a), the cosine of two of them is +-1 and the weight gradients vanish
      # identically -- rounding noise on both sides, bounded against the scale of d x
      assert float(a.abs().max()) <= 1e-4 * dxscale, name
      continue
    _grad_close(name, a, b64, b32, None if (name == 'dx' or b64.numel() == 1) else wscale)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. GRAND-nl: one evaluation of f and its backward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('square_plus,norm_idx', [(False, 0), (True, 0), (False, 1), (True, 1)])
@pytest.mark.parametrize('h,A', [(4, 8), (3, 9), (2, 10), (3, 12), (1, 6)])
def test_grand_nl_vjp_any_head_shape(dev, h, A, square_plus, norm_idx):
  n, d = 400, 24
  ei = random_graph(n, 6, seed=81, hubs=1, hub_deg=700, isolated=3)
  g = torch.Generator().manual_seed(82)
  x, go = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
  opt = dict(OPT, hidden_dim=d, heads=h, attention_dim=A, attention_norm_idx=norm_idx, square_plus=square_plus)
  func = G.ODEFuncTransformerAtt(d, d, opt, Data(x.to(dev), ei.to(dev)), dev).to(dev)
  _rand_params(func, 83, dev)
  assert AG._native_transformer_vjp_ok(func)
  lay = func.multihead_att_layer
  AG._warned.clear()
  xd = x.to(dev).requires_grad_(True)
  func.x0 = x.to(dev)
  f = func(0.0, xd)
  f.backward(go.to(dev))
  assert not AG._warned, 'a composite backward announced itself: %s' % AG._warned
  edge = func.edge_index.cpu()
  ours = [lay.Q.weight, lay.Q.bias, lay.K.weight, lay.K.bias, func.alpha_train, func.beta_train]

  def reference(dtype):
    cast = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)   # noqa: E731
    xc = cast(x)
    ps = [cast(p) for p in ours]
    fr = R.rhs_transformer(xc, edge, ps[0], ps[1], ps[2], ps[3], h, ps[4], ps[5], x.to(dtype), False, True, norm_idx=norm_idx,
                           square_plus=square_plus)
    fr.backward(go.to(dtype))
    return fr.detach(), [xc.grad] + [p.grad for p in ps]

  f64, g64 = reference(torch.float64)
  f32, g32 = reference(torch.float32)
  assert_parity(f, f64.float(), what='f')
  scale = max(float(t.abs().max()) for t in g64[1:5])
  names = ['dx', 'dWq', 'dbq', 'dWk', 'dbk', 'dalpha', 'dbeta']
  for name, a, b32, b64 in zip(names, [xd.grad] + [p.grad for p in ours], g32, g64):
    _grad_close(name, a, b64, b32, None if name in ('dx', 'dalpha', 'dbeta') else scale)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. GAT with a head count that is not a power of two
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mix', [False, True])
@pytest.mark.parametrize('h', [3, 5, 6])
def test_gat_vjp_any_head_count(dev, h, mix):
  n, d = 300, 16
  ei = random_graph(n, 6, seed=91, hubs=1, hub_deg=600, isolated=3)
  g = torch.Generator().manual_seed(92)
  x, go = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
  A = 4 * h
  opt = dict(OPT, hidden_dim=d, function='GAT', mix_features=mix, attention_dim=A, heads=h)
  func = G.ODEFuncAtt(d, d, opt, Data(x.to(dev), ei.to(dev)), dev).to(dev)
  _rand_params(func, 93, dev)
  lay = func.multihead_att_layer
  AG._warned.clear()
  xd = x.to(dev).requires_grad_(True)
  func.x0 = x.to(dev)
  f = func(0.0, xd)
  f.backward(go.to(dev))
  assert not AG._warned, 'a composite backward announced itself: %s' % AG._warned
  edge = func.edge_index.cpu()
  ours = [lay.W, lay.a] + ([lay.Wout] if mix else []) + [func.alpha_train, func.beta_train]

  def reference(dtype):
    cast = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)   # noqa: E731
    xc = cast(x)
    ps = [cast(p) for p in ours]
    if not mix:
      fr = R.rhs_gat(xc, edge, ps[0], ps[1], h, ps[-2], ps[-1], x.to(dtype), False, True, 0.2, 0)
    else:      # reference src/function_GAT_attention.py:33-38,56-64
      att, wx = R.gat_attention(xc, edge, ps[0], ps[1], h, 0.2, 0)
      ax = torch.mm(R.spmm(edge, att.mean(dim=1), n, wx), ps[2])
      fr = torch.sigmoid(ps[-2]) * (ax - xc) + ps[-1] * x.to(dtype)
    fr.backward(go.to(dtype))
    return fr.detach(), [xc.grad] + [p.grad for p in ps]

  f64, g64 = reference(torch.float64)
  f32, g32 = reference(torch.float32)
  assert_parity(f, f64.float(), what='f')
  for name, a, b32, b64 in zip(['dx', 'dW', 'da'] + (['dWout'] if mix else []) + ['dalpha', 'dbeta'],
                               [xd.grad] + [p.grad for p in ours], g32, g64):
    _grad_close(name, a, b64, b32)


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the native VJP stage of scaled-dot GRAND-nl at these shapes
# ------------------------------------------------------------------------------------------------------------------------------
def _train(dev, opt, ei, x, c):
  block = G.ConstantODEblock(G.ODEFuncTransformerAtt, [], opt, Data(x, ei), dev, t=torch.tensor([0, opt['time']])).to(dev)
  _rand_params(block, 101, dev)
  with torch.no_grad():
    block.odefunc.alpha_train.fill_(0.3)
    block.odefunc.beta_train.fill_(0.2)
  block.train()
  xin = x.clone().requires_grad_(True)
  block.set_x0(xin)
  z = block(xin)
  (z * c).sum().backward()
  grads = {k: p.grad.detach().clone() for k, p in block.named_parameters() if p.grad is not None}
  return block, z.detach(), xin.grad.detach().clone(), grads


def _compare(tag, gx_a, gp_a, gx_b, gp_b):
  tol = 2e-4
  assert_parity(gx_a, gx_b, tol, tag + ' grad_x')
  assert set(gp_a) == set(gp_b)
  scale = max(float(v.abs().max()) for v in gp_b.values())
  for k in sorted(gp_b):
    if float(gp_b[k].abs().max()) < 1e-5 * max(scale, 1.0):      # mathematically zero (a row softmax does not see the key bias)
      assert float(gp_a[k].abs().max()) < 1e-4 * max(scale, 1.0), k
    else:
      assert_parity(gp_a[k], gp_b[k], tol, tag + ' ' + k)


@pytest.mark.parametrize('h,A', [(4, 8), (8, 8), (3, 12)])
def test_stage_recorded_fixed_grid_any_dk(dev, h, A):
  """rk4 training with the adjoint off: the recorded native solve + native reverse sweep, against the host loop and float64."""
  n, d, T = 700, 24, 2.0
  opt = dict(OPT, hidden_dim=d, heads=h, attention_dim=A, time=T)
  ei = random_graph(n, 6, seed=111, hubs=2, hub_deg=700, isolated=3, dup=20).to(dev)
  x = (0.5 * torch.randn(n, d, generator=torch.Generator().manual_seed(112))).to(dev)
  c = torch.randn(n, d, generator=torch.Generator().manual_seed(113)).to(dev)
  AG._warned.clear()
  blk_n, z_n, gx_n, gp_n = _train(dev, opt, ei, x, c)
  assert blk_n.odefunc._last_train_solve.startswith('native recorded fixed-grid'), blk_n.odefunc._last_train_solve
  blk_h, z_h, gx_h, gp_h = _train(dev, dict(opt, gnpde_host_fixed_training=True), ei, x, c)
  host_solve = blk_h.odefunc.__dict__.get('_last_train_solve', 'differentiable host loop')
  assert not host_solve.startswith('native recorded'), host_solve
  assert not AG._warned, 'a composite backward announced itself: %s' % AG._warned
  assert blk_n.odefunc.nfe == blk_h.odefunc.nfe
  assert_parity(z_n, z_h, 1e-5, 'z')
  _compare('recorded vs host loop', gx_n, gp_n, gx_h, gp_h)
  # float64 autograd through the oracle's rk4
  f = blk_n.odefunc
  lay = f.multihead_att_layer
  edge = f.edge_index.cpu()
  keys = ['odefunc.multihead_att_layer.Q.weight', 'odefunc.multihead_att_layer.Q.bias', 'odefunc.multihead_att_layer.K.weight',
          'odefunc.multihead_att_layer.K.bias', 'odefunc.alpha_train', 'odefunc.beta_train']
  params = dict(blk_n.named_parameters())

  def reference(dtype):
    cast = lambda t: t.detach().cpu().to(dtype).clone().requires_grad_(True)   # noqa: E731
    xc = cast(x)
    ps = [cast(params[k]) for k in keys]
    x0 = x.cpu().to(dtype)                               # ODEblock.set_x0 detaches the source term
    rhs = lambda t, y: R.rhs_transformer(y, edge, ps[0], ps[1], ps[2], ps[3], h, ps[4], ps[5], x0, False, True)   # noqa: E731
    zr = R.odeint_fixed(rhs, xc, T, 1.0, 'rk4')
    (zr * c.cpu().to(dtype)).sum().backward()
    return [xc.grad] + [p.grad for p in ps]

  g64, g32 = reference(torch.float64), reference(torch.float32)
  scale = max(float(t.abs().max()) for t in g64[1:5])
  for name, a, b32, b64 in zip(['dx'] + keys, [gx_n] + [gp_n.get(k, torch.zeros_like(params[k])) for k in keys], g32, g64):
    own = name == 'dx' or 'alpha' in name or 'beta' in name
    _grad_close(name, a, b64, b32, None if own else scale)
  assert lay.h == h


@pytest.mark.parametrize('h,A', [(4, 8), (8, 8), (3, 12)])
def test_stage_native_adjoint_any_dk(dev, h, A):
  """adjoint=True with a fixed-grid adjoint method: the native adjoint solve, against the stage-by-stage loop."""
  n, d = 700, 24
  opt = dict(OPT, hidden_dim=d, heads=h, attention_dim=A, adjoint=True, adjoint_method='rk4', adjoint_step_size=1.0,
             tol_scale_adjoint=1.0, att_samp_pct=1.0, use_flux=False, time=3.0)
  ei = random_graph(n, 6, seed=121, hubs=2, hub_deg=700, isolated=3, dup=20).to(dev)
  x = (0.5 * torch.randn(n, d, generator=torch.Generator().manual_seed(122))).to(dev)
  c = torch.randn(n, d, generator=torch.Generator().manual_seed(123)).to(dev)
  AG._warned.clear()
  blk_n, z_n, gx_n, gp_n = _train(dev, opt, ei, x, c)
  assert blk_n.odefunc.__dict__.get('_adjoint_state'), 'the native adjoint did not run'
  blk_h, z_h, gx_h, gp_h = _train(dev, dict(opt, gnpde_host_adjoint=True), ei, x, c)
  assert not blk_h.odefunc.__dict__.get('_adjoint_state')
  assert not AG._warned, 'a composite backward announced itself: %s' % AG._warned
  assert blk_n.odefunc.nfe == blk_h.odefunc.nfe
  assert torch.equal(z_n, z_h)
  _compare('native adjoint vs stage loop', gx_n, gp_n, gx_h, gp_h)
