"""The BLEND split kernel (`--beltrami --function transformer --attention_type exp_kernel`: reference
src/function_transformer_attention.py:133-171, evaluated at every right-hand-side evaluation) on the native VJP stage of
csrc/adjoint.hip -- the recorded fixed-grid reverse sweep and the native adjoint solve -- up to kernel width 256, and the plain exp
kernel up to attention_dim 256:
  * gnpde_split_kernel_grads alone against a float64 restatement of the chain rule (bounds derived from the magnitudes),
  * the recorded solve against the differentiable host loop (opt['gnpde_host_fixed_training']) on the same block,
  * both against float64 autograd through the oracle's split attention in a fixed-grid loop written here,
  * the native adjoint solve against the stage loop (opt['gnpde_host_adjoint']),
  * an optimiser-style update between forward and backward."""
import math

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib
from oracle import restate as R
from helpers import Data, assert_parity, random_graph

pytestmark = pytest.mark.gpu

OPT = dict(heads=2, attention_dim=16, attention_type='exp_kernel', attention_norm_idx=0, square_plus=False, reweight_attention=False,
           beltrami=True, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9, add_source=True, no_alpha_sigmoid=False,
           mix_features=False, hidden_dim=20, augment=False, adjoint=False, adjoint_method='rk4', adjoint_step_size=1.0, tol_scale=1.0,
           tol_scale_adjoint=1.0, data_norm='rw', method='rk4', step_size=1.0, max_iters=100, block='constant', function='transformer',
           time=2.0, att_samp_pct=1.0, use_flux=False)
SPLIT_NAMES = ['Qx.weight', 'Qx.bias', 'Kx.weight', 'Kx.bias', 'Qp.weight', 'Qp.bias', 'Kp.weight', 'Kp.bias',
               'lengthscale_x', 'lengthscale_p', 'output_var_x', 'output_var_p']
SCALARS = dict(lengthscale_x=1.7, lengthscale_p=1.5, output_var_x=1.1, output_var_p=0.9)      # typical scores 1e-3 (d_k = 8) .. 1e-6 (d_k = 16): none underflows


def _module_scaled(grads, refs, tol, what):
  """Every gradient within tol of the largest reference gradient of its module (as tests/test_tape_gpu.py: a gradient that is zero in
  exact arithmetic -- a key bias under a softmax over rows -- is rounding noise on both sides)."""
  scale = {}
  for k, ref in refs.items():
    mod = k.rsplit('.', 2)[0] if 'multihead' in k else k
    scale[mod] = max(scale.get(mod, 0.0), float(ref.abs().max()))
  for k, ref in refs.items():
    mod = k.rsplit('.', 2)[0] if 'multihead' in k else k
    got = grads[k]
    assert got is not None, '%s: %s received no gradient' % (what, k)
    err = float((got.detach().cpu().reshape(ref.shape) - ref.cpu()).abs().max())
    print('%s %s: abs err %.3e, module scale %.3e' % (what, k, err, scale[mod]))
    assert err <= tol * scale[mod], '%s %s: abs err %.3e against module scale %.3e (tol %.1e)' % (what, k, err, scale[mod], tol)


def _block(dev, n, d, heads, A, seed, method, time, step_size=1.0, hubs=0, hub_deg=0, f0=None, p0=None, **over):
  """A ConstantODEblock over ODEFuncTransformerAtt with random weights, built the way tests/test_tape_gpu.py::_fixed_block does; f0 / p0
  given: the BLEND split kernel (d - f0 - p0 label columns behind the positional block), else the plain exp kernel."""
  ei = random_graph(n, 5, seed=seed, hubs=hubs, hub_deg=hub_deg)
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, d, generator=g)
  opt = dict(OPT, hidden_dim=d, heads=heads, attention_dim=A, method=method, time=time, step_size=step_size, adjoint_step_size=step_size, **over)
  if f0 is None:
    opt['beltrami'] = False
  else:
    opt.update(beltrami=True, feat_hidden_dim=f0, pos_enc_hidden_dim=p0)
  block = G.ConstantODEblock(G.ODEFuncTransformerAtt, [], opt, Data(x.to(dev), ei.to(dev)), dev, t=torch.tensor([0, time])).to(dev)
  with torch.no_grad():
    for p in block.parameters():
      if p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      else:
        p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(dev))
    for f in (block.odefunc, block.reg_odefunc.odefunc):
      lay = f.multihead_att_layer
      if f0 is None:
        lay.lengthscale.fill_(1.7)
        lay.output_var.fill_(0.8)
      else:
        for nm, v in SCALARS.items():
          getattr(lay, nm).fill_(v)
  return block, x


def _train_once(block, x, dev, c, between=None):
  for p in block.parameters():
    p.grad = None
  block.train()
  xin = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xin)
  block.odefunc.nfe = 0
  block.odefunc._last_train_solve = ''     # (the host loop leaves the attribute alone)
  z = block(xin)
  if between is not None:
    between()
  (z * c).sum().backward()
  return z.detach(), xin.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in block.named_parameters()}, block.odefunc.nfe


def _set_host(block, key, value):
  block.odefunc.opt[key] = value
  block.reg_odefunc.odefunc.opt[key] = value


# ---- 1. the chain-rule entry alone ---------------------------------------------------------------------------------------------
def _cat_operands(h, dk, d, f0, p0, P, dtype):
  """Wcat [4A, d], bcat [4A] from the twelve parameters, the layout of SpGraphTransAttentionLayer._split_qk_weights restated."""
  A, lab = h * dk, f0 + p0
  W = torch.zeros(2, h, 2 * dk, d, dtype=dtype)
  b = torch.zeros(2, h, 2 * dk, dtype=dtype)
  for half, (nx, np_) in enumerate((('Qx', 'Qp'), ('Kx', 'Kp'))):
    wx = (P[nx + '.weight'].to(dtype) / P['lengthscale_x'].to(dtype)).view(h, dk, -1)
    wp = (P[np_ + '.weight'].to(dtype) / P['lengthscale_p'].to(dtype)).view(h, dk, -1)
    W[half, :, :dk, :f0] = wx[:, :, :f0]
    W[half, :, :dk, lab:] = wx[:, :, f0:]
    W[half, :, dk:, f0:lab] = wp
    b[half, :, :dk] = (P[nx + '.bias'].to(dtype) / P['lengthscale_x'].to(dtype)).view(h, dk)
    b[half, :, dk:] = (P[np_ + '.bias'].to(dtype) / P['lengthscale_p'].to(dtype)).view(h, dk)
  return W.reshape(4 * A, d), b.reshape(4 * A)


@pytest.mark.parametrize('h,dk,f0,p0,labels', [(2, 4, 5, 3, 2), (8, 16, 40, 24, 0)])
def test_split_kernel_grads_against_float64(dev, h, dk, f0, p0, labels):
  """The entry is a division per weight / bias, a double-precision sum per length scale and a product per output variance.  Bounds,
  from the magnitudes: a weight gradient is ONE float32 division of float32 operands (error <= 2^-24 |result|); a length-scale gradient
  is a sum carried in double (error ~ items * 2^-53, nothing at this scale), one double division and one rounding to float32 (error <=
  2^-24 |result| <= 2^-24 sum |dW| |W| / l); an output-variance gradient one float32 product.  4 ulp (2^-21) of the largest magnitude
  of each group is allowed: 8x the bound, so a wrong slot or a dropped term (each >= a whole entry) cannot hide."""
  A, d = h * dk, f0 + p0 + labels
  fx = d - p0
  g = torch.Generator().manual_seed(100 + h)
  P = {'Qx.weight': torch.randn(A, fx, generator=g), 'Kx.weight': torch.randn(A, fx, generator=g), 'Qp.weight': torch.randn(A, p0, generator=g),
       'Kp.weight': torch.randn(A, p0, generator=g)}
  for nm in ('Qx', 'Kx', 'Qp', 'Kp'):
    P[nm + '.bias'] = torch.randn(A, generator=g)
  P.update(lengthscale_x=torch.tensor([1.3]), lengthscale_p=torch.tensor([0.9]), output_var_x=torch.tensor([1.1]), output_var_p=torch.tensor([0.7]))
  wcat, bcat = _cat_operands(h, dk, d, f0, p0, P, torch.float32)
  assert int((wcat == 0).sum()) >= 4 * A * min(f0, p0)           # the structural zeros are there
  gcat = torch.randn(4 * A * d + 4 * A + 2, generator=g)          # dense: non-zero at the structural zeros of Wcat as well
  scal = torch.cat([P[k] for k in ('lengthscale_x', 'lengthscale_p', 'output_var_x', 'output_var_p')]).to(dev)
  L = G.lib()
  nf = L.gnpde_split_kernel_grad_floats(h, dk, d)
  assert nf == 2 * A * (d + 2) + 4
  out = torch.full((nf + 64,), float('nan'), device=dev)          # (the tail must stay untouched)
  gd, wd, bd = gcat.to(dev), wcat.to(dev), bcat.to(dev)
  _lib.check(L.gnpde_split_kernel_grads(_lib.ptr(gd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(scal[0:1]), _lib.ptr(scal[1:2]), _lib.ptr(scal[2:3]),
                                        _lib.ptr(scal[3:4]), h, dk, d, f0, p0, _lib.ptr(out), _lib.stream_of(out)))
  torch.cuda.synchronize()
  assert torch.isnan(out[nf:]).all() and torch.isfinite(out[:nf]).all()
  got = out[:nf].cpu().double()
  # float64 restatement: the gradient of <gcat, (Wcat, bcat, ov_x ov_p)> with respect to the twelve parameters
  f64 = torch.float64
  dW = gcat[:4 * A * d].to(f64).view(2, h, 2 * dk, d)
  db = gcat[4 * A * d:4 * A * d + 4 * A].to(f64).view(2, h, 2 * dk)
  dov = float(gcat[4 * A * d + 4 * A])
  lx, lp, ovx, ovp = (float(P[k]) for k in ('lengthscale_x', 'lengthscale_p', 'output_var_x', 'output_var_p'))
  W64, b64 = wcat.to(f64).view(2, h, 2 * dk, d), bcat.to(f64).view(2, h, 2 * dk)
  ref, mag = [], []
  for kind in ('x', 'p'):
    rows = slice(0, dk) if kind == 'x' else slice(dk, 2 * dk)
    l = lx if kind == 'x' else lp
    for half in (0, 1):
      gw = dW[half, :, rows, :]
      gw = torch.cat((gw[..., :f0], gw[..., f0 + p0:]), dim=-1) if kind == 'x' else gw[..., f0:f0 + p0]
      ref += [(gw / l).reshape(-1), (db[half, :, rows] / l).reshape(-1)]
      mag += [torch.full_like(ref[-2], float(dW.abs().max()) / l), torch.full_like(ref[-1], float(db.abs().max()) / l)]
  for kind in ('x', 'p'):
    rows = slice(0, dk) if kind == 'x' else slice(dk, 2 * dk)
    l = lx if kind == 'x' else lp
    s = (dW[:, :, rows, :] * W64[:, :, rows, :]).sum() + (db[:, :, rows] * b64[:, :, rows]).sum()
    sabs = (dW[:, :, rows, :] * W64[:, :, rows, :]).abs().sum() + (db[:, :, rows] * b64[:, :, rows]).abs().sum()
    ref.append((-s / l).reshape(1))
    mag.append((sabs / l).reshape(1))
  ref += [torch.tensor([dov * ovp], dtype=f64), torch.tensor([dov * ovx], dtype=f64)]
  mag += [ref[-2].abs(), ref[-1].abs()]
  ref, mag = torch.cat(ref), torch.cat(mag)
  assert ref.numel() == nf
  err = (got - ref).abs()
  bound = 2.0 ** -21 * mag
  worst = int(torch.argmax(err / bound))
  print('largest error %.3e at %d (bound there %.3e); length scales: err %s bound %s' % (
    float(err[worst]), worst, float(bound[worst]), err[-4:-2].tolist(), bound[-4:-2].tolist()))
  assert bool((err <= bound).all()), 'entry %d: %.9g against %.9g (bound %.3e)' % (worst, float(got[worst]), float(ref[worst]), float(bound[worst]))
  # the structural zeros really were dropped: the outputs hold as many entries as the sources, and every one matched its own slot above
  assert float(ref.abs().min()) > 0.0


# ---- 2. / 5. recorded fixed-grid solve against the host loop ---------------------------------------------------------------------
RECORDED = {
  # rk4 with a short last step, two hub rows of 700 entries
  'split_rk4_hubs': dict(n=1500, d=20, heads=2, A=16, f0=12, p0=8, method='rk4', time=2.3, hubs=2, hub_deg=700),
  # two label columns behind the positional block (padded rows, the label mapping), euler, no source term
  'split_d22_labels_euler': dict(n=600, d=22, heads=2, A=16, f0=12, p0=8, method='euler', time=2.5, step_size=0.5, add_source=False),
  'split_midpoint_squareplus_cols': dict(n=700, d=20, heads=2, A=16, f0=12, p0=8, method='midpoint', time=2.2, step_size=0.4,
                                         square_plus=True, attention_norm_idx=1),
  # the Cora best_params width: A = 128 / 8 heads -> kernel width 256, q||k rows of 512 floats
  'split_a128_h8_rk4': dict(n=300, d=32, heads=8, A=128, f0=20, p0=12, method='rk4', time=2.3),
  # the plain exp kernel at the new upper width, and at the width the one-column form of exp_node_bwd_kernel already took
  'plain_a256_h8_rk4': dict(n=300, d=32, heads=8, A=256, method='rk4', time=2.3),
  'plain_a16_h4_rk4': dict(n=800, d=32, heads=4, A=16, method='rk4', time=2.3),
}


@pytest.mark.parametrize('case', sorted(RECORDED))
def test_recorded_fixed_grid_equals_the_host_loop(dev, case):
  """Same block, same weights: the recorded solve + native reverse sweep against the differentiable host loop over the kernel-backed
  autograd Functions (the only path of these configurations before the split kernel / width 256 reached the native stage); a second
  recorded iteration replays both captured graphs and reproduces the first bit for bit."""
  kw = dict(RECORDED[case])
  block, x = _block(dev, seed=61, **kw)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
  z1, gx1, g1, nfe1 = _train_once(block, x, dev, c)
  assert str(block.odefunc._last_train_solve).startswith('native recorded fixed-grid'), block.odefunc._last_train_solve
  _set_host(block, 'gnpde_host_fixed_training', True)
  z2, gx2, g2, nfe2 = _train_once(block, x, dev, c)
  assert not str(block.odefunc._last_train_solve).startswith('native recorded'), block.odefunc._last_train_solve
  assert nfe1 == nfe2, (nfe1, nfe2)
  assert_parity(z1, z2, 1e-5, case + ' z')
  assert_parity(gx1, gx2, 2e-4, case + ' grad_x')
  refs = {k: v for k, v in g2.items() if v is not None}
  assert refs, 'the host loop produced no parameter gradients'
  if 'f0' in kw:
    for nm in SPLIT_NAMES:
      k = 'odefunc.multihead_att_layer.' + nm
      assert g1.get(k) is not None, k + ' received no gradient on the native path'
      assert k in refs, k + ' received no gradient on the host loop'
      assert float(g1[k].abs().max()) > 0.0, k      # (a distance kernel sees the key bias too)
  _module_scaled(g1, refs, 2e-4, case)
  _set_host(block, 'gnpde_host_fixed_training', False)
  z3, gx3, g3, _ = _train_once(block, x, dev, c)
  assert str(block.odefunc._last_train_solve).startswith('native recorded fixed-grid')
  assert torch.equal(z1, z3) and torch.equal(gx1, gx3)
  for k, v in g1.items():
    if v is not None:
      assert torch.equal(v, g3[k]), k


# ---- 3. against float64 autograd through the oracle ---------------------------------------------------------------------------------
def _grid_steps(t1, step):
  """torchdiffeq's fixed grid over [0, t1] (FixedGridODESolver: ceil(t1 / h + 1) points i h, the last replaced by t1), in float32
  like the block's `t`."""
  t = torch.tensor([0.0, t1], dtype=torch.float32)
  niters = int(torch.ceil((t[1] - t[0]) / step + 1).item())
  grid = torch.arange(0, niters, dtype=torch.float32) * step + t[0]
  grid[-1] = t[1]
  return [float(v) for v in (grid[1:] - grid[:-1])]


def test_native_and_host_gradients_against_float64_autograd(dev):
  """d/dx and d/dtheta of sum(c z(T)) by float64 autograd on the CPU through oracle.restate.transformer_attention_split +
  rhs_from_attention in an rk4 (3/8 rule) loop over torchdiffeq's grid: the recorded native sweep and the host loop both meet the
  project's gradient bar of 2e-4, module-scaled."""
  n, f0, p0, h, A = 400, 12, 8, 2, 16
  d = f0 + p0 + 2                                     # two label columns
  kw = dict(n=n, d=d, heads=h, A=A, f0=f0, p0=p0, method='rk4', time=2.3)
  block, x = _block(dev, seed=71, **kw)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
  f = block.odefunc
  lay = f.multihead_att_layer
  e_n = f.edge_index.cpu()
  f64 = torch.float64
  cast = lambda t: t.detach().cpu().to(f64).clone().requires_grad_(True)   # noqa: E731
  x64 = cast(x)
  P = {k: cast(dict(lay.named_parameters())[k]) for k in SPLIT_NAMES}
  al, be = cast(f.alpha_train), cast(f.beta_train)
  x0 = x.to(f64)                                      # ODEblock.set_x0 detaches the source term

  def rhs(y):
    att, _ = R.transformer_attention_split(y, e_n, P, h, f0, p0)
    return R.rhs_from_attention(y, e_n, att, al, be, x0, False, True)
  y = x64
  steps = _grid_steps(2.3, 1.0)
  assert len(steps) == 3 and steps[-1] < 0.5          # a short last step
  for hstep in steps:
    k1 = rhs(y)
    k2 = rhs(y + hstep * k1 / 3)
    k3 = rhs(y + hstep * (k2 - k1 / 3))
    k4 = rhs(y + hstep * (k1 - k2 + k3))
    y = y + hstep * (k1 + 3 * (k2 + k3) + k4) / 8
  (y * c.to(f64)).sum().backward()
  refs = {'odefunc.multihead_att_layer.' + k: P[k].grad for k in SPLIT_NAMES}
  refs['odefunc.alpha_train'] = al.grad
  refs['odefunc.beta_train'] = be.grad
  cd = c.to(dev)
  for host in (False, True):
    _set_host(block, 'gnpde_host_fixed_training', host)
    z, gx, g, nfe = _train_once(block, x, dev, cd)
    what = 'host loop' if host else 'native'
    assert str(f._last_train_solve).startswith('native recorded fixed-grid') == (not host), f._last_train_solve
    assert nfe == 4 * len(steps)
    assert_parity(z, y.detach().float(), 2e-5, what + ' z vs float64')
    assert_parity(gx, x64.grad.float(), 2e-4, what + ' grad_x vs float64')
    _module_scaled(g, {k: v.float() for k, v in refs.items()}, 2e-4, what + ' vs float64')


# ---- 4. the adjoint route ------------------------------------------------------------------------------------------------------------
def _run_adjoint(dev, kw, host):
  block, x = _block(dev, seed=61, adjoint=True, gnpde_host_adjoint=bool(host), **kw)
  with torch.no_grad():
    for f in (block.odefunc, block.reg_odefunc.odefunc):
      f.alpha_train.fill_(0.3)
      f.beta_train.fill_(0.2)
  block.train()
  xin = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xin)
  z = block(xin)
  c = torch.randn(z.shape, generator=torch.Generator().manual_seed(12)).to(dev)
  (z * c).sum().backward()
  grads = {k: p.grad.detach().clone() for k, p in block.named_parameters() if p.grad is not None}
  return z.detach(), xin.grad.detach().clone(), grads, bool(block.odefunc.__dict__.get('_adjoint_state')), block.odefunc.nfe


@pytest.mark.parametrize('adjoint_method', ['rk4', 'euler'])
def test_native_adjoint_matches_stage_loop(dev, adjoint_method):
  """opt['adjoint']: the backward interval as one native object against the stage-by-stage loop (opt['gnpde_host_adjoint']), with the
  assertions of tests/test_adjoint_native_gpu.py::test_native_adjoint_matches_stage_loop."""
  kw = dict(n=1500, d=20, heads=2, A=16, f0=12, p0=8, method='rk4', time=2.3, hubs=2, hub_deg=700, adjoint_method=adjoint_method,
            step_size=1.0 if adjoint_method == 'rk4' else 0.5)
  z_h, gx_h, gp_h, native_h, nfe_h = _run_adjoint(dev, kw, host=True)
  z_n, gx_n, gp_n, native_n, nfe_n = _run_adjoint(dev, kw, host=False)
  assert not native_h and native_n, 'path selection: host %s native %s' % (native_h, native_n)
  assert nfe_h == nfe_n
  assert torch.equal(z_h, z_n)
  tol = 2e-4
  assert_parity(gx_n, gx_h, tol, 'grad_x')
  assert set(gp_n) == set(gp_h)
  for nm in SPLIT_NAMES:
    assert 'odefunc.multihead_att_layer.' + nm in gp_n
  checked = 0
  scale = max(float(v.abs().max()) for v in gp_h.values())
  for k in sorted(gp_h):
    ref = gp_h[k]
    if float(ref.abs().max()) < 1e-5 * max(scale, 1.0):      # mathematically zero (a row softmax does not see the key bias): rounding noise on both sides
      assert float(gp_n[k].abs().max()) < 1e-4 * max(scale, 1.0), k
    else:
      assert_parity(gp_n[k], ref, tol, k)
      checked += 1
  assert checked >= 8


# ---- 6. forward / backward skew ------------------------------------------------------------------------------------------------------
def test_update_between_forward_and_backward_does_not_change_the_gradients(dev):
  """An optimiser-style in-place update of lengthscale_x after the forward pass: the sweep differentiates the solve that ran (its
  derived projection, its length scales), so the gradients equal those of a run without the update, bit for bit."""
  kw = dict(n=500, d=22, heads=2, A=16, f0=12, p0=8, method='rk4', time=2.0)
  block, x = _block(dev, seed=81, **kw)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(9)).to(dev)
  lay = block.odefunc.multihead_att_layer
  z1, gx1, g1, _ = _train_once(block, x, dev, c)
  assert str(block.odefunc._last_train_solve).startswith('native recorded fixed-grid')

  def step():
    with torch.no_grad():
      lay.lengthscale_x.add_(0.25)
  z2, gx2, g2, _ = _train_once(block, x, dev, c, between=step)
  assert abs(float(lay.lengthscale_x.detach()) - (SCALARS['lengthscale_x'] + 0.25)) < 1e-6
  assert torch.equal(z1, z2) and torch.equal(gx1, gx2)
  for k, v in g1.items():
    if v is not None:
      assert torch.equal(v, g2[k]), k
  # the next forward sees the new value
  z3, gx3, g3, _ = _train_once(block, x, dev, c)
  assert not torch.equal(z1, z3)
  assert math.isfinite(float(gx3.abs().max()))
