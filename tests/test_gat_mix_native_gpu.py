"""The GAT function's mix_features form, f = alpha (A(x) (x W) Wout - x) + beta x0 (reference src/function_GAT_attention.py:32-38), on
the native no-grad solvers: the out-projection kernel with the diffusion epilogue and the stage algebra behind it (csrc/out_proj.hip,
gnpde_linear_epilogue) and the flagged descriptor (GNPDE_RHS_MIX_FEATURES) under every solver that evaluates through it.

References: a float64 restatement written here (the kernel's stages, the whole function), the reference's own recorded solves
(tests/golden/gatmix_constant_*.npz, tools/record_gat_mix_fixtures.py) and this package's host loops over the eager evaluation."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
from helpers import Data, Fixture, assert_parity, random_graph

O = importlib.import_module('gnpde_amd.odeint')
R = importlib.import_module('gnpde_amd.routes')
pytestmark = pytest.mark.gpu

OPT = dict(heads=4, attention_dim=16, attention_type='scaled_dot', attention_norm_idx=0, square_plus=False, reweight_attention=False,
           beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9, add_source=True, no_alpha_sigmoid=False,
           mix_features=True, hidden_dim=24, augment=False, adjoint=False, tol_scale=1.0, data_norm='rw', method='rk4', step_size=1.0,
           max_iters=100, block='constant', function='GAT', time=2.0)
S = _lib
ESHAPE, EINVAL = -2, -1          # GNPDE_ESHAPE, GNPDE_EINVAL of include/gnpde.h


def last_error():
  return _lib.lib().gnpde_last_error().decode(errors='replace')


PLAIN = ['RHS', 'EULER', 'RK1', 'RK2', 'RK3', 'RK4', 'RK1C', 'RK2C', 'RK3C', 'RK4C']
# (name, n_prev, coef_scale, out_k, out_y)
LINCOMB = [('LINCOMB', p, cs, True, True) for p in (0, 1, 6) for cs in (False, True)] + [('LINCOMB', 1, False, False, True),
                                                                                         ('LINCOMB', 6, True, True, False)]
CONFIGS = [(s, 0, False, True, True) for s in PLAIN] + LINCOMB
DT = float(np.float32(0.37))
COEF = [float(np.float32(c)) for c in (0.31, -0.27, 0.4, 0.11, -0.35, 0.22, 0.18)]
SCALE = float(np.float32(0.83))
SENTINEL = 777.0


# ---- float64 restatements ------------------------------------------------------------------------------------------------------------
def stage_ref(name, k, u, ops64, n_prev, cs):
  """(out_k, out_y) of a stage in float64 (gnpde_epilogue_t in include/gnpde.h); None where the stage writes nothing."""
  y, k1, k2, k3, prev = ops64['y'], ops64['k1'], ops64['k2'], ops64['k3'], ops64['prev']
  dt = DT
  if name == 'RHS':
    return k, None
  if name == 'EULER':
    return None, y + dt * k
  if name == 'RK1':
    return k, y + dt * k / 3
  if name == 'RK2':
    return k, y + dt * (k - k1 / 3)
  if name == 'RK3':
    return k, y + dt * (k1 - k2 + k)
  if name == 'RK4':
    return None, y + (k1 + 3 * (k2 + k3) + k) * dt / 8
  if name == 'RK1C':
    return None, u + dt * k / 3
  if name == 'RK2C':
    return None, (2 * y - u) + dt * k
  if name == 'RK3C':
    return None, (2 * k1 - u) + dt * k
  if name == 'RK4C':
    return None, ((6 * k1 + 3 * u) - y + dt * k) / 8
  assert name == 'LINCOMB'
  sc = SCALE if cs else 1.0
  out = y + sum(COEF[j] * sc * prev[j] for j in range(n_prev)) + COEF[n_prev] * sc * k
  return k, out


def gat_mix_ref(x, edge, W, Wout, a, heads, slope, norm_idx, alpha, beta, x0, sigmoid):
  """ODEFuncAtt.forward with mix_features (reference src/function_GAT_attention.py:32-38, 45-65, 105-115) in the dtype of x."""
  n, A = x.shape[0], W.shape[1]
  dk = A // heads
  wx = x @ W
  h = wx.view(n, heads, dk)
  av = a.reshape(-1)
  s = (h[edge[0]] * av[:dk]).sum(-1) + (h[edge[1]] * av[dk:]).sum(-1)          # [E, heads]
  s = torch.nn.functional.leaky_relu(s, slope)
  idx = edge[norm_idx]
  m = torch.full((n, heads), -float('inf'), dtype=x.dtype, device=x.device)
  m = m.scatter_reduce(0, idx[:, None].expand_as(s), s.detach(), 'amax', include_self=True)
  p = (s - m[idx]).exp()
  den = torch.zeros(n, heads, dtype=x.dtype, device=x.device).index_add(0, idx, p)
  w = (p / (den[idx] + 1e-16)).mean(dim=1)
  agg = torch.zeros(n, A, dtype=x.dtype, device=x.device).index_add(0, edge[0], w[:, None] * wx[edge[1]])
  al = torch.sigmoid(alpha) if sigmoid else alpha
  f = al * (agg @ Wout - x)
  return f if x0 is None else f + beta * x0


def func_ref(func, x0):
  """t, y -> f(y) of a package ODEFuncAtt, restated in float64 on the CPU."""
  lay, o = func.multihead_att_layer, func.opt
  c = lambda t: t.detach().double().cpu()        # noqa: E731
  edge = func.edge_index.cpu()
  src = c(x0) if o['add_source'] else None
  return lambda t, y: gat_mix_ref(y, edge, c(lay.W), c(lay.Wout), c(lay.a), lay.h, o['leaky_relu_slope'], o['attention_norm_idx'],
                                  c(func.alpha_train), c(func.beta_train), src, not o['no_alpha_sigmoid'])


def rk4_ref(f, y, T, step):
  grid = O.time_grid(torch.tensor([0.0, T]), step).double()
  for t0, t1 in zip(grid[:-1], grid[1:]):
    dt = t1 - t0
    k1 = f(t0, y)
    k2 = f(t0, y + dt * k1 / 3)
    k3 = f(t0, y + dt * (k2 - k1 / 3))
    k4 = f(t1, y + dt * (k1 - k2 + k3))
    y = y + (k1 + 3 * (k2 + k3) + k4) * dt / 8
  return y


# ---- construction --------------------------------------------------------------------------------------------------------------------
def randomise(module, seed, dev):
  g = torch.Generator().manual_seed(seed)
  with torch.no_grad():
    for name, p in module.named_parameters():
      if p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      elif name.endswith('alpha_train'):
        p.fill_(0.3)
      elif name.endswith('beta_train'):
        p.fill_(0.2)


def make_func(ei, x, dev, seed, **over):
  d = x.shape[1]
  opt = dict(OPT, hidden_dim=d, **over)
  func = G.ODEFuncAtt(d, d, opt, Data(x, ei.to(dev)), dev).to(dev)
  randomise(func, seed, dev)
  func.x0 = x
  return func


def make_block(ei, x, dev, seed, **over):
  opt = dict(OPT, hidden_dim=x.shape[1], **over)
  block = G.ConstantODEblock(G.ODEFuncAtt, [], opt, Data(x, ei.to(dev)), dev, t=torch.tensor([0, opt['time']])).to(dev)
  randomise(block, seed, dev)
  block.eval()
  block.set_x0(x)
  return block


def block_of(fx, dev):
  x = fx.t('x', dev)
  block = G.ConstantODEblock(G.ODEFuncAtt, [], fx.opt, Data(x, fx.t('edge_index', dev)), dev, t=torch.tensor([0, fx.opt['time']])).to(dev)
  block.load_state_dict(fx.params, strict=True)
  block.eval()
  block.set_x0(x)
  return block, x


def state(n, d, ld, dev, gen, fill=None):
  """[n, d] view of an [n, ld] allocation."""
  buf = torch.full((n, ld), SENTINEL if fill is None else fill, dtype=torch.float32)
  if fill is None and gen is not None:
    buf[:, :d] = torch.randn(n, d, generator=gen)
  return buf.to(dev)[:, :d]


# ---- 1. the kernel, every stage, against float64 -------------------------------------------------------------------------------------
def run_stages(launch, ax_of, u, n, d, ld, dev, gen, padded, variants):
  """Every stage configuration x (x0 null / not) x alpha_sigmoid through `launch(e, x0 present, sigmoid)`; ax_of(x0 present, sigmoid) ->
  (ax, alpha', beta, x0) in float64.  Outputs start as a sentinel in all ld columns."""
  names = ('y', 'k1', 'k2', 'k3')
  t32 = {nm: state(n, d, ld, dev, gen) for nm in names}
  prev32 = [state(n, d, ld, dev, gen) for _ in range(6)]
  scale_dev = torch.tensor([SCALE], dtype=torch.float32, device=dev)
  ops64 = {nm: t32[nm].double() for nm in names}
  ops64['prev'] = [p.double() for p in prev32]
  u64 = u.double()
  for with_x0, sigmoid in variants:
    ax, al, be, x064 = ax_of(with_x0, sigmoid)
    k = al * (ax - u64)
    if with_x0:
      k = k + be * x064
    for name, n_prev, cs, want_k, want_y in CONFIGS:
      ref_k, ref_y = stage_ref(name, k, u64, ops64, n_prev, cs)
      got = []
      for rep in range(2):
        e = S.EpilogueStruct()
        e.stage, e.dt = getattr(S, 'STAGE_' + name), DT
        y_in = t32['y']
        if name in ('RK4', 'RK4C'):          # these two run in place on y
          full = torch.full((n, ld), SENTINEL, dtype=torch.float32, device=dev)
          full[:, :d] = t32['y']
          y_in = full[:, :d]
        out_k = state(n, d, ld, dev, None) if (ref_k is not None and want_k) else None
        out_y = y_in if name in ('RK4', 'RK4C') else (state(n, d, ld, dev, None) if (ref_y is not None and want_y) else None)
        for nm, t in (('y', y_in), ('k1', t32['k1']), ('k2', t32['k2']), ('k3', t32['k3']), ('out_k', out_k), ('out_y', out_y)):
          setattr(e, nm, t.data_ptr() if t is not None else None)
        e.n_prev = n_prev
        for j in range(n_prev):
          e.prev[j] = prev32[j].data_ptr()
        for j in range(n_prev + 1):
          e.coef[j] = COEF[j]
        e.coef_scale = scale_dev.data_ptr() if cs else None
        launch(e, with_x0, sigmoid)
        got.append((out_k, out_y))
      what = '%s n_prev=%d cs=%d x0=%d sigmoid=%d n=%d d=%d ld=%d' % (name, n_prev, cs, with_x0, sigmoid, n, d, ld)
      for (a, b), ref, tag in ((g2, r, t) for g2, r, t in zip(zip(*got), (ref_k, ref_y), ('out_k', 'out_y'))):
        if a is None:
          continue
        assert_parity(a, ref, what=what + ' ' + tag)
        assert torch.equal(a, b), what + ' ' + tag + ': the second launch differs'
        if not padded and ld > d:
          full = torch.as_strided(a, (n, ld), (ld, 1))
          assert bool((full[:, d:] == SENTINEL).all()), what + ' ' + tag + ': columns [d, ld) were written'


SHAPES = [(4, 4, 4), (16, 24, 24), (12, 22, 22), (12, 22, 24), (64, 80, 80), (256, 256, 256)]
NS = [1, 15, 16, 17, 100]
ALL_VARIANTS = [(x0, sg) for x0 in (False, True) for sg in (False, True)]


@pytest.mark.parametrize('A,d,ld', SHAPES)
@pytest.mark.parametrize('n', NS)
def test_out_projection_kernel_every_stage(dev, n, A, d, ld):
  """gnpde_linear_epilogue: every GNPDE_STAGE_*, x0 null / non-null, both alpha forms, ragged row tiles, guarded column and K tiles,
  scalar lanes (d % 4 != 0; with ld > d the padding columns keep their sentinel), against float64; a second launch is bit-equal."""
  gen = torch.Generator().manual_seed(1000 * n + d)
  z = torch.randn(n, A, generator=gen).to(dev)
  wt = (torch.randn(d, A, generator=gen) / A ** 0.5).to(dev)
  u, x0 = state(n, d, ld, dev, gen), state(n, d, ld, dev, gen)
  alpha = torch.tensor([0.3], device=dev)
  beta = torch.tensor([0.45], device=dev)
  ax = z.double() @ wt.double().t()

  def ax_of(with_x0, sigmoid):
    al = torch.sigmoid(alpha.double()) if sigmoid else alpha.double()
    return ax, al, beta.double(), x0.double()

  def launch(e, with_x0, sigmoid):
    e.alpha, e.alpha_sigmoid = alpha.data_ptr(), int(sigmoid)
    e.beta, e.x0 = (beta.data_ptr(), x0.data_ptr()) if with_x0 else (None, None)
    ops.linear_epilogue(z, wt, u, e)

  run_stages(launch, ax_of, u, n, d, ld, dev, gen, padded=False, variants=ALL_VARIANTS)


@pytest.mark.parametrize('n', NS)
def test_out_projection_kernel_padded_rows(dev, n):
  """(A, d, ld) = (8, 162, 164) with GNPDE_RHS_PADDED_ROWS: 16-byte lanes over the padding columns.  The C entry point has no flag
  argument, so the kernel is reached as launch 4 of a flagged descriptor (gnpde_rhs_stage); ax is the float64 restatement of
  A(x) (x W) Wout on the same graph."""
  A, d, ld, heads = 8, 162, 164, 2
  gen = torch.Generator().manual_seed(2000 + n)
  ei = random_graph(n, 3, seed=50 + n)
  u = _lib.alloc_state(n, d, dev)
  u.copy_(torch.randn(n, d, generator=gen).to(dev))
  x0 = _lib.alloc_state(n, d, dev)
  x0.copy_(torch.randn(n, d, generator=gen).to(dev))
  assert u.stride(0) == ld and _lib.is_padded(u)
  funcs, descs = {}, {}
  for with_x0, sigmoid in ALL_VARIANTS:
    f = make_func(ei, u, dev, 7, attention_dim=A, heads=heads, add_source=with_x0, no_alpha_sigmoid=not sigmoid)
    f.x0 = x0 if with_x0 else None
    funcs[with_x0, sigmoid] = f
    descs[with_x0, sigmoid] = f._descriptor(u)
    st = descs[with_x0, sigmoid].struct
    assert st.flags == _lib.RHS_PADDED_ROWS | _lib.RHS_MIX_FEATURES and st.ld == ld and st.out_ld == A

  def ax_of(with_x0, sigmoid):
    f = funcs[with_x0, sigmoid]
    lay = f.multihead_att_layer
    c = lambda t: t.detach().double()        # noqa: E731
    one, zero = torch.ones((), dtype=torch.float64, device=dev), torch.zeros((), dtype=torch.float64, device=dev)
    agg_wout_minus_u = gat_mix_ref(c(u), f.edge_index, c(lay.W), c(lay.Wout), c(lay.a), heads, 0.2, 0, one, zero, None, False)
    al = torch.sigmoid(c(f.alpha_train)) if sigmoid else c(f.alpha_train)
    return agg_wout_minus_u + c(u), al, c(f.beta_train), c(x0)

  L = _lib.lib()

  def launch(e, with_x0, sigmoid):
    desc = descs[with_x0, sigmoid]
    ws = desc.graph.workspace('rhs%d_%d' % (desc.struct.kind, desc.struct.d), L.gnpde_rhs_workspace_bytes(desc.ref()))
    ops.check(L.gnpde_rhs_stage(desc.ref(), ops.ptr(u), ctypes.byref(e), ops.ptr(ws), ws.numel(), ops.stream_of(u)))

  run_stages(launch, ax_of, u, n, d, ld, dev, gen, padded=True, variants=ALL_VARIANTS)


def test_out_projection_kernel_refuses_other_shapes(dev):
  z = torch.zeros(4, 260, device=dev)
  out = torch.zeros(4, 8, device=dev)
  alpha = torch.zeros(1, device=dev)
  e = ops.make_epilogue(alpha, None, None, True, out_k=out)
  L = _lib.lib()
  call = lambda A, d, zz, w, u: L.gnpde_linear_epilogue(ops.ptr(zz), 4, A, zz.stride(0), ops.ptr(w), d, w.stride(0), ops.ptr(u), u.stride(0),  # noqa: E731
                                                        ctypes.byref(e), None)
  assert call(260, 8, z, torch.zeros(8, 260, device=dev), out.clone()) == ESHAPE           # A > 256
  assert call(6, 8, z[:, :8].contiguous(), torch.zeros(8, 8, device=dev), out.clone()) == ESHAPE      # A % 4 != 0
  wide = torch.zeros(4, 260, device=dev)
  e2 = ops.make_epilogue(alpha, None, None, True, out_k=wide)
  assert L.gnpde_linear_epilogue(ops.ptr(z), 4, 8, 260, ops.ptr(torch.zeros(260, 8, device=dev)), 260, 8, ops.ptr(wide.clone()), 260,
                                 ctypes.byref(e2), None) == ESHAPE                          # d > 256


# ---- 2. one evaluation against the reference's recorded one --------------------------------------------------------------------------
def test_one_evaluation_against_the_reference(dev):
  fx = Fixture('func_gat_mix')
  x = fx.t('x', dev)
  func = G.ODEFuncAtt(x.shape[1], x.shape[1], fx.opt, Data(x, fx.t('edge_index', dev)), dev).to(dev)
  func.load_state_dict(fx.params, strict=True)
  func.x0 = fx.t('x0', dev)
  assert func._has_native_rhs(x) and func._descriptor(x).struct.flags & _lib.RHS_MIX_FEATURES
  with torch.no_grad():
    f = func(0.0, x)
  assert func.nfe == 1
  assert_parity(f, fx.t('f'), what='func_gat_mix through the flagged descriptor')


# ---- 3. solves against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,tol', [('gatmix_constant_rk4', 1e-5), ('gatmix_constant_euler_h05', 1e-5), ('gatmix_constant_dopri5', 2e-5)])
def test_solves_against_the_reference(dev, name, tol):
  fx = Fixture(name)
  print('%s: the reference\'s float32 solve deviates from its float64 solve by %.3e (nfe %d / %d)'
        % (name, float(fx.arr['ref_dev']), int(fx.arr['nfe']), int(fx.arr['nfe64'])))
  assert float(fx.arr['ref_dev']) <= tol / 16
  block, x = block_of(fx, dev)
  with torch.no_grad():
    z = block(x)
  e_inf = float((z.double().cpu() - fx.t('z').double()).abs().max() / fx.t('z').double().abs().max())
  print('%s: native solve vs the reference %.3e (bound %.1e), nfe %d' % (name, e_inf, tol, block.odefunc.nfe))
  assert_parity(z, fx.t('z'), tol=tol, what=name)
  assert block.odefunc.nfe == int(fx.arr['nfe'])
  assert block.odefunc.__dict__.get('_solver_state') or block.odefunc.__dict__.get('_dopri5_device'), 'the solve did not take a native path'


# ---- 4. midpoint and adaptive_heun against the host loops ----------------------------------------------------------------------------
def test_midpoint_and_adaptive_heun_against_the_host_loops(dev):
  fx = Fixture('gatmix_constant_rk4')
  block, x = block_of(fx, dev)
  f = block.odefunc
  t = torch.tensor([0.0, 2.3], device=dev)
  with torch.no_grad():
    z_mid = G.odeint(f, x, t, method='midpoint', options=dict(step_size=0.5))[1].clone()
    nfe0 = f.nfe
    z_host = O._solve_fixed_host(f, x, t, 'midpoint', 0.5)[1]
    assert f.nfe - nfe0 == nfe0 == 10
    assert_parity(z_mid, z_host, tol=2e-6, what='midpoint: native solve vs host loop')
    kw = dict(atol=2000.0 * 1e-7, rtol=2000.0 * 1e-9)
    f.nfe = 0
    z_dev = G.odeint(f, x, t, method='adaptive_heun', **kw)[1].clone()
    nfe_dev = f.nfe
    f.nfe = 0
    z_h = G.odeint(f, x, t, method='adaptive_heun', options={'host_controller': True}, **kw)[1]
    assert nfe_dev == f.nfe and nfe_dev >= 8
    assert_parity(z_dev, z_h, tol=2e-6, what='adaptive_heun: device controller vs host controller')


# ---- 5. graph and eager agree --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,step', [('rk4', 1.0), ('euler', 0.5), ('midpoint', 0.5)])
def test_graph_replay_and_eager_launches_agree_bitwise(dev, method, step):
  fx = Fixture('gatmix_constant_rk4')
  block, x = block_of(fx, dev)
  f = block.odefunc
  t = torch.tensor([0.0, 2.3], device=dev)
  with torch.no_grad():
    z1 = G.odeint(f, x, t, method=method, options=dict(step_size=step))[1].clone()
    z2 = G.odeint(f, x, t, method=method, options=dict(step_size=step))[1].clone()
    z3 = G.odeint(f, x, t, method=method, options=dict(step_size=step), use_graph=False)[1].clone()
  assert torch.equal(z1, z2), 'two captured solves differ'
  assert torch.equal(z1, z3), 'eager launches differ from the graph replay'


# ---- 6. weights are live -------------------------------------------------------------------------------------------------------------
def test_weights_are_live_in_a_captured_solve(dev):
  fx = Fixture('gatmix_constant_rk4')
  block, x = block_of(fx, dev)
  lay = block.odefunc.multihead_att_layer
  with torch.no_grad():
    z0 = block(x).clone()
    lay.Wout.mul_(0.5)
    lay.W.add_(0.01)
    block.set_x0(x)
    z1 = block(x).clone()
  assert not torch.equal(z0, z1)
  fresh, _ = block_of(fx, dev)
  with torch.no_grad():
    fresh.odefunc.multihead_att_layer.Wout.copy_(lay.Wout)
    fresh.odefunc.multihead_att_layer.W.copy_(lay.W)
    z2 = fresh(x)
  assert torch.equal(z1, z2), 'the captured solve did not see the optimiser step'


# ---- 7. hub rows and empty rows ------------------------------------------------------------------------------------------------------
def test_hub_rows_and_empty_rows(dev):
  n, d = 700, 24
  ei = random_graph(n, 4, 61, hubs=2, hub_deg=600, isolated=3)
  x = (torch.randn(n, d, generator=torch.Generator().manual_seed(62)) * 0.5).to(dev)
  block = make_block(ei, x, dev, 63, self_loop_weight=0, time=2.0)
  f = block.odefunc
  g = f._graph(x)
  assert g.n_long_rows == 2 and int((torch.bincount(f.edge_index[0], minlength=n) == 0).sum()) >= 3
  ref = func_ref(f, x)
  with torch.no_grad():
    got = f(0.0, x)
    z = block(x)
  assert_parity(got, ref(0.0, x.double().cpu()), what='one evaluation with hub rows and empty rows')
  assert_parity(z, rk4_ref(ref, x.double().cpu(), 2.0, 1.0), what='rk4 with hub rows and empty rows')
  assert f.__dict__.get('_solver_state')


# ---- 8. shapes outside the rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d,A,heads', [(260, 16, 4), (24, 6, 3)])
def test_shapes_outside_the_rule_solve_on_the_host_loop(dev, d, A, heads):
  n = 150
  ei = random_graph(n, 5, 71)
  x = (torch.randn(n, d, generator=torch.Generator().manual_seed(72)) * 0.5).to(dev)
  block = make_block(ei, x, dev, 73, attention_dim=A, heads=heads, time=2.0)
  f = block.odefunc
  t = torch.tensor([0.0, 2.0], device=dev)
  assert not f._has_native_rhs(x)
  with torch.no_grad():
    assert R.forward(f, x, t, 'rk4', {'step_size': 0.5}) == ('host_fixed', R.NO_RHS) and R.forward(f, x, t, 'dopri5', {}) == ('host_loop', R.NO_RHS)
  with pytest.raises(NotImplementedError):
    f._descriptor(x)
  ref = func_ref(f, x)
  with torch.no_grad():
    got = f(0.0, x)
    z = block(x)
    z5 = G.odeint(f, x, t, method='dopri5', atol=1e-5, rtol=1e-7)[1]
  assert not f.__dict__.get('_solver_state') and not f.__dict__.get('_dopri5_device')
  assert_parity(got, ref(0.0, x.double().cpu()), what='one evaluation outside the rule')
  assert_parity(z, rk4_ref(ref, x.double().cpu(), 2.0, 1.0), what='rk4 on the host loop')
  assert torch.isfinite(z5).all()


# ---- 9. early stopping ---------------------------------------------------------------------------------------------------------------
def test_early_stop_rk4_in_the_graph_equals_stepping_on_the_host(dev):
  """EarlyStopInt with rk4: the evaluator inside the captured solve of the flagged descriptor returns the best time and the accuracy
  trace of the same solve stepped on the host (O._solve_fixed_host + one evaluator call per step).  The two states differ by fp32
  rounding (the host forms the stage algebra in separate ops), which can flip one node on a near-tie: 1 / |mask| per accuracy."""
  fx = Fixture('early_rk4_laplacian_arxiv')
  n, d, c = 400, 24, 7
  ei = random_graph(n, 5, 81)
  g = torch.Generator().manual_seed(82)
  x = (torch.randn(n, d, generator=g) * 0.5).to(dev)
  labels = torch.randint(0, c, (n,), generator=g)
  role = torch.randperm(n, generator=g)
  masks = [role < 100, (role >= 100) & (role < 250), role >= 250]
  opt = dict(fx.opt, **OPT)
  opt.update(hidden_dim=d, time=4.0, step_size=1.0, method='rk4', dataset='Cora')
  data = Data(x, ei.to(dev))
  data.y = labels.to(dev)
  data.train_mask, data.val_mask, data.test_mask = [m.to(dev) for m in masks]
  block = G.ConstantODEblock(G.ODEFuncAtt, [], opt, data, dev, t=torch.tensor([0, opt['time']])).to(dev)
  randomise(block, 83, dev)
  w, b = torch.randn(c, d, generator=g).to(dev), (torch.randn(c, generator=g) * 0.1).to(dev)
  integ = G.EarlyStopInt(opt['time'], opt, dev)
  integ.keep_trace = True
  integ.data, integ.m2_weight, integ.m2_bias = data, w, b
  block.test_integrator = integ
  block.eval()
  block.set_x0(x)
  with torch.no_grad():
    z = block(x)
  f = block.odefunc
  assert f.__dict__.get('_solver_state'), 'the early-stopping solve did not take the captured fixed-step solver'
  sol = integ.solver
  steps = int(opt['earlystopxT'] * opt['time'])
  assert len(sol.trace) == steps
  ev = ops.EarlyStopEvaluator(w, b, data.y, data.train_mask, data.val_mask, data.test_mask, max_trace=64)
  ev.reset()
  with torch.no_grad():
    z_host = O._solve_fixed_host(f, x, integ.t.to(dev), 'rk4', 1.0, on_step=lambda y, i: ev.evaluate(y.contiguous(), i))[1]
  host = ev.read()
  assert_parity(z, z_host, tol=2e-6, what='state')
  assert len(host['trace']) == steps
  sizes = [int(m.sum()) for m in masks]
  for got, ref in zip(sol.trace, host['trace']):
    assert got['step'] == ref['step']
    assert all(abs(a - r) <= 1.0 / s + 1e-12 for a, r, s in zip(got['acc'], ref['acc'], sizes)), (got, ref)
  grid = O.time_grid(integ.t.cpu(), 1.0)
  assert float(sol.best_time) == float(grid[host['step']])
  assert abs(sol.best_val - host['best'][1]) <= 1.0 / sizes[1] + 1e-12


# ---- 10. refusals --------------------------------------------------------------------------------------------------------------------
def _flagged(dev, n=150, d=24):
  ei = random_graph(n, 5, 91)
  x = (torch.randn(n, d, generator=torch.Generator().manual_seed(92)) * 0.5).to(dev)
  f = make_func(ei, x, dev, 93)
  return f, x, f._descriptor(x)


def test_adjoint_tape_and_sharded_objects_refuse_the_flag(dev):
  f, x, desc = _flagged(dev)
  L = _lib.lib()
  ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
  dts = (ctypes.c_float * 2)(1.0, 1.0)
  for method in (_lib.METHOD_EULER, _lib.METHOD_RK4, _lib.METHOD_DOPRI5_TAPE):
    h = ctypes.c_void_p()
    nd, ns = (None, 0) if method == _lib.METHOD_DOPRI5_TAPE else (dts, 2)
    rc = L.gnpde_adjoint_create(ctypes.byref(h), desc.ref(), None, None, None, None, method, nd, ns, ops.ptr(ws), ws.numel())
    assert rc == ESHAPE and not h.value and 'mix_features' in last_error(), (method, rc)
  h = ctypes.c_void_p()
  rc = L.gnpde_adjoint_adaptive_create(ctypes.byref(h), desc.ref(), None, None, _lib.ADAPTIVE_DOPRI5, ctypes.c_float(1e-5), ctypes.c_float(1e-7),
                                       ops.ptr(ws), ws.numel())
  assert rc == ESHAPE and not h.value and 'mix_features' in last_error()
  solver = ops.FixedStepSolver(desc, 'rk4', [1.0, 1.0], dev)
  try:
    tape = torch.zeros(int(L.gnpde_solver_tape_bytes(desc.ref(), _lib.METHOD_RK4, 2)) + 256, dtype=torch.uint8, device=dev)
    assert L.gnpde_solver_set_tape(solver.handle, ops.ptr(tape), tape.numel()) == ESHAPE and 'mix_features' in last_error()
    assert L.gnpde_solver_set_tape(solver.handle, None, 0) == 0
    with pytest.raises(_lib.GnpdeError):
      solver.set_gather('bf16')
    assert L.gnpde_solver_gather_bytes(desc.ref(), _lib.METHOD_RK4) == 0
  finally:
    solver.close()
  # the row-partitioned solver: a world of one rank, whole-graph descriptors
  zero = (ctypes.c_int32 * 1)(0)
  halo = _lib.HaloStruct()
  halo.world, halo.rank, halo.n_own, halo.n_halo = 1, 0, x.shape[0], 0
  halo.send_counts = ctypes.cast(zero, ctypes.POINTER(ctypes.c_int32))
  halo.recv_counts = ctypes.cast(zero, ctypes.POINTER(ctypes.c_int32))
  h = ctypes.c_void_p()
  rc = L.gnpde_sharded_solver_create(ctypes.byref(h), None, ctypes.byref(halo), desc.ref(), desc.ref(), _lib.METHOD_RK4, dts, 2,
                                     ops.ptr(ws), ws.numel())
  assert rc == ESHAPE and not h.value and 'mix_features' in last_error()


def test_the_flag_on_other_descriptors(dev):
  f, x, desc = _flagged(dev)
  L = _lib.lib()
  st = desc.struct
  st.kind = _lib.RHS_TRANSFORMER
  st.proj_m = 2 * st.att.att_dim
  assert L.gnpde_rhs_workspace_bytes(desc.ref()) == 0 and 'GAT' in last_error()
  out = torch.empty_like(x)
  ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
  assert L.gnpde_rhs_eval(desc.ref(), ops.ptr(x), ops.ptr(out), ops.ptr(ws), ws.numel(), None) == EINVAL
  st.kind, st.proj_m = _lib.RHS_GAT, st.att.att_dim
  assert L.gnpde_rhs_workspace_bytes(desc.ref()) > 0
  st.proj_row_begin, st.proj_row_end = 0, 64                     # a partitioned descriptor
  assert L.gnpde_rhs_eval(desc.ref(), ops.ptr(x), ops.ptr(out), ops.ptr(ws), ws.numel(), None) == ESHAPE
  st.proj_row_end = 0
  st.n_state_rows = x.shape[0] + 8
  assert L.gnpde_rhs_eval(desc.ref(), ops.ptr(x), ops.ptr(out), ops.ptr(ws), ws.numel(), None) == ESHAPE
  st.n_state_rows = 0
  st.out_w = None
  assert L.gnpde_rhs_eval(desc.ref(), ops.ptr(x), ops.ptr(out), ops.ptr(ws), ws.numel(), None) == EINVAL


def test_training_keeps_the_differentiable_host_loop(dev):
  """With gradients nothing changes: the solve runs the host loop over autograd.py's mix_features evaluation, and its gradients are
  those of the float64 restatement under torch autograd (2e-4 of the largest entry, the bound of the recorded-vs-host gradient tests)."""
  n, d = 150, 24
  ei = random_graph(n, 5, 95)
  g = torch.Generator().manual_seed(96)
  xc, c = torch.randn(n, d, generator=g) * 0.5, torch.randn(n, d, generator=g)
  block = make_block(ei, xc.to(dev), dev, 97, time=2.0)
  f = block.odefunc
  t = torch.tensor([0.0, 2.0], device=dev)
  assert R.forward(f, xc.to(dev).requires_grad_(True), t, 'rk4', {'step_size': 0.5}) == ('host_fixed', R.NO_VJP_STAGE) and not O._gat_stage_native(f)
  block.train()
  xin = xc.to(dev).clone().requires_grad_(True)
  block.set_x0(xin)
  f._last_train_solve = ''
  z = block(xin)
  assert not str(f._last_train_solve).startswith('native recorded'), f._last_train_solve
  assert not f.__dict__.get('_solver_state') and not f.__dict__.get('_fixed_tape_state')
  (z * c.to(dev)).sum().backward()
  lay = f.multihead_att_layer
  ours = [lay.W, lay.Wout, lay.a, f.alpha_train, f.beta_train]
  ps = [p.detach().double().cpu().requires_grad_(True) for p in ours]
  x64 = xc.double().requires_grad_(True)
  edge = f.edge_index.cpu()
  rhs = lambda tq, y: gat_mix_ref(y, edge, ps[0], ps[1], ps[2], lay.h, 0.2, 0, ps[3], ps[4], xc.double(), True)      # noqa: E731  (x0 = the detached input)
  z64 = rk4_ref(rhs, x64, 2.0, 1.0)
  (z64 * c.double()).sum().backward()
  assert_parity(z.detach(), z64.detach(), what='training forward')
  for name, a, b in zip(['dx', 'dW', 'dWout', 'da', 'dalpha', 'dbeta'], [xin.grad] + [p.grad for p in ours], [x64.grad] + [p.grad for p in ps]):
    assert a is not None, name
    assert_parity(a.reshape(b.shape), b, tol=2e-4, what=name)
