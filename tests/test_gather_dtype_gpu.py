"""The optional bf16 gather operand of the aggregation (INTEGRATION.md "bf16 gather operand"): conversion, plain aggregation from a
given shadow, one stage against the derived bound, whole solves against a float64 restatement of the reference's own fixtures, scope."""
import copy

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops, _lib
from oracle import restate as R
from helpers import Fixture, Data, assert_parity, random_graph, TOL

pytestmark = pytest.mark.gpu

U_BF16 = 2.0 ** -8      # unit roundoff of bf16 round-to-nearest-even (8 significant bits)


def _weights(e, seed):
  g = torch.Generator().manual_seed(seed)
  return torch.rand(e, generator=g) * 0.3 + 0.01


def _padded(t, dev, dtype=None):
  """t [n, d] as a view of a zero-filled [n, ld] device allocation, ld = d rounded up to a multiple of 4."""
  n, d = t.shape
  ld = (d + 3) // 4 * 4
  out = torch.zeros(n, ld, dtype=dtype or t.dtype, device=dev)[:, :d]
  out.copy_(t)
  return out


def _bits(t):
  return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. convert, bitwise
# ---------------------------------------------------------------------------------------------------------------------------------
def test_to_bf16_is_round_to_nearest_even_bit_for_bit(dev):
  """gnpde_to_bf16 == tensor.to(torch.bfloat16) bit for bit: seeded normal values, +-0, and ties (low half 0x8000 above an even and an
  odd upper mantissa, both signs).  d = 162 with ld = 164: the padding columns are unconstrained.  (No subnormal inputs: the denormal
  mode is not the subject.)"""
  n, d = 257, 162
  g = torch.Generator().manual_seed(3)
  x = torch.randn(n, d, generator=g) * torch.logspace(-6, 6, d).unsqueeze(0)
  x[0, 0], x[0, 1] = 0.0, -0.0
  ties = []
  for upper in (0x3F80, 0x3F81, 0x4000, 0x40FF, 0x7F00, 0x0081, 0x3FFF):      # even and odd upper halves, a carry into the exponent
    for sign in (0, 0x8000):
      for low in (0x8000, 0x7FFF, 0x8001, 0x0001, 0xFFFF):
        ties.append((((upper | sign) << 16) | low) - (1 << 32 if (upper | sign) & 0x8000 else 0))
  tie_t = torch.tensor(ties, dtype=torch.int32).view(torch.float32)
  assert torch.isfinite(tie_t).all()
  x.view(-1)[2:2 + tie_t.numel()] = tie_t
  want = x.to(torch.bfloat16)
  xd = _padded(x, dev)
  assert xd.stride(0) == 164
  got = ops.to_bf16(xd)
  assert got.dtype == torch.bfloat16 and got.shape == (n, d) and got.stride(0) == 164
  assert torch.equal(_bits(got.cpu()), _bits(want))
  # the ties really were ties: both neighbours at the same distance, the even one taken
  t16 = tie_t.to(torch.bfloat16)
  exact = (tie_t.view(torch.int32) & 0xFFFF) == 0x8000
  assert int(exact.sum()) == 14 and bool(((_bits(t16)[exact].int() & 1) == 0).all())
  # contiguous rows (ld == d, d % 4 == 0) and a width that takes the element-wise path
  for dd in (128, 7):
    y = torch.randn(33, dd, generator=g)
    assert torch.equal(_bits(ops.to_bf16(y.to(dev)).cpu()), _bits(y.to(torch.bfloat16)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. plain aggregation from a given shadow
# ---------------------------------------------------------------------------------------------------------------------------------
GRAPHS = {
  # hub rows above GNPDE_LONG_ROW (chunk partials + fold) and isolated rows
  'hubs': dict(n=3000, avg_deg=4, seed=7, hubs=3, hub_deg=2500, isolated=5),
  # mean degree 8: mostly rows of <= 16 entries -> row pairs at d = 128
  'deg8': dict(n=2000, avg_deg=7, seed=8, isolated=3, dup=40),
  # mean degree 24: the wide kernel at d = 128
  'deg24': dict(n=1500, avg_deg=23, seed=9),
}


@pytest.mark.parametrize('kind', sorted(GRAPHS))
@pytest.mark.parametrize('d', [24, 64, 128, 162, 256])
def test_spmm_lo_from_a_given_shadow(dev, kind, d):
  """gnpde_spmm_lo(shadow) against the float64 aggregation of the widened shadow at the project's fp32 tolerance (the shadow is an
  INPUT here: no rounding ambiguity).  Every bf16 kernel keeps the lane mapping and summation order of the fp32 kernel that gnpde_spmm
  picks for the same width and graph -- spmm_rows_kernel (d = 24, 64), spmm_pair_kernel (d = 128, short rows), spmm_wide_kernel
  (d = 128 with longer rows, d = 256), the hub-chunk partials and their fold -- so for d % 4 == 0 the result also equals gnpde_spmm on
  the widened table bit for bit.  d = 162 (padded to ld = 164) takes 16-byte lanes here but 8-byte lanes in gnpde_spmm, which is not
  told about the padding: a different summation order, no bit equality asserted."""
  kw = dict(GRAPHS[kind])
  n = kw.pop('n')
  ei = random_graph(n, kw.pop('avg_deg'), **kw)
  graph = G.CSRGraph(ei.to(dev), n)
  if kind == 'hubs':
    assert graph.n_long_rows >= 3
  elif kind == 'deg8':
    assert 2 * graph.n_bin16 >= n
  else:
    assert 2 * graph.n_bin16 < n
  w = _weights(ei.size(1), d + 1)
  x = torch.randn(n, d, generator=torch.Generator().manual_seed(d + 2))
  lo = x.to(torch.bfloat16)
  wide = lo.to(torch.float32)
  ref = R.spmm(ei, w.double(), n, wide.double())
  w_csr = ops.edge_to_csr_mean(graph, w.to(dev))
  lo_d = _padded(lo, dev)
  out = ops.spmm_lo(graph, w_csr, lo_d)
  assert out.dtype == torch.float32 and out.shape == (n, d)
  assert_parity(out, ref, tol=TOL, what='spmm_lo %s d=%d' % (kind, d))
  if d % 4 == 0:
    same = ops.spmm(graph, w_csr, wide.to(dev))
    assert torch.equal(out, same), 'spmm_lo differs from gnpde_spmm on the widened table (%s, d=%d)' % (kind, d)


def test_spmm_lo_refuses_what_it_does_not_cover(dev):
  n, d = 64, 22
  ei = random_graph(n, 4, seed=1)
  graph = G.CSRGraph(ei.to(dev), n)
  w_csr = ops.edge_to_csr_mean(graph, _weights(ei.size(1), 2).to(dev))
  lo = torch.zeros(n, d, dtype=torch.bfloat16, device=dev)      # ld = 22: no 16-byte lanes
  with pytest.raises(_lib.GnpdeError, match='16-byte lanes'):
    ops.spmm_lo(graph, w_csr, lo)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. one stage, derived bound
# ---------------------------------------------------------------------------------------------------------------------------------
# (stage, operands it reads, outputs it writes, factor of ax in out_k / out_y as a multiple of alpha')
DT = 0.7
STAGES = [
  ('RHS', _lib.STAGE_RHS, (), ('out_k',), 1.0, None),
  ('EULER', _lib.STAGE_EULER, ('y',), ('out_y',), None, DT),
  ('RK1', _lib.STAGE_RK1, ('y',), ('out_k', 'out_y'), 1.0, DT / 3),
  ('RK2', _lib.STAGE_RK2, ('y', 'k1'), ('out_k', 'out_y'), 1.0, DT),
  ('RK3', _lib.STAGE_RK3, ('y', 'k1', 'k2'), ('out_k', 'out_y'), 1.0, DT),
  ('RK4', _lib.STAGE_RK4, ('y', 'k1', 'k2', 'k3'), ('out_y',), None, DT / 8),
  ('RK1C', _lib.STAGE_RK1C, (), ('out_y',), None, DT / 3),
  ('RK2C', _lib.STAGE_RK2C, ('y',), ('out_y',), None, DT),
  ('RK3C', _lib.STAGE_RK3C, ('k1',), ('out_y',), None, DT),
  ('RK4C', _lib.STAGE_RK4C, ('y', 'k1'), ('out_y',), None, DT / 8),
  ('LINCOMB', _lib.STAGE_LINCOMB, ('y',), ('out_y',), None, 0.5 * DT),      # midpoint: n_prev = 0, coef[0] = dt / 2 or dt
]


@pytest.mark.parametrize('d,kind', [(128, 'hubs'), (128, 'deg24'), (64, 'deg8'), (256, 'deg8')])
@pytest.mark.parametrize('stage', STAGES, ids=[s[0] for s in STAGES])
def test_one_stage_within_the_derived_bound(dev, stage, d, kind):
  """gnpde_spmm_rhs_lo(u, to_bf16(u)) against gnpde_spmm_rhs(u), every stage the fixed-step solvers launch (euler, midpoint's
  LINCOMB, both rk4 forms) and the plain derivative.  Only the gathered rows are rounded, |bf16(v) - v| <= 2^-8 |v|, so
    |Delta| <= c 2^-8 B + 1e-5 max|out|,   B = sum_e |w_e| |u[col_e]|  (float64),
  c = alpha' for the derivative and alpha' times the stage's coefficient of k for out_y; the 1e-5 term is the project's fp32
  tolerance (the two kernels may sum in another order).  The inputs are not bf16-representable, so Delta != 0; the shadow written
  by the launch is out_y.to(bfloat16) bit for bit."""
  name, code, reads, writes, c_k, c_y = stage
  kw = dict(GRAPHS[kind])
  n = kw.pop('n')
  ei = random_graph(n, kw.pop('avg_deg'), **kw)
  graph = G.CSRGraph(ei.to(dev), n)
  w = _weights(ei.size(1), 5)
  g = torch.Generator().manual_seed(17 + d)
  u = torch.randn(n, d, generator=g)
  x0 = torch.randn(n, d, generator=g)
  extra = {k: torch.randn(n, d, generator=g).to(dev) for k in reads}
  alpha, beta = torch.tensor(0.3), torch.tensor(-0.7)
  a_eff = float(torch.sigmoid(alpha))
  B = R.spmm(ei, w.double(), n, u.double().abs())
  w_csr = ops.edge_to_csr_mean(graph, w.to(dev))
  ud, x0d = u.to(dev), x0.to(dev)
  u_lo = ops.to_bf16(ud)
  assert not torch.equal(u_lo.float(), ud)

  def run(gather_lo):
    outs = {k: torch.full((n, d), float('nan'), device=dev) for k in writes}
    kwargs = dict(stage=code, dt=DT, **extra, **outs)
    if code == _lib.STAGE_LINCOMB:
      kwargs.update(prev=(), coef=(0.5 * DT,))
    ops.spmm_rhs(graph, w_csr, ud, alpha.to(dev), beta.to(dev), x0d, True, gather_lo=gather_lo, **kwargs)
    return outs

  ref = run(None)
  out_y_lo = torch.full((n, d), float('nan'), dtype=torch.bfloat16, device=dev) if 'out_y' in writes else None
  got = run((u_lo, out_y_lo))
  for key, c in (('out_k', c_k), ('out_y', c_y)):
    if key not in writes:
      continue
    a, b = got[key].double().cpu(), ref[key].double().cpu()
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    delta = (a - b).abs()
    bound = abs(c) * a_eff * U_BF16 * B + 1e-5 * float(b.abs().max())
    worst = float((delta / bound).max())
    print('%s %s d=%d %s: max|Delta| %.3e, max Delta/bound %.3f' % (name, key, d, kind, float(delta.max()), worst))
    assert bool((delta <= bound).all()), '%s %s: |Delta| exceeds the derived bound by %.3fx' % (name, key, worst)
    assert float(delta.max()) > 0, '%s %s: the bf16 operand left no trace' % (name, key)
  if out_y_lo is not None:
    assert torch.equal(_bits(out_y_lo), _bits(got['out_y'].to(torch.bfloat16))), 'written shadow != bf16(out_y)'


@pytest.mark.parametrize('kind', ['hubs', 'deg8'])
@pytest.mark.parametrize('d', [128, 96, 72])
def test_lane_mappings_of_the_row_kernels_agree_bit_for_bit(dev, kind, d):
  """Rows of 17..32 16-byte lanes in graphs of mostly short rows have two bf16 kernels: two rows per wave (32 lanes x 4 elements,
  8-byte gathers: the fp32 mapping) and four rows per wave (16 lanes x 8 elements, 16-byte gathers; gnpde_tune(18, 2)).  Same
  per-row summation order: plain aggregation, a stage's out_y and its shadow are bit-identical."""
  kw = dict(GRAPHS[kind])
  n = kw.pop('n')
  ei = random_graph(n, kw.pop('avg_deg'), **kw)
  graph = G.CSRGraph(ei.to(dev), n)
  assert 2 * graph.n_bin16 >= n
  w_csr = ops.edge_to_csr_mean(graph, _weights(ei.size(1), 5).to(dev))
  g = torch.Generator().manual_seed(d)
  u, x0, y = (torch.randn(n, d, generator=g).to(dev) for _ in range(3))
  u_lo = ops.to_bf16(u)
  alpha, beta = torch.tensor(0.3, device=dev), torch.tensor(-0.7, device=dev)
  res = {}
  for mapping in (1, 2):
    _lib.check(_lib.lib().gnpde_tune(_lib.TUNE_LO_MAPPING, mapping))
    try:
      plain = ops.spmm_lo(graph, w_csr, u_lo)
      out_y, out_lo = torch.full_like(u, float('nan')), torch.zeros_like(u_lo)
      ops.spmm_rhs(graph, w_csr, u, alpha, beta, x0, True, gather_lo=(u_lo, out_lo), stage=_lib.STAGE_RK2C, dt=DT, y=y, out_y=out_y)
      plain_k = torch.full_like(u, float('nan'))
      ops.spmm_rhs(graph, w_csr, u, alpha, beta, x0, True, gather_lo=(u_lo, None), stage=_lib.STAGE_RHS, out_k=plain_k)
    finally:
      _lib.check(_lib.lib().gnpde_tune(_lib.TUNE_LO_MAPPING, 0))
    res[mapping] = (plain, out_y, out_lo, plain_k)
  for a, b in zip(res[1], res[2]):
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
  ref = R.spmm(ei, _weights(ei.size(1), 5).double(), n, u_lo.float().cpu().double())
  assert_parity(res[2][0], ref, what='quad mapping d=%d' % d)


def test_stage_shadow_must_not_be_the_gathered_one(dev):
  n, d = 64, 24
  ei = random_graph(n, 4, seed=1)
  graph = G.CSRGraph(ei.to(dev), n)
  w_csr = ops.edge_to_csr_mean(graph, _weights(ei.size(1), 2).to(dev))
  u = torch.randn(n, d, device=dev)
  lo = ops.to_bf16(u)
  with pytest.raises(_lib.GnpdeError, match='must not write the shadow it gathers from'):
    ops.spmm_rhs(graph, w_csr, u, torch.tensor(0.1, device=dev), gather_lo=(lo, lo), stage=_lib.STAGE_RK1C, dt=0.5,
                 out_y=torch.empty_like(u))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. whole solves against the reference's own fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
FUNCS = {'laplacian': G.LaplacianODEFunc, 'transformer': G.ODEFuncTransformerAtt, 'GAT': G.ODEFuncAtt}
SOLVE_FIXTURES = ['block_constant_laplacian_euler', 'block_constant_transformer_rk4', 'block_constant_transformer_euler_h05']


def _restated_rhs(fx, round_gather):
  """float64 f(t, y) of a constant-block fixture from the oracle's pieces; round_gather: the neighbour rows the aggregation gathers
  pass through bf16 (the attention, the row's own term and the source term do not)."""
  opt = fx.opt
  p = {k: v.double() for k, v in fx.params.items()}
  x = fx.t('x').double()
  n = x.shape[0]
  ei = fx.t('edge_index')
  pre = 'odefunc.'
  gathered = (lambda y: y.float().to(torch.bfloat16).double()) if round_gather else (lambda y: y)
  if opt['function'] == 'laplacian':
    edge, w = R.get_rw_adj(ei, None, 1, opt['self_loop_weight'], n, dtype=torch.float64)
    weights = lambda y: w      # noqa: E731
  else:
    edge, _ = R.add_remaining_self_loops(ei, None, opt['self_loop_weight'], int(ei.max()) + 1)
    lay = pre + 'multihead_att_layer.'

    def weights(y):
      att, _ = R.transformer_attention(y, edge, p[lay + 'Q.weight'], p[lay + 'Q.bias'], p[lay + 'K.weight'], p[lay + 'K.bias'],
                                       opt['heads'], attention_type=opt['attention_type'], norm_idx=opt['attention_norm_idx'],
                                       square_plus=opt['square_plus'])
      return att.mean(dim=1)

  def f(t, y):
    ax = R.spmm(edge, weights(y), n, gathered(y))
    return R._epilogue(ax, y, p[pre + 'alpha_train'], p[pre + 'beta_train'], x, opt['no_alpha_sigmoid'], opt['add_source'])
  return f


def _rel_l2(a, b):
  a, b = a.detach().double().cpu(), b.detach().double().cpu()
  return float((a - b).norm() / b.norm())


def _block(fx, dev, opt):
  x = fx.t('x', dev)
  block = G.ConstantODEblock(FUNCS[opt['function']], [], opt, Data(x, fx.t('edge_index', dev)), dev,
                             t=torch.tensor([0, opt['time']])).to(dev)
  block.load_state_dict(fx.params, strict=True)
  return block.eval(), x


def _forward(block, x):
  block.odefunc.nfe = 0
  block.set_x0(x)
  with torch.no_grad():
    return block(x)


@pytest.mark.parametrize('name', SOLVE_FIXTURES)
def test_whole_solve_moves_by_what_the_rounding_predicts(dev, name, monkeypatch):
  """D_gpu (native solve, option on vs off) against D_ref (float64 restatement, gather operand through bf16 vs not), relative l2:
  0.9 D_ref <= D_gpu <= 1.1 D_ref.  The lower side shows the mode ran.  (Not 1e-5 against the rounded restatement: a value whose fp32
  and float64 forms round to different bf16 neighbours moves an output by up to alpha' w 2^-8 |x|.)"""
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  fx = Fixture(name)
  opt = fx.opt
  x64 = fx.t('x').double()
  z_plain = R.odeint_fixed(_restated_rhs(fx, False), x64, opt['time'], opt['step_size'], opt['method'])
  assert _rel_l2(z_plain, fx.t('z')) <= 5e-7, 'the float64 restatement does not reproduce the fixture'
  z_round = R.odeint_fixed(_restated_rhs(fx, True), x64, opt['time'], opt['step_size'], opt['method'])
  d_ref = _rel_l2(z_round, z_plain)

  block, x = _block(fx, dev, dict(opt))
  z_before = _forward(block, x)                    # before the option was ever set on this function
  assert block.odefunc.gather_dtype_used == 'fp32'
  assert_parity(z_before, fx.t('z'), what=name + ' (option absent)')
  block.odefunc.opt['gnpde_gather_dtype'] = 'bf16'
  z_lo = _forward(block, x)
  assert block.odefunc.gather_dtype_used == 'bf16'
  assert block.odefunc.nfe == int(fx.arr['nfe'])
  assert z_lo.dtype == torch.float32 and torch.isfinite(z_lo).all()
  z_lo2 = _forward(block, x)
  assert torch.equal(z_lo, z_lo2), 'the mode is not deterministic'
  del block.odefunc.opt['gnpde_gather_dtype']
  z_after = _forward(block, x)
  assert block.odefunc.gather_dtype_used == 'fp32'
  assert torch.equal(z_after, z_before), 'the default path changed after the option was used'
  block.odefunc.opt['gnpde_gather_dtype'] = 'fp32'
  assert torch.equal(_forward(block, x), z_before) and block.odefunc.gather_dtype_used == 'fp32'

  d_gpu = _rel_l2(z_lo, z_before)
  print('%s: D_ref %.4e  D_gpu %.4e  ratio %.4f' % (name, d_ref, d_gpu, d_gpu / d_ref))
  assert 0.9 * d_ref <= d_gpu <= 1.1 * d_ref, 'D_gpu / D_ref = %.4f (D_ref %.3e, D_gpu %.3e)' % (d_gpu / d_ref, d_ref, d_gpu)


def test_environment_form_of_the_option(dev, monkeypatch):
  """GNPDE_GATHER_DTYPE=bf16 switches the mode on for functions whose opt does not name it (how an unchanged benchmark times it);
  opt wins over the environment."""
  fx = Fixture('block_constant_transformer_rk4')
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  block, x = _block(fx, dev, dict(fx.opt))
  z32 = _forward(block, x)
  monkeypatch.setenv('GNPDE_GATHER_DTYPE', 'bf16')
  z16 = _forward(block, x)
  assert block.odefunc.gather_dtype_used == 'bf16' and not torch.equal(z16, z32)
  block.odefunc.opt['gnpde_gather_dtype'] = 'fp32'
  assert torch.equal(_forward(block, x), z32) and block.odefunc.gather_dtype_used == 'fp32'


def test_midpoint_and_classic_rk4_and_eager_launches(dev, monkeypatch):
  """The stage-input shadows of midpoint and of the torchdiffeq-order rk4 stages, and the launches outside a captured graph: each
  within 10 % of the float64 prediction as above, on the laplacian and the transformer fixture."""
  import functools
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  for name in ('block_constant_laplacian_euler', 'block_constant_transformer_rk4'):
    fx = Fixture(name)
    for method, classic, use_graph in (('midpoint', 0, True), ('rk4', 1, True), ('rk4', 0, False), ('euler', 0, False)):
      opt = dict(fx.opt, method=method, step_size=0.5, time=2.2)
      x64 = fx.t('x').double()
      fx2 = copy.copy(fx)
      fx2.opt = opt
      z_plain = R.odeint_fixed(_restated_rhs(fx2, False), x64, opt['time'], opt['step_size'], method)
      z_round = R.odeint_fixed(_restated_rhs(fx2, True), x64, opt['time'], opt['step_size'], method)
      d_ref = _rel_l2(z_round, z_plain)
      block, x = _block(fx, dev, opt)
      if not use_graph:
        block.test_integrator = functools.partial(G.odeint, use_graph=False)
      _lib.check(_lib.lib().gnpde_tune(_lib.TUNE_RK4_CLASSIC, classic))
      try:
        z32 = _forward(block, x)
        assert_parity(z32, z_plain, what='%s %s fp32' % (name, method))
        block.odefunc.opt['gnpde_gather_dtype'] = 'bf16'
        z16 = _forward(block, x)
      finally:
        _lib.check(_lib.lib().gnpde_tune(_lib.TUNE_RK4_CLASSIC, 0))
      assert block.odefunc.gather_dtype_used == 'bf16'
      d_gpu = _rel_l2(z16, z32)
      print('%s %s classic=%d graph=%s: D_ref %.4e D_gpu %.4e ratio %.4f' % (name, method, classic, use_graph, d_ref, d_gpu, d_gpu / d_ref))
      assert 0.9 * d_ref <= d_gpu <= 1.1 * d_ref


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. scope
# ---------------------------------------------------------------------------------------------------------------------------------
def _synthetic_block(dev, d, method, seed=0, function='transformer'):
  opt = dict(heads=4, attention_dim=16, attention_type='scaled_dot', attention_norm_idx=0, square_plus=False,
             reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=1000,
             add_source=True, no_alpha_sigmoid=False, mix_features=False, hidden_dim=d, augment=False, adjoint=False,
             tol_scale=1.0, data_norm='rw', method=method, step_size=1.0, max_iters=100, block='constant',
             function=function, time=2.0)
  n = 400
  ei = random_graph(n, 5, seed=seed)
  g = torch.Generator().manual_seed(seed + 1)
  x = torch.randn(n, d, generator=g).to(dev)
  block = G.ConstantODEblock(FUNCS[function], [], opt, Data(x, ei.to(dev)), dev, t=torch.tensor([0, opt['time']])).to(dev)
  with torch.no_grad():
    for p in block.parameters():
      if p.dim() >= 2:
        p.copy_(torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5)
    block.odefunc.beta_train.fill_(0.1)
  return block.eval(), x


@pytest.mark.parametrize('case', ['grad', 'dopri5', 'd22'])
def test_out_of_scope_solves_run_fp32_exactly_as_before(dev, case, monkeypatch):
  """Under autograd, with an adaptive method, and at a width without 16-byte rows of its own (d = 22) the option changes nothing:
  bit-identical to the solve without it, and the function reports 'fp32'."""
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  d = 22 if case == 'd22' else 32
  method = 'dopri5' if case == 'dopri5' else 'rk4'
  block, x = _synthetic_block(dev, d, method)

  def forward():
    block.odefunc.nfe = 0
    block.set_x0(x)
    if case == 'grad':
      block.train()
      with torch.enable_grad():
        return block(x.clone().requires_grad_(True)).detach()
    with torch.no_grad():
      return block(x)

  z0 = forward()
  block.odefunc.opt['gnpde_gather_dtype'] = 'bf16'
  z1 = forward()
  assert block.odefunc.gather_dtype_used == 'fp32'
  assert torch.equal(z0, z1)
  if case != 'grad':      # ... while the same function in scope does take the mode
    block2, x2 = _synthetic_block(dev, 32, 'rk4')
    block2.odefunc.opt['gnpde_gather_dtype'] = 'bf16'
    _forward(block2, x2)
    assert block2.odefunc.gather_dtype_used == 'bf16'


def test_adjoint_training_step_keeps_fp32(dev, monkeypatch):
  """opt['adjoint']: the forward solve of the adjoint method runs under no_grad inside the autograd function -- it is part of
  training and keeps the fp32 operand: output and gradients bit-identical with and without the option."""
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  fx = Fixture('adjoint_constant_transformer_rk4_rk4')
  assert fx.opt['adjoint']
  block, x = _block(fx, dev, dict(fx.opt))
  block.train()

  def step():
    block.zero_grad()
    block.odefunc.nfe = 0
    block.set_x0(x)
    xin = x.clone().requires_grad_(True)
    with torch.enable_grad():
      z = block(xin)
      z.square().sum().backward()
    return z.detach().clone(), xin.grad.clone()

  z0, g0 = step()
  block.odefunc.opt['gnpde_gather_dtype'] = 'bf16'
  z1, g1 = step()
  assert block.odefunc.gather_dtype_used == 'fp32'
  assert torch.equal(z0, z1) and torch.equal(g0, g1)


def test_bad_option_value_raises(dev, monkeypatch):
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  block, x = _synthetic_block(dev, 32, 'rk4')
  block.odefunc.opt['gnpde_gather_dtype'] = 'fp16'
  block.set_x0(x)
  with torch.no_grad(), pytest.raises(ValueError, match='gnpde_gather_dtype'):
    block(x)
  block.odefunc.opt['method'] = 'dopri5'      # whatever path the solve would take
  with torch.no_grad(), pytest.raises(ValueError, match='gnpde_gather_dtype'):
    G.odeint(block.odefunc, x, torch.tensor([0.0, 1.0], device=dev), method='dopri5')


def test_gat_function_takes_the_mode(dev, monkeypatch):
  """GAT: attention launches of its own + the same aggregation.  A loose sanity band here (the tight statement is test 4's): the
  deviation is there and is of the order of the rounding."""
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  block, x = _synthetic_block(dev, 32, 'rk4', function='GAT')
  z32 = _forward(block, x)
  block.odefunc.opt['gnpde_gather_dtype'] = 'bf16'
  z16 = _forward(block, x)
  assert block.odefunc.gather_dtype_used == 'bf16'
  dist = _rel_l2(z16, z32)
  assert 0 < dist < 4 * U_BF16, dist


@pytest.mark.parametrize('function', ['laplacian', 'transformer'])
def test_early_stop_evaluator_and_relabelled_graph_take_the_mode(dev, function, monkeypatch):
  """rk4 with the in-graph early-stopping evaluator, on the graph as given and on the relabelled one (graph.LocalityView): the mode
  runs in all of them, and -- as in fp32 -- the relabelling changes no bit of the state and no hit count."""
  from gnpde_amd import synthetic
  monkeypatch.delenv('GNPDE_GATHER_DTYPE', raising=False)
  n, d, c = 5000, 64, 40
  ei = torch.as_tensor(synthetic.community_powerlaw_graph(n, 30000, seed=6, n_comm=10)[0])
  g = torch.Generator().manual_seed(9)
  x = torch.randn(n, d, generator=g)
  labels = torch.randint(0, c, (n,), generator=g)
  role = torch.randperm(n, generator=g)
  masks = [role < 1000, (role >= 1000) & (role < 2500), role >= 2500]
  fx = Fixture('early_rk4_laplacian_arxiv')
  opt = dict(fx.opt, block='constant', function=function, time=4.0, step_size=1.0, hidden_dim=d, dataset='Cora',
             heads=4, attention_dim=16, attention_type='scaled_dot', attention_norm_idx=0, square_plus=False, reweight_attention=False,
             beltrami=False, mix_features=False)
  data = Data(x.to(dev), ei.to(dev))
  data.y = labels.to(dev)
  data.train_mask, data.val_mask, data.test_mask = [m.to(dev) for m in masks]
  block = G.ConstantODEblock(FUNCS[function], [], opt, data, dev, t=torch.tensor([0, opt['time']])).to(dev)
  with torch.no_grad():
    block.odefunc.alpha_train.fill_(0.3)
    block.odefunc.beta_train.fill_(0.2)
  integ = G.EarlyStopInt(opt['time'], opt, dev)
  integ.keep_trace = True
  integ.data, integ.m2_weight, integ.m2_bias = data, torch.randn(c, d, generator=g).to(dev), (torch.randn(c, generator=g) * 0.1).to(dev)
  block.test_integrator = integ
  block.eval()
  block.set_x0(x.to(dev))
  res = {}
  for gather in ('fp32', 'bf16'):
    block.odefunc.opt['gnpde_gather_dtype'] = gather
    for mode in ('0', 'parts', 'degree'):
      block.odefunc.opt['gnpde_reorder'] = mode
      with torch.no_grad():
        z = block(x.to(dev)).clone()
      assert block.odefunc.gather_dtype_used == gather
      sol = integ.solver
      assert len(sol.trace) == int(opt['earlystopxT'] * opt['time'])
      res[gather, mode] = (z, [(r['time'], tuple(r['hits'])) for r in sol.trace])
  for mode in ('parts', 'degree'):
    assert torch.equal(res['bf16', '0'][0], res['bf16', mode][0])
    assert res['bf16', '0'][1] == res['bf16', mode][1]
  dist = _rel_l2(res['bf16', '0'][0], res['fp32', '0'][0])
  assert 0 < dist < 4 * U_BF16, dist


def test_set_gather_and_set_tape_exclude_each_other(dev):
  n, d = 200, 32
  ei = random_graph(n, 5, seed=4)
  graph = G.CSRGraph(ei.to(dev), n)
  w_csr = ops.edge_to_csr_mean(graph, _weights(ei.size(1), 2).to(dev))
  y = torch.randn(n, d, device=dev)
  alpha = torch.tensor(0.2, device=dev)
  desc = ops.RhsDescriptor(_lib.RHS_LAPLACIAN, graph, d, d, alpha, None, None, True, w_csr=w_csr)
  s = ops.FixedStepSolver(desc, 'rk4', [0.5, 0.5], dev)
  y32 = s.run(y.clone(), use_graph=True).clone()
  s.set_gather('bf16')
  with pytest.raises(_lib.GnpdeError, match='solver_set_tape: a recorded solve keeps the fp32 gather operand'):
    s.set_tape(True)
  y16 = s.run(y.clone(), use_graph=True).clone()
  assert not torch.equal(y16, y32)
  assert torch.equal(s.run(y.clone(), use_graph=False), y16), 'captured and eager launches differ in the mode'
  s.set_gather('fp32')                              # detaches, drops the captured graph
  assert torch.equal(s.run(y.clone(), use_graph=True), y32)
  s.set_tape(True)
  with pytest.raises(_lib.GnpdeError, match='solver_set_gather: a recorded solve keeps the fp32 gather operand'):
    s.set_gather('bf16')
  s.set_tape(False)
  s.set_gather('bf16')
  assert torch.equal(s.run(y.clone(), use_graph=True), y16)
  with pytest.raises(ValueError):
    s.set_gather('fp16')
  # a width without 16-byte lanes: refused with a message, never a silent fp32 run
  y22 = torch.randn(n, 22, device=dev)
  desc22 = ops.RhsDescriptor(_lib.RHS_LAPLACIAN, graph, 22, 22, alpha, None, None, True, w_csr=w_csr)
  s22 = ops.FixedStepSolver(desc22, 'euler', [0.5], dev)
  with pytest.raises(_lib.GnpdeError, match='16-byte lanes'):
    s22.set_gather('bf16')
  s22.run(y22)
