"""GRAND-nl and GAT trained through dopri5 WITHOUT the adjoint method (`python run_GNN.py --function transformer` with no other flag)
on the native recorded solve: forward = the device-controlled dopri5 leaving the accepted steps' stage inputs on a tape
(csrc/dopri5.hip), backward = the walk of csrc/tape_reverse.h with one VJP stage of csrc/adjoint.hip per recorded evaluation
(gnpde_adjoint_set_dopri5_tape) -- against
  * the reference's own gradients (tests/golden/nltrain_*.npz: reference src/ over oracle/shims, torch autograd through torchdiffeq),
  * this package's differentiable host loop over the kernel-backed autograd Functions (opt['gnpde_host_dopri5_training']),
  * float64 torch autograd through a differentiable replay of the DEVICE's accepted steps on the CPU oracle right-hand side,
and the safety nets of the Laplacian path (tape growth, live record, stale tape, growth cap, max_nfe) on a GRAND-nl block."""
import gc
import importlib

import pytest
import torch

import gnpde_amd as G
from helpers import Fixture, fixtures, assert_parity
from nl_dopri5_oracle import oracle_rhs, replay
from test_tape_gpu import _module_scaled, _fixture_block, _train_once, _fixed_block
from test_split_kernel_stage_gpu import _block as _split_block

pytestmark = pytest.mark.gpu

O = importlib.import_module('gnpde_amd.odeint')
R = importlib.import_module('gnpde_amd.routes')
MaxNFEException = importlib.import_module('gnpde_amd.utils').MaxNFEException
NATIVE = 'native recorded-tape dopri5'
NAMES = fixtures('nltrain_')


def _set_host(block, value):
  block.odefunc.opt['gnpde_host_dopri5_training'] = value
  block.reg_odefunc.odefunc.opt['gnpde_host_dopri5_training'] = value


def _solver(f):
  return next(iter(f.__dict__['_tape_state'].values()))['solver']


# ---- 1. the reference's own gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('host_loop', [False, True])
def test_training_without_adjoint_against_the_reference(dev, name, host_loop):
  assert len(NAMES) == 7
  fx = Fixture(name)
  block, x = _fixture_block(fx, dev, gnpde_host_dopri5_training=host_loop)
  block.train()
  assert block.train_integrator is G.odeint
  xin = x.clone().requires_grad_(True)
  block.set_x0(xin)
  z = block(xin)
  assert z.requires_grad
  f = block.odefunc
  path = str(getattr(f, '_last_train_solve', ''))
  assert path.startswith(NATIVE) == (not host_loop), 'solve path: %r' % path
  assert f.nfe == int(fx.arr['nfe']), 'nfe %d vs reference %d' % (f.nfe, int(fx.arr['nfe']))
  if not host_loop:      # a rejected trial step leaves nothing on the record
    stats = f._dopri5_stats
    ratios = fx.arr['ratios']
    assert stats['accepted'] == int((ratios <= 1).sum()) and stats['rejected'] == int((ratios > 1).sum()), (stats, ratios)
    assert _solver(f).tape_steps() == stats['accepted']
  assert_parity(z, fx.t('z'), max(1e-5, 2 * fx.opt['tol_scale'] * 1e-7), name + ' z')
  (z * fx.t('c', dev)).sum().backward()
  assert f.nfe == int(fx.arr['nfe_after_backward'])        # the reference's backward evaluates nothing either
  gtol = 2e-4
  assert_parity(xin.grad, fx.t('grad_x'), gtol, name + ' grad_x')
  refs = {k[5:]: fx.t(k) for k in fx.arr if k.startswith('grad/')}
  grads = dict((k, p.grad) for k, p in block.named_parameters())
  _module_scaled(grads, refs, gtol, name)
  for k, p in block.named_parameters():
    if k not in refs:
      assert p.grad is None or float(p.grad.abs().max()) == 0.0, '%s received a gradient the reference does not produce' % k


# ---- 2. recorded solve against the host loop, every kernel path of the stage ---------------------------------------------------------
# (tol_scale = 20: the two solves take step sizes that differ by the rounding in their error estimates; at rtol = 2e-6 what that moves in z
#  and in the gradients stays an order below the bars, and the controller's ratios -- about 0.6 -- stay clear of 1 on both sides)
CASES = {
  # hub rows: longer than one 512-entry chunk of the row kernel and of the attention backward
  'hubs': dict(kind='transformer', n=1500, d=32, heads=4, A=16, time=3.0, tol_scale=20.0, hubs=2, hub_deg=700),
  # a width that is no multiple of 4: padded rows
  'padded_d22': dict(kind='transformer', n=600, d=22, heads=2, A=8, time=2.5, tol_scale=20.0),
  # d_k = 2: d q / d k by the generic head-SpMM
  'dk2': dict(kind='transformer', n=500, d=16, heads=4, A=8, time=2.5, tol_scale=20.0),
  'h8_squareplus_columns': dict(kind='transformer', n=600, d=32, heads=8, A=32, time=2.5, tol_scale=20.0, square_plus=True, attention_norm_idx=1),
  'exp_kernel': dict(kind='transformer', n=600, d=32, heads=4, A=16, time=2.5, tol_scale=20.0, attention_type='exp_kernel'),
  'pearson': dict(kind='transformer', n=600, d=32, heads=4, A=32, time=2.5, tol_scale=20.0, attention_type='pearson'),
  'gat_h2_columns': dict(kind='GAT', n=600, d=32, heads=2, A=32, time=2.5, tol_scale=20.0, attention_norm_idx=1),
  'gat_h8_columns': dict(kind='GAT', n=600, d=32, heads=8, A=32, time=2.5, tol_scale=20.0, attention_norm_idx=1),
  'raw_alpha': dict(kind='transformer', n=600, d=32, heads=4, A=16, time=2.5, tol_scale=20.0, no_alpha_sigmoid=True),
  # the BLEND split kernel: beltrami + exp_kernel, two label columns behind the positional block
  'split_kernel': dict(split=True, n=600, d=22, heads=2, A=16, f0=12, p0=8, time=2.5, tol_scale=20.0),
}


def _case_block(dev, case, seed=61):
  kw = dict(CASES[case])
  if kw.pop('split', False):
    return _split_block(dev, seed=seed, method='dopri5', **kw)
  return _fixed_block(dev, block_kind='constant', seed=seed, method='dopri5', **kw)


def _same_steps_once(block, x, dev, c, hs, xfrac):
  """The host loop's arithmetic -- the kernel-backed autograd Functions of the block's function, one per evaluation, torch autograd
  through them -- on GIVEN step sizes: (z, dL/dx, parameter gradients)."""
  for p in block.parameters():
    p.grad = None
  block.train()
  xin = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xin)
  z = replay(block.odefunc, xin, hs, xfrac)
  (z * c).sum().backward()
  return z.detach(), xin.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in block.named_parameters()}


# What the comparison with the host loop can hold.  The two solves run the same formulae, but their error estimates round differently
# (torch reductions on one side, a double-precision fold on the other), so their accepted step sizes differ by 1e-4 .. 2e-2 relative.
# z does not care (shares of the 1e-5 bar <= 0.44 over every case and seed below).  The GRADIENT of the discrete solution does where the
# attention is normalised over columns: measured on one MI355X at seeds 61 / 62 / 63, recorded solve against the adaptive host loop,
# largest share of the 2e-4 bar: squareplus over columns with 8 heads 4.3 / 8.5 / 10.7 (steps differ 3e-3), GAT with 8 heads over
# columns 1.5 / 3.9 / 11.3 (steps differ 7e-5 .. 7e-4: a LeakyReLU argument changes side), every row-normalised case <= 0.85 -- while
# EACH side agrees with float64 autograd through a replay of ITS OWN steps (host loop <= 0.16, recorded solve <= 0.09), and the two
# sides agree on the SAME steps (<= 0.04).  So the adaptive host loop is asked for what it can give -- the evaluation count and z --
# and the gradients are compared where the comparison is about the sweep: the host loop's arithmetic (its kernel-backed autograd
# Functions, one per evaluation, torch autograd through them) replayed on the recorded solve's step sizes.
# test_each_side_matches_float64_through_its_own_steps keeps the evidence for the two sensitive cases in the suite.
# Seeds: 61 and 62 for every case.  Two (case, seed) pairs are not used, for reasons on the reference's side: 'hubs' at 61 -- the host
# loop's own d alpha_train, a small difference of large sums there, is 1.67 bars off float64 through its own steps (the sweep: 0.33) --
# takes 63 instead; 'gat_h2_columns' at 63 has the two controllers disagree on a rejection (62 / 68 evaluations).
SEEDS = {case: (61, 62) for case in CASES}
SEEDS['hubs'] = (62, 63)


def _host_steps(trace, T):
  """(step sizes, end-point fraction) of the accepted steps of a host-loop solve from its trial trace (t, dt, ratio)."""
  acc = [(t, dt) for t, dt, r in trace if r <= 1]
  return [dt for _, dt in acc], (T - acc[-1][0]) / acc[-1][1]


@pytest.mark.parametrize('case,seed', [(c, s) for c in sorted(CASES) for s in SEEDS[c]])
def test_recorded_solve_equals_the_host_loop(dev, case, seed):
  """Same block, same weights.  Against the adaptive host loop: the same accept / reject sequence (evaluation count) and z.  Against
  the host loop's arithmetic on the recorded solve's own step sizes: z and every gradient.  A second recorded iteration reproduces
  the first bit for bit (no float atomics anywhere)."""
  what = '%s/%d' % (case, seed)
  block, x = _case_block(dev, case, seed=seed)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
  z1, gx1, g1, nfe1 = _train_once(block, x, dev, c)
  f = block.odefunc
  assert str(f._last_train_solve).startswith(NATIVE), f._last_train_solve
  assert f._dopri5_stats['accepted'] >= 2
  hs, xfrac = _solver(f).tape_record()
  _set_host(block, True)
  f._last_train_solve = ''     # (the host loop leaves the attribute alone)
  z2, gx2, g2, nfe2 = _train_once(block, x, dev, c)
  assert not str(f._last_train_solve).startswith('native recorded'), f._last_train_solve
  assert nfe1 == nfe2, (nfe1, nfe2)
  assert_parity(z1, z2, 1e-5, what + ' z against the adaptive host loop')
  zs, gxs, gs = _same_steps_once(block, x, dev, c, hs, xfrac)
  assert_parity(z1, zs, 1e-5, what + ' z on the same steps')
  assert_parity(gx1, gxs, 2e-4, what + ' grad_x on the same steps')
  refs = {k: v for k, v in gs.items() if v is not None}
  assert refs and set(refs) == set(k for k, v in g2.items() if v is not None), 'parameters with a gradient: %s' % sorted(refs)
  _module_scaled(g1, refs, 2e-4, what)
  for k, v in g1.items():
    if k not in refs:
      assert v is None or float(v.abs().max()) == 0.0, '%s received a gradient the host loop does not produce' % k
  _set_host(block, False)
  z3, gx3, g3, _ = _train_once(block, x, dev, c)
  assert str(f._last_train_solve).startswith(NATIVE)
  assert torch.equal(z1, z3) and torch.equal(gx1, gx3)
  for k, v in g1.items():
    if v is not None:
      assert torch.equal(v, g3[k]), k


def _float64_through(block, x, c, hs, xfrac):
  """(z, dL/dx, parameter gradients) of float64 torch autograd through a replay of the given steps on the CPU oracle right-hand side."""
  f = block.odefunc
  f64 = torch.float64
  p = {k: v.detach().cpu().to(f64).requires_grad_(True) for k, v in block.named_parameters()}
  x64 = x.to(f64).clone().requires_grad_(True)
  # (the function's edge list has its self loops: adding the remaining ones is idempotent)
  out = replay(oracle_rhs(f.opt, p, f.edge_index.cpu(), x.to(f64)), x64, hs, xfrac)
  (out * c.cpu().to(f64)).sum().backward()
  return out.detach(), x64.grad, {k: v.grad for k, v in p.items() if v.grad is not None and float(v.grad.abs().max()) > 0.0}


@pytest.mark.parametrize('case', ['h8_squareplus_columns', 'gat_h8_columns'])
def test_each_side_matches_float64_through_its_own_steps(dev, case):
  """The two cases whose gradients move with the step sizes (see above): the recorded solve AND the adaptive host loop are each held
  against float64 autograd through a replay of their own accepted steps, at the bars of the host-loop comparison -- neither side is
  wrong, they differentiate two slightly different discrete solves."""
  block, x = _case_block(dev, case)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
  f = block.odefunc
  T = float(f.opt['time'])
  z1, gx1, g1, _ = _train_once(block, x, dev, c)
  hs, xfrac = _solver(f).tape_record()
  _set_host(block, True)
  O._TRIAL_TRACE = []
  try:
    z2, gx2, g2, _ = _train_once(block, x, dev, c)
    trace = O._TRIAL_TRACE
  finally:
    O._TRIAL_TRACE = None
  for side, (z, gx, g), steps in (('recorded solve', (z1, gx1, g1), (hs, xfrac)), ('host loop', (z2, gx2, g2), _host_steps(trace, T))):
    zo, gxo, go = _float64_through(block, x, c, *steps)
    assert_parity(z, zo, 2e-5, '%s: %s z vs float64' % (case, side))
    assert_parity(gx, gxo, 2e-4, '%s: %s grad_x vs float64' % (case, side))
    _module_scaled({k: (None if v is None else v.cpu().to(torch.float64)) for k, v in g.items()}, go, 2e-4, '%s: %s vs float64' % (case, side))


# ---- 3. device gradients against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['h8_squareplus_columns', 'exp_kernel', 'gat_h2_columns', 'padded_d22'])
def test_recorded_gradients_against_float64_autograd(dev, case):
  """The device's own accepted step sizes and end-point fraction (sol.tape_record()) replayed in float64 on the CPU oracle right-hand
  side, torch autograd through the replay: independent of the float32 accept / reject decisions, so the bars are plain float32
  rounding (those of test_tape_gpu.py::test_recorded_gradients_against_the_float64_reverse_sweep)."""
  block, x = _case_block(dev, case, seed=71)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(8))
  z, gx, g, nfe = _train_once(block, x, dev, c.to(dev))
  f = block.odefunc
  assert str(f._last_train_solve).startswith(NATIVE)
  sol = _solver(f)
  hs, xfrac = sol.tape_record()
  S = sol.tape_steps()
  assert S == len(hs) == f._dopri5_stats['accepted'] >= 2
  T = float(f.opt['time'])
  assert abs(sum(hs[:-1]) + xfrac * hs[-1] - T) <= 1e-4 * T
  f64 = torch.float64
  out, gx64, refs = _float64_through(block, x, c, hs, xfrac)
  assert_parity(z, out, 2e-5, case + ' z vs float64')
  used = [float((gx.cpu().to(f64) - gx64).abs().max() / gx64.abs().max()) / 2e-4]
  assert_parity(gx, gx64, 2e-4, case + ' grad_x vs float64')
  assert 'odefunc.alpha_train' in refs and len(refs) >= 3
  scale = {}
  for k, ref in refs.items():
    mod = k.rsplit('.', 2)[0] if 'multihead' in k else k
    scale[mod] = max(scale.get(mod, 0.0), float(ref.abs().max()))
  for k, ref in refs.items():
    mod = k.rsplit('.', 2)[0] if 'multihead' in k else k
    used.append(float((g[k].cpu().to(f64).reshape(ref.shape) - ref).abs().max()) / scale[mod] / 2e-4)
  print('%s: largest share of the 2e-4 bar used %.3f (grad_x %.3f)' % (case, max(used), used[0]))
  _module_scaled({k: (None if v is None else v.cpu().to(f64)) for k, v in g.items()}, refs, 2e-4, case + ' vs float64')


# ---- 4. the safety nets, on a GRAND-nl block -----------------------------------------------------------------------------------------
LONG = 'nltrain_transformer_dopri5_rejects_many'      # 15 accepted steps: more than the smallest tape holds


def test_tape_grows_when_a_solve_accepts_more_steps_than_it_holds(dev, monkeypatch):
  monkeypatch.setattr(O, '_TAPE_BUDGET_BYTES', 1)          # -> the smallest tape (8 slots)
  fx = Fixture(LONG)
  block, x = _fixture_block(fx, dev)
  z, gx, g, nfe = _train_once(block, x, dev, fx.t('c', dev))
  f = block.odefunc
  assert str(f._last_train_solve).startswith(NATIVE)
  assert f._dopri5_stats['accepted'] > 8 and _solver(f).tape_capacity >= f._dopri5_stats['accepted']
  assert nfe == int(fx.arr['nfe'])          # (the solve that did not fit is not counted twice)
  assert_parity(gx, fx.t('grad_x'), 2e-4, 'grad_x after the tape grew')
  _module_scaled(g, {k[5:]: fx.t(k) for k in fx.arr if k.startswith('grad/')}, 2e-4, 'after the tape grew')


def test_two_forwards_before_one_backward_stay_differentiable(dev):
  block, x = _case_block(dev, 'dk2', seed=51)
  block.train()
  xa = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xa)
  za = block(xa)
  assert str(block.odefunc._last_train_solve).startswith(NATIVE)
  xb = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xb)
  zb = block(xb)
  assert str(block.odefunc._last_train_solve).startswith('differentiable host loop')
  zb.sum().backward()
  za.sum().backward()
  assert_parity(xa.grad, xb.grad, 2e-4, 'grad_x of the recorded pass vs the host-loop pass')
  # the record is free again: the next pass is recorded
  xc = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xc)
  block(xc).sum().backward()
  assert str(block.odefunc._last_train_solve).startswith(NATIVE)
  # an abandoned forward pass (output dropped, no backward) does not block the record either
  xd = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xd)
  zd = block(xd)
  del zd
  gc.collect()
  xe = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xe)
  block(xe)
  assert str(block.odefunc._last_train_solve).startswith(NATIVE)


def test_stale_tape_raises(dev, monkeypatch):
  """Forward A (short), the live-record marker cleared, forward B that outgrows the 8-slot tape: A's backward raises instead of
  differentiating B's record; B's runs."""
  monkeypatch.setattr(O, '_TAPE_BUDGET_BYTES', 1)
  fx = Fixture(LONG)
  block, x = _fixture_block(fx, dev)
  block.train()
  f = block.odefunc
  xa = x.clone().requires_grad_(True)
  block.set_x0(xa)
  t_long = block.t.clone()
  block.t = torch.tensor([0.0, 0.5]).to(dev)              # a short solve: fits the 8 slots
  za = block(xa)
  sol = _solver(f)
  assert sol.tape_capacity == 8
  gen_a = sol.tape_generation
  f.__dict__.pop('_tape_live_dopri5')                      # (pretend A's pass is not waiting: the case the stamp exists for)
  block.t = t_long
  xb = x.clone().requires_grad_(True)
  block.set_x0(xb)
  zb = block(xb)
  assert str(f._last_train_solve).startswith(NATIVE)
  sol_b = _solver(f)
  assert sol_b.tape_capacity > 8 and sol_b.tape_generation > gen_a
  with pytest.raises(G.GnpdeError):
    za.sum().backward()
  (zb * fx.t('c', dev)).sum().backward()
  assert_parity(xb.grad, fx.t('grad_x'), 2e-4, 'grad_x of the later pass')


def test_tape_growth_is_capped(dev, monkeypatch):
  monkeypatch.setattr(O, '_TAPE_BUDGET_BYTES', 1)
  monkeypatch.setattr(O, '_TAPE_GROWTH_CAP_BYTES', 1 << 10)
  fx = Fixture(LONG)
  block, x = _fixture_block(fx, dev)
  z1, gx1, g1, nfe1 = _train_once(block, x, dev, fx.t('c', dev))
  assert str(block.odefunc._last_train_solve).startswith('differentiable host loop'), block.odefunc._last_train_solve
  assert nfe1 == int(fx.arr['nfe'])
  monkeypatch.setattr(O, '_TAPE_GROWTH_CAP_BYTES', 96 << 30)
  z2, gx2, g2, nfe2 = _train_once(block, x, dev, fx.t('c', dev))
  assert str(block.odefunc._last_train_solve).startswith(NATIVE)
  assert nfe1 == nfe2
  assert_parity(gx1, gx2, 2e-4, 'grad_x host loop vs recorded')


def test_max_nfe_raises_as_the_host_loop_does(dev):
  fx = Fixture(LONG)
  left = []
  for host in (True, False):
    block, x = _fixture_block(fx, dev, gnpde_host_dopri5_training=host, max_nfe=40)
    block.train()
    xin = x.clone().requires_grad_(True)
    block.set_x0(xin)
    with pytest.raises(MaxNFEException):
      block(xin)
    left.append(block.odefunc.nfe)
  assert left[0] == left[1] == 41, left


# ---- 5. what keeps the host loop -----------------------------------------------------------------------------------------------------
def test_refusals_take_the_host_loop(dev):
  # mix_features (GAT: the reference's transformer function cannot run it at all)
  block, x = _fixed_block(dev, kind='GAT', block_kind='constant', n=300, d=16, heads=2, A=16, seed=81, method='dopri5', time=1.5, tol_scale=200.0,
                          mix_features=True)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(9)).to(dev)
  block.odefunc._last_train_solve = ''
  z, gx, g, nfe = _train_once(block, x, dev, c)
  assert not str(block.odefunc._last_train_solve).startswith('native recorded') and torch.isfinite(gx).all()
  # a caller's norm: the same function and state that are admitted without it
  block, x = _case_block(dev, 'dk2', seed=82)
  f = block.odefunc
  block.train()
  block.set_x0(x.to(dev))
  t = torch.tensor([0.0, 1.5], device=dev)
  state = x.to(dev).clone().requires_grad_(True)
  assert R.forward(f, state, t, 'dopri5', {}) == ('recorded_dopri5', None)
  assert R.forward(f, state, t, 'dopri5', {'norm': O._rms}) == ('host_loop', R.CALLER_NORM)
  f._last_train_solve = ''
  out = G.odeint(f, state, t, rtol=2e-5, atol=2e-7, method='dopri5', options={'norm': O._rms})[1]
  assert not str(f._last_train_solve).startswith('native recorded'), f._last_train_solve
  out.sum().backward()
  assert state.grad is not None and torch.isfinite(state.grad).all()
  # a tuple state: the block's own regularised solve (kinetic energy) integrates (x, r) through reg_odefunc, whose function -- admitted
  # with the plain state -- must not be recorded
  fns, _ = G.create_regularization_fns(dict(f.opt, kinetic_energy=0.1))
  assert len(fns) == 1
  block.reg_odefunc.regularization_fns, block.nreg = fns, 1
  inner = block.reg_odefunc.odefunc
  xin = x.to(dev).clone().requires_grad_(True)
  block.set_x0(xin)
  assert R.forward(inner, xin, block.t.to(dev), 'dopri5', {}) == ('recorded_dopri5', None)
  inner._last_train_solve = ''
  z, regs = block(xin)
  assert len(regs) == 1 and not str(inner._last_train_solve).startswith('native recorded'), inner._last_train_solve
  assert not inner.__dict__.get('_tape_state')
  (z.sum() + regs[0].mean()).backward()
  assert xin.grad is not None and torch.isfinite(xin.grad).all()
