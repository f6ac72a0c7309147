"""Native solves with several output times on the device: the routes, the refusals, bit-identity with the two-time native solves,
interior outputs against float64 interpolation, the adaptive outputs against the host loop and the restated torchdiffeq over the oracle,
adjoint gradients, ODEblock.trajectory / GNN.forward_at, max_nfe and the bf16 gather operand."""
import ctypes
import os

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
from oracle.shims import install as REF_TORCHDIFFEQ
from helpers import Data, Fixture, assert_parity, fixtures, parity
import output_times_cases as C

pytestmark = pytest.mark.gpu
O = C.O
T_FIXED = C.FIXED_TIMES
FIX = dict(options={'step_size': C.FIXED_STEP})


def _t(times, dev):
  return torch.tensor(times, dtype=torch.float32, device=dev)


def _solve(f, x, times, **kw):
  f.nfe = 0
  with torch.no_grad():
    return G.odeint(f, x, _t(times, x.device), **kw).clone()


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
  monkeypatch.delenv('GNPDE_HOST_OUTPUTS', raising=False)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_solvers_refuse_outputs_with_a_tape_or_an_evaluator(dev):
  blk, x, _ = C.make_block('a', dev)
  f = blk.odefunc
  y = _lib.alloc_state(x.shape[0], x.shape[1], dev).copy_(x)
  desc = f._descriptor(y)
  L = G.lib()
  dec = _lib.DecoderStruct()
  state = torch.zeros(8, dtype=torch.int32, device=dev)
  out = torch.empty(2, x.shape[0], x.shape[1], device=dev)
  fixed = ops.FixedStepSolver(desc, 'rk4', [0.5, 0.5], dev)
  with pytest.raises(G.GnpdeError, match='scratch'):      # an interior output without the scratch buffer
    _lib.check(L.gnpde_solver_set_outputs(fixed.handle, 1, (ctypes.c_int32 * 1)(1), (ctypes.c_float * 1)(0.5), _lib.ptr(out), out.stride(1), None))
  with pytest.raises(G.GnpdeError, match='step'):         # a step outside the grid
    fixed.set_outputs([(3, 1.0)], out[:1])
  fixed.set_outputs([(1, 0.5), (2, 1.0)], out)
  with pytest.raises(G.GnpdeError, match='output'):
    fixed.set_tape(True)
  assert L.gnpde_solver_set_early_stop(fixed.handle, ctypes.byref(dec), _lib.ptr(state), None, 0) == -1 and b'outputs' in L.gnpde_last_error()
  fixed.set_outputs(None)
  fixed.set_tape(True)
  with pytest.raises(G.GnpdeError, match='tape'):
    fixed.set_outputs([(2, 1.0)], out[:1])
  fixed.set_tape(False)
  fixed.close()
  # the row-partitioned engine's descriptors (a slice of the projection rows, halo rows behind the graph's rows, a row sub-range): each
  # of the three terms alone refuses, and the whole-graph descriptor is taken again afterwards
  st = desc.struct
  one = ((ctypes.c_int32 * 1)(2), (ctypes.c_float * 1)(1.0))
  for field, value in (('proj_row_end', 16), ('n_state_rows', x.shape[0] + 8), ('row_begin', 4)):
    holder = st.graph.contents if field == 'row_begin' else st
    keep = getattr(holder, field)
    setattr(holder, field, value)
    part = ops.FixedStepSolver(desc, 'rk4', [0.5, 0.5], dev)
    setattr(holder, field, keep)
    assert L.gnpde_solver_set_outputs(part.handle, 1, one[0], one[1], _lib.ptr(out), out.stride(1), None) == -1, field
    assert b'partitioned' in L.gnpde_last_error(), field
    part.close()
  whole = ops.FixedStepSolver(desc, 'rk4', [0.5, 0.5], dev)
  whole.set_outputs([(2, 1.0)], out[:1])
  whole.close()
  ad = ops.Dopri5Solver(desc, 1e-6, 1e-6, dev)
  ad.set_outputs([0.5, 1.0], out)
  with pytest.raises(G.GnpdeError, match='output'):
    ad.set_tape(8)
  assert L.gnpde_dopri5_set_early_stop(ad.handle, ctypes.byref(dec), _lib.ptr(state), None, 0, None, 0, 4) == -1 and b'outputs' in L.gnpde_last_error()
  with pytest.raises(G.GnpdeError, match='last output time'):      # t1 of the run must be the last output time
    ad.run(x, 0.0, 2.0, out[1])
  ad.set_outputs(None)
  ad.set_tape(8)
  with pytest.raises(G.GnpdeError, match='tape'):
    ad.set_outputs([0.5, 1.0], out)
  ad.close()


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def test_three_time_solves_take_the_native_routes(dev, monkeypatch):
  """The tests that fail without the feature: a three-time no-grad rk4 solve and a dopri5 solve run natively."""
  blk, x, _ = C.make_block('a', dev)
  f = blk.odefunc
  for slot in ('_solver_state', '_dopri5_device'):
    O._close_slot(f, slot)
  _solve(f, x, [0.0, 0.75, 1.5], method='rk4', **FIX)
  assert f._last_output_solve == 'native fixed grid' and f.__dict__.get('_solver_state') and f.nfe == 12
  _solve(f, x, [0.0, 0.75, 1.5], method='dopri5', rtol=1e-6, atol=1e-6)
  assert f._last_output_solve == 'native device controller' and f.__dict__.get('_dopri5_device')
  _solve(f, x, [0.0, 0.75, 1.5], method='adaptive_heun', rtol=1e-4, atol=1e-4)
  assert f._last_output_solve == 'native device controller'
  _solve(f, x, [0.0, 1.5, 0.75], method='rk4', **FIX)
  assert f._last_output_solve == 'host loop (output times are not strictly increasing)'
  f.opt['gnpde_host_outputs'] = True
  a = _solve(f, x, [0.0, 0.75, 1.5], method='rk4', **FIX)
  assert f._last_output_solve == 'host loop (gnpde_host_outputs)'
  del f.opt['gnpde_host_outputs']
  monkeypatch.setenv('GNPDE_HOST_OUTPUTS', '1')
  _solve(f, x, [0.0, 0.75, 1.5], method='dopri5', rtol=1e-6, atol=1e-6)
  assert f._last_output_solve == 'host loop (gnpde_host_outputs)'
  monkeypatch.delenv('GNPDE_HOST_OUTPUTS')
  b = _solve(f, x, [0.0, 0.75, 1.5], method='rk4', **FIX)
  assert f._last_output_solve == 'native fixed grid'
  assert_parity(b, a, what='native outputs vs host loop')


# ---- fixed grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,function,method', [('a', 'laplacian', 'rk4'), ('a', 'laplacian', 'euler'), ('a', 'laplacian', 'midpoint'),
                                                  ('b', 'laplacian', 'rk4'), ('b', 'laplacian', 'euler'), ('c', 'laplacian', 'rk4'),
                                                  ('c', 'laplacian', 'euler'), ('d', 'laplacian', 'rk4'), ('a', 'transformer', 'rk4'),
                                                  ('d', 'transformer', 'rk4'), ('c', 'transformer', 'euler')])
def test_fixed_grid_outputs(dev, case, function, method):
  blk, x, _ = C.make_block(case, dev, function=function)
  f = blk.odefunc
  kw = dict(method=method, **FIX)
  out = _solve(f, x, T_FIXED, **kw)
  nfe = f.nfe
  assert f._last_output_solve == 'native fixed grid' and out.shape == (len(T_FIXED),) + tuple(x.shape)
  if 'gnpde_reorder' in C.CASES[case]:
    assert next(iter(f._solver_state.values()))['view'] is not None, 'the case is meant to run on a relabelled graph'
  assert torch.equal(out[0], x)
  again = _solve(f, x, T_FIXED, **kw)               # a second replay
  eager = _solve(f, x, T_FIXED, use_graph=False, **kw)
  assert torch.equal(again, out) and torch.equal(eager, out)
  two = {tj: _solve(f, x, [0.0, tj], **kw)[1] for tj in (0.5, 1.0, 1.5, 2.0, 2.3)}
  assert f.nfe == nfe, 'NFE of the two-time solve over the same grid'
  for j, tj in enumerate(T_FIXED):
    if tj in two and j > 0:                         # grid points (dyadic: the grids of the shorter solves are the same floats) and the end
      assert torch.equal(out[j], two[tj]), 'output at t = %g' % tj
  # the interior output against the float64 interpolation of the two bracketing native states: seven roundings of 2^-24 at most
  ya, yb = two[1.0].double(), two[1.5].double()
  want = ya + 0.5 * (yb - ya)
  bound = 2.0 ** -21 * torch.maximum(ya.abs(), yb.abs())
  err = (out[2].double() - want).abs()
  print('interior output: worst error / bound = %.3f' % float((err / bound.clamp_min(1e-300)).max()))
  assert bool((err <= bound).all())


# ---- adaptive -----------------------------------------------------------------------------------------------------------------------
ADAPTIVE_CASES = sorted(C.ADAPTIVE)      # every shape under both pairs


def _adaptive_setup(case, pair, dev):
  A = C.adaptive(case, pair)
  blk, x, xc = C.make_block(case, dev, alpha_train=A['alpha_train'])
  kw = dict(method=pair, rtol=A['tol_scale'] * 1e-9, atol=A['tol_scale'] * 1e-7)
  f = blk.odefunc
  trace, host_two = C.host_trace(f, x, A['T'], pair, A['tol_scale'])      # the host loop over the native evaluations
  times = C.pick_times(trace, A['T'])
  C.check_times(trace, times)
  return blk, f, x, xc, kw, times, trace


@pytest.mark.parametrize('case,pair', ADAPTIVE_CASES)
def test_adaptive_outputs_do_not_change_the_solve(dev, case, pair):
  blk, f, x, xc, kw, times, trace = _adaptive_setup(case, pair, dev)
  a, b, b_lo, T = times[3], times[4], times[1], times[-1]
  for tps in (1, 8):
    opts = {'trials_per_sync': tps}
    two = _solve(f, x, [0.0, T], options=opts, **kw)
    nfe2, st2 = f.nfe, dict(f._dopri5_stats)
    out = _solve(f, x, times, options=opts, **kw)
    assert f._last_output_solve == 'native device controller'
    st = dict(f._dopri5_stats)
    assert torch.equal(out[-1], two[-1]) and torch.equal(out[0], x)
    assert f.nfe == nfe2 and (st['accepted'], st['rejected']) == (st2['accepted'], st2['rejected'])
    assert st['accepted'] + st['rejected'] == len(trace) and st['rejected'] == sum(1 for r in trace if r[2] > 1)
    s1 = _solve(f, x, [0.0, a, T], options=opts, **kw)
    s2 = _solve(f, x, [0.0, a, b, T], options=opts, **kw)
    s3 = _solve(f, x, [0.0, b_lo, a, T], options=opts, **kw)
    assert torch.equal(s1[1], out[3]) and torch.equal(s2[1], out[3]) and torch.equal(s3[2], out[3])
    assert torch.equal(s2[2], out[4]) and torch.equal(s3[1], out[1])
    assert torch.equal(s1[-1], two[-1]) and torch.equal(s2[-1], two[-1]) and torch.equal(s3[-1], two[-1])
    if tps == 1:
      first = out
  assert torch.equal(first, out), 'the batch size of the record reads changed an output'


def _against_references(blk, f, x, xc, kw, times, pair, sensitive=()):
  dev = x.device
  out = _solve(f, x, times, **kw)
  assert f._last_output_solve == 'native device controller'
  nfe = f.nfe
  f.nfe = 0
  with torch.no_grad():
    host = O._solve_dopri5(f, x, _t(times, dev), kw['rtol'], kw['atol'], tableau=pair)
  assert f.nfe == nfe
  calls = [0]
  rhs0 = C.oracle_laplacian(blk, xc)

  def rhs(tq, y):
    calls[0] += 1
    return rhs0(tq, y)
  ref = REF_TORCHDIFFEQ.odeint(rhs, xc, torch.tensor(times), method=pair, options={}, rtol=kw['rtol'], atol=kw['atol'])
  assert calls[0] == nfe
  for j in range(1, len(times)):
    print('output %d: vs host loop %.2e, vs restated torchdiffeq %.2e' % (j, parity(out[j], host[j])[0], parity(out[j], ref[j])[0]))
  for j in range(1, len(times)):
    assert_parity(out[j], host[j], tol=2e-5, what='output %d vs the host loop' % j)
    if j not in sensitive:      # (output_times_cases.EVAL_SENSITIVE: the references themselves move by more than the bound there)
      assert_parity(out[j], ref[j], tol=2e-5, what='output %d vs the restated torchdiffeq over the oracle' % j)
  return out, nfe


@pytest.mark.parametrize('case,pair', ADAPTIVE_CASES)
def test_adaptive_outputs_against_the_references(dev, case, pair):
  """Every output -- three inside one accepted step, one behind a rejected trial step, the end (check_times on the host loop's trace) --
  within 2e-5 of the host loop and of the restated torchdiffeq over the oracle, equal NFE.  The 2e-6 bound between the device and the
  host controller on native stages can be applied to the end point only: that controller (options eager_stages) is a two-time route,
  with more output times the option takes the host loop compared above; it exists for dopri5 alone.  Measured on the MI355X for case d
  under adaptive_heun, output 4 (behind the rejected step): 7.1e-6 from the host loop, 5.7e-5 from the restated torchdiffeq over the
  oracle, whose own movement under another rounding of f is 6e-5 there (EVAL_SENSITIVE): that one figure is printed, not asserted."""
  blk, f, x, xc, kw, times, trace = _adaptive_setup(case, pair, dev)
  out, nfe = _against_references(blk, f, x, xc, kw, times, pair, C.EVAL_SENSITIVE.get((case, pair), ()))
  if pair == 'dopri5':
    eager = _solve(f, x, [0.0, times[-1]], options={'eager_stages': True}, **kw)
    assert f.nfe == nfe
    assert_parity(out[-1], eager[-1], tol=2e-6, what='device vs host controller')


# ---- adjoint ------------------------------------------------------------------------------------------------------------------------
def test_adjoint_with_losses_at_several_times(dev, method='rk4'):
  blk, x, _ = C.make_block('a', dev)
  f = blk.odefunc
  t = _t([0.0, 1.25, 2.0], dev)
  w = torch.randn(3, *x.shape, generator=torch.Generator().manual_seed(9)).to(dev)
  params = [f.alpha_train, f.beta_train]

  def grads(host):
    f.opt['gnpde_host_outputs'] = host
    f.nfe = 0
    xr = x.clone().requires_grad_(True)
    out = G.odeint_adjoint(f, xr, t, method=method, options={'step_size': 0.5}, rtol=1e-6, atol=1e-6, adjoint_method='rk4',
                           adjoint_options={'step_size': 0.25}, adjoint_params=params)
    route = f._last_output_solve
    return route, torch.autograd.grad((out * w).sum(), [xr] + params)
  try:
    route_n, g_native = grads(False)
    route_h, g_host = grads(True)
  finally:
    f.opt.pop('gnpde_host_outputs', None)
  assert route_n == ('native fixed grid' if method == 'rk4' else 'native device controller') and route_h.startswith('host loop (')
  # dL/dx: within 2e-6 of its own largest entry.  dL/dalpha and dL/dbeta are single numbers -- "the largest entry" of such a tensor is the
  # number itself -- and sums of n d products of either sign whose rounding scales with the products, which are of the size of the
  # entries of dL/dx, not with the sum that is left: for them the scale is the largest entry over all gradients
  largest = max(float(b.abs().max()) for b in g_host)
  for name, a, b in zip(('x', 'alpha_train', 'beta_train'), g_native, g_host):
    print('d/d%s: largest difference %.3e, largest entry %.3e (of all gradients %.3e)' % (name, float((a - b).abs().max()), float(b.abs().max()), largest))
  assert float((g_native[0] - g_host[0]).abs().max()) <= 2e-6 * float(g_host[0].abs().max())
  for a, b in zip(g_native[1:], g_host[1:]):
    assert float((a - b).abs().max()) <= 2e-6 * largest


# ---- blocks and model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block,function', [('constant', 'laplacian'), ('attention', 'laplacian'), ('constant', 'transformer')])
def test_trajectory_equals_per_time_forwards(dev, block, function):
  blk, x, _ = C.make_block('a', dev, function=function, block=block, time=2.0)
  times = [0.0, 0.5, 1.0, 2.0]
  with torch.no_grad():
    blk.set_x0(x)
    before = blk(x).clone()
    traj = blk.trajectory(x, times).clone()
    assert blk.odefunc._last_output_solve == 'native fixed grid' and traj.shape == (4,) + tuple(x.shape)
    after = blk(x).clone()
    kept = blk._trajectory_kept[1]
    blk.trajectory(x, list(times))
    assert blk._trajectory_kept[1] is kept, 'the same times keep their device tensor (cached host reads)'
    assert torch.equal(before, after) and torch.equal(traj[-1], before), 'forward is unchanged'
    for j, tj in enumerate(times[1:], 1):
      blk.set_time(tj)
      assert torch.equal(blk(x), traj[j]), 'trajectory at t = %g' % tj


def test_forward_at_decodes_every_output(dev):
  name = [n for n in fixtures('gnn_') if 'pos' not in Fixture(n).arr][0]
  fx = Fixture(name)
  feat = int(fx.arr['num_features']) if 'num_features' in fx.arr else fx.arr['x'].shape[1]
  data = Data(fx.t('x', dev)[:, :feat], fx.t('edge_index', dev))
  opt = dict(fx.opt, method='rk4', step_size=0.5, time=2.0)
  model = G.GNN(opt, G.DummyDataset(data, int(fx.arr['num_classes'])), dev).to(dev)
  model.load_state_dict(fx.params, strict=True)
  model.eval()
  times = [0.0, 0.5, 1.25, 2.0]
  xin = fx.t('x', dev)
  with torch.no_grad():
    logits = model.forward_at(xin, times)
    assert model.odeblock.odefunc._last_output_solve == 'native fixed grid'
    enc = model.encode(xin)
    model.odeblock.set_x0(enc)
    states = model.odeblock.trajectory(enc, times)
    assert logits.shape == (4, enc.shape[0], int(fx.arr['num_classes']))
    for j in range(4):
      assert torch.equal(logits[j], model.decode(states[j], enc.shape[1]))
    assert torch.equal(logits[-1], model(xin)), 'forward_at at T equals forward'


# ---- options ------------------------------------------------------------------------------------------------------------------------
def test_max_nfe_raises_as_for_the_two_time_solves(dev):
  blk, x, _ = C.make_block('a', dev, max_nfe=20)
  f = blk.odefunc
  seen = {}
  for times in ([0.0, 50.0], [0.0, 10.0, 20.0, 50.0]):
    f.nfe = 0
    with torch.no_grad(), pytest.raises(G.MaxNFEException):
      G.odeint(f, x, _t(times, dev), method='dopri5', atol=1e-7, rtol=1e-9, options={'trials_per_sync': 2})
    seen[len(times)] = f.nfe
  assert seen[2] == seen[4] == 21
  for times in ([0.0, 3.0], [0.0, 1.0, 2.0, 3.0]):      # rk4: 6 steps of 4 evaluations do not fit 21
    f.nfe = 0
    with torch.no_grad(), pytest.raises(G.MaxNFEException):
      G.odeint(f, x, _t(times, dev), method='rk4', **FIX)
    seen[len(times)] = f.nfe
  assert seen[2] == seen[4] == 21


def test_bf16_gather_operand_composes_with_outputs(dev):
  blk, x, _ = C.make_block('a', dev, gnpde_gather_dtype='bf16')
  f = blk.odefunc
  out = _solve(f, x, T_FIXED, method='rk4', **FIX)
  assert f._last_output_solve == 'native fixed grid' and f.gather_dtype_used == 'bf16'
  two = _solve(f, x, [0.0, T_FIXED[-1]], method='rk4', **FIX)
  assert f.gather_dtype_used == 'bf16' and torch.equal(out[-1], two[1])
  f.opt['gnpde_gather_dtype'] = 'fp32'
  fp32 = _solve(f, x, T_FIXED, method='rk4', **FIX)
  assert not torch.equal(fp32[-1], out[-1])
