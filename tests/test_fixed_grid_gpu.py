"""The call sites of csrc/fixed_grid.h: one fixed-grid solve formed three ways must give the same bits -- (a) ops.rhs_stage calls
whose stage, y, k1 and out_y are written out here by hand, (b) ops.FixedStepSolver launching eagerly, (c) the same solver replaying
its captured graph -- for euler with an odd number of steps (the result ends in the second buffer and is copied back), midpoint
and the compact rk4, over a grid with a short last step.  A wrong buffer choice in solver.hip fails here by name; a wrong table
fails tests/test_fixed_grid_cpu.py.  Two small problems cover both evaluation paths: a laplacian block, and a scaled-dot transformer
at a width with padded rows and two hub rows.  The laplacian solve is also recorded (gnpde_solver_set_tape): it writes no
per-evaluation record, so the recorded solve is the same launches over tape slots."""
import importlib

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
from helpers import Data, random_graph

pytestmark = pytest.mark.gpu

ODEINT = importlib.import_module('gnpde_amd.odeint')
OPT = dict(heads=2, attention_dim=8, attention_type='scaled_dot', attention_norm_idx=0, square_plus=False, reweight_attention=False,
           beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=1000, add_source=True, no_alpha_sigmoid=False,
           mix_features=False, augment=False, adjoint=False, tol_scale=1.0, data_norm='rw', method='rk4', step_size=0.5, max_iters=100,
           block='constant', time=2.2)
PROBLEMS = {'laplacian': dict(function='laplacian', d=32, hubs=0, hub_deg=0),
            'transformer': dict(function='transformer', d=22, hubs=2, hub_deg=200)}
TIMES = {'euler': 1.2, 'midpoint': 2.2, 'rk4': 2.2}     # step 0.5: three steps for euler, five for the others, the last one of 0.2


@pytest.fixture(scope='module', params=sorted(PROBLEMS))
def problem(request, dev):
  """(name, descriptor, start state x, four state-sized buffers y / ua / ub / uc with the descriptor's row stride)"""
  p = PROBLEMS[request.param]
  n, d = 300, p['d']
  ei = random_graph(n, 5, seed=71, hubs=p['hubs'], hub_deg=p['hub_deg'])
  g = torch.Generator().manual_seed(72)
  x = torch.randn(n, d, generator=g).to(dev)
  opt = dict(OPT, function=p['function'], hidden_dim=d)
  fcls = {'laplacian': G.LaplacianODEFunc, 'transformer': G.ODEFuncTransformerAtt}[p['function']]
  block = G.ConstantODEblock(fcls, [], opt, Data(x, ei.to(dev)), dev, t=torch.tensor([0, opt['time']])).to(dev)
  with torch.no_grad():
    for q in block.parameters():
      if q.dim() >= 2:
        q.copy_(torch.randn(q.shape, generator=g) / q.shape[-1] ** 0.5)
    block.odefunc.beta_train.fill_(0.1)
  block.eval()
  bufs = [_lib.alloc_state(n, d, dev) for _ in range(4)]
  x0 = _lib.alloc_state(n, d, dev)
  x0.copy_(x)
  desc = block.odefunc._descriptor(bufs[0], x0_override=x0)
  return request.param, desc, x, bufs, block


def _literal(desc, method, dts, bufs):
  """The solve as rhs_stage calls, every operand named; returns the buffer that holds y(T)."""
  y, ua, ub, uc = bufs
  if method == 'euler':
    cur, nxt = y, ua
    for dt in dts:
      ops.rhs_stage(desc, cur, _lib.STAGE_EULER, dt=dt, y=cur, out_y=nxt)
      cur, nxt = nxt, cur
    return cur
  for dt in dts:
    if method == 'midpoint':     # y_mid = y + f(y) * (dt / 2);  y += dt * f(y_mid)
      ops.rhs_stage(desc, y, _lib.STAGE_LINCOMB, y=y, coef=[0.5 * dt], out_y=ua)
      ops.rhs_stage(desc, ua, _lib.STAGE_LINCOMB, y=y, coef=[dt], out_y=y)
    else:                        # compact rk4: stage states from the previous stage inputs, the last stage in place on y
      ops.rhs_stage(desc, y, _lib.STAGE_RK1C, dt=dt, out_y=ua)
      ops.rhs_stage(desc, ua, _lib.STAGE_RK2C, dt=dt, y=y, out_y=ub)
      ops.rhs_stage(desc, ub, _lib.STAGE_RK3C, dt=dt, k1=ua, out_y=uc)
      ops.rhs_stage(desc, uc, _lib.STAGE_RK4C, dt=dt, y=y, k1=ub, out_y=y)
  return y


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
def test_literal_stages_eager_solver_and_replayed_graph_give_the_same_bits(problem, method):
  name, desc, x, bufs, _ = problem
  dts = ODEINT.step_sizes(torch.tensor([0, TIMES[method]]), 0.5)
  assert len(dts) == (3 if method == 'euler' else 5) and abs(dts[-1] - 0.2) < 1e-6 and dts[0] == 0.5
  y = bufs[0]
  y.copy_(x)
  literal = _literal(desc, method, dts, bufs).clone()
  assert torch.isfinite(literal).all() and not torch.equal(literal, x)
  sol = ops.FixedStepSolver(desc, method, dts, x.device)
  try:
    y.copy_(x)
    eager = sol.run(y, use_graph=False).clone()
    y.copy_(x)
    replay = sol.run(y, use_graph=True).clone()
    assert torch.equal(eager, literal), '%s %s: eager solver vs literal stages, max diff %.3e' % (name, method, float((eager - literal).abs().max()))
    assert torch.equal(replay, literal), '%s %s: replayed graph vs literal stages, max diff %.3e' % (name, method, float((replay - literal).abs().max()))
    if name == 'laplacian':
      assert _lib.lib().gnpde_solver_tape_bytes(desc.ref(), sol.method, len(dts)) > 0
      sol.set_tape(True)
      for use_graph in (False, True):
        y.copy_(x)
        recorded = sol.run(y, use_graph=use_graph).clone()
        assert torch.equal(recorded, literal), '%s %s: recorded solve (graph=%s) vs recycled buffers' % (name, method, use_graph)
      # the tape holds the stage inputs in evaluation order: slot 0 = y0, the last slot = y(T)
      n, ld = x.shape[0], desc.struct.ld
      stride = (n * ld * 4 + 255) // 256 * 256 // 4
      slots = sol.tape.view(torch.float32)[:(sol.n_rhs_evals + 1) * stride].view(sol.n_rhs_evals + 1, stride)[:, :n * ld].view(-1, n, ld)[:, :, :x.shape[1]]
      assert torch.equal(slots[0], x) and torch.equal(slots[-1], literal)
      sol.set_tape(False)
  finally:
    sol.close()
