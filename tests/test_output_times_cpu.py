"""Native solves with several output times, everything that needs no device: the step / frac plan of the fixed-grid solves against the
host loop, the route rule, the new symbols and their argument refusals, and the adaptive test times on the host loop over the oracle."""
import ctypes
import os
import re

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib
import output_times_cases as C

O = C.O
R = G.routes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_solver_set_outputs', 'gnpde_solver_set_output_order', 'gnpde_dopri5_set_outputs', 'gnpde_snapshot_rows')


def test_symbols_prototypes_and_abi_number():
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
  assert in_header >= 26 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION
  assert 'static_assert(sizeof(Ctl) == 96' in open(os.path.join(ROOT, 'graph-neural-pde_amd', 'csrc', 'dopri5.hip')).read()
  assert hasattr(G.ops.FixedStepSolver, 'set_outputs') and hasattr(G.ops.Dopri5Solver, 'set_outputs')


def test_entry_points_refuse_bad_arguments_before_any_launch():
  L = G.lib()
  a, b, out = torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 8)
  snap = lambda ya, yb, frac, n, d, ld, o, ld_out: L.gnpde_snapshot_rows(_lib.ptr(ya), _lib.ptr(yb), frac, n, d, ld, _lib.ptr(o), ld_out, None, None)
  assert snap(a, None, 0.5, 4, 8, 8, out, 8) == -1 and b'snapshot_rows' in L.gnpde_last_error()
  assert snap(None, b, 0.5, 4, 8, 8, out, 8) == -1          # an interior fraction reads ya
  assert snap(a, b, 0.5, 4, 8, 8, None, 8) == -1
  assert snap(a, b, 0.5, 4, 8, 6, out, 8) == -1             # state stride under the width
  assert snap(a, b, 0.5, 4, 8, 8, out, 6) == -1             # output stride under the width
  assert snap(a, b, 0.5, -1, 8, 8, out, 8) == -1
  assert snap(a, b, 0.5, 0, 8, 8, out, 8) == 0              # nothing to do: no launch
  assert L.gnpde_solver_set_outputs(None, 0, None, None, None, 0, None) == -1
  assert L.gnpde_solver_set_output_order(None, None) == -1
  assert L.gnpde_dopri5_set_outputs(None, None, 0, None, 0) == -1


def _per_step_states(rhs, y0, t, method, step):
  """The state after every step of the host loop over [t[0], t[-1]]."""
  states = [y0]
  O._solve_fixed_host(rhs, y0, torch.stack([t[0], t[-1]]), method, step, on_step=lambda y, i: states.append(y.clone()))
  return states


@pytest.mark.parametrize('method', ['euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize('dtype,step,times', [(torch.float32, C.FIXED_STEP, C.FIXED_TIMES), (torch.float64, C.FIXED_STEP, C.FIXED_TIMES),
                                              (torch.float32, 0.3, [0.0, 0.1, 0.3, 0.31, 0.59, 0.9, 1.0])])
def test_plan_reproduces_the_host_loop_on_a_linear_function(method, dtype, step, times):
  """Output j of `_solve_fixed_host` equals, bit for bit, what the plan says: the state after step `step` (frac 1) or
  y + fl32(frac) (y_next - y) of that step -- the arithmetic of gnpde_snapshot_rows up to the fused multiply-add."""
  g = torch.Generator().manual_seed(3)
  A = torch.randn(5, 5, generator=g) * 0.3
  y0 = torch.randn(5, 4, generator=g)
  rhs = lambda tq, y: A @ y
  t = torch.tensor(times, dtype=dtype)
  ref = O._solve_fixed_host(rhs, y0, t, method, step)
  plan = O.output_plan(t, step)
  states = _per_step_states(rhs, y0, t, method, step)
  assert len(plan) == len(times) - 1 and len(states) == len(O.step_sizes(t, step)) + 1
  assert all(1 <= i <= len(states) - 1 and 0.0 < f <= 1.0 for i, f in plan) and [i for i, _ in plan] == sorted(i for i, _ in plan)
  for j, (i, frac) in enumerate(plan):
    ya, yb = states[i - 1], states[i]
    want = yb if frac == 1.0 else ya + torch.tensor(frac, dtype=torch.float32) * (yb - ya)
    assert torch.equal(ref[j + 1], want), (j, i, frac)
  assert plan[-1] == (len(states) - 1, 1.0)
  if times is C.FIXED_TIMES:
    assert plan == ((1, 1.0), (3, 0.5), (3, 1.0), (4, 1.0), (5, 1.0))


class _Stub(object):
  """What the route rule asks of a function object."""
  opt = {}

  def _descriptor(self, *a, **k):
    raise AssertionError('no native solve on the host')

  def _needs_grad(self, y):
    return False

  def _has_native_rhs(self, y):
    return True

  def __call__(self, t, y):
    return -y


def test_route_rule_and_report_on_the_host():
  f, y0 = _Stub(), torch.ones(3, 2)
  t = torch.tensor([0.0, 0.5, 1.0])
  for method, options, host in (('rk4', {'step_size': 0.5}, 'host_fixed'), ('dopri5', {}, 'host_loop')):
    route, reason = R.forward(f, y0, t, method, options)
    assert route == host and 'HIP device' in reason
    assert R.forward(lambda tq, y: -y, y0, t, method, options) == (host, 'foreign callable')
  out = G.odeint(f, y0, t, method='rk4', options={'step_size': 0.5})
  assert out.shape == (3, 3, 2) and f._last_output_solve.startswith('host loop (')
  G.odeint(f, y0, t, method='dopri5', rtol=1e-6, atol=1e-8)
  assert f._last_output_solve.startswith('host loop (')
  assert O._strictly_increasing(t) and not O._strictly_increasing(torch.tensor([0.0, 1.0, 1.0])) and not O._strictly_increasing(torch.tensor([0.0, 1.0, 0.5]))
  assert O.output_times(t) == (0.5, 1.0)
  f.opt = {'gnpde_host_outputs': True}
  assert R.host_outputs_requested(f) and not R.host_outputs_requested(_Stub())


def test_trajectory_refuses_training_with_regularisers():
  blk, x, _ = C.make_block('a', 'cpu')
  blk.nreg = 1
  blk.train()
  with pytest.raises(G.GnpdeError):
    blk.trajectory(x, [0.0, 0.5, 1.0])
  with pytest.raises(ValueError):
    blk.eval().trajectory(x, [0.0])
  assert getattr(blk, '_trajectory_times', None) is None


@pytest.mark.parametrize('case,pair', sorted(C.ADAPTIVE))
def test_adaptive_times_have_the_wanted_properties_on_the_host_loop(case, pair):
  """The five output times of the adaptive GPU tests, picked from the two-time trace of the host loop over the CPU oracle: three inside one
  accepted step, one behind a rejected trial step, the last at the end; no trial step is marginal; the host loop with those outputs
  takes the same trial steps; and the two references the GPU tests compare against agree with each other within the bound asked of
  the device (figures printed)."""
  from oracle.shims import install as REF_TORCHDIFFEQ
  from helpers import parity
  A = C.adaptive(case, pair)
  blk, _, xc = C.make_block(case, 'cpu', alpha_train=A['alpha_train'])
  rhs = C.oracle_laplacian(blk, xc)
  trace, two = C.host_trace(rhs, xc, A['T'], pair, A['tol_scale'])
  assert any(r > 1 for _, _, r in trace) and all(abs(r - 1) > 0.05 for _, _, r in trace), 'a rejected trial step, none marginal'
  times = C.pick_times(trace, A['T'])
  C.check_times(trace, times)
  kw = dict(rtol=A['tol_scale'] * 1e-9, atol=A['tol_scale'] * 1e-7)
  O._TRIAL_TRACE = []
  try:
    with torch.no_grad():
      many = O._solve_dopri5(rhs, xc, torch.tensor(times), kw['rtol'], kw['atol'], tableau=pair)
    assert O._TRIAL_TRACE == trace
  finally:
    O._TRIAL_TRACE = None
  assert torch.equal(many[-1], two[-1])
  ref = REF_TORCHDIFFEQ.odeint(rhs, xc, torch.tensor(times), method=pair, options={}, **kw)
  apart = [parity(many[j], ref[j])[0] for j in range(1, len(times))]
  print('host loop vs restated torchdiffeq, per output: ' + ' '.join('%.1e' % v for v in apart))
  assert max(apart) <= 2e-5


@pytest.mark.parametrize('case,pair', sorted(C.ADAPTIVE))
def test_references_do_not_move_with_the_rounding_of_the_evaluation(case, pair):
  """The restated torchdiffeq runs over the oracle, the device over the native kernels: at every output that the GPU tests compare, the
  references move by less than the 2e-5 asked of the device when the evaluation of f changes in its last bits.  The outputs listed in
  EVAL_SENSITIVE move by more, and are not compared with the restated torchdiffeq."""
  margin, apart = C.reference_sensitivity(case, pair, C.adaptive(case, pair))
  print('references under another rounding of f, per output: ' + ' '.join('%.1e' % v for v in apart))
  skip = C.EVAL_SENSITIVE.get((case, pair), ())
  assert margin > 0.05
  for j, v in enumerate(apart, 1):
    assert (v > 2e-5) if j in skip else (v <= 2e-5), (j, v)


def test_no_searched_heun_horizon_of_the_hub_case_is_better_conditioned():
  """Case d under adaptive_heun: every configuration tried either has no rejected trial step, or a marginal one, or references that move
  by more than 2e-5 at some output when the evaluation is rounded differently."""
  for A in C.HEUN_D_SEARCH:
    res = C.reference_sensitivity('d', 'adaptive_heun', A)
    print(A, None if res is None else ('margin %.3f' % res[0], ' '.join('%.1e' % v for v in res[1])))
    assert res is None or res[0] <= 0.05 or max(res[1]) > 2e-5, A
