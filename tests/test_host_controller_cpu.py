"""The host-controlled embedded-pair engine (odeint._solve_pair_host) on plain-torch CPU stand-ins of its components, against
torchdiffeq's loop restated for callables (odeint._solve_dopri5) on the same float32 problem: f(y) = 0.8 (A y - y) + 0.3 x0 with A
a row-normalised random 12 x 12 matrix and states of shape 12 x 4."""
import importlib
import types

import pytest
import torch

O = importlib.import_module('gnpde_amd.odeint')

CASES = [('dopri5', 1e-6, 1e-8, 6.0, 3.0), ('adaptive_heun', 1e-3, 1e-5, 3.0, 1.0), ('dopri5', 1e-4, 1e-6, 6.0, 1.0)]   # (.., T, |y0| scale)
# The reference (24 trials, 1 rejected, closest ratio 0.0956 from 1 | 114, 15, 0.00279 | 10, 0, 0.375) rounds through tensor ops with
# a float64 tolerance, the engine through numpy scalars and float32.  Largest relative difference measured, engine against reference:
#   dt of a trial step   0.095 | 4.1e-6 | 0.0071     (dopri5's first trial steps are far below the tolerance: their error estimate --
#                                                     1e-4 of a tolerance of 1e-6 |y| -- is float32 rounding noise of the stages,
#                                                     and one ulp of float32(dt) moves it by half, the next dt by a tenth)
#   end state            1.6e-7 | 3.3e-7 | 2.7e-7
# The bars: ten times the figure, rounded up to one digit -- for dt case by case, so that the quiet cases are not judged by the noisy one.
DT_BAR = dict(zip(CASES, (1.0, 5e-5, 0.08)))
STATE_BAR = 4e-6


def _problem(scale):
  g = torch.Generator().manual_seed(0)
  A = torch.rand(12, 12, generator=g)
  A = A / A.sum(1, keepdim=True)
  return A, torch.randn(12, 4, generator=g), scale * torch.randn(12, 4, generator=g)


def _lin(terms, coefs):
  """sum_j c_j v_j in float32, zeros skipped, the terms summed first (odeint._combine)"""
  acc = None
  for v, c in zip(terms, coefs):
    if c != 0.0:
      term = v * torch.tensor(c, dtype=torch.float32)
      acc = term if acc is None else acc + term
  return acc


class Comp(O._StageComponent):
  """y' = sign f(y) under the component protocol, every buffer a CPU tensor; `log`: what scaled_rms returned, call by call."""

  def __init__(self, A, x0, y0, sign, stages, rtol, atol):
    self.A, self.x0, self.sign, self.tols, self.log = A, x0, sign, (atol, rtol), []
    self.y, self.y1, self.u = y0.clone(), torch.empty_like(y0), [torch.empty_like(y0), torch.empty_like(y0)]
    self.K = [torch.empty_like(y0) for _ in range(stages + 1)]

  def f(self, t, y):
    return 0.8 * (self.A @ y - y) + 0.3 * self.x0

  def stage(self, j, src, dst=None, row=()):
    self.K[j].copy_(self.f(None, src))
    if dst is not None:
      dst.copy_(self.y + _lin(self.K[:j + 1], self.signed(row)))

  def scaled_rms(self, terms, coefs, y1=None):
    tol = self.tols[0] + self.tols[1] * torch.max(self.y.abs(), (self.y if y1 is None else y1).abs())
    out = (_lin(terms, coefs) / tol).pow(2).mean().sqrt().reshape(1)
    self.log.append(float(out))
    return out


def _quartic(x, h, v0, v1, k0, k1, mid):
  ca = 2 * h * (k1 - k0) - 8 * (v1 + v0) + 16 * mid
  cb = h * (5 * k0 - 3 * k1) + 18 * v0 + 14 * v1 - 32 * mid
  cc = h * (k1 - 4 * k0) - 11 * v0 - 5 * v1 + 16 * mid
  return v0 + x * (h * k0) + x ** 2 * cc + x ** 3 * cb + x ** 4 * ca


def _engine(method, rtol, atol, T, scale, **hooks):
  """(end state, trace, stopped, the component) of the engine on one stand-in component of sign +1"""
  A, x0, y0 = _problem(scale)
  c = Comp(A, x0, y0, 1, len(O._TABLEAUS[method]['alpha']), rtol, atol)
  end = {}

  def interp(x, h, c_mid):
    end['y'] = _quartic(x, h, c.y, c.y1, c.K[0], c.K[-1], c.axpys(c_mid, torch.empty_like(c.y)))
  O._TRIAL_TRACE = []
  try:
    n_steps = O._solve_pair_host(method, [c], 0.0, T, lambda: None, interp=interp, **hooks)[1]
    trace = O._TRIAL_TRACE
  finally:
    O._TRIAL_TRACE = None
  stopped = hooks.get('stop_after') is not None and n_steps >= hooks['stop_after']
  return (c.y if stopped else end['y']), trace, stopped, c


def _reference(method, rtol, atol, T, scale, **hooks):
  A, x0, y0 = _problem(scale)
  c = Comp(A, x0, y0, 1, 1, rtol, atol)
  O._TRIAL_TRACE = []
  try:
    with torch.no_grad():
      out = O._solve_dopri5(c.f, y0, torch.tensor([0.0, T]), rtol, atol, tableau=method, **hooks)
    return out[1], O._TRIAL_TRACE
  finally:
    O._TRIAL_TRACE = None


@pytest.fixture(scope='module')
def references():
  return {case: _reference(*case) for case in CASES}


def _rel(a, b):
  return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s-%g' % c[:2])
def test_engine_follows_the_restated_controller(case, references):
  ref_y, ref = references[case]
  gap = min(abs(r - 1) for _, _, r in ref)
  print('reference: %d trials, %d rejected, closest ratio %.3g from 1' % (len(ref), sum(r > 1 for _, _, r in ref), gap))
  assert gap >= 1e-3          # (precondition on the reference alone: no decision hangs on the last bits of a ratio)
  y, trace, stopped, _ = _engine(*case)
  assert not stopped and len(trace) == len(ref)
  assert [r <= 1 for _, _, r in trace] == [r <= 1 for _, _, r in ref]
  dt_err = max(abs(a[1] - b[1]) / b[1] for a, b in zip(trace, ref))
  print('dt: largest relative difference %.2g; end state %.2g' % (dt_err, _rel(y, ref_y)))
  assert dt_err < DT_BAR[case] and _rel(y, ref_y) < STATE_BAR


@pytest.mark.parametrize('stop_after', [None, 8, 100])
def test_engine_hooks_follow_the_restated_controller(stop_after):
  """on_accept / on_reject / stop_after as test_adjoint_cpu.py's hook test has them for _solve_dopri5: a rejected trial counts
  towards the limit, the hooks see the same times and states, and when the limit ends the loop the state where it stopped is
  returned instead of the interpolation at the end time."""
  case = CASES[1]             # (adaptive_heun: its eighth trial step is the first rejected one, 15 of its first hundred are)
  res = []
  for solve in (_reference, _engine):
    acc, rej = [], []
    out = solve(*case, on_accept=lambda y, t: acc.append((t, y.clone())), on_reject=lambda y, t: rej.append((t, y.clone())),
                stop_after=stop_after)
    res.append((out[0], acc, rej))
  (ref_y, ref_acc, ref_rej), (y, acc, rej) = res
  assert len(acc) == len(ref_acc) and len(rej) == len(ref_rej) and len(rej) >= 1
  if stop_after is not None:
    assert len(acc) + len(rej) == stop_after
  for got, want in ((acc, ref_acc), (rej, ref_rej)):
    for (t, state), (t_ref, state_ref) in zip(got, want):
      assert abs(t - t_ref) <= DT_BAR[case] * t_ref and _rel(state, state_ref) < STATE_BAR
  assert _rel(y, ref_y) < STATE_BAR
  if stop_after is not None:
    assert torch.equal(y, acc[-1][1])          # (cut short: the state where it stopped, not the interpolation at the end time)


@pytest.mark.parametrize('method', ['dopri5', 'adaptive_heun'])
def test_mixed_norm_is_the_largest_part(method):
  """Two components of opposite sign and a pair of scalars: every ratio the controller acts on -- the three of the initial step
  aside, which only the step size shows -- is the largest of the parts' own."""
  rtol, atol = 1e-4, 1e-6
  A, x0, y0 = _problem(1.0)
  stages = len(O._TABLEAUS[method]['alpha'])
  cy, ca = Comp(A, x0, y0, -1, stages, rtol, atol), Comp(A.t().contiguous(), 0 * x0, 40 * x0, 1, stages, rtol, atol)
  log = []

  def ratio(v, g0, g1):
    out = (v / (atol + rtol * torch.max(g0.abs(), g1.abs()))).abs().max().reshape(1)
    log.append(float(out))
    return out
  sc = types.SimpleNamespace(g=torch.zeros(2), g1=None, K=[None] * (stages + 1), ratio=ratio,
                             stage=lambda j, src: torch.stack([(src[1] * cy.K[j]).sum(), (src[1] * x0).sum()]))
  O._TRIAL_TRACE = []
  try:
    O._solve_pair_host(method, [cy, ca], 0.0, 2.0, lambda: None, scalars=sc)
    trace = O._TRIAL_TRACE
  finally:
    O._TRIAL_TRACE = None
  assert len(trace) >= 5 and len(cy.log) == len(ca.log) == len(log) == 3 + len(trace)
  parts = list(zip(cy.log[3:], ca.log[3:], log[3:]))
  assert [r for _, _, r in trace] == [max(p) for p in parts]
  assert len({p.index(max(p)) for p in parts}) >= 2      # (not one part all the way)
