"""Shared plumbing of test_output_times_cpu.py / test_output_times_gpu.py: the four shapes, the fixed-grid times, and the choice of
adaptive output times from a trial-step trace of the HOST loop (odeint._TRIAL_TRACE) -- never from the code under test."""
import importlib

import torch

import gnpde_amd as G
from oracle import restate as R
from helpers import Data, random_graph

O = importlib.import_module('gnpde_amd.odeint')

BASE = dict(heads=4, attention_dim=16, attention_type='scaled_dot', attention_norm_idx=0, square_plus=False,
            reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9,
            add_source=True, no_alpha_sigmoid=False, mix_features=False, hidden_dim=24, augment=False, adjoint=False,
            tol_scale=1.0, data_norm='rw', method='rk4', step_size=0.5, max_iters=100, block='constant',
            function='laplacian', time=2.3, gnpde_reorder='0')

# the new kernels are elementwise: strides and predicates are what can break
CASES = {
  'a': dict(n=37, d=24, hubs=0),                                # plain aligned rows
  'b': dict(n=37, d=6, hubs=0),                                 # state rows padded to ld = 8, outputs ld_out = 6: scalar output lanes
  'c': dict(n=150, d=24, hubs=0, gnpde_reorder='degree'),       # a LocalityView order
  'd': dict(n=600, d=24, hubs=1),                               # one hub row of more than 512 entries
}

# grid points, one interior time (1.25), a short last step (2.0 -> 2.3) and an output at its end; step 0.5: every time but the last is dyadic
FIXED_TIMES = [0.0, 0.5, 1.25, 1.5, 2.0, 2.3]
FIXED_STEP = 0.5

# Horizon, tolerance scale and alpha_train of the adaptive solves: long and loose enough that the step size outgrows the stability limit,
# so the host loop's trace has a rejected trial step -- with an error ratio well away from 1 (no trial step of these traces lies within
# 5 % of it: host loop and device controller sum their error norms in different orders) -- and short enough that the two float32
# references, the host loop and the restated torchdiffeq, agree with EACH OTHER within the 2e-5 asked of the device at every output.
# Near the steady state the quartic's coefficients cancel and the references drift apart (4.5e-4 for adaptive_heun at T = 70, 8e-5 at
# the end of dopri5's case d at T = 60): test_output_times_cpu.py asserts both properties on the CPU oracle for every entry.
ADAPTIVE = {
  ('a', 'dopri5'): dict(T=60.0, tol_scale=50.0, alpha_train=0.2),
  ('b', 'dopri5'): dict(T=60.0, tol_scale=50.0, alpha_train=0.2),
  ('c', 'dopri5'): dict(T=60.0, tol_scale=50.0, alpha_train=0.2),
  ('d', 'dopri5'): dict(T=40.0, tol_scale=50.0, alpha_train=0.2),      # (ends inside the accepted step behind its rejected one)
  ('a', 'adaptive_heun'): dict(T=17.5, tol_scale=200000.0, alpha_train=2.0),
  ('b', 'adaptive_heun'): dict(T=17.5, tol_scale=200000.0, alpha_train=2.0),
  ('c', 'adaptive_heun'): dict(T=17.5, tol_scale=200000.0, alpha_train=2.0),
  ('d', 'adaptive_heun'): dict(T=17.0, tol_scale=200000.0, alpha_train=1.0),
}


def adaptive(case, pair):
  return ADAPTIVE[(case, pair)]


# The restated torchdiffeq runs over the CPU oracle, the device over the native kernels: the two evaluations of f differ in their last
# bits (the hub row of case d sums 560 entries in another order).  reference_sensitivity() measures, on the CPU, how far the references
# themselves move when the evaluation changes by such roundings (the oracle in float32 against the oracle in float64 rounded to
# float32).  For every entry above that is below the 2e-5 asked of the device at every output -- except the output behind the rejected
# step of case d under adaptive_heun (6e-5), and no configuration of HEUN_D_SEARCH does better there without a marginal trial step or
# without a rejection (test_output_times_cpu.py asserts all of this).  That one output is compared with the host loop over the native
# evaluations only; its figure against the restated torchdiffeq is printed, not asserted.
EVAL_SENSITIVE = {('d', 'adaptive_heun'): (4,)}
HEUN_D_SEARCH = [dict(alpha_train=a, T=T, tol_scale=ts) for a, T, ts in
                 [(1.0, 17.0, 2e5), (0.5, 20.0, 2e5), (0.2, 24.0, 2e5), (2.0, 17.5, 2e5), (3.0, 16.0, 2e5), (1.0, 20.0, 4e5), (1.0, 17.0, 1e5),
                  (1.5, 17.0, 2e5)]]


def reference_sensitivity(case, pair, A):
  """(smallest |error ratio - 1| of the trace, per output: the largest relative distance between the host loop and the restated
  torchdiffeq over the float32 oracle and the same two over the oracle evaluated in float64 and rounded), or None where the trace has
  no rejected trial step to pick the times from.  CPU only."""
  from oracle.shims import install as REF
  from helpers import parity
  blk, _, xc = make_block(case, 'cpu', alpha_train=A['alpha_train'])
  f = blk.odefunc
  d = lambda v: v.detach().double()
  rhs = oracle_laplacian(blk, xc)
  rhs64 = lambda t, y: R.rhs_laplacian(y.double(), f.edge_index, d(f.edge_weight), d(f.alpha_train), d(f.beta_train), xc.double(), False, True).float()
  trace, _ = host_trace(rhs, xc, A['T'], pair, A['tol_scale'])
  try:
    times = pick_times(trace, A['T'])
  except StopIteration:
    return None
  kw = dict(rtol=A['tol_scale'] * 1e-9, atol=A['tol_scale'] * 1e-7)
  tt = torch.tensor(times)
  with torch.no_grad():
    runs = [O._solve_dopri5(r, xc, tt, kw['rtol'], kw['atol'], tableau=pair) for r in (rhs, rhs64)]
    runs += [REF.odeint(r, xc, tt, method=pair, options={}, **kw) for r in (rhs, rhs64)]
  apart = [max(parity(p[j], q[j])[0] for p in runs for q in runs) for j in range(1, len(times))]
  return min(abs(r - 1) for _, _, r in trace), apart


def make_block(case, dev, function='laplacian', block='constant', alpha_train=0.2, **over):
  """(block in evaluation mode, x on dev, x on the host) of a case; seeded."""
  c = CASES[case]
  ei = random_graph(c['n'], 4, 5, hubs=c['hubs'], hub_deg=560 if c['hubs'] else 0)
  x = torch.randn(c['n'], c['d'], generator=torch.Generator().manual_seed(6))
  opt = dict(BASE, hidden_dim=c['d'], function=function, block=block, gnpde_reorder=c.get('gnpde_reorder', '0'))
  opt.update(over)
  fcls = {'transformer': G.ODEFuncTransformerAtt, 'laplacian': G.LaplacianODEFunc}[function]
  bcls = {'constant': G.ConstantODEblock, 'attention': G.AttODEblock}[block]
  blk = bcls(fcls, [], opt, Data(x.to(dev), ei.to(dev)), dev, t=torch.tensor([0, opt['time']])).to(dev)
  g = torch.Generator().manual_seed(0)
  with torch.no_grad():
    for name, p in blk.named_parameters():
      if p.dim() >= 2 and 'multihead_att_layer' in name:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
    for f in (blk.odefunc, blk.reg_odefunc.odefunc):
      f.alpha_train.fill_(alpha_train)
      f.beta_train.fill_(0.1)
  blk.eval()
  blk.odefunc.x0 = x.to(dev)
  return blk, x.to(dev), x


def oracle_laplacian(blk, xc):
  """The Laplacian function of the block over the CPU oracle."""
  f = blk.odefunc
  cpu = lambda v: v.detach().cpu()
  return lambda t, y: R.rhs_laplacian(y, cpu(f.edge_index), cpu(f.edge_weight), cpu(f.alpha_train), cpu(f.beta_train), xc, False, True)


def host_trace(rhs, x, T, pair, tol_scale):
  """(trial steps (t, dt, ratio), result) of the two-time host loop from 0 to T."""
  O._TRIAL_TRACE = []
  try:
    with torch.no_grad():
      out = O._solve_dopri5(rhs, x, torch.tensor([0.0, T], device=x.device), tol_scale * 1e-9, tol_scale * 1e-7, tableau=pair)
    return list(O._TRIAL_TRACE), out
  finally:
    O._TRIAL_TRACE = None


def accepted_steps(trace):
  """[(ta, tb, a rejected trial step stands right before it)] of the accepted steps of a trace."""
  steps, after_reject = [], False
  for t, dt, ratio in trace:
    if ratio <= 1:
      steps.append((t, t + dt, after_reject))
      after_reject = False
    else:
      after_reject = True
  return steps


def _grid(v):
  return round(v * 64) / 64      # exact in float32 and float64


def pick_times(trace, T):
  """[0, a1, a2, a3, a4, T]: a1..a3 inside the longest accepted step that ends before the first rejected trial step, a4 inside the
  accepted step that follows that rejection, T the end.  Stepping never looks at the outputs, so the two-time trace decides."""
  steps = accepted_steps(trace)
  k = next(i for i, s in enumerate(steps) if s[2] and s[0] < T)
  ta, tb, _ = max(steps[:k], key=lambda s: s[1] - s[0])
  a = [_grid(ta + q * (tb - ta)) for q in (0.2, 0.5, 0.8)]
  ra, rb, _ = steps[k]
  return [0.0] + a + [_grid(ra + 0.5 * (min(rb, T) - ra)), T]


def check_times(trace, times):
  """The properties the adaptive tests want of their five output times, on a host-loop trace."""
  steps = accepted_steps(trace)
  owner = [next(i for i, s in enumerate(steps) if s[1] >= t) for t in times[1:]]
  assert all(b > a for a, b in zip(times, times[1:]))
  assert max(owner.count(i) for i in set(owner)) >= 3, 'three outputs inside one accepted step: %s' % owner
  assert any(steps[i][2] and steps[i][0] < t < steps[i][1] for i, t in zip(owner[:-1], times[1:-1])), 'an output behind a rejected step'
  assert times[-1] == trace[-1][0] + trace[-1][1] or steps[-1][1] >= times[-1]      # the last output is the end of the solve
