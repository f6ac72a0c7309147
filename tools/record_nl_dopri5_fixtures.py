"""Record the fixtures of GRAND-nl / GAT training through dopri5 WITHOUT the adjoint method by running the REFERENCE's own code on a
CPU (container-only, as oracle/gen_golden.py): tests/golden/nltrain_<name>.npz.

  python tools/record_nl_dopri5_fixtures.py

Each fixture holds what oracle/gen_golden.py gen_training() records -- edge_index, x, c, z, z_eval, grad_x, nfe, nfe_after_backward,
grad/*, param/*, opt_json -- and `ratios`: the error ratio of every trial step of the TRAINING solve, in order.

Condition on the inputs (asserted here, not a measurement): a float32 solve on another machine must take the same accept / reject
sequence, so no trial step may have an error ratio near 1 -- a fixture with any ratio inside (0.85, 1.2) is refused.  Two cases have
rejected steps on purpose: a rejected trial step must leave nothing on the record of a native solve, and the evaluation count must
still be the reference's.

The seeds of `randomise`.  The band above is necessary, not sufficient: at these tolerances the error estimate of a trial step carries
float32 rounding of the evaluations, and a ratio moves by more than the band between two float32 implementations of the same
formulae when the weights make the gradients of the attention parameters small differences of large terms (squareplus over columns),
put a LeakyReLU argument of GAT next to its kink, or place a trial step where the estimate is mostly rounding.  A seed is kept only
if the REFERENCE's own result is reproducible: the oracle's right-hand side under this package's host loop on the CPU, in float32 AND
in float64, takes the reference's evaluation count and agrees with its gradients well inside the bars of
tests/test_nltrain_oracle_cpu.py (that test is the float32 half of the rule; figures in DESIGN.md section 5).  1901, 1904 and 1950
satisfy the band and fail this: the reference's float32 gradients there lie 1e-2 (Q / K, module scale), 6e-4 (dL/dx) from the
float64 ones, and the float32 / float64 oracles count 128 / 110 evaluations where the reference counts 122."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402  (activates the reference over oracle/shims)
from shims import install as shim  # noqa: E402  (oracle/shims, as ref_env.activate imports it: the module RKAdaptiveStepsizeODESolver lives in)

BAND = (0.85, 1.2)

# name -> (options over BASE + method dopri5, block constant; seed of `randomise`; rejected steps expected)
CASES = {
  'transformer_dopri5': (dict(time=3.0, tol_scale=200.0), 1900, False),
  'transformer_dopri5_columns_squareplus': (dict(time=2.0, tol_scale=100.0, square_plus=True, attention_norm_idx=1, heads=8, attention_dim=32),
                                            1989, False),
  'transformer_dopri5_exp_kernel': (dict(time=2.5, tol_scale=50.0, attention_type='exp_kernel'), 1902, False),
  'transformer_dopri5_cosine_no_source': (dict(time=2.5, tol_scale=300.0, attention_type='cosine_sim', add_source=False), 1903, False),
  'gat_dopri5': (dict(function='GAT', time=3.0, tol_scale=200.0), 1910, False),
  'transformer_dopri5_rejects_one': (dict(time=8.0, tol_scale=20.0), 2012, True),
  'transformer_dopri5_rejects_many': (dict(time=12.0, tol_scale=500.0), 1951, True),
}


class RatioLog(object):
  """Wraps the shim's _compute_error_ratio while a solve runs; keeps every ratio it returns."""

  def __init__(self):
    self.ratios = []

  def __enter__(self):
    self.inner = shim._compute_error_ratio

    def logged(*args, **kw):
      r = self.inner(*args, **kw)
      self.ratios.append(float(r.detach()) if torch.is_tensor(r) else float(r))
      return r
    shim._compute_error_ratio = logged
    return self

  def __exit__(self, *exc):
    shim._compute_error_ratio = self.inner


def record(name, over, seed, want_rejects):
  n, d = 140, 24
  ei = G.make_graph(n, 6, 71)
  g = torch.Generator().manual_seed(72)
  x = torch.randn(n, d, generator=g)
  c = torch.randn(n, d, generator=g)
  opt = {**G.BASE, 'method': 'dopri5', 'block': 'constant', **over}
  fcls = {'transformer': G.ODEFuncTransformerAtt, 'GAT': G.ODEFuncAtt}[opt['function']]
  block = G.ConstantODEblock(fcls, [], opt, G.data_of(ei, x), torch.device('cpu'), t=torch.tensor([0, opt['time']]))
  G.randomise(block, seed)
  block.eval()
  block.set_x0(x)
  with torch.no_grad():
    z_eval = block(x)
  block.odefunc.nfe = 0
  block.train()
  xin = x.clone().requires_grad_(True)
  block.set_x0(xin)
  with RatioLog() as log:
    z = block(xin)
  nfe = block.odefunc.nfe
  (z * c).sum().backward()
  ratios = np.asarray(log.ratios, dtype=np.float64)
  inside = ratios[(ratios > BAND[0]) & (ratios < BAND[1])]
  assert inside.size == 0, '%s: trial steps with an error ratio near 1 (%s): pick another seed' % (name, inside)
  rejected = ratios[ratios > 1.0]
  assert (rejected.size > 0) == want_rejects, (name, rejected)
  assert nfe == 2 + 6 * ratios.size, (name, nfe, ratios.size)       # (f0, the initial step's probe, six per trial step)
  rec = {'edge_index': ei, 'x': x, 'c': c, 'z': z, 'z_eval': z_eval, 'grad_x': xin.grad, 'nfe': np.int64(nfe),
         'nfe_after_backward': np.int64(block.odefunc.nfe), 'ratios': ratios}
  for k, p in block.named_parameters():
    if p.grad is not None:
      rec['grad/' + k] = p.grad
  G.save('nltrain_' + name, opt, rec, block)
  print('    nfe %d, %d trial steps, largest accepted ratio %.3f, rejected: %s; grads: %s'
        % (nfe, ratios.size, ratios[ratios <= 1.0].max(), np.round(rejected, 2).tolist() or 'none',
           ', '.join(k[5:] for k in rec if k.startswith('grad/'))))


if __name__ == '__main__':
  for case, (over_, seed_, rejects_) in CASES.items():
    if len(sys.argv) == 1 or case in sys.argv[1:]:
      record(case, over_, seed_, rejects_)
