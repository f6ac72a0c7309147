"""fp32 against bf16 gather operand (opt['gnpde_gather_dtype']) at the two benchmark shapes of synthetic.py, timed
ALTERNATELY in one process so that clock and cache state drift hits both modes alike.

  python tools/gather_dtype_ab.py [--graph arxiv|rmat|both] [--steps K] [--repeats R] [--function transformer|laplacian]
                                  [--mapping 0|1|2]

Per shape one JSON line: steps/s of ConstantODEblock.forward (rk4, K steps, one captured graph launch) in both modes -- median and
min / max over the repeats --, the ratio bf16 / fp32, and D_gpu = ||z_bf16 - z_fp32||_2 / ||z_fp32||_2 of the final state.
--mapping: gnpde_tune(18, .) for the bf16 kernel of the d = 68..128 / short-rows class (1: 32 lanes x 4 elements, 2: 16 lanes x 8
elements; 0: the library's default)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import _lib  # noqa: E402


class _Data(object):
  pass


def make_block(name, function, steps, dev, seed=0):
  cfg = G.synthetic.CONFIGS[name]
  ei, n = G.synthetic.make_graph(name, seed=seed)
  d = cfg['d']
  x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
  opt = dict(heads=cfg['heads'], attention_dim=cfg['att_dim'], attention_type='scaled_dot', attention_norm_idx=0, square_plus=False,
             reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9, add_source=True,
             no_alpha_sigmoid=False, mix_features=False, hidden_dim=d, augment=False, adjoint=False, tol_scale=1.0, data_norm='rw',
             method='rk4', step_size=1.0, max_iters=100, block='constant', function=function, time=float(steps))
  data = _Data()
  data.x, data.edge_index, data.edge_attr, data.num_nodes = x, ei.to(dev), None, n
  fcls = G.ODEFuncTransformerAtt if function == 'transformer' else G.LaplacianODEFunc
  block = G.ConstantODEblock(fcls, [], opt, data, dev, t=torch.tensor([0, float(steps)])).to(dev)
  g = torch.Generator().manual_seed(seed + 2)
  with torch.no_grad():
    for pname, p in block.named_parameters():
      if p.dim() >= 2 and 'multihead_att_layer' in pname:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      elif pname.endswith('.bias'):
        p.zero_()
    block.odefunc.alpha_train.fill_(0.0)
    block.odefunc.beta_train.fill_(0.1)
  return block.eval(), x, n, int(ei.shape[1]) + n, d


def forward(block, x, mode):
  block.odefunc.opt['gnpde_gather_dtype'] = mode
  block.set_x0(x)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  with torch.no_grad():
    z = block(x)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  assert block.odefunc.gather_dtype_used == mode, (block.odefunc.gather_dtype_used, mode)
  return z, dt


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--graph', default='both', choices=['arxiv', 'rmat', 'both'])
  ap.add_argument('--steps', type=int, default=None, help='rk4 steps per forward (default: 50 at arxiv, 4 at rmat)')
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--function', default='transformer', choices=['transformer', 'laplacian'])
  ap.add_argument('--mapping', type=int, default=0, choices=[0, 1, 2])
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  _lib.check(_lib.lib().gnpde_tune(_lib.TUNE_LO_MAPPING, args.mapping))
  for name in (['arxiv', 'rmat'] if args.graph == 'both' else [args.graph]):
    steps = args.steps or (50 if name == 'arxiv' else 4)
    block, x, n, e, d = make_block(name, args.function, steps, dev)
    # the two modes keep one solver each alive in turn (one live solver per function): every switch rebuilds and re-captures, so
    # each timed forward is preceded by an untimed one in the same mode
    times = {'fp32': [], 'bf16': []}
    z = {}
    for rep in range(args.repeats):
      for mode in ('fp32', 'bf16'):
        forward(block, x, mode)                 # build / capture / warm
        z[mode], dt = forward(block, x, mode)
        times[mode].append(dt)
    rate = {m: sorted(steps / t for t in ts) for m, ts in times.items()}
    med = {m: statistics.median(r) for m, r in rate.items()}
    d_gpu = float((z['bf16'].double() - z['fp32'].double()).norm() / z['fp32'].double().norm())
    out = {'tool': 'gather_dtype_ab', 'graph': name, 'function': args.function, 'nodes': n, 'edges_with_self_loops': e, 'd': d,
           'rk4_steps': steps, 'repeats': args.repeats, 'mapping': args.mapping,
           'steps_per_s': {m: {'median': round(med[m], 2), 'min': round(rate[m][0], 2), 'max': round(rate[m][-1], 2)} for m in rate},
           'ratio_bf16_over_fp32': round(med['bf16'] / med['fp32'], 4),
           'spread_rel': {m: round((rate[m][-1] - rate[m][0]) / med[m], 4) for m in rate},
           'D_gpu': d_gpu, 'finite': bool(torch.isfinite(z['bf16']).all())}
    print(json.dumps(out), flush=True)
    del block, x, z
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
