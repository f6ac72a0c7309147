"""Solves with several output times: the native routes against the Python host loops (opt['gnpde_host_outputs']), timed
ALTERNATELY in one process so that clock and cache state drift hits both alike.

  python tools/output_times_ab.py [--graph cora|arxiv|both] [--function transformer|laplacian] [--repeats R] [--out FILE]

Per shape and solve one JSON line: rk4 with 16 evaluations (4 steps) and 8 outputs, and dopri5 with 8 outputs; wall time of one
no-grad `odeint` call that ends in a device synchronise, best of R after one warm-up call of each route, the ratio host / native, the
routes taken (func._last_output_solve) and the largest relative difference of the two results.  Lines are appended to --out
(default profiles/output_times_ab.jsonl).  Needs a HIP device: there is no fallback."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402


class _Data(object):
  pass


def make_block(name, function, dev, seed=0):
  cfg = G.synthetic.CONFIGS[name]
  ei, n = G.synthetic.make_graph(name, seed=seed)
  d = cfg['d']
  x = torch.randn(n, d, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
  opt = dict(heads=cfg['heads'], attention_dim=cfg['att_dim'], attention_type='scaled_dot', attention_norm_idx=0, square_plus=False,
             reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9, add_source=True,
             no_alpha_sigmoid=False, mix_features=False, hidden_dim=d, augment=False, adjoint=False, tol_scale=1.0, data_norm='rw',
             method='rk4', step_size=1.0, max_iters=100, block='constant', function=function, time=4.0)
  data = _Data()
  data.x, data.edge_index, data.edge_attr, data.num_nodes = x, ei.to(dev), None, n
  fcls = G.ODEFuncTransformerAtt if function == 'transformer' else G.LaplacianODEFunc
  block = G.ConstantODEblock(fcls, [], opt, data, dev, t=torch.tensor([0, 4.0])).to(dev)
  g = torch.Generator().manual_seed(seed + 2)
  with torch.no_grad():
    for pname, p in block.named_parameters():
      if p.dim() >= 2 and 'multihead_att_layer' in pname:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      elif pname.endswith('.bias'):
        p.zero_()
    block.odefunc.alpha_train.fill_(0.0)
    block.odefunc.beta_train.fill_(0.1)
  block.eval()
  block.odefunc.x0 = x
  return block, x, n, int(ei.shape[1]) + n, d


def timed(f, x, t, host, kw):
  f.opt['gnpde_host_outputs'] = host
  f.nfe = 0
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  with torch.no_grad():
    out = G.odeint(f, x, t, **kw)
  torch.cuda.synchronize()
  return time.perf_counter() - t0, out, f._last_output_solve, f.nfe


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--graph', default='both', choices=['cora', 'arxiv', 'both'])
  ap.add_argument('--function', default='transformer', choices=['transformer', 'laplacian'])
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'output_times_ab.jsonl'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('output_times_ab: no HIP device (nothing is measured without one)')
  dev = torch.device('cuda:0')
  solves = [('rk4, 16 evaluations, 8 outputs', [0.5 * k for k in range(9)], dict(method='rk4', options={'step_size': 1.0})),
            ('dopri5, 8 outputs', [0.5 * k for k in range(9)], dict(method='dopri5', rtol=50e-9, atol=50e-7))]
  for name in (['cora', 'arxiv'] if args.graph == 'both' else [args.graph]):
    block, x, n, e, d = make_block(name, args.function, dev)
    f = block.odefunc
    for label, times, kw in solves:
      t = torch.tensor(times, dtype=torch.float32, device=dev)
      best, outs, routes, nfes = {}, {}, {}, {}
      for host in (False, True):      # warm-up: builds, captures, first launches
        timed(f, x, t, host, kw)
      for _ in range(args.repeats):
        for host in (False, True):
          dt, out, route, nfe = timed(f, x, t, host, kw)
          best[host] = min(best.get(host, dt), dt)
          outs[host], routes[host], nfes[host] = out, route, nfe
      f.opt.pop('gnpde_host_outputs', None)
      diff = float((outs[False] - outs[True]).abs().max() / outs[True].abs().max())
      line = dict(tool='output_times_ab', graph=name, function=args.function, n=n, entries=e, d=d, solve=label, outputs=len(times) - 1,
                  nfe_native=nfes[False], nfe_host=nfes[True], native_ms=round(best[False] * 1e3, 4), host_ms=round(best[True] * 1e3, 4),
                  host_over_native=round(best[True] / best[False], 3), route_native=routes[False], route_host=routes[True],
                  max_rel_diff=diff, repeats=args.repeats, timing='host clock around one odeint call ending in a device synchronise, best of repeats')
      print(json.dumps(line), flush=True)
      with open(args.out, 'a') as fh:
        fh.write(json.dumps(line) + '\n')


if __name__ == '__main__':
  main()
