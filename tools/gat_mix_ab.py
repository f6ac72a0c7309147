"""No-grad rk4 solve of the GAT function's mix_features form, f = alpha (A(x) (x W) Wout - x) + beta x0: the captured native solve over
the flagged descriptor (GNPDE_RHS_MIX_FEATURES: projection, attention, aggregation of projection rows, out-projection with the stage
epilogue -- csrc/out_proj.hip) against what such a solve ran before it, the host loop over the eager evaluation (ODEFuncAtt._eager_chain:
the same four kinds of launch plus an elementwise tail in torch, and the stage algebra in torch).

  python tools/gat_mix_ab.py [--shapes cora,arxiv] [--repeats R] [--scale S] [--steps K] [--out FILE]

  cora    2 708 nodes, d = 80, attention_dim 64 / 8 heads
  arxiv   the synthetic ogbn-arxiv graph (169 343 nodes), d = 128, attention_dim 64 / 4 heads

ONE process, the two sides alternating (a warm-up solve each, then R timed solves each, HIP event timing), best of R with the
run-to-run spread (max - min) / min; the two results are compared on the way.  The out-projection kernel is also timed alone (stages
RHS and RK4C, best of 20 launches) against its byte model: reads z [n, A] + u [n, d] + the stage's operands, writes out_k / out_y.
One JSON line per side and per kernel stage, APPENDED to --out (default profiles/gat_mix_ab.jsonl) and printed."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import _lib, ops  # noqa: E402

O = importlib.import_module('gnpde_amd.odeint')
SHAPES = {'cora': dict(d=80, heads=8, attention_dim=64), 'arxiv': dict(d=128, heads=4, attention_dim=64)}


class _Data(object):
  pass


def make_block(dev, ei, x, cfg, steps):
  d = cfg['d']
  opt = dict(heads=cfg['heads'], attention_dim=cfg['attention_dim'], attention_type='scaled_dot', attention_norm_idx=0, square_plus=False,
             reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9, add_source=True,
             no_alpha_sigmoid=False, mix_features=True, hidden_dim=d, augment=False, adjoint=False, tol_scale=1.0, data_norm='rw',
             method='rk4', step_size=1.0, max_iters=100, block='constant', function='GAT', time=float(steps))
  data = _Data()
  data.x, data.edge_index, data.edge_attr, data.num_nodes, data.num_features = x, ei, None, x.shape[0], d
  block = G.ConstantODEblock(G.ODEFuncAtt, [], opt, data, dev, t=torch.tensor([0, opt['time']])).to(dev)
  g = torch.Generator().manual_seed(5)
  with torch.no_grad():
    for name, p in block.named_parameters():
      if p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
    for f in (block.odefunc, block.reg_odefunc.odefunc):
      f.alpha_train.fill_(0.4)
      f.beta_train.fill_(0.1)
  block.eval()
  block.set_x0(x)
  return block


def timed(fn):
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record()
  out = fn()
  ev[1].record()
  torch.cuda.synchronize()
  return ev[0].elapsed_time(ev[1]), out


def kernel_alone(dev, n, d, A, shape, out):
  """gnpde_linear_epilogue by itself against its byte model."""
  g = torch.Generator().manual_seed(9)
  z = torch.randn(n, A, generator=g).to(dev)
  wt = (torch.randn(d, A, generator=g) / A ** 0.5).to(dev)
  u, x0, y, k1 = [torch.randn(n, d, generator=g).to(dev) for _ in range(4)]
  alpha, beta = torch.tensor([0.4], device=dev), torch.tensor([0.1], device=dev)
  res = torch.empty(n, d, device=dev)
  stages = {
    'RHS': (ops.make_epilogue(alpha, beta, x0, True, stage=_lib.STAGE_RHS, out_k=res), 2, 1),                       # reads u, x0; writes out_k
    'RK4C': (ops.make_epilogue(alpha, beta, x0, True, stage=_lib.STAGE_RK4C, dt=1.0, y=y, k1=k1, out_y=res), 4, 1),  # reads u, x0, y, k1
  }
  lines = []
  for name, (e, reads, writes) in stages.items():
    ops.linear_epilogue(z, wt, u, e)
    best = min(timed(lambda: ops.linear_epilogue(z, wt, u, e))[0] for _ in range(20))
    model = 4 * n * (A + (reads + writes) * d)
    lines.append({'tool': 'gat_mix_ab', 'what': 'out_proj_kernel', 'shape': shape, 'stage': name, 'n': n, 'd': d, 'attention_dim': A,
                  'us': round(best * 1e3, 2), 'model_bytes': model, 'model_gb_per_s': round(model / (best * 1e-3) / 1e9, 1)})
  return lines


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cora,arxiv')
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--scale', type=float, default=1.0, help='shrinks the synthetic ogbn-arxiv graph (nodes and edges)')
  ap.add_argument('--steps', type=int, default=4, help='rk4 steps of size 1 (4 evaluations each)')
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gat_mix_ab.jsonl'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  for shape in args.shapes.split(','):
    cfg = SHAPES[shape]
    ei_cpu, n = G.synthetic.make_graph(shape, seed=0, scale=args.scale if shape == 'arxiv' else 1.0)
    d = cfg['d']
    x = (torch.randn(n, d, generator=torch.Generator().manual_seed(41)) * 0.5).to(dev)
    block = make_block(dev, ei_cpu.to(dev), x, cfg, args.steps)
    f = block.odefunc
    t = block.t.to(dev).float()
    chain = lambda tq, y: f._eager_chain(y)        # noqa: E731

    def native():
      with torch.no_grad():
        return G.odeint(f, x, t, method='rk4', options=dict(step_size=1.0))[1]

    def host():
      with torch.no_grad():
        return O._solve_fixed_host(chain, x, t, 'rk4', 1.0)[1]

    sides = {'native': native, 'host': host}
    runs = {s: [] for s in sides}
    last = {}
    for s, fn in sides.items():
      fn()                                         # warm-up: code objects, allocator, graph capture
    torch.cuda.synchronize()
    for _ in range(args.repeats):
      for s, fn in sides.items():                  # the sides alternate
        ms, last[s] = timed(fn)
        runs[s].append(ms)
    assert f.__dict__.get('_solver_state'), 'the native side did not take the captured fixed-step solver'
    lines = []
    for s in sides:
      best = min(runs[s])
      lines.append({'tool': 'gat_mix_ab', 'what': 'rk4_solve', 'shape': shape, 'side': s, 'n': n, 'edges_with_self_loops': int(f.edge_index.shape[1]),
                    'd': d, 'attention_dim': cfg['attention_dim'], 'heads': cfg['heads'], 'evals': 4 * args.steps, 'repeats': args.repeats,
                    'solve_ms': round(best, 3), 'ms_per_eval': round(best / (4 * args.steps), 4),
                    'spread': round((max(runs[s]) - best) / best, 4)})
    lines[0]['host_over_native'] = round(lines[1]['solve_ms'] / lines[0]['solve_ms'], 3)
    lines[0]['z_rel_diff_to_host'] = float((last['native'] - last['host']).abs().max() / last['host'].abs().max())
    lines += kernel_alone(dev, n, d, cfg['attention_dim'], shape, args.out)
    with open(args.out, 'a') as fh:
      for ln in lines:
        print(json.dumps(ln), flush=True)
        fh.write(json.dumps(ln) + '\n')
    del block
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
