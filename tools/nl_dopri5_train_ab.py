"""Training GRAND-nl through dopri5 WITHOUT the adjoint method (`python run_GNN.py --function transformer`: adjoint off, method dopri5)
on the recorded device solve + native VJP-stage sweep (csrc/adjoint.hip, gnpde_adjoint_set_dopri5_tape) against the path it had
before, which is still in the tree behind the opt-out: the differentiable host loop (opt['gnpde_host_dopri5_training']).

  python tools/nl_dopri5_train_ab.py [--shapes cora,arxiv] [--repeats R] [--scale S] [--arxiv-time T] [--arxiv-tol-scale K] [--out FILE]

  cora    a Cora-like block: 2 485 nodes, d = 80, attention_dim 128 / 8 heads, squareplus over columns, T and tol_scale of best_params Cora
  arxiv   the synthetic ogbn-arxiv graph: d = 128, attention_dim 16 / 4 heads; T / tol_scale chosen so that about 10 steps are accepted

ONE process, the two sides alternating (a warm-up iteration each, then R timed iterations each -- 4 R for the small shape, whose host
side is launch-bound and noisy --, HIP event timing).  One JSON line per
side to --out (default profiles/nl_dopri5_train_ab.jsonl, REWRITTEN by every run: the file holds one run) and to stdout: forward ms, backward ms, ms per recorded
evaluation (backward / evaluations of the accepted steps), all as best of R, with the run-to-run spread (max - min) / min of the
iteration time, the accepted / rejected steps, and the ratio host / native on the native side's line.  Both sides' outputs and input
gradients are compared on the way (the lines carry the largest relative difference)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402

SHAPES = {
  'cora': dict(d=80, heads=8, attention_dim=128, time=18.294754260552843, tol_scale=821.9773048827274, square_plus=True, attention_norm_idx=1),
  'arxiv': dict(d=128, heads=4, attention_dim=16, time=8.0, tol_scale=100.0, square_plus=False, attention_norm_idx=0),
}


class _Data(object):
  pass


def make_block(dev, ei, x, cfg, host):
  d = cfg['d']
  opt = dict(heads=cfg['heads'], attention_dim=cfg['attention_dim'], attention_type='scaled_dot', attention_norm_idx=cfg['attention_norm_idx'],
             square_plus=cfg['square_plus'], reweight_attention=False, beltrami=False, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9,
             add_source=True, no_alpha_sigmoid=False, mix_features=False, hidden_dim=d, augment=False, adjoint=False, tol_scale=cfg['tol_scale'],
             data_norm='rw', method='dopri5', step_size=1.0, max_iters=100, block='constant', function='transformer', time=cfg['time'],
             gnpde_host_dopri5_training=bool(host))
  data = _Data()
  data.x, data.edge_index, data.edge_attr, data.num_nodes, data.num_features = x, ei, None, x.shape[0], d
  block = G.ConstantODEblock(G.ODEFuncTransformerAtt, [], opt, data, dev, t=torch.tensor([0, opt['time']])).to(dev)
  g = torch.Generator().manual_seed(5)
  with torch.no_grad():
    for name, p in block.named_parameters():
      if 'multihead_att_layer' in name and p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      elif 'multihead_att_layer' in name:        # (nn.Linear draws its default biases from the global generator: the same block on both sides)
        p.copy_((torch.randn(p.shape, generator=g) * 0.1).to(dev))
    for f in (block.odefunc, block.reg_odefunc.odefunc):
      f.alpha_train.fill_(0.4)
      f.beta_train.fill_(0.1)
  block.train()
  return block


def iteration(block, x, c):
  """One training iteration; (forward ms, backward ms, evaluations of the forward, z, dL/dx)."""
  for p in block.parameters():
    p.grad = None
  xin = x.clone().requires_grad_(True)
  block.set_x0(xin)
  f = block.odefunc
  f.nfe = 0
  f._last_train_solve = ''
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
  ev[0].record()
  z = block(xin)
  loss = (z * c).sum()
  ev[1].record()
  nfe_f = f.nfe
  loss.backward()
  ev[2].record()
  torch.cuda.synchronize()
  assert torch.isfinite(xin.grad).all()
  return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), nfe_f, z.detach(), xin.grad.detach()


def rel(a, b):
  return float((a - b).abs().max() / b.abs().max())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', default='cora,arxiv')
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--scale', type=float, default=1.0, help='shrinks the synthetic ogbn-arxiv graph (nodes and edges)')
  ap.add_argument('--arxiv-time', type=float, default=SHAPES['arxiv']['time'])
  ap.add_argument('--arxiv-tol-scale', type=float, default=SHAPES['arxiv']['tol_scale'])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nl_dopri5_train_ab.jsonl'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  open(args.out, 'w').close()
  for shape in args.shapes.split(','):
    repeats = 4 * args.repeats if shape == 'cora' else args.repeats
    cfg = dict(SHAPES[shape])
    if shape == 'arxiv':
      cfg.update(time=args.arxiv_time, tol_scale=args.arxiv_tol_scale)
      ei_cpu, n = G.synthetic.make_graph('arxiv', seed=0, scale=args.scale)
    else:
      ei_cpu, n = G.synthetic.make_graph('cora', seed=0, scale=2485 / 2708)
    d = cfg['d']
    x = (torch.randn(n, d, generator=torch.Generator().manual_seed(41)) * 0.5).to(dev)
    c = torch.randn(n, d, generator=torch.Generator().manual_seed(42)).to(dev)
    ei = ei_cpu.to(dev)
    sides = ['native', 'host']
    blocks = {s: make_block(dev, ei, x, cfg, s == 'host') for s in sides}
    runs = {s: [] for s in sides}
    for s in sides:
      iteration(blocks[s], x, c)                       # warm-up: code objects, allocator, graph capture
    for _ in range(repeats):
      for s in sides:                                  # the sides alternate
        runs[s].append(iteration(blocks[s], x, c))
    lines = {}
    for s in sides:
      f = blocks[s].odefunc
      took = str(getattr(f, '_last_train_solve', ''))
      assert took.startswith('native recorded-tape dopri5') == (s == 'native'), took
      tot = [r[0] + r[1] for r in runs[s]]
      fwd, bwd = min(r[0] for r in runs[s]), min(r[1] for r in runs[s])
      nfe = runs[s][0][2]
      lines[s] = {'tool': 'nl_dopri5_train_ab', 'shape': shape, 'side': s, 'n': n, 'edges_with_self_loops': int(f.edge_index.shape[1]), 'd': d,
                  'attention_dim': cfg['attention_dim'], 'heads': cfg['heads'], 'time': cfg['time'], 'tol_scale': cfg['tol_scale'],
                  'evals_forward': nfe, 'repeats': repeats, 'forward_ms': round(fwd, 3), 'backward_ms': round(bwd, 3),
                  'iteration_ms': round(min(tot), 3), 'spread': round((max(tot) - min(tot)) / min(tot), 4)}
    st = blocks['native'].odefunc._dopri5_stats
    recorded = 6 * st['accepted'] + 1
    for s in sides:
      lines[s].update(accepted=st['accepted'], rejected=st['rejected'], recorded_evals=recorded,
                      ms_per_recorded_eval=round(lines[s]['backward_ms'] / recorded, 4))
    lines['native']['host_over_native'] = round(lines['host']['iteration_ms'] / lines['native']['iteration_ms'], 3)
    lines['native']['host_over_native_forward'] = round(lines['host']['forward_ms'] / lines['native']['forward_ms'], 3)
    lines['native']['host_over_native_backward'] = round(lines['host']['backward_ms'] / lines['native']['backward_ms'], 3)
    lines['native']['same_evals_as_host'] = lines['host']['evals_forward'] == lines['native']['evals_forward']
    lines['native']['z_rel_diff_to_host'] = rel(runs['native'][-1][3], runs['host'][-1][3])
    lines['native']['grad_x_rel_diff_to_host'] = rel(runs['native'][-1][4], runs['host'][-1][4])
    with open(args.out, 'a') as fh:
      for s in sides:
        print(json.dumps(lines[s]), flush=True)
        fh.write(json.dumps(lines[s]) + '\n')
    del blocks
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
