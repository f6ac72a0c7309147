"""Training through the BLEND split kernel (`--beltrami --function transformer --attention_type exp_kernel`, reference
src/function_transformer_attention.py:133-171) on the native VJP stage against the paths it had before: a C4-shaped GRAND-nl block
(synthetic ogbn-arxiv graph, 64 feature + 98 positional channels = d 162, attention_dim 32 / 2 heads, rk4, 10 steps).

  python tools/split_kernel_train_ab.py [--scale S] [--steps K] [--repeats R] [--legs recorded,adjoint] [--only native|host] [--out FILE]

Two legs, each an A/B in ONE process with the two sides alternating (a warm-up iteration each, then R timed iterations each, HIP
event timing):
  recorded  adjoint=False: the recorded solve + native reverse sweep    against   opt['gnpde_host_fixed_training'] (differentiable host loop)
  adjoint   adjoint=True, adjoint_method rk4: the native adjoint solve   against   opt['gnpde_host_adjoint'] (stage-by-stage loop)
One JSON line per side to --out (default profiles/split_kernel_train_ab.jsonl, appended) and to stdout: forward ms, backward ms, ms per
VJP stage (backward / evaluations), solver steps per second of a training iteration, all as best of R, with the run-to-run spread
(max - min) / min of the iteration time, plus the ratio host / native on the native side's line.
--only native (with --repeats 1): a single side, for a kernel trace of the stage (rocprofv3 --kernel-trace --stats -- python tools/...)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402

F0, P0, A, HEADS = 64, 98, 32, 2


class _Data(object):
  pass


def make_block(dev, ei, x, steps, adjoint, host):
  d = F0 + P0
  opt = dict(heads=HEADS, attention_dim=A, attention_type='exp_kernel', attention_norm_idx=0, square_plus=False, reweight_attention=False,
             beltrami=True, feat_hidden_dim=F0, pos_enc_hidden_dim=P0, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=10 ** 9,
             add_source=True, no_alpha_sigmoid=False, mix_features=False, hidden_dim=d, augment=False, adjoint=adjoint, adjoint_method='rk4',
             adjoint_step_size=1.0, tol_scale=1.0, tol_scale_adjoint=1.0, data_norm='rw', method='rk4', step_size=1.0, max_iters=100,
             block='constant', function='transformer', time=float(steps), att_samp_pct=1.0, use_flux=False,
             gnpde_host_fixed_training=bool(host and not adjoint), gnpde_host_adjoint=bool(host and adjoint))
  data = _Data()
  data.x, data.edge_index, data.edge_attr, data.num_nodes, data.num_features = x, ei, None, x.shape[0], d
  block = G.ConstantODEblock(G.ODEFuncTransformerAtt, [], opt, data, dev, t=torch.tensor([0, opt['time']])).to(dev)
  g = torch.Generator().manual_seed(5)
  with torch.no_grad():
    for name, p in block.named_parameters():
      if 'multihead_att_layer' in name and p.dim() >= 2:
        p.copy_((torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5).to(dev))
      elif 'lengthscale' in name:
        p.fill_(1.7)
      elif 'output_var' in name:
        p.fill_(1.1)
    for f in (block.odefunc, block.reg_odefunc.odefunc):
      f.alpha_train.fill_(0.4)
      f.beta_train.fill_(0.1)
  block.train()
  return block


def iteration(block, x, c):
  """One training iteration; (forward ms, backward ms, evaluations of the forward, evaluations of the backward)."""
  for p in block.parameters():
    p.grad = None
  xin = x.clone().requires_grad_(True)
  block.set_x0(xin)
  f = block.odefunc
  f.nfe = 0
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
  return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), nfe_f, f.nfe - nfe_f


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--scale', type=float, default=1.0, help='shrinks the synthetic ogbn-arxiv graph (nodes and edges)')
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--legs', default='recorded,adjoint')
  ap.add_argument('--only', default=None, choices=['native', 'host'])
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'split_kernel_train_ab.jsonl'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  ei_cpu, n = G.synthetic.make_graph('arxiv', seed=0, scale=args.scale)
  d = F0 + P0
  x = (torch.randn(n, d, generator=torch.Generator().manual_seed(41)) * 0.5).to(dev)
  c = torch.randn(n, d, generator=torch.Generator().manual_seed(42)).to(dev)
  ei = ei_cpu.to(dev)
  sides = [args.only] if args.only else ['native', 'host']
  for leg in args.legs.split(','):
    adjoint = leg == 'adjoint'
    blocks = {s: make_block(dev, ei, x, args.steps, adjoint, s == 'host') for s in sides}
    runs = {s: [] for s in sides}
    for s in sides:
      iteration(blocks[s], x, c)                       # warm-up: code objects, allocator, graph capture
    for _ in range(args.repeats):
      for s in sides:                                  # the sides alternate
        runs[s].append(iteration(blocks[s], x, c))
    lines = {}
    for s in sides:
      f = blocks[s].odefunc
      tot = [r[0] + r[1] for r in runs[s]]
      fwd, bwd = min(r[0] for r in runs[s]), min(r[1] for r in runs[s])
      nfe_f, nfe_b = runs[s][0][2], runs[s][0][3]
      stages = nfe_b if adjoint else nfe_f             # VJP stages of the backward: its own evaluations, or one per recorded evaluation
      path = 'native' if s == 'native' else 'host'
      if not adjoint:
        took = str(getattr(f, '_last_train_solve', ''))
        assert took.startswith('native recorded fixed-grid') == (s == 'native'), took
      else:
        assert bool(f.__dict__.get('_adjoint_state')) == (s == 'native')
      lines[s] = {'tool': 'split_kernel_train_ab', 'leg': leg, 'side': path, 'n': n, 'edges_with_self_loops': int(f.edge_index.shape[1]), 'd': d,
                  'feat_hidden_dim': F0, 'pos_enc_hidden_dim': P0, 'attention_dim': A, 'heads': HEADS, 'method': 'rk4', 'steps': args.steps,
                  'evals_forward': nfe_f, 'evals_backward': nfe_b, 'repeats': args.repeats,
                  'forward_ms': round(fwd, 3), 'backward_ms': round(bwd, 3), 'ms_per_vjp_stage': round(bwd / max(stages, 1), 4),
                  'iteration_ms': round(min(tot), 3), 'steps_per_s': round(args.steps / (min(tot) * 1e-3), 2),
                  'spread': round((max(tot) - min(tot)) / min(tot), 4)}
    if len(sides) == 2:
      lines['native']['host_over_native'] = round(lines['host']['iteration_ms'] / lines['native']['iteration_ms'], 3)
      lines['native']['host_over_native_backward'] = round(lines['host']['backward_ms'] / lines['native']['backward_ms'], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'a') as fh:
      for s in sides:
        print(json.dumps(lines[s]), flush=True)
        fh.write(json.dumps(lines[s]) + '\n')
    del blocks
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
