"""The native graph diffusion rewiring (ops.gdc / gnpde_gdc_*) against the dense torch composite on this device,
    ppr:  alpha * torch.linalg.inv(I - (1 - alpha) T)      heat:  torch.matrix_exp(t (T - I))      then  .topk(k, dim=0)  and the column sums,
at the Cora shape (2 708 nodes); at the ogbn-arxiv shape (169 343 nodes) the native path alone -- the dense matrix would take 115 GB, so
no composite exists there.  Graphs are the synthetic stand-ins of gnpde_amd.synthetic.

  python tools/gdc_ab.py [--shape cora|arxiv|both] [--method ppr|heat] [--alpha A] [--t T] [--k K] [--tol TOL] [--block B] [--repeats R]
                         [--out profiles/gdc_ab.jsonl]

Per shape one JSON line (printed, and appended to --out): best-of-R event time after a warm-up call, the number of series terms, and at the
Cora shape the composite's time, the ratio, and the share of (row, col) entries on which the two selections agree.  Nothing here asserts a
speed.

  python tools/gdc_ab.py --push [--shape ...] [--alpha A] [--eps EPS] [--repeats R] [--exact-repeats R2] [--out profiles/gdc_push_ab.jsonl]

times the approximate pipeline GDCWrapper(approx='push', exact=False) -- forward push with tolerance EPS, threshold EPS, 'col' out, as
apply_gdc maps opt['gdc_threshold'] -- against the exact native path (the same wrapper without approx: ops.gdc with threshold EPS) on the
same graph: event time of the whole call, best of R after a warm-up (the exact path: best of R2, 0 skips it), edges returned by both
and the sources that took the push's slow path."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import ops  # noqa: E402


def composite(ei, n, method, param, k):
  """The dense path: transition matrix ('sym', unit loops), closed-form diffusion, per-column top-k, column normalisation."""
  dev = ei.device
  A = torch.zeros(n, n, device=dev)
  A.index_put_((ei[0], ei[1]), torch.ones(ei.shape[1], device=dev), accumulate=True)
  A += torch.eye(n, device=dev)
  r = A.sum(1).pow(-0.5)
  T = r[:, None] * A * r[None, :]
  eye = torch.eye(n, device=dev)
  S = param * torch.linalg.inv(eye - (1.0 - param) * T) if method == 'ppr' else torch.matrix_exp(param * (T - eye))
  val, row = S.topk(k, dim=0)
  return row, val / val.sum(0, keepdim=True)


def best_ms(fn, repeats):
  fn()                                      # warm-up (allocator, code objects)
  torch.cuda.synchronize()
  best, out = float('inf'), None
  for _ in range(repeats):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    best = min(best, e0.elapsed_time(e1))
  return best, out


class _Data(object):
  def __init__(self, n, ei):
    self.num_nodes, self.edge_index, self.edge_attr = n, ei, None


def push_ab(args, dev):
  W = G.graph_rewiring.GDCWrapper
  out_path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, 'profiles', 'gdc_push_ab.jsonl')
  diff = dict(method='ppr', alpha=args.alpha, eps=args.eps)
  sparse = dict(method='threshold', eps=args.eps)
  for name in (['cora', 'arxiv'] if args.shape == 'both' else [args.shape]):
    ei, n = G.synthetic.make_graph(name, seed=0)
    ei = ei.to(dev)
    push = W(1, 'sym', 'col', diff, sparse, exact=False, approx='push')
    t_push, res = best_ms(lambda: push(_Data(n, ei)), args.repeats)
    _, _, info = ops.gdc_push(ei, n, args.alpha, args.eps, return_info=True)
    out = {'tool': 'gdc_ab --push', 'shape': name, 'n': n, 'edges': int(ei.shape[1]), 'alpha': args.alpha, 'eps': args.eps,
           'push_ms': round(t_push, 3), 'push_edges': int(res.edge_attr.numel()), 'slow_sources': info['slow_sources']}
    del res, info
    torch.cuda.empty_cache()
    reps = args.repeats if args.exact_repeats is None else args.exact_repeats
    if reps > 0:
      exact = W(1, 'sym', 'col', diff, sparse, exact=True, tol=args.tol, block=args.block)
      t_exact, res = best_ms(lambda: exact(_Data(n, ei)), reps)
      out.update(exact_ms=round(t_exact, 3), exact_edges=int(res.edge_attr.numel()), exact_repeats=reps, exact_over_push=round(t_exact / t_push, 3))
      del res
    print(json.dumps(out), flush=True)
    with open(out_path, 'a') as f:
      f.write(json.dumps(out) + '\n')
    torch.cuda.empty_cache()


DEFAULT_OUT = os.path.join(ROOT, 'profiles', 'gdc_ab.jsonl')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--push', action='store_true', help='time the approximate push pipeline against the exact native path')
  ap.add_argument('--eps', type=float, default=1e-4, help='--push: the push tolerance and the threshold')
  ap.add_argument('--exact-repeats', type=int, default=None, help='--push: timed calls of the exact path (default --repeats; 0 skips it)')
  ap.add_argument('--shape', default='both', choices=['cora', 'arxiv', 'both'])
  ap.add_argument('--method', default='ppr', choices=['ppr', 'heat'])
  ap.add_argument('--alpha', type=float, default=0.05)
  ap.add_argument('--t', type=float, default=3.0)
  ap.add_argument('--k', type=int, default=64)
  ap.add_argument('--tol', type=float, default=1e-6)
  ap.add_argument('--block', type=int, default=256)
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--out', default=DEFAULT_OUT)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  if args.push:
    return push_ab(args, dev)
  param = args.alpha if args.method == 'ppr' else args.t
  kw = dict(method=args.method, k=args.k, tol=args.tol, block=args.block, **({'alpha': param} if args.method == 'ppr' else {'t': param}))
  for name in (['cora', 'arxiv'] if args.shape == 'both' else [args.shape]):
    ei, n = G.synthetic.make_graph(name, seed=0)
    ei = ei.to(dev)
    t_native, res = best_ms(lambda: ops.gdc(ei, None, n, **kw), args.repeats)
    out = {'tool': 'gdc_ab', 'shape': name, 'n': n, 'edges': int(ei.shape[1]), 'method': args.method, 'param': param, 'k': args.k, 'tol': args.tol,
           'block': args.block, 'terms': len(ops.gdc_terms(args.method, param, args.tol)), 'kept_edges': int(res[1].numel()),
           'native_ms': round(t_native, 3)}
    if name == 'cora':
      t_comp, (row, _) = best_ms(lambda: composite(ei, n, args.method, param, args.k), args.repeats)
      got = torch.zeros(n, n, dtype=torch.bool, device=dev)
      got[res[0][0], res[0][1]] = True
      want = torch.zeros(n, n, dtype=torch.bool, device=dev)
      want[row, torch.arange(n, device=dev)[None, :].expand_as(row)] = True
      out.update(composite_ms=round(t_comp, 3), composite_over_native=round(t_comp / t_native, 3),
                 selection_agreement=round(float((got & want).sum()) / max(int(got.sum()), 1), 6))
    print(json.dumps(out), flush=True)
    with open(args.out, 'a') as f:
      f.write(json.dumps(out) + '\n')
    del res
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
