"""The native NMF half-sweep (gnpde_nmf_cd_sweep) timed against a torch composite of the same coordinate descent on this device.

  timeout -k 10 600 python tools/nmf_ab.py --shape dense2708 && timeout -k 10 900 python tools/nmf_ab.py --shape sparse169343

  native     ops.nmf_iteration: X H^T / X^T W (torch.mm, or ops.spmm for the sparse X), the two k x k Grams (ops.tall_skinny_gram)
             and two launches of the sweep kernel
  composite  the SAME products and Grams, and the sweep as a user would write it without the kernel: column by column over [n]
             vectors (W @ G[t] - P[:, t], where, clamp, one sum per column), the diagonal of G read by the host once per sweep
  products   the products and Grams alone (what both sides share)

Shapes: dense2708 = a dense 2 708 x 2 708 matrix, k = 64 (the Cora size); sparse169343 = a sparse 169 343 x 169 343 matrix with 64
entries per column, k = 128 (the ogbn-arxiv size after top-k GDC).  Per-iteration time: 5 iterations per timed window, event timing,
best of 3 after one warm-up window.  Both sides start every window from the same factors; the composite's factors after the
window are compared with the native ones.  One JSON line per shape, appended to --out (default profiles/nmf_ab.jsonl) and printed."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gnpde_amd import ops  # noqa: E402

ITERS, REPEATS = 5, 3
SHAPES = {'dense2708': dict(n=2708, k=64, sparse=False), 'sparse169343': dict(n=169343, k=128, sparse=True, per_column=64)}


def composite_sweep(W, G, P):
  diag = G.diagonal().tolist()
  violation = torch.zeros((), dtype=torch.float64, device=W.device)
  for t in range(W.shape[1]):
    grad = W @ G[t] - P[:, t]
    wt = W[:, t]
    violation += torch.where(wt == 0, grad.clamp(max=0), grad).abs().sum(dtype=torch.float64)
    if diag[t] != 0:
      W[:, t] = (wt - grad / diag[t]).clamp(min=0)
  return violation


def make_x(shape, dev):
  gen = torch.Generator(device=dev).manual_seed(0)
  n = shape['n']
  if not shape['sparse']:
    a = torch.randn(n, 8, generator=gen, device=dev).abs()
    return a @ torch.randn(8, n, generator=gen, device=dev).abs() + 0.05 * torch.randn(n, n, generator=gen, device=dev).abs(), n * n
  per = shape['per_column']
  col = torch.arange(n, device=dev).repeat_interleave(per)
  row = torch.randint(0, n, (n * per,), generator=gen, device=dev)
  key = torch.unique(row * n + col)                                    # a column draws a row twice now and then: kept once
  ei = torch.stack([torch.div(key, n, rounding_mode='floor'), key % n])
  return (ei, torch.rand(key.numel(), generator=gen, device=dev) + 0.01, (n, n)), int(key.numel())


def best_ms(fn):
  fn()
  torch.cuda.synchronize()
  best = float('inf')
  for _ in range(REPEATS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    best = min(best, e0.elapsed_time(e1))
  return best / ITERS


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shape', required=True, choices=sorted(SHAPES))
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nmf_ab.jsonl'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  shape = SHAPES[args.shape]
  n, k = shape['n'], shape['k']
  X, nnz = make_x(shape, dev)
  _, _, x_ht, xt_w, x_sum, _, _ = ops._nmf_operand(X)
  gen = torch.Generator(device=dev).manual_seed(1)
  avg = float(torch.sqrt(x_sum / (float(n) * n * k)))
  W0 = avg * torch.randn(n, k, generator=gen, device=dev).abs()
  Ht0 = avg * torch.randn(n, k, generator=gen, device=dev).abs()
  ws = torch.empty(int(ops._lib.lib().gnpde_nmf_cd_sweep_workspace_bytes(n)), dtype=torch.uint8, device=dev)
  state = {}

  def native():
    W, Ht = W0.clone(), Ht0.clone()
    for _ in range(ITERS):
      v = ops.nmf_iteration(x_ht, xt_w, W, Ht, ws)
    state['native'] = (W, Ht, v)

  def composite():
    W, Ht = W0.clone(), Ht0.clone()
    for _ in range(ITERS):
      v = composite_sweep(W, ops.tall_skinny_gram(Ht, Ht), x_ht(Ht))
      v = v + composite_sweep(Ht, ops.tall_skinny_gram(W, W), xt_w(W))
    state['composite'] = (W, Ht, v)

  def products():
    for _ in range(ITERS):
      ops.tall_skinny_gram(Ht0, Ht0), x_ht(Ht0), ops.tall_skinny_gram(W0, W0), xt_w(W0)

  t_native, t_comp, t_prod = best_ms(native), best_ms(composite), best_ms(products)
  (Wn, Hn, vn), (Wc, Hc, vc) = state['native'], state['composite']
  rec = dict(tool='nmf_ab', shape=args.shape, n=n, k=k, nnz=nnz, iterations=ITERS, repeats=REPEATS,
             native_iteration_ms=round(t_native, 4), composite_iteration_ms=round(t_comp, 4), products_iteration_ms=round(t_prod, 4),
             native_half_sweep_ms=round(max(t_native - t_prod, 0.0) / 2, 4), composite_half_sweep_ms=round(max(t_comp - t_prod, 0.0) / 2, 4),
             speedup_iteration=round(t_comp / t_native, 2), max_abs_dW=float((Wn - Wc).abs().max()), max_abs_dH=float((Hn - Hc).abs().max()),
             max_abs_W=float(Wn.abs().max()), violation_native=float(vn), violation_composite=float(vc),
             device=torch.cuda.get_device_name(0))
  print(json.dumps(rec), flush=True)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'a') as f:
    f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
  main()
