"""The native positional-distance rewiring (ops.knn(metric='poincare') / ops.radius_graph) timed on this device.

  python tools/posdist_ab.py [--shape cora|arxiv16|arxiv64|all] [--repeats R] [--splits S] [--out FILE]

  cora      2 708 x 16, Poincare, q = 1/1000 and k = 64: native against the dense torch composite it replaces at this size,
            Gram matrix -> D -> R = D / (a_i a_j) -> kthvalue (quantile) / topk (k-NN) -> nonzero; the share of edges / index
            entries on which the two agree (they differ where fp32 rounding reorders near-equal keys)
  arxiv16,  169 343 x 16 and x 64, Poincare, q = 1/1000: native only (the dense composite would need 115 GB in fp32): the three
  arxiv64   phases separately -- quantile (three sweeps of the tile pipeline), count, fill -- the time per sweep, and 2 n^2 d /
            sweep time against the 157.3 TF fp32 peak (at d = 16 a sweep is bound by the epilogue, not by the matrix cores)

Event timing, best of R after a warm-up call.  One JSON line per measurement, appended to --out (default
profiles/posdist_ab.jsonl) and printed.  --splits: gnpde_tune(19, S) (0: the library's rule)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import _lib  # noqa: E402
from gnpde_amd._lib import ptr, check, stream_of  # noqa: E402

SHAPES = {'cora': (2708, 16), 'arxiv16': (169343, 16), 'arxiv64': (169343, 64)}
PEAK_FP32_TF = 157.3
Q = 1 / 1000
K = 64


def ball_points(n, d, seed=0):
  """Uniform in the ball of radius 0.95 (the construction of the tests)."""
  g = torch.Generator().manual_seed(seed)
  z = torch.randn(n, d, generator=g)
  r = torch.rand(n, generator=g) ** (1.0 / d) * 0.95
  return z / z.norm(dim=1, keepdim=True) * r[:, None]


def composite_keys(x):
  s = (x * x).sum(1)
  a = torch.clamp(1.0 - s, min=2.0 ** -24)
  D = torch.clamp(s[:, None] + s[None, :] - 2.0 * (x @ x.T), min=0.0)
  D.fill_diagonal_(0.0)
  return D / (a[:, None] * a[None, :])


def composite_radius(x, q):
  R = composite_keys(x)
  n = x.shape[0]
  tau = R.reshape(-1).kthvalue(int((n * n - 1) * q) + 1).values
  return (R <= tau).nonzero().T.contiguous()


def composite_knn(x, k):
  return composite_keys(x).topk(k, dim=1, largest=False).indices


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


def phases(x, q, metric, repeats):
  """Best-of-R event time of gnpde_radius_quantile, _count and _fill, each on its own."""
  L = _lib.lib()
  n, d = x.shape
  m = G.ops.METRICS[metric]
  ws = torch.empty(int(L.gnpde_radius_workspace_bytes(n, d)), dtype=torch.uint8, device=x.device)
  tau = torch.empty(2, dtype=torch.float32, device=x.device)
  rowptr = torch.empty(n + 1, dtype=torch.int64, device=x.device)
  st = stream_of(x)
  t_q, _ = best_ms(lambda: check(L.gnpde_radius_quantile(ptr(x), n, d, x.stride(0), m, q, ptr(tau), ptr(ws), ws.numel(), st)), repeats)
  t_c, _ = best_ms(lambda: check(L.gnpde_radius_count(ptr(x), n, d, x.stride(0), m, ptr(tau), 0.0, ptr(rowptr), ptr(ws), ws.numel(), st)),
                   repeats)
  E = int(rowptr[-1].item())
  ei = torch.empty(2, E, dtype=torch.int64, device=x.device)
  t_f, _ = best_ms(lambda: check(L.gnpde_radius_fill(ptr(x), n, d, x.stride(0), m, ptr(tau), 0.0, ptr(ei), E, ptr(ws), ws.numel(), st)),
                   repeats)
  return t_q, t_c, t_f, E, float(tau[0].item())


def emit(rec, path):
  line = json.dumps(rec)
  print(line, flush=True)
  os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
  with open(path, 'a') as f:
    f.write(line + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shape', default='all', choices=sorted(SHAPES) + ['all'])
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--splits', type=int, default=0)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'posdist_ab.jsonl'))
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('posdist_ab: no GPU -- nothing is measured without one')
  dev = torch.device('cuda:0')
  G.ops.tune(_lib.TUNE_KNN_SPLITS, args.splits)
  for name in (sorted(SHAPES) if args.shape == 'all' else [args.shape]):
    n, d = SHAPES[name]
    x = ball_points(n, d).to(dev)
    base = {'tool': 'posdist_ab', 'shape': name, 'n': n, 'd': d, 'metric': 'poincare', 'q': Q, 'splits_knob': args.splits,
            'repeats': args.repeats}
    t_q, t_c, t_f, E, tau = phases(x, Q, 'poincare', args.repeats)
    sweep = t_q / 3.0
    tf = 2.0 * n * n * d / (sweep * 1e-3) / 1e12
    emit(dict(base, what='radius phases', quantile_ms=round(t_q, 3), ms_per_sweep=round(sweep, 3), count_ms=round(t_c, 3),
              fill_ms=round(t_f, 3), edges=E, tau_key=tau, sweep_tf=round(tf, 3), share_of_fp32_peak=round(tf / PEAK_FP32_TF, 5)), args.out)
    t_native, ei = best_ms(lambda: G.ops.radius_graph(x, quantile=Q, metric='poincare'), args.repeats)
    rec = dict(base, what='radius_graph end to end', native_ms=round(t_native, 3), edges=int(ei.shape[1]))
    if name == 'cora':
      t_comp, ref = best_ms(lambda: composite_radius(x, Q), args.repeats)
      both = torch.zeros(n, n, dtype=torch.int8, device=dev)
      both[ei[0], ei[1]] += 1
      both[ref[0], ref[1]] += 2
      rec.update(composite_ms=round(t_comp, 3), composite_over_native=round(t_comp / t_native, 3), composite_edges=int(ref.shape[1]),
                 edges_in_both=int((both == 3).sum()))
    emit(rec, args.out)
    del ei
    if name == 'cora':
      t_native, idx = best_ms(lambda: G.ops.knn(x, K, metric='poincare'), args.repeats)
      t_comp, ref = best_ms(lambda: composite_knn(x, K), args.repeats)
      emit(dict(base, what='knn', k=K, native_ms=round(t_native, 3), composite_ms=round(t_comp, 3),
                composite_over_native=round(t_comp / t_native, 3), index_agreement=round(float((idx == ref).double().mean()), 6)), args.out)
    del x
    torch.cuda.empty_cache()
  G.ops.tune(_lib.TUNE_KNN_SPLITS, 0)


if __name__ == '__main__':
  main()
