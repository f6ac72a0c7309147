"""The native k-nearest-neighbour search (ops.knn / gnpde_knn) against the chunked torch composite it replaces on this device,
    torch.cdist(x[a:b], x).pow(2).topk(k, largest=False)       (slabs of [chunk, n] distances in memory),
at the two shapes BLEND's rewiring meets: Cora (2 708 x 80, k = 64) and ogbn-arxiv (169 343 x 162 on 164-float rows, k = 64).

  python tools/knn_ab.py [--shape cora|arxiv|both] [--repeats R] [--chunk-floats F] [--splits S] [--variant V] [--k K]

Per shape one JSON line: best-of-R event time of both (after a warm-up call each), 2 n^2 d / time in TF for the native kernel
and its share of the 157.3 TF fp32 peak, the ratio composite / native, and the share of index entries on which the two agree
(they differ where fp32 rounding reorders near-equal distances: the composite's cdist is a different evaluation).
--splits: gnpde_tune(19, S), the column split of the native kernel (0: the library's rule).  --variant 2: gnpde_tune(20, 2), the
256-key row buffers for every k (an open lead at small n: DESIGN 4c)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import _lib  # noqa: E402

SHAPES = {'cora': (2708, 80, 80, 64), 'arxiv': (169343, 162, 164, 64)}     # n, d, row stride, k
PEAK_FP32_TF = 157.3


def composite(x, k, chunk):
  out = torch.empty(x.shape[0], k, dtype=torch.int64, device=x.device)
  for a in range(0, x.shape[0], chunk):
    out[a:a + chunk] = torch.cdist(x[a:a + chunk], x).pow(2).topk(k, dim=1, largest=False).indices
  return out


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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shape', default='both', choices=['cora', 'arxiv', 'both'])
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--chunk-floats', type=int, default=1 << 26, help='size of one [chunk, n] distance slab of the composite')
  ap.add_argument('--splits', type=int, default=0)
  ap.add_argument('--variant', type=int, default=0, choices=[0, 2],
                  help='gnpde_tune(20, .): 2 = the 256-key row buffers for every k (0: the default)')
  ap.add_argument('--k', type=int, default=None, help='override k of both shapes')
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  G.ops.tune(_lib.TUNE_KNN_SPLITS, args.splits)
  G.ops.tune(_lib.TUNE_KNN_VARIANT, args.variant)
  for name in (['cora', 'arxiv'] if args.shape == 'both' else [args.shape]):
    n, d, ld, k = SHAPES[name]
    k = args.k or k
    x = torch.zeros(n, ld, device=dev)[:, :d]
    x.copy_(torch.randn(n, d, generator=torch.Generator().manual_seed(0)).to(dev))
    chunk = max(1, min(n, args.chunk_floats // n))
    t_native, idx = best_ms(lambda: G.ops.knn(x, k), args.repeats)
    t_comp, ref = best_ms(lambda: composite(x, k, chunk), max(1, args.repeats // 2))
    tf = 2.0 * n * n * d / (t_native * 1e-3) / 1e12
    out = {'tool': 'knn_ab', 'shape': name, 'n': n, 'd': d, 'row_stride': ld, 'k': k, 'splits_knob': args.splits, 'variant_knob': args.variant,
           'native_ms': round(t_native, 3), 'composite_ms': round(t_comp, 3), 'composite_chunk_rows': chunk,
           'native_tf': round(tf, 2), 'share_of_fp32_peak': round(tf / PEAK_FP32_TF, 4),
           'composite_over_native': round(t_comp / t_native, 3),
           'index_agreement': round(float((idx == ref).double().mean()), 6),
           'set_agreement': round(float((idx.sort(1).values == ref.sort(1).values).double().mean()), 6)}
    print(json.dumps(out), flush=True)
    del x, idx, ref
    torch.cuda.empty_cache()
  G.ops.tune(_lib.TUNE_KNN_SPLITS, 0)
  G.ops.tune(_lib.TUNE_KNN_VARIANT, 0)


if __name__ == '__main__':
  main()
