"""One native epoch of the hyperbolic encodings (gnpde_amd.hyperbolic_embeddings.PoincareEmbedding.fit) timed against a torch composite
of the same step on this device.

  python tools/hyp_ab.py [--shape cora|arxiv|all] [--dims 2,16] [--repeats R] [--out FILE]

  native     PoincareEmbedding.fit(1, batch_size=128): epoch order, walks, pair kernel, radix sort, update kernel, loss kernel
  composite  per batch: the SAME walks (drawn by the native walk kernels: torch has no random-walk operator of its own), the window
             pairs by torch indexing, a gather of both ends, the closed-form coefficients of include/gnpde.h, index_add_ of the
             contributions and of the pair-end counts, the per-row divide, the rescaled update and the projection; the loss stays on
             the device, one host read per epoch as in the native trainer

The yardstick is the composite on the same device, never the code under test; no ratio is fixed in advance.  Shapes: Cora (2 708
nodes) and ogbn-arxiv (169 343 nodes) from synthetic.make_graph; the trainer's defaults (walk length 20, context 2, 16 walks per node,
1 negative, lr 1, R 2, T 1), batches of 128.  Event timing, best of R after a warm-up epoch.  One JSON line per measurement, appended
to --out (default profiles/hyp_ab.jsonl) and printed."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import ops  # noqa: E402
from gnpde_amd.hyperbolic_embeddings import PoincareEmbedding, initial_embedding, EPS  # noqa: E402

L, C, WPN, NEG, B = 20, 2, 16, 1, 128
LR, RADIUS, TEMPERATURE = 1.0, 2.0, 1.0
EDGE = 1 - 1e-5


def pair_ends(rw):
  a = torch.arange(L + 2 - C, device=rw.device).repeat_interleave(C - 1)
  b = a + 1 + torch.arange(C - 1, device=rw.device).repeat(L + 2 - C)
  return rw[:, a].reshape(-1), rw[:, b].reshape(-1)


class Composite(object):
  def __init__(self, edge_index, n, d, dev, seed=0):
    self.n, self.dev, self.seed, self.epoch = n, dev, seed, 0
    self.graph = ops.walk_csr(edge_index, n)
    self.emb = initial_embedding(n, d, seed).to(dev)

  def side(self, rw, positive, g, c):
    """Adds one side's contributions to g [n, d] and its pair-end counts to c [n]; returns the side's mean loss term."""
    e = self.emb
    u, v = pair_ends(rw)
    eu, ev = e[u], e[v]
    alpha, beta = 1 - (eu * eu).sum(1), 1 - (ev * ev).sum(1)
    diff = eu - ev
    q = (diff * diff).sum(1)
    ab = alpha * beta
    r = q / ab
    apart = r > 0
    rs = torch.where(apart, r, torch.ones_like(r))
    dist = torch.where(apart, 2 * torch.log(torch.sqrt(rs) + torch.sqrt(1 + rs)), torch.zeros_like(r))
    x = (RADIUS - dist) / TEMPERATURE
    sp, sm = torch.sigmoid(x), torch.sigmoid(-x)
    denom = (sp if positive else sm) + EPS
    dldd = sp * sm / denom / TEMPERATURE
    w = torch.where(apart, (dldd if positive else -dldd) / torch.sqrt(rs * (1 + rs)) * 2 / ab, torch.zeros_like(r))
    g.index_add_(0, u, w[:, None] * (diff + (q / alpha)[:, None] * eu))
    g.index_add_(0, v, w[:, None] * ((q / beta)[:, None] * ev - diff))
    ones = torch.ones_like(r)
    c.index_add_(0, u, ones)
    c.index_add_(0, v, ones)
    return -torch.log(denom).mean()

  def fit_epoch(self):
    n, ep = self.n, self.epoch
    perm = ops.random_permutation(n, self.seed, ops.STREAM_HYP_EPOCH_ORDER, ep, device=self.dev)
    flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
    total = torch.zeros((), device=self.dev)
    n_batches = (n + B - 1) // B
    for b in range(n_batches):
      batch = perm[b * B:(b + 1) * B]
      pos = ops.random_walks(self.graph, n, batch, L, self.seed, ops.STREAM_HYP_POS_WALKS, ep, b * B * WPN, repeats=WPN, flag=flag)
      neg = ops.negative_walks(n, batch, L, self.seed, ops.STREAM_HYP_NEG_WALKS, ep, b * B * WPN * NEG, repeats=WPN * NEG, flag=flag)
      e = self.emb
      g, c = torch.zeros_like(e), torch.zeros(n, device=self.dev)
      total += self.side(pos, True, g, c) + self.side(neg, False, g, c)
      alpha = 1 - (e * e).sum(1)
      y = e - (LR * (alpha * alpha / 4) / c.clamp(min=1))[:, None] * g
      norm = y.norm(dim=1)
      y = torch.where((norm < EDGE)[:, None], y, y * (EDGE / norm.clamp(min=1e-30))[:, None])
      self.emb = torch.where((c > 0)[:, None], y, e)
    self.epoch += 1
    return float(total) / n_batches


def best_ms(fn, repeats):
  fn()                                      # warm-up epoch (allocator, code objects)
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
  ap.add_argument('--shape', default='all', choices=('cora', 'arxiv', 'all'))
  ap.add_argument('--dims', default='2,16')
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hyp_ab.jsonl'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  lines = []
  for shape in (('cora', 'arxiv') if args.shape == 'all' else (args.shape,)):
    ei, n = G.synthetic.make_graph(shape, seed=0)
    ei = ei.to(dev)
    n_batches = (n + B - 1) // B
    for d in (int(x) for x in args.dims.split(',')):
      native = PoincareEmbedding(ei, n, d, walk_length=L, context_size=C, walks_per_node=WPN, num_negative_samples=NEG, lr=LR, radius=RADIUS,
                                 temperature=TEMPERATURE, seed=0)
      t_native, loss_native = best_ms(lambda: native.fit(1, batch_size=B)[0], args.repeats)
      comp = Composite(ei, n, d, dev)
      t_comp, loss_comp = best_ms(lambda: comp.fit_epoch(), args.repeats)
      rec = dict(tool='hyp_ab', shape=shape, n=n, edges=int(ei.shape[1]), d=d, walk_length=L, context_size=C, walks_per_node=WPN,
                 negatives=NEG, batch_size=B, steps_per_epoch=n_batches, repeats=args.repeats, native_epoch_ms=round(t_native, 3),
                 composite_epoch_ms=round(t_comp, 3), native_step_us=round(1e3 * t_native / n_batches, 2),
                 composite_step_us=round(1e3 * t_comp / n_batches, 2), speedup=round(t_comp / t_native, 2),
                 native_epoch_loss=round(loss_native, 4), composite_epoch_loss=round(loss_comp, 4), device=torch.cuda.get_device_name(0))
      print(json.dumps(rec), flush=True)
      lines.append(rec)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'a') as f:
    for rec in lines:
      f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
  main()
