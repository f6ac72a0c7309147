"""One native DeepWalk epoch (gnpde_amd.deepwalk_embeddings.DeepWalk.fit) timed against a torch composite of the same step on this device.

  python tools/deepwalk_ab.py [--shape cora|arxiv|all] [--dims 64,128] [--repeats R] [--out FILE]

  native     DeepWalk.fit(1, batch_size=128): epoch order, walks, pair kernel, radix sort, sum + Adam kernel, loss kernel
  composite  per batch: the SAME walks (drawn by the native walk kernels: torch has no random-walk operator of its own), walk
             windows by torch indexing (PyG's cat([rw[:, j:j + C]])), nn.Embedding(sparse=True), the loss with sigma(-x), autograd,
             torch.optim.SparseAdam; the loss stays on the device, one host read per epoch as in the native trainer

Shapes: Cora (2 708 nodes) and ogbn-arxiv (169 343 nodes) from synthetic.make_graph; walk length 20, context 16, 16 walks per node,
1 negative, batches of 128.  Event timing, best of R after a
warm-up epoch.  One JSON line per measurement, appended to --out (default profiles/deepwalk_ab.jsonl) and printed."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gnpde_amd as G  # noqa: E402
from gnpde_amd import ops  # noqa: E402
from gnpde_amd.deepwalk_embeddings import DeepWalk, EPS  # noqa: E402

L, C, WPN, NEG, B = 20, 16, 16, 1, 128


def pair_scores(emb, rw):
  win = torch.cat([rw[:, j:j + C] for j in range(L + 2 - C)], dim=0)
  h_start = emb(win[:, 0]).view(win.shape[0], 1, -1)
  h_rest = emb(win[:, 1:].reshape(-1)).view(win.shape[0], C - 1, -1)
  return (h_start * h_rest).sum(dim=-1).view(-1)


class Composite(object):
  def __init__(self, edge_index, n, d, dev, seed=0):
    self.n, self.dev, self.seed, self.epoch = n, dev, seed, 0
    self.graph = ops.walk_csr(edge_index, n)
    self.emb = torch.nn.Embedding(n, d, sparse=True).to(dev)
    with torch.no_grad():
      self.emb.weight.copy_(torch.randn(n, d, generator=torch.Generator().manual_seed(seed)))
    self.opt = torch.optim.SparseAdam(list(self.emb.parameters()), lr=0.01)

  def fit_epoch(self):
    n, e = self.n, self.epoch
    perm = ops.random_permutation(n, self.seed, ops.STREAM_EPOCH_ORDER, e, device=self.dev)
    flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
    total = torch.zeros((), device=self.dev)
    n_batches = (n + B - 1) // B
    for b in range(n_batches):
      batch = perm[b * B:(b + 1) * B]
      pos = ops.random_walks(self.graph, n, batch, L, self.seed, ops.STREAM_POS_WALKS, e, b * B * WPN, repeats=WPN, flag=flag)
      neg = ops.negative_walks(n, batch, L, self.seed, ops.STREAM_NEG_WALKS, e, b * B * WPN * NEG, repeats=WPN * NEG, flag=flag)
      self.opt.zero_grad()
      loss = (-torch.log(torch.sigmoid(pair_scores(self.emb, pos)) + EPS).mean()
              - torch.log(torch.sigmoid(-pair_scores(self.emb, neg)) + EPS).mean())
      loss.backward()
      self.opt.step()
      total += loss.detach()
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
  ap.add_argument('--dims', default='64,128')
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deepwalk_ab.jsonl'))
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  lines = []
  for shape in (('cora', 'arxiv') if args.shape == 'all' else (args.shape,)):
    ei, n = G.synthetic.make_graph(shape, seed=0)
    ei = ei.to(dev)
    n_batches = (n + B - 1) // B
    for d in (int(x) for x in args.dims.split(',')):
      native = DeepWalk(ei, n, embedding_dim=d, walk_length=L, context_size=C, walks_per_node=WPN, num_negative_samples=NEG, seed=0)
      t_native, loss_native = best_ms(lambda: native.fit(1, batch_size=B)[0], args.repeats)
      comp = Composite(ei, n, d, dev)
      t_comp, loss_comp = best_ms(lambda: comp.fit_epoch(), args.repeats)
      rec = dict(tool='deepwalk_ab', shape=shape, n=n, edges=int(ei.shape[1]), d=d, walk_length=L, context_size=C, walks_per_node=WPN,
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
