"""Hyperbolic positional encodings (BLEND's `--pos_enc_type HYPS<dd>`): an embedding of the nodes in the Poincare ball.

The reference loads `<dataset>_HYPS<dd>.pkl` (graph_rewiring.apply_beltrami, hyperbolic_distances.py) and ships no program that
writes such a file; include/gnpde.h is the authority for what is trained here.  Uniform random walks and negative walks exactly as
DeepWalk's (on Philox stream ids of their own), the window pairs of the walks, the score (R - dist) / T on the hyperbolic distance,
and a row-normalised Riemannian SGD step with projection into the ball (csrc/hyperbolic.hip).  An epoch is a plain sequence of native
launches on the current stream: the epoch order, then per batch the positive walks, the negative walks and one step (pair kernel,
radix sort, update kernel, loss kernel).  Nothing is read back inside an epoch; the per-step losses and the error flag are read
once at its end.

The defaults (context_size 2, lr 1, R 2, T 1, 16 walks of length 20 per node) are this package's choice, taken from a small float64
prototype on trees.  The encodings have not been evaluated on a real dataset."""
import os
import pickle

import torch

from . import _lib, ops

EPS = 1e-15
INIT_RANGE = 1e-3


def initial_embedding(num_nodes, embedding_dim, seed):
  """[n, d] float32, uniform in [-1e-3, 1e-3], drawn on the host: device independent, and a CPU oracle can share it."""
  u = torch.rand(int(num_nodes), int(embedding_dim), generator=torch.Generator().manual_seed(int(seed)))
  return (2.0 * u - 1.0) * INIT_RANGE


class PoincareEmbedding(object):
  """Native trainer of Poincare-ball embeddings.  edge_index: [2, E] int64 (moved to the HIP device); .embedding is [n, d] float32 on
  the device, every row inside the unit ball."""

  def __init__(self, edge_index, num_nodes, embedding_dim, walk_length=20, context_size=2, walks_per_node=16, num_negative_samples=1,
               lr=1.0, radius=2.0, temperature=1.0, seed=0, device=None):
    n, d = int(num_nodes), int(embedding_dim)
    self.walk_length, self.context_size = int(walk_length), int(context_size)
    self.walks_per_node, self.num_negative_samples = int(walks_per_node), int(num_negative_samples)
    if not 1 <= n <= ops.INT32_MAX:
      raise _lib.GnpdeError('PoincareEmbedding: num_nodes = %d outside 1 .. INT32_MAX' % n)
    ops.poincare_check_shape(self.walk_length, self.context_size, d, who='PoincareEmbedding')
    if self.walks_per_node < 1 or self.num_negative_samples < 1:
      raise _lib.GnpdeError('PoincareEmbedding: walks_per_node and num_negative_samples must be at least 1')
    if not (float(lr) >= 0 and float(temperature) > 0):
      raise _lib.GnpdeError('PoincareEmbedding: lr >= 0 and temperature > 0 are required (lr %r, temperature %r)' % (lr, temperature))
    if not isinstance(edge_index, torch.Tensor):
      raise _lib.GnpdeError('PoincareEmbedding: edge_index must be a [2, E] tensor')
    if device is None and not edge_index.is_cuda:
      if not torch.cuda.is_available():
        raise _lib.GnpdeError('PoincareEmbedding runs only on a HIP device and none is available; there is no CPU fallback')
      device = torch.device('cuda', torch.cuda.current_device())
    self.device = edge_index.device if device is None else torch.device(device)
    self.num_nodes, self.embedding_dim, self.seed = n, d, int(seed)
    self.lr, self.radius, self.temperature = float(lr), float(radius), float(temperature)
    self.graph = ops.walk_csr(edge_index.to(self.device), n)
    self.embedding = initial_embedding(n, d, self.seed).to(self.device)
    self.step_count = 0
    self.epoch = 0

  def fit(self, epochs, batch_size=128):
    """Train for `epochs` more epochs; returns the list of per-epoch mean losses (one host read per epoch)."""
    n, B, L = self.num_nodes, int(batch_size), self.walk_length
    if B < 1:
      raise _lib.GnpdeError('PoincareEmbedding.fit: batch_size = %d' % B)
    wpn, nns = self.walks_per_node, self.num_negative_samples
    n_batches = (n + B - 1) // B
    dev = self.device
    losses = torch.zeros(n_batches, dtype=torch.float32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    rb = min(B, n)
    pos = torch.empty(rb * wpn, L + 1, dtype=torch.int32, device=dev)
    neg = torch.empty(rb * wpn * nns, L + 1, dtype=torch.int32, device=dev)
    ws = {}      # at most two sizes: full batches and the short last one
    lib, ptr = _lib.lib(), _lib.ptr
    g = self.graph
    out = []
    with torch.cuda.device(dev):
      stream = _lib.stream_of(self.embedding)
      for _ in range(int(epochs)):
        e = self.epoch
        perm = ops.random_permutation(n, self.seed, ops.STREAM_HYP_EPOCH_ORDER, e, device=dev)
        for b in range(n_batches):
          nb = min(B, n - b * B)
          starts = perm[b * B:b * B + nb]
          r_pos, r_neg = nb * wpn, nb * wpn * nns
          _lib.check(lib.gnpde_random_walks(ptr(g.rowptr), ptr(g.col), g.col.numel(), n, ptr(starts), nb, r_pos, L, self.seed,
                                            ops.STREAM_HYP_POS_WALKS, e, b * B * wpn, ptr(pos), ptr(flag), stream))
          _lib.check(lib.gnpde_negative_walks(n, ptr(starts), nb, r_neg, L, self.seed, ops.STREAM_HYP_NEG_WALKS, e, b * B * wpn * nns,
                                              ptr(neg), ptr(flag), stream))
          if nb not in ws:
            ws[nb] = ops.poincare_workspace(r_pos, r_neg, L, self.context_size, self.embedding_dim, dev)
          self.step_count += 1
          ops.poincare_step(self.embedding, pos[:r_pos], neg[:r_neg], self.context_size, lr=self.lr, radius=self.radius,
                            temperature=self.temperature, loss_out=losses[b:b + 1], flag=flag, workspace=ws[nb])
        self.epoch += 1
        ops._raise_flags(flag, 'PoincareEmbedding.fit', ops.DEEPWALK_FLAGS)
        out.append(float(losses.double().mean().item()))
    return out


def embedding_dim_of(pos_enc_type):
  """The width dd of 'HYPS<dd>'; ValueError for anything else."""
  kind = str(pos_enc_type)
  if not kind.startswith('HYPS') or not kind[4:].isdigit() or int(kind[4:]) < 1:
    raise ValueError('cannot read the embedding width from pos_enc_type %r (expected HYPS<dd>)' % (pos_enc_type,))
  return int(kind[4:])


def pickle_name(opt):
  return '%s_HYPS%02d.pkl' % (opt['dataset'], int(opt['embedding_dim']))


DEFAULTS = dict(embedding_dim=16, walk_length=20, context_size=2, walks_per_node=16, neg_pos_ratio=1, epochs=100, lr=1.0, radius=2.0,
                temperature=1.0)


def main(opt, data, out_dir='../data/pos_encodings'):
  """Train and store `<out_dir>/<dataset>_HYPS<dd>.pkl`: a CPU float32 tensor [n, dd], the layout the reference's apply_beltrami and
  hyperbolize read.  opt: dataset, embedding_dim and optionally walk_length, context_size, walks_per_node, neg_pos_ratio, epochs, lr,
  radius, temperature, seed; data: an object with edge_index and num_nodes.  Returns the path."""
  opt = dict(DEFAULTS, **opt)
  print('[i] Generating hyperbolic embeddings for dataset: %s' % opt['dataset'])
  n = data.num_nodes[0] if isinstance(data.num_nodes, list) else data.num_nodes
  model = PoincareEmbedding(data.edge_index, n, opt['embedding_dim'], walk_length=opt['walk_length'], context_size=opt['context_size'],
                            walks_per_node=opt['walks_per_node'], num_negative_samples=opt['neg_pos_ratio'], lr=opt['lr'],
                            radius=opt['radius'], temperature=opt['temperature'], seed=opt.get('seed', 0))
  for epoch, loss in enumerate(model.fit(opt['epochs'], batch_size=128), 1):
    print('Epoch: %02d, Loss: %.4f' % (epoch, loss))
  z = model.embedding.detach().to(torch.device('cpu'))
  print('[i] Embedding shape is %s, largest norm %.6f' % (tuple(z.shape), float(z.norm(dim=1).max())))
  os.makedirs(out_dir, exist_ok=True)
  fname = os.path.join(out_dir, pickle_name(opt))
  print('[i] Storing embeddings in %s' % fname)
  with open(fname, 'wb') as f:
    pickle.dump(z, f)
  return fname
