"""DeepWalk positional encodings under the reference's name (src/deepwalk_embeddings.py), without torch_geometric / torch_cluster.

The reference trains torch_geometric's Node2Vec (p = q = 1, sparse embedding) with torch.optim.SparseAdam at lr 0.01 in batches of
128 start nodes.  Here an epoch is a plain sequence of native launches on the current stream (csrc/deepwalk.hip; include/gnpde.h has
the definitions): the epoch order, then per batch the positive walks, the negative walks and one step (pair kernel, radix sort,
sum + Adam kernel, loss kernel).  The host knows every size, so nothing is read back inside an epoch; the per-step losses and the
error flag are read once at its end.

Deliberate differences from the reference: the random numbers are this package's Philox4x32-10 streams (equal seeds give equal
embeddings, bit for bit, on every run); the negative term of the loss is -log(sigma(-x) + EPS), not PyG's literal
-log(1 - sigma(x) + EPS), which is log(EPS) in fp32 once x > ~17; biased (p, q) walks are not built."""
import os
import pickle

import torch

from . import _lib, ops

EPS = 1e-15


class DeepWalk(object):
  """Native DeepWalk trainer.  edge_index: [2, E] int64 (moved to the HIP device); .embedding is [n, d] float32 on the device."""

  def __init__(self, edge_index, num_nodes, embedding_dim=128, walk_length=20, context_size=16, walks_per_node=16, num_negative_samples=1,
               lr=0.01, seed=0, p=1, q=1, device=None):
    if p != 1 or q != 1:
      raise NotImplementedError('DeepWalk: biased node2vec walks (p = %r, q = %r) are not built; p = q = 1 only' % (p, q))
    n, d = int(num_nodes), int(embedding_dim)
    self.walk_length, self.context_size = int(walk_length), int(context_size)
    self.walks_per_node, self.num_negative_samples = int(walks_per_node), int(num_negative_samples)
    if not 1 <= n <= ops.INT32_MAX:
      raise _lib.GnpdeError('DeepWalk: num_nodes = %d outside 1 .. INT32_MAX' % n)
    ops.deepwalk_check_shape(self.walk_length, self.context_size, d, who='DeepWalk')
    if self.walks_per_node < 1 or self.num_negative_samples < 1:
      raise _lib.GnpdeError('DeepWalk: walks_per_node and num_negative_samples must be at least 1')
    if not isinstance(edge_index, torch.Tensor):
      raise _lib.GnpdeError('DeepWalk: edge_index must be a [2, E] tensor')
    if device is None and not edge_index.is_cuda:
      if not torch.cuda.is_available():
        raise _lib.GnpdeError('DeepWalk runs only on a HIP device and none is available; there is no CPU fallback')
      device = torch.device('cuda', torch.cuda.current_device())
    self.device = edge_index.device if device is None else torch.device(device)
    self.num_nodes, self.embedding_dim, self.lr, self.seed = n, d, float(lr), int(seed)
    self.graph = ops.walk_csr(edge_index.to(self.device), n)
    # nn.Embedding's N(0, 1), drawn on the host: device-independent, and a CPU oracle can share it
    self.embedding = torch.randn(n, d, generator=torch.Generator().manual_seed(self.seed)).to(self.device)
    self.exp_avg = torch.zeros_like(self.embedding)
    self.exp_avg_sq = torch.zeros_like(self.embedding)
    self.step_count = 0
    self.epoch = 0

  def fit(self, epochs, batch_size=128):
    """Train for `epochs` more epochs; returns the list of per-epoch mean losses (one host read per epoch)."""
    n, B, L = self.num_nodes, int(batch_size), self.walk_length
    if B < 1:
      raise _lib.GnpdeError('DeepWalk.fit: batch_size = %d' % B)
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
        perm = ops.random_permutation(n, self.seed, ops.STREAM_EPOCH_ORDER, e, device=dev)
        for b in range(n_batches):
          nb = min(B, n - b * B)
          starts = perm[b * B:b * B + nb]
          r_pos, r_neg = nb * wpn, nb * wpn * nns
          _lib.check(lib.gnpde_random_walks(ptr(g.rowptr), ptr(g.col), g.col.numel(), n, ptr(starts), nb, r_pos, L, self.seed,
                                            ops.STREAM_POS_WALKS, e, b * B * wpn, ptr(pos), ptr(flag), stream))
          _lib.check(lib.gnpde_negative_walks(n, ptr(starts), nb, r_neg, L, self.seed, ops.STREAM_NEG_WALKS, e, b * B * wpn * nns, ptr(neg),
                                              ptr(flag), stream))
          if nb not in ws:
            ws[nb] = ops.deepwalk_workspace(r_pos, r_neg, L, self.context_size, self.embedding_dim, dev)
          self.step_count += 1
          ops.deepwalk_step(self.embedding, self.exp_avg, self.exp_avg_sq, self.step_count, pos[:r_pos], neg[:r_neg], self.context_size,
                            lr=self.lr, loss_out=losses[b:b + 1], flag=flag, workspace=ws[nb])
        self.epoch += 1
        ops._raise_flags(flag, 'DeepWalk.fit', ops.DEEPWALK_FLAGS)
        out.append(float(losses.double().mean().item()))
    return out


def node_classification_accuracy(z, data, max_iter=150):
  """PyG's Node2Vec.test: LogisticRegression(solver='lbfgs', multi_class='auto') on the train mask, accuracy on the test mask.  0.0
  when `data` lacks y / train_mask / test_mask or sklearn is not installed."""
  if any(getattr(data, k, None) is None for k in ('y', 'train_mask', 'test_mask')):
    return 0.0
  try:
    from sklearn.linear_model import LogisticRegression
  except ImportError:
    return 0.0
  z = z.detach().cpu()
  y, tr, te = data.y.cpu(), data.train_mask.cpu(), data.test_mask.cpu()
  try:
    clf = LogisticRegression(solver='lbfgs', multi_class='auto', max_iter=max_iter)
  except TypeError:            # newer sklearn dropped multi_class ('auto' is what remains)
    clf = LogisticRegression(solver='lbfgs', max_iter=max_iter)
  clf.fit(z[tr].numpy(), y[tr].numpy())
  return float(clf.score(z[te].numpy(), y[te].numpy()))


def pickle_name(opt):
  return 'DW_%s_emb_%03d_wl_%03d_cs_%02d_wn_%02d_epochs_%03d.pickle' % (
    opt['dataset'], opt['embedding_dim'], opt['walk_length'], opt['context_size'], opt['walks_per_node'], opt['epochs'])


DEFAULTS = dict(embedding_dim=128, walk_length=20, context_size=16, walks_per_node=16, neg_pos_ratio=1, epochs=100)


def main(opt, data, out_dir='../data/pos_encodings'):
  """The reference script's main on the native trainer.  opt: its options (dataset, embedding_dim, walk_length, context_size,
  walks_per_node, neg_pos_ratio, epochs; optional seed); data: an object with edge_index and num_nodes (and y / train_mask /
  test_mask for the accuracy).  Writes <out_dir>/DW_<dataset>_emb_..._epochs_....pickle with {'data': cpu tensor, 'acc': acc} and
  returns its path."""
  opt = dict(DEFAULTS, **opt)
  print('[i] Generating embeddings for dataset: %s' % opt['dataset'])
  model = DeepWalk(data.edge_index, data.num_nodes, embedding_dim=opt['embedding_dim'], walk_length=opt['walk_length'],
                   context_size=opt['context_size'], walks_per_node=opt['walks_per_node'], num_negative_samples=opt['neg_pos_ratio'],
                   lr=0.01, seed=opt.get('seed', 0))
  for epoch, loss in enumerate(model.fit(opt['epochs'], batch_size=128), 1):
    print('Epoch: %02d, Loss: %.4f' % (epoch, loss))
  z = model.embedding
  acc = node_classification_accuracy(z, data)
  print('[i] Final accuracy is %s' % acc)
  print('[i] Embedding shape is %s' % (tuple(z.shape),))
  os.makedirs(out_dir, exist_ok=True)
  fname = os.path.join(out_dir, pickle_name(opt))
  print('[i] Storing embeddings in %s' % fname)
  with open(fname, 'wb') as f:
    pickle.dump({'data': z.detach().to(torch.device('cpu')), 'acc': acc}, f)
  return fname
