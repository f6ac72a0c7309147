"""CPU oracle of the DeepWalk positional encodings (csrc/deepwalk.hip, gnpde_amd.deepwalk_embeddings): restatements of what
include/gnpde.h defines.

  walks, negative walks, epoch order   numpy, on the Philox words of edge_sampling_oracle.words: compared for integer equality
  step                                  torch: nn.Embedding(sparse=True), PyG's window construction cat([rw[:, j:j + C]]), the loss
                                        -log(sigma(x) + EPS) / -log(sigma(-x) + EPS), autograd, torch.optim.SparseAdam; float64 is the
                                        yardstick
  trainer                               composed of these, batch by batch as the header's "Epoch e, batch b" says

Tolerance of a step / trainer case (never derived from the code under test): the SAME oracle run in float32 next to the float64 run,
d32 = max |fp32 - fp64| over weights, exp_avg, exp_avg_sq and the losses; the absolute tolerance of the case is 8 * d32 (TOL_FACTOR).
The factor covers the device's different summation order (inside the walk first, then across walks) and expf at 2 ulp.  d32 is
recomputed where the tests run (case_result / trainer_result); the figures below are one recorded run of
print_tolerances() (torch CPU kernels):

  case                   d32       8 * d32   | case                   d32       8 * d32
  grid-L20C16-d4-k1      2.11e-07  1.68e-06    | grid-L20C16-d4-k2      1.76e-07  1.41e-06
  grid-L20C16-d64-k1     2.95e-07  2.36e-06    | grid-L20C16-d64-k2     2.32e-07  1.85e-06
  grid-L20C16-d100-k1    9.74e-07  7.80e-06    | grid-L20C16-d100-k2    6.76e-07  5.41e-06
  grid-L20C16-d256-k1    5.53e-06  4.42e-05    | grid-L20C16-d256-k2    7.81e-06  6.25e-05
  grid-L5C5-d4-k1        2.32e-07  1.85e-06    | grid-L5C5-d4-k2        1.81e-07  1.45e-06
  grid-L5C5-d64-k1       4.83e-06  3.86e-05    | grid-L5C5-d64-k2       1.86e-06  1.49e-05
  grid-L5C5-d100-k1      6.58e-06  5.27e-05    | grid-L5C5-d100-k2      4.29e-07  3.43e-06
  grid-L5C5-d256-k1      2.08e-06  1.66e-05    | grid-L5C5-d256-k2      2.03e-06  1.63e-05
  grid-L3C2-d4-k1        1.20e-07  9.58e-07    | grid-L3C2-d4-k2        1.99e-07  1.59e-06
  grid-L3C2-d64-k1       1.23e-04  9.80e-04    | grid-L3C2-d64-k2       5.69e-06  4.55e-05
  grid-L3C2-d100-k1      9.76e-05  7.81e-04    | grid-L3C2-d100-k2      6.59e-05  5.28e-04
  grid-L3C2-d256-k1      6.03e-05  4.82e-04    | grid-L3C2-d256-k2      5.56e-06  4.45e-05
  grid-L80C2-d4-k1       2.10e-07  1.68e-06    | grid-L80C2-d4-k2       2.20e-07  1.76e-06
  grid-L80C2-d64-k1      7.37e-07  5.90e-06    | grid-L80C2-d64-k2      6.63e-07  5.31e-06
  grid-L80C2-d100-k1     1.15e-06  9.22e-06    | grid-L80C2-d100-k2     9.89e-07  7.91e-06
  grid-L80C2-d256-k1     refused (LDS limit)   | grid-L80C2-d256-k2     refused (LDS limit)
  collide-n7             1.58e-06  1.26e-05    | sparse-n300            1.19e-05  9.55e-05
  steps8-n300            2.23e-06  1.79e-05    | large-scores           1.39e-06  1.11e-05
  trainer                2.34e-06  1.87e-05
  (trainer: n = 300, d = 64, 2 walks per node, 2 epochs of 3 batches; weights of magnitude <= 4.3)

The literal PyG form of the negative term, log(1 - sigma(x) + EPS), is kept here as `literal=True` for the CPU test that shows why
the native step does not follow it: in fp32 it saturates at -log(EPS) once x > ~17."""
import functools

import numpy as np
import torch

from edge_sampling_oracle import words

EPS = 1e-15
TOL_FACTOR = 8
STREAM_POS, STREAM_NEG, STREAM_ORDER = 16, 17, 18
U64 = np.uint64


# ---- graphs ----------------------------------------------------------------------------------------------------------------------
def csr(edge_index, n):
  """(rowptr [n + 1], col [E]) int64 numpy: a node's out-neighbours with multiplicity, ascending."""
  ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
  key = np.sort(ei[0] * n + ei[1], kind='stable')
  src = key // n
  rowptr = np.zeros(n + 1, dtype=np.int64)
  np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
  return rowptr, key - src * n


def ring(n=5):
  i = np.arange(n)
  return np.stack([np.concatenate([i, i]), np.concatenate([(i + 1) % n, (i - 1) % n])]), n


def odd_graph():
  """9 nodes: 7 isolated, 5 a sink (in-edges only), a self-loop at 2, the edge 0 -> 1 twice."""
  e = [(0, 1), (0, 1), (0, 3), (1, 0), (1, 2), (2, 2), (2, 4), (3, 5), (4, 5), (4, 0), (6, 8), (8, 6), (8, 3), (3, 0)]
  return np.array(e, dtype=np.int64).T, 9


def star(leaves=70001):
  """Hub 0 with out-degree `leaves`; every leaf points back."""
  l = np.arange(1, leaves + 1)
  z = np.zeros(leaves, dtype=np.int64)
  return np.stack([np.concatenate([z, l]), np.concatenate([l, z])]), leaves + 1


def random_graph(n, deg, seed):
  g = np.random.default_rng(seed)
  src = np.repeat(np.arange(n), deg)
  dst = g.integers(0, n, size=n * deg)
  return np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]), n


def two_communities(n=256, deg=8, extra=0.2, seed=0):
  """The 'use' graph: halves as communities, `deg` random intra-community neighbours per node, one more uniformly random edge with
  probability `extra` per node, symmetrised."""
  g = np.random.default_rng(seed)
  half = n // 2
  src = np.repeat(np.arange(n), deg)
  dst = g.integers(0, half, size=n * deg) + (src >= half) * half
  more = np.nonzero(g.random(n) < extra)[0]
  src = np.concatenate([src, more])
  dst = np.concatenate([dst, g.integers(0, n, size=more.size)])
  return np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]), n


def community_cosines(z, n):
  """(mean cosine between rows of one community, mean cosine between rows of different communities), self pairs excluded."""
  z = torch.as_tensor(z).detach().cpu().double()
  z = z / z.norm(dim=1, keepdim=True)
  c = z @ z.T
  same = (torch.arange(n) < n // 2)
  same = same[:, None] == same[None, :]
  off = ~torch.eye(n, dtype=torch.bool)
  return float(c[same & off].mean()), float(c[~same].mean())


# ---- walks -----------------------------------------------------------------------------------------------------------------------
def walk_words(R, L, seed, stream, call, first_walk=0):
  """[R, L] uint64: word(w, t) = word (t & 3) of block w ceil(L / 4) + (t >> 2), w = first_walk + r (64-bit block numbers)."""
  nb = (L + 3) // 4
  first_block = (int(first_walk) * nb) % 2 ** 64
  return words(seed, stream, call, first_block, R * nb * 4).reshape(R, nb * 4)[:, :L]


def random_walks(rowptr, col, starts, L, seed, stream, call, first_walk=0, W=None):
  """W: the words walk_words(len(starts), L, ...) when the caller has them already."""
  starts = np.asarray(starts, dtype=np.int64)
  R = starts.size
  out = np.empty((R, L + 1), dtype=np.int64)
  out[:, 0] = cur = starts.copy()
  if R == 0:
    return out
  if W is None:
    W = walk_words(R, L, seed, stream, call, first_walk)
  for t in range(L):
    b = rowptr[cur]
    deg = rowptr[cur + 1] - b
    idx = ((W[:, t] * deg.astype(U64)) >> U64(32)).astype(np.int64)
    nxt = col[np.minimum(b + idx, max(col.size - 1, 0))] if col.size else cur
    cur = np.where(deg > 0, nxt, cur)
    out[:, t + 1] = cur
  return out


def negative_walks(n, starts, L, seed, stream, call, first_walk=0, W=None):
  starts = np.asarray(starts, dtype=np.int64)
  out = np.empty((starts.size, L + 1), dtype=np.int64)
  out[:, 0] = starts
  if starts.size:
    if W is None:
      W = walk_words(starts.size, L, seed, stream, call, first_walk)
    out[:, 1:] = ((W * U64(n)) >> U64(32)).astype(np.int64)
  return out


def random_permutation(n, seed, stream, call):
  key = (words(seed, stream, call, 0, n) << U64(32)) | np.arange(n, dtype=U64)
  return np.argsort(key, kind='stable').astype(np.int64)


def window_pairs(L, C):
  """The position pairs (a, b) of one walk: 0 <= a < J = L + 2 - C, a < b <= a + C - 1."""
  return [(a, b) for a in range(L + 2 - C) for b in range(a + 1, a + C)]


# ---- the step --------------------------------------------------------------------------------------------------------------------
def pair_scores(emb, rw, C):
  """x over PyG's windows: cat([rw[:, j:j + C] for j in range(J)]), first column against the others."""
  L = rw.shape[1] - 1
  win = torch.cat([rw[:, j:j + C] for j in range(L + 2 - C)], dim=0)
  start, rest = win[:, 0], win[:, 1:].contiguous()
  h_start = emb(start).view(win.shape[0], 1, -1)
  h_rest = emb(rest.view(-1)).view(win.shape[0], C - 1, -1)
  return (h_start * h_rest).sum(dim=-1).view(-1)


def loss_of(emb, pos_rw, neg_rw, C, literal=False):
  xp, xn = pair_scores(emb, pos_rw, C), pair_scores(emb, neg_rw, C)
  pos = -torch.log(torch.sigmoid(xp) + EPS).mean()
  if literal:
    neg = -torch.log(1 - torch.sigmoid(xn) + EPS).mean()
  else:
    neg = -torch.log(torch.sigmoid(-xn) + EPS).mean()
  return pos + neg


class Model(object):
  """Embedding + SparseAdam in `dtype`; weight: the initial [n, d] rows (any dtype)."""

  def __init__(self, weight, dtype, lr=0.01, betas=(0.9, 0.999), eps=1e-8, literal=False):
    n, d = weight.shape
    self.emb = torch.nn.Embedding(n, d, sparse=True).to(dtype)
    with torch.no_grad():
      self.emb.weight.copy_(weight.to(dtype))
    self.opt = torch.optim.SparseAdam(list(self.emb.parameters()), lr=lr, betas=betas, eps=eps)
    self.literal = literal

  def step(self, pos_rw, neg_rw, C):
    self.opt.zero_grad()
    loss = loss_of(self.emb, torch.as_tensor(pos_rw), torch.as_tensor(neg_rw), C, self.literal)
    loss.backward()
    self.opt.step()
    return float(loss.detach().double())

  def state(self):
    st = self.opt.state[self.emb.weight]
    z = torch.zeros_like(self.emb.weight)
    return (self.emb.weight.detach().double(), st.get('exp_avg', z).detach().double(), st.get('exp_avg_sq', z).detach().double())


def initial_weights(n, d, seed):
  return torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


class Result(object):
  """fp64 state and losses of a case, and its d32 / tolerance."""

  def __init__(self, r64, r32):
    self.weight, self.exp_avg, self.exp_avg_sq, self.losses = r64
    self.d32 = max(max(float((a - b).abs().max()) for a, b in zip(r64[:3], r32[:3])),
                   max(abs(a - b) for a, b in zip(r64[3], r32[3])))
    self.tol = TOL_FACTOR * self.d32


def _run_steps(weight, batches, C, dtype, lr):
  m = Model(weight, dtype, lr=lr)
  losses = [m.step(p, q, C) for p, q in batches]
  return m.state() + (losses,)


# ---- step cases of the GPU test: name -> dict(n, d, L, C, walks, k (negatives per positive), steps, scale, seed) ------------------
GRID_LC = ((20, 16), (5, 5), (3, 2), (80, 2))
GRID_D = (4, 64, 100, 256)
GRID_K = (1, 2)
LDS_FLOATS = 16384
CASES = {}
for _L, _C in GRID_LC:
  for _d in GRID_D:
    for _k in GRID_K:
      CASES['grid-L%dC%d-d%d-k%d' % (_L, _C, _d, _k)] = dict(n=50, d=_d, L=_L, C=_C, walks=10, k=_k, steps=2, scale=1.0, seed=3)
CASES['collide-n7'] = dict(n=7, d=64, L=20, C=16, walks=130, k=1, steps=8, scale=1.0, seed=4)       # every row touched hundreds of times
CASES['sparse-n300'] = dict(n=300, d=64, L=3, C=2, walks=5, k=1, steps=2, scale=1.0, seed=5)        # most rows untouched
CASES['steps8-n300'] = dict(n=300, d=64, L=20, C=16, walks=128, k=1, steps=8, scale=1.0, seed=6)    # bias correction, carried state
CASES['large-scores'] = dict(n=50, d=64, L=20, C=16, walks=40, k=1, steps=2, scale=3.0, seed=7)     # scores beyond +-50


def case_refused(name):
  """True for the grid shapes the native step refuses: (L + 1) d + J (C - 1) > 16384 floats."""
  c = CASES[name]
  return (c['L'] + 1) * c['d'] + (c['L'] + 2 - c['C']) * (c['C'] - 1) > LDS_FLOATS


def case_inputs(name):
  """(weight [n, d] float32, [(pos_rw, neg_rw)] per step as int64 tensors): walks of the oracle on a random graph, a fresh draw of
  start nodes per step."""
  c = CASES[name]
  ei, n = random_graph(c['n'], 3, c['seed'])
  rowptr, col = csr(ei, n)
  g = np.random.default_rng(c['seed'])
  batches = []
  for s in range(c['steps']):
    starts = g.integers(0, n, size=c['walks'])
    pos = random_walks(rowptr, col, starts, c['L'], c['seed'], STREAM_POS, s)
    neg = negative_walks(n, np.tile(starts, c['k']), c['L'], c['seed'], STREAM_NEG, s)
    batches.append((torch.from_numpy(pos), torch.from_numpy(neg)))
  return initial_weights(n, c['d'], c['seed']) * c['scale'], batches


@functools.lru_cache(maxsize=None)
def case_result(name, lr=0.01):
  w, batches = case_inputs(name)
  C = CASES[name]['C']
  return Result(_run_steps(w, batches, C, torch.float64, lr), _run_steps(w, batches, C, torch.float32, lr))


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def train(edge_index, n, d, L, C, walks_per_node, k, lr, seed, epochs, batch_size, dtype=torch.float64):
  """The header's epoch / batch schedule on the oracle's walks and step.  Returns (weight, exp_avg, exp_avg_sq, per-step losses,
  per-epoch mean losses)."""
  rowptr, col = csr(edge_index, n)
  m = Model(initial_weights(n, d, seed), dtype, lr=lr)
  B, steps, epoch_means = batch_size, [], []
  for e in range(epochs):
    perm = random_permutation(n, seed, STREAM_ORDER, e)
    mine = []
    for b in range((n + B - 1) // B):
      batch = perm[b * B:(b + 1) * B]
      pos = random_walks(rowptr, col, np.tile(batch, walks_per_node), L, seed, STREAM_POS, e, b * B * walks_per_node)
      neg = negative_walks(n, np.tile(batch, walks_per_node * k), L, seed, STREAM_NEG, e, b * B * walks_per_node * k)
      mine.append(m.step(pos, neg, C))
    steps += mine
    epoch_means.append(float(np.mean(mine)))
  return m.state() + (steps, epoch_means)


TRAINER = dict(n=300, d=64, L=20, C=16, walks_per_node=2, k=1, lr=0.01, epochs=2, batch_size=128, graph_seed=8)
USE = dict(n=256, d=16, L=20, C=8, walks_per_node=4, k=1, lr=0.05, epochs=30, batch_size=128)


def trainer_graph():
  return random_graph(TRAINER['n'], 3, TRAINER['graph_seed'])


@functools.lru_cache(maxsize=None)
def trainer_result(seed=0):
  t = TRAINER
  ei, n = trainer_graph()
  run = lambda dt: train(ei, n, t['d'], t['L'], t['C'], t['walks_per_node'], t['k'], t['lr'], seed, t['epochs'], t['batch_size'], dt)
  r64, r32 = run(torch.float64), run(torch.float32)
  res = Result(r64[:4], r32[:4])
  res.epoch_means = r64[4]
  return res


@functools.lru_cache(maxsize=None)
def use_result(seed=0):
  u = USE
  ei, n = two_communities(u['n'])
  return train(ei, n, u['d'], u['L'], u['C'], u['walks_per_node'], u['k'], u['lr'], seed, u['epochs'], u['batch_size'])[0]


def print_tolerances():
  for name in CASES:
    if not case_refused(name):
      r = case_result(name)
      print('%-24s d32 %.2e  tol %.2e' % (name, r.d32, r.tol))
  r = trainer_result()
  print('%-24s d32 %.2e  tol %.2e' % ('trainer', r.d32, r.tol))


if __name__ == '__main__':
  print_tolerances()
