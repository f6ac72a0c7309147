"""CPU oracle of the hyperbolic positional encodings (csrc/hyperbolic.hip, gnpde_amd.hyperbolic_embeddings): restatements of what
include/gnpde.h defines, not of any third-party library.

  walks, negative walks, epoch order   deepwalk_oracle's Philox restatement on the stream ids 19, 20, 21
  step                                  torch: dist = 2 log(sqrt(r) + sqrt(1 + r)) on gathered rows, the per-pair loss terms SUMMED,
                                        autograd for g_u, a bincount of the pair ends for c_u, the rescaled update and the projection;
                                        float64 is the yardstick.  The closed-form gradient of the header is NOT used by the step:
                                        test_hyperbolic_cpu.py compares it with autograd.
  trainer                               composed of these, batch by batch as the header's "Epoch e, batch b" says

Tolerance of a step / trainer case (never derived from the code under test): the SAME oracle run in float32 next to the float64 run,
d32 = max |fp32 - fp64| over the embedding and the losses; the absolute tolerance of the case is 8 * d32 (TOL_FACTOR), the convention
of deepwalk_oracle.py.  The factor covers the device's different summation order (inside the walk first, then across walks) and logf /
expf at 2 ulp.  d32 is recomputed where the tests run (case_result / trainer_result).  The figures below are one recorded run of
print_tolerances() (torch CPU kernels) and, where a device run has been recorded, the native step's largest deviation from the
float64 oracle on an MI355X (`dev`):

  case                   d32       8 * d32   dev      | case                   d32       8 * d32   dev
  grid-L3C2-d2-k1        8.49e-08  6.80e-07  1.14e-07 | grid-L20C16-d4-k2      7.00e-08  5.60e-07  5.10e-08
  grid-L3C2-d2-k2        1.92e-07  1.53e-06  8.74e-08 | grid-L20C16-d16-k1     4.29e-08  3.43e-07  7.63e-08
  grid-L3C2-d4-k1        1.04e-07  8.31e-07  1.04e-07 | grid-L20C16-d16-k2     3.45e-08  2.76e-07  8.83e-08
  grid-L3C2-d4-k2        1.25e-07  1.00e-06  6.61e-08 | grid-L20C16-d100-k1    5.24e-08  4.19e-07  5.24e-08
  grid-L3C2-d16-k1       5.88e-08  4.70e-07  5.88e-08 | grid-L20C16-d100-k2    7.11e-08  5.69e-07  7.10e-08
  grid-L3C2-d16-k2       1.73e-07  1.39e-06  5.41e-08 | grid-L80C2-d2-k1       1.05e-07  8.43e-07  6.10e-08
  grid-L3C2-d100-k1      8.10e-08  6.48e-07  3.82e-08 | grid-L80C2-d2-k2       6.97e-08  5.57e-07  4.95e-08
  grid-L3C2-d100-k2      2.34e-07  1.87e-06  3.63e-08 | grid-L80C2-d4-k1       1.67e-07  1.34e-06  1.06e-07
  grid-L5C5-d2-k1        6.15e-08  4.92e-07  1.32e-07 | grid-L80C2-d4-k2       7.70e-08  6.16e-07  7.70e-08
  grid-L5C5-d2-k2        1.41e-07  1.13e-06  1.00e-07 | grid-L80C2-d16-k1      2.80e-08  2.24e-07  3.16e-08
  grid-L5C5-d4-k1        6.98e-08  5.58e-07  6.13e-08 | grid-L80C2-d16-k2      1.45e-07  1.16e-06  3.09e-08
  grid-L5C5-d4-k2        9.30e-08  7.44e-07  6.32e-08 | grid-L80C2-d100-k1     1.18e-07  9.42e-07  4.95e-08
  grid-L5C5-d16-k1       8.99e-08  7.19e-07  8.99e-08 | grid-L80C2-d100-k2     1.08e-07  8.65e-07  1.89e-08
  grid-L5C5-d16-k2       5.50e-08  4.40e-07  5.50e-08 | boundary               1.25e-06  1.00e-05  2.96e-07
  grid-L5C5-d100-k1      1.01e-07  8.07e-07  1.01e-07 | collide-n7             5.55e-07  4.44e-06  1.68e-07
  grid-L5C5-d100-k2      1.13e-07  9.03e-07  3.32e-08 | sparse-n300            7.80e-08  6.24e-07  4.12e-08
  grid-L20C16-d2-k1      7.23e-08  5.79e-07  7.23e-08 | steps8-n300            1.87e-07  1.50e-06  8.68e-08
  grid-L20C16-d2-k2      4.96e-08  3.97e-07  8.11e-08 | twins                  7.56e-08  6.05e-07  7.56e-08
  grid-L20C16-d4-k1      1.88e-07  1.50e-06  6.87e-08 | trainer                1.24e-07  9.94e-07  8.50e-08
  (trainer: n = 300, d = 16, L = 20, C = 2, 2 walks per node, 2 epochs of 3 batches; dev: the larger of the embedding and loss
  deviations.  The functional condition on the tree: MAP 0.085 at initialisation, 0.562 float64 oracle, 0.562 native.)
"""
import functools

import numpy as np
import torch

import deepwalk_oracle as DO

EPS = 1e-15
TOL_FACTOR = 8
STREAM_POS, STREAM_NEG, STREAM_ORDER = 19, 20, 21
BALL_EDGE = 1 - 1e-5
INIT_RANGE = 1e-3


# ---- the definition --------------------------------------------------------------------------------------------------------------
def pair_key(eu, ev):
  """(r, q, alpha, beta) of rows eu, ev [m, d]."""
  alpha, beta = 1 - (eu * eu).sum(-1), 1 - (ev * ev).sum(-1)
  q = ((eu - ev) ** 2).sum(-1)
  return q / (alpha * beta), q, alpha, beta


def distance(eu, ev):
  """dist = arccosh(1 + 2 r) as 2 log(sqrt(r) + sqrt(1 + r)); a pair with r == 0 has dist = 0 and no gradient."""
  r = pair_key(eu, ev)[0]
  apart = r > 0
  rs = torch.where(apart, r, torch.ones_like(r))
  return torch.where(apart, 2 * torch.log(torch.sqrt(rs) + torch.sqrt(1 + rs)), torch.zeros_like(r))


def distance_gradient(eu, ev):
  """The header's closed form of d dist / d e_u (rows [m, d]); zero where r == 0."""
  r, q, alpha, beta = pair_key(eu, ev)
  apart = r > 0
  rs = torch.where(apart, r, torch.ones_like(r))
  k = torch.where(apart, 1 / torch.sqrt(rs * (1 + rs)) * 2 / (alpha * beta), torch.zeros_like(r))
  return k[:, None] * ((eu - ev) + (q / alpha)[:, None] * eu)


def pair_ends(rw, C):
  """(u, v) node vectors of all window pairs of the walks rw [R, L + 1]."""
  L = rw.shape[1] - 1
  pairs = DO.window_pairs(L, C)
  a, b = [p[0] for p in pairs], [p[1] for p in pairs]
  return rw[:, a].reshape(-1), rw[:, b].reshape(-1)


def loss_terms(e, rw, C, radius, temperature, positive):
  u, v = pair_ends(rw, C)
  x = (radius - distance(e[u], e[v])) / temperature
  return -torch.log(torch.sigmoid(x if positive else -x) + EPS)


class Step(object):
  """One step on emb [n, d] (its dtype is the precision of the run): .emb the new rows, .loss, .move the Euclidean length of every
  row's move BEFORE the projection, .alpha = 1 - |e|^2 before the step, .counts = c_u, .grad = g_u."""

  def __init__(self, emb, pos_rw, neg_rw, C, lr=1.0, radius=2.0, temperature=1.0):
    pos_rw, neg_rw = torch.as_tensor(pos_rw), torch.as_tensor(neg_rw)
    e = emb.detach().clone().requires_grad_(True)
    tp = loss_terms(e, pos_rw, C, radius, temperature, True)
    tn = loss_terms(e, neg_rw, C, radius, temperature, False)
    (tp.sum() + tn.sum()).backward()                       # every pair's OWN loss term: no 1 / count factor
    self.loss = float((tp.mean() + tn.mean()).detach().double())
    g, e = e.grad, e.detach()
    ends = torch.cat(pair_ends(pos_rw, C) + pair_ends(neg_rw, C))
    c = torch.bincount(ends, minlength=e.shape[0])
    touched = c > 0
    alpha = 1 - (e * e).sum(1)
    y = e - (lr * (alpha * alpha / 4) / c.clamp(min=1).to(e.dtype))[:, None] * g
    norm = y.norm(dim=1)
    inside = norm < BALL_EDGE
    proj = torch.where(inside[:, None], y, y * (BALL_EDGE / norm.clamp(min=1e-30))[:, None])
    self.emb = torch.where(touched[:, None], proj, e)
    self.move, self.alpha, self.counts, self.grad, self.touched = (y - e).norm(dim=1), alpha, c, g, touched


def initial_embedding(n, d, seed):
  """The trainer's initialisation: uniform in [-1e-3, 1e-3] from torch.Generator().manual_seed(seed), float32."""
  return (2.0 * torch.rand(n, d, generator=torch.Generator().manual_seed(seed)) - 1.0) * INIT_RANGE


def spread_rows(n, d, seed, lo, hi):
  """[n, d] float32 rows with random directions and norms uniform in [lo, hi]."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, d, generator=g, dtype=torch.float64)
  x = x / x.norm(dim=1, keepdim=True)
  w = (x * (lo + (hi - lo) * torch.rand(n, 1, generator=g, dtype=torch.float64))).float()
  assert float(w.double().norm(dim=1).max()) < 1
  return w


class Result(object):
  """fp64 embedding and losses of a case, and its d32 / tolerance."""

  def __init__(self, r64, r32):
    self.emb, self.losses = r64
    self.d32 = max(float((r64[0] - r32[0].double()).abs().max()), max(abs(a - b) for a, b in zip(r64[1], r32[1])))
    self.tol = TOL_FACTOR * self.d32


def _run_steps(weight, batches, C, dtype, lr, radius=2.0, temperature=1.0):
  e, losses = weight.to(dtype), []
  for p, q in batches:
    s = Step(e, p, q, C, lr, radius, temperature)
    e = s.emb
    losses.append(s.loss)
  return e.double(), losses


# ---- step cases of the GPU test: name -> dict(n, d, L, C, walks, k (negatives per positive), steps, lo, hi (row norms), seed) ------
GRID_LC = ((3, 2), (5, 5), (20, 16), (80, 2))
GRID_D = (2, 4, 16, 100)
GRID_K = (1, 2)
CASES = {}
for _L, _C in GRID_LC:
  for _d in GRID_D:
    for _k in GRID_K:
      CASES['grid-L%dC%d-d%d-k%d' % (_L, _C, _d, _k)] = dict(n=50, d=_d, L=_L, C=_C, walks=10, k=_k, steps=2, lo=0.05, hi=0.9, seed=3)
CASES['collide-n7'] = dict(n=7, d=16, L=20, C=16, walks=130, k=1, steps=2, lo=0.05, hi=0.9, seed=4)       # every window full of repeats
CASES['boundary'] = dict(n=50, d=16, L=5, C=3, walks=40, k=1, steps=2, lo=0.9, hi=0.999, seed=5)           # alpha down to 2e-3
CASES['twins'] = dict(n=6, d=4, L=5, C=3, walks=24, k=1, steps=2, lo=0.05, hi=0.9, seed=6, twins=True)     # rows 0 and 1 identical
CASES['sparse-n300'] = dict(n=300, d=16, L=3, C=2, walks=5, k=1, steps=1, lo=0.05, hi=0.9, seed=8)         # most rows untouched
CASES['steps8-n300'] = dict(n=300, d=16, L=20, C=16, walks=128, k=1, steps=8, lo=0.05, hi=0.9, seed=7)     # carried state


def case_inputs(name):
  """(weight [n, d] float32, [(pos_rw, neg_rw)] per step as int64 tensors): walks of the oracle on a random graph, a fresh draw of
  start nodes per step."""
  c = CASES[name]
  ei, n = DO.random_graph(c['n'], 3, c['seed'])
  rowptr, col = DO.csr(ei, n)
  g = np.random.default_rng(c['seed'])
  batches = []
  for s in range(c['steps']):
    starts = g.integers(0, n, size=c['walks'])
    pos = DO.random_walks(rowptr, col, starts, c['L'], c['seed'], STREAM_POS, s)
    neg = DO.negative_walks(n, np.tile(starts, c['k']), c['L'], c['seed'], STREAM_NEG, s)
    batches.append((torch.from_numpy(pos), torch.from_numpy(neg)))
  w = spread_rows(n, c['d'], c['seed'], c['lo'], c['hi'])
  if c.get('twins'):
    w[1] = w[0]
  return w, batches


@functools.lru_cache(maxsize=None)
def case_result(name, lr=1.0):
  w, batches = case_inputs(name)
  C = CASES[name]['C']
  return Result(_run_steps(w, batches, C, torch.float64, lr), _run_steps(w, batches, C, torch.float32, lr))


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def train(edge_index, n, d, L, C, walks_per_node, k, lr, seed, epochs, batch_size, dtype=torch.float64, radius=2.0, temperature=1.0):
  """The header's epoch / batch schedule on the oracle's walks and step.  Returns (embedding as float64, per-step losses, per-epoch
  mean losses)."""
  rowptr, col = DO.csr(edge_index, n)
  e = initial_embedding(n, d, seed).to(dtype)
  B, steps, epoch_means = batch_size, [], []
  for ep in range(epochs):
    perm = DO.random_permutation(n, seed, STREAM_ORDER, ep)
    mine = []
    for b in range((n + B - 1) // B):
      batch = perm[b * B:(b + 1) * B]
      pos = DO.random_walks(rowptr, col, np.tile(batch, walks_per_node), L, seed, STREAM_POS, ep, b * B * walks_per_node)
      neg = DO.negative_walks(n, np.tile(batch, walks_per_node * k), L, seed, STREAM_NEG, ep, b * B * walks_per_node * k)
      s = Step(e, torch.from_numpy(pos), torch.from_numpy(neg), C, lr, radius, temperature)
      e = s.emb
      mine.append(s.loss)
    steps += mine
    epoch_means.append(float(np.mean(mine)))
  return e.double(), steps, epoch_means


TRAINER = dict(n=300, d=16, L=20, C=2, walks_per_node=2, k=1, lr=1.0, epochs=2, batch_size=128, graph_seed=8)
# the functional condition: a tree of branching 3 and depth 4, trained as the prototype of the issue was
USE = dict(branching=3, depth=4, d=2, L=5, C=2, walks_per_node=4, k=1, lr=1.0, epochs=40, batch_size=32)
USE_MAP_FACTOR = 4            # the float64 oracle's MAP after training >= 4 x its MAP at initialisation
USE_NATIVE_SHARE = 0.75       # the native trainer's MAP >= 0.75 x the float64 oracle's


def trainer_graph():
  return DO.random_graph(TRAINER['n'], 3, TRAINER['graph_seed'])


@functools.lru_cache(maxsize=None)
def trainer_result(seed=0):
  t = TRAINER
  ei, n = trainer_graph()
  run = lambda dt: train(ei, n, t['d'], t['L'], t['C'], t['walks_per_node'], t['k'], t['lr'], seed, t['epochs'], t['batch_size'], dt)
  r64, r32 = run(torch.float64), run(torch.float32)
  res = Result(r64[:2], r32[:2])
  res.epoch_means = r64[2]
  return res


def tree(branching=3, depth=4):
  """(edge_index [2, E] int64 numpy, both directions, n): the complete tree, node 0 the root, children of i at branching i + 1 ..."""
  n = (branching ** (depth + 1) - 1) // (branching - 1)
  child = np.arange(1, n)
  parent = (child - 1) // branching
  return np.stack([np.concatenate([parent, child]), np.concatenate([child, parent])]), n


def neighbour_map(emb, edge_index, n):
  """Mean average precision of the true neighbours under the learned distance: every node ranks all others by r (monotone in dist),
  ties by index; AP = the mean over its neighbours of (neighbours among the first k) / k at the neighbour's rank k."""
  e = torch.as_tensor(emb).detach().cpu().double()
  alpha = 1 - (e * e).sum(1)
  r = torch.cdist(e, e) ** 2 / (alpha[:, None] * alpha[None, :])
  adj = np.zeros((n, n), dtype=bool)
  adj[edge_index[0], edge_index[1]] = True
  r = r.numpy()
  aps = []
  for u in range(n):
    order = np.argsort(np.where(np.arange(n) == u, np.inf, r[u]), kind='stable')[:n - 1]
    hit = adj[u, order]
    if hit.any():
      ranks = np.nonzero(hit)[0] + 1
      aps.append(float(np.mean(np.arange(1, ranks.size + 1) / ranks)))
  return float(np.mean(aps))


@functools.lru_cache(maxsize=None)
def use_result(seed=0):
  """(MAP at initialisation, MAP of the float64 oracle trainer) on the tree."""
  u = USE
  ei, n = tree(u['branching'], u['depth'])
  before = neighbour_map(initial_embedding(n, u['d'], seed), ei, n)
  e = train(ei, n, u['d'], u['L'], u['C'], u['walks_per_node'], u['k'], u['lr'], seed, u['epochs'], u['batch_size'])[0]
  return before, neighbour_map(e, ei, n)


def print_tolerances():
  for name in CASES:
    r = case_result(name)
    print('%-24s d32 %.2e  tol %.2e' % (name, r.d32, r.tol))
  r = trainer_result()
  print('%-24s d32 %.2e  tol %.2e' % ('trainer', r.d32, r.tol))
  print('use: MAP %.3f at initialisation, %.3f after training (float64 oracle)' % use_result())


if __name__ == '__main__':
  print_tolerances()
