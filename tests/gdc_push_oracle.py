"""Float64 yardstick of the approximate forward push (shared by test_gdc_push_*.py): the dense personalised PageRank matrix
Pi = alpha (I - (1 - alpha) D^-1 A)^-1 from numpy, two float64 pushes of the test's own (LIFO and synchronous), the three relations
every admissible push satisfies, and the fixed-point slack of the native kernel.

Undirected graph with unit self loops: deg(v) pi_v(u) = deg(u) pi_u(v), and the push invariant pi_s = p_s + sum_v (r_s(v) / alpha) pi_v
give, for every admissible order of pushes,
    0 <= Pi[s, u] - p_s(u) < eps deg(u),      sum_u p_s(u) + sum_v r_s(v) / alpha = 1,      r_s(v) < alpha eps deg(v).

The native kernel computes p and r as integers with quantum q = 2^-60 and converts an output value to fp32 once:
  * one rounding per returned value: N = 1, gamma = u / (1 - u), u = 2^-24;
  * a push at u rounds DOWN twice (floor((1 - alpha) res), then the division by deg(u)) and so loses less than deg(u) + 2 quanta
    of residual mass; it never creates mass.  Every push but a source's first moves at least (alpha eps - q) deg(u) into p and
    sum p <= 1, so the pushed degrees sum to at most 1 / (alpha eps - q) + deg(s) and the mass lost by one source stays below
        LOST = 3 (1 / (alpha eps - q) + deg_max) q                                   (`lost_mass`);
  * lost mass only lowers p:  pi_s = p_s + sum_v (r_s(v) / alpha) pi_v + (lost terms), each lost quantum l at v adding (l / alpha) pi_v(u)
    <= l / alpha.  Hence, with p and r the returned fp32 values,
        -gamma p <= Pi - p < eps deg(u) + gamma Pi + LOST / alpha,       r < alpha eps deg(v) (1 + gamma),
        | sum p + sum r / alpha - 1 | <= gamma + (LOST + q) / alpha        (alpha itself is rounded down to a quantum).
ORACLE_TOL covers the float64 inverse (condition number <= 2 / alpha - 1 <= 39 for alpha >= 0.05: errors near 1e-14)."""
import functools

import numpy as np

U = 2.0 ** -24
GAMMA = U / (1.0 - U)          # N = 1: the single conversion of a fixed-point value to fp32
QUANTUM = 2.0 ** -60
ORACLE_TOL = 1e-12
OPEN_CAP = 0.02                # share of the oracle's kept entries the bound may leave open in the pipeline test

PIPELINE_SHAPE, PIPELINE_THRESHOLD = 'fine600', 0.01       # the wrapper's pipeline test: 12 of 3 788 kept entries stay open

# the issue's table: name -> n, random undirected edges, leaves of a hub at node 0, alpha, push eps
SHAPES = {
  'random600': dict(n=600, edges=1500, hub=0, alpha=0.15, eps=1e-4, seed=21),
  'hub600': dict(n=600, edges=1200, hub=530, alpha=0.15, eps=1e-4, seed=22),
  'hub600_a05': dict(n=600, edges=1200, hub=530, alpha=0.05, eps=1e-4, seed=22),
  'local300': dict(n=300, edges=600, hub=0, alpha=0.15, eps=1e-3, seed=23),
  'fine600': dict(n=600, edges=1500, hub=0, alpha=0.05, eps=1e-5, seed=24),
}


def make_graph(n, edges, hub, seed):
  """[2, E] int64, both directions of `edges` random pairs (no loops) and of the hub's leaves, duplicates removed."""
  r = np.random.RandomState(seed)
  a, b = r.randint(0, n, edges), r.randint(0, n, edges)
  a, b = a[a != b], b[a != b]
  if hub:
    leaves = 1 + r.permutation(n - 1)[:hub]
    a, b = np.concatenate([a, np.zeros(hub, dtype=np.int64)]), np.concatenate([b, leaves])
  key = np.unique(np.concatenate([a * n + b, b * n + a]))
  return np.stack([key // n, key % n]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def shape(name):
  """(edge_index without loops, dense 0/1 A with unit loops, deg, Pi) of a shape of the table."""
  c = SHAPES[name]
  ei = make_graph(c['n'], c['edges'], c['hub'], c['seed'])
  A = np.zeros((c['n'], c['n']))
  A[ei[0], ei[1]] = 1.0
  A[np.arange(c['n']), np.arange(c['n'])] = 1.0
  deg = A.sum(1)
  Pi = c['alpha'] * np.linalg.inv(np.eye(c['n']) - (1.0 - c['alpha']) * A / deg[:, None])
  return ei, A, deg, Pi


def rows_of(A):
  return [np.flatnonzero(A[u]) for u in range(A.shape[0])]


def push_lifo(rows, deg, s, alpha, eps):
  """torch_geometric's __calc_ppr__ order: a LIFO work list (float64), one source."""
  n = len(rows)
  p, r = np.zeros(n), np.zeros(n)
  thr = alpha * eps * deg
  r[s] = alpha
  stack, queued, first = [s], np.zeros(n, dtype=bool), True
  queued[s] = True
  while stack:
    u = stack.pop()
    queued[u] = False
    res = r[u]
    if not first and res < thr[u]:
      continue
    first = False
    p[u] += res
    r[u] = 0.0
    nb = rows[u]
    r[nb] += (1.0 - alpha) * res / deg[u]
    new = nb[(r[nb] >= thr[nb]) & ~queued[nb]]
    queued[new] = True
    stack.extend(new.tolist())
  return p, r


def push_sync(A, deg, alpha, eps, sources=None):
  """Synchronous rounds (the native kernel's schedule) in float64 for all sources at once: row s of (P, R) is the push of source
  s.  A round of a source pushes every node whose residual is >= alpha eps deg at its start (round 0: the source alone)."""
  n = A.shape[0]
  sources = np.arange(n) if sources is None else np.asarray(sources)
  W = (1.0 - alpha) * A / deg[:, None]
  P = np.zeros((sources.shape[0], n))
  R = np.zeros((sources.shape[0], n))
  R[np.arange(sources.shape[0]), sources] = alpha
  active = R > 0
  while active.any():
    X = np.where(active, R, 0.0)
    P += X
    R = np.where(active, 0.0, R) + X @ W
    active = R >= alpha * eps * deg[None, :]
  return P, R


@functools.lru_cache(maxsize=None)
def push_all(name):
  """(P [n, n], R [n, n]) float64 of the synchronous push: row s = source s."""
  c = SHAPES[name]
  _, A, deg, _ = shape(name)
  return push_sync(A, deg, c['alpha'], c['eps'])


def lost_mass(alpha, eps, deg_max):
  return 3.0 * (1.0 / (alpha * eps - QUANTUM) + deg_max) * QUANTUM


def check_relations(P, R, Pi, deg, alpha, eps, gamma=0.0, lost=0.0, label=''):
  """The three relations with the slack of the producer (gamma = lost = 0: a float64 push, where only float64 rounding is
  allowed for); prints the figures before it asserts."""
  P, R = np.asarray(P, dtype=np.float64), np.asarray(R, dtype=np.float64)
  gap = Pi - P
  tol64 = ORACLE_TOL
  ratio = float((gap / (eps * deg[None, :])).max())
  mass = P.sum(1) + R.sum(1) / alpha
  rmax = float((R / (alpha * eps * deg[None, :])).max())
  print('%s: max (Pi - p) / (eps deg) %.4f, min Pi - p %.3e, |mass - 1| %.3e, max r / (alpha eps deg) %.6f, support %.1f'
        % (label, ratio, float(gap.min()), float(np.abs(mass - 1.0).max()), rmax, float((P > 0).sum(1).mean())))
  assert (P >= 0).all() and (R >= 0).all()
  assert (gap >= -gamma * P - tol64).all(), 'p exceeds Pi by %.3e beyond the slack' % float((-gap - gamma * P).max())
  assert (gap < eps * deg[None, :] + gamma * Pi + lost / alpha + tol64).all(), 'Pi - p reaches eps deg'
  assert (np.abs(mass - 1.0) <= gamma + (lost + QUANTUM) / alpha + tol64).all(), 'mass is not conserved'
  assert (R < alpha * eps * deg[None, :] * (1.0 + gamma)).all(), 'a residual at or above alpha eps deg is left'
  return ratio


def sym_scale(P, deg):
  """torch_geometric's approximate branch for normalization_in = 'sym': deg(s)^1/2 p_s(u) deg(u)^-1/2."""
  return np.sqrt(deg)[:, None] * P / np.sqrt(deg)[None, :]


def col_normalise(W):
  s = W.sum(0)
  return W / np.where(s > 0, s, 1.0)[None, :]


def pipeline_band(name, threshold):
  """The pipeline of the wrapper ('sym' in, threshold, 'col' out) on the float64 synchronous push, and what the bound leaves open.
  Native and float64 push both lie in (Pi - eps deg(u) - slack, Pi + slack], so the scaled values differ by less than
  sqrt(deg(s) deg(u)) eps + 3 gamma value + slack: an entry farther than that from the threshold must agree in membership."""
  c = SHAPES[name]
  _, _, deg, _ = shape(name)
  P, _ = push_all(name)
  S = sym_scale(P, deg)
  # three fp32 roundings on the native side: p itself, the scaled value, the threshold
  width = (np.sqrt(deg[:, None] * deg[None, :]) * c['eps'] + 3.0 * GAMMA * np.maximum(S, threshold)
           + lost_mass(c['alpha'], c['eps'], deg.max()) / c['alpha'] + ORACLE_TOL)
  kept = S >= threshold
  inside = S - width >= threshold
  outside = (S + width < threshold) | (S == 0)
  # an entry the float64 push never reached may still be reached by another order: open unless the bound excludes it
  outside = np.where(S == 0, width < threshold, outside)
  open_ = ~inside & ~outside
  return dict(S=S, kept=kept, inside=inside, outside=outside, open=open_, share=float(open_.sum()) / max(int(kept.sum()), 1),
              out=col_normalise(np.where(kept, S, 0.0)), width=width)
