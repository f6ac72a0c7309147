"""numpy restatement of the coordinate-descent NMF that csrc/nmf.hip runs (include/gnpde.h has the definition; sklearn's
solver='cd', beta_loss='frobenius', no regularisation, shuffle=False): the half-sweep in its fresh-gradient form (sklearn's own
loop order) and in the incremental form (q = W G - P kept up to date, what the kernel does), a dtype argument, the fit loop and the
Gram-identity reconstruction error.  Also the inputs of the sweep tests, so that the CPU and the GPU tests share them."""
import functools

import numpy as np


def sweep(W, G, P, dtype=np.float64, incremental=False, want_margin=False):
  """One half-sweep on copies: (W_new, violation) -- and, with want_margin, the smallest |W[i, t] - grad / G[t, t]| met, the distance
  of the closest update from the clip at 0.  Every product and update is rounded to `dtype`; the violation is summed in double."""
  W, G, P = np.array(W, dtype=dtype), np.asarray(G, dtype=dtype), np.asarray(P, dtype=dtype)
  k = W.shape[1]
  violation, margin = 0.0, np.inf
  Q = (W @ G - P).astype(dtype) if incremental else None
  for t in range(k):
    grad = Q[:, t].copy() if incremental else (-P[:, t] + W @ G[t, :]).astype(dtype)
    pg = np.where(W[:, t] == 0, np.minimum(0, grad), grad)
    violation += float(np.abs(pg).astype(np.float64).sum())
    if G[t, t] != 0:
      raw = (W[:, t] - grad / G[t, t]).astype(dtype)
      margin = min(margin, float(np.abs(raw).min()))
      new = np.maximum(raw, 0).astype(dtype)
      if incremental:
        Q += np.outer(new - W[:, t], G[t, :]).astype(dtype)
      W[:, t] = new
  return (W, violation, margin) if want_margin else (W, violation)


def iteration(X, W, Ht, dtype=np.float64, incremental=False):
  """Both half-sweeps of one iteration; returns (W, Ht, violation)."""
  X = np.asarray(X, dtype=dtype)
  W, v1 = sweep(W, (Ht.T @ Ht).astype(dtype), (X @ Ht).astype(dtype), dtype, incremental)
  Ht, v2 = sweep(Ht, (W.T @ W).astype(dtype), (X.T @ W).astype(dtype), dtype, incremental)
  return W, Ht, v1 + v2


def fit(X, W0, H0, max_iter, tol, dtype=np.float64, incremental=False):
  """(W, H, n_iter, ratios): the fit stops after iteration it when violation_it / violation_1 <= tol, or at once when
  violation_1 == 0; ratios[it - 1] = violation_it / violation_1."""
  W, Ht = np.array(W0, dtype=dtype), np.array(np.asarray(H0).T, dtype=dtype)
  ratios, first, it = [], None, 0
  for it in range(1, max_iter + 1):
    W, Ht, v = iteration(X, W, Ht, dtype, incremental)
    if it == 1:
      first = v
    if first == 0:
      break
    ratios.append(v / first)
    if v / first <= tol:
      break
  return W, np.ascontiguousarray(Ht.T), it, ratios


def reconstruction_err(X, W, H, dtype=np.float64):
  """sqrt(max(0, |X|^2 - 2 <W, X H^T> + <W^T W, H H^T>)): the three products in `dtype`, the inner products in double."""
  X, W, H = np.asarray(X, dtype=dtype), np.asarray(W, dtype=dtype), np.asarray(H, dtype=dtype)
  P, Gw, Gh = (X @ H.T).astype(np.float64), (W.T @ W).astype(np.float64), (H @ H.T).astype(np.float64)
  e2 = float((X.astype(np.float64) ** 2).sum()) - 2.0 * float((W.astype(np.float64) * P).sum()) + float((Gw * Gh).sum())
  return float(np.sqrt(max(0.0, e2)))


# ---- the inputs of the sweep tests ---------------------------------------------------------------------------------------------
SWEEP_N = (1, 7, 130)                                  # one row, fewer rows than a workgroup has waves, more than one workgroup
SWEEP_K = (1, 2, 17, 64, 65, 128, 129, 256)            # the lane-register counts 1 .. 4, their edges, and the edge of the LDS path
SWEEP_SEED = 7
MIN_MARGIN = 0.04                                      # see sweep_case


def sweep_case(n, k, kind):
  """float32 inputs (W, G, P) of one half-sweep.  W has ~30 % exact zeros (the pg branch); G = H^T H is a full Gram matrix, and for
  k >= 2 component k // 2 has G[t, :] = G[:, t] = 0 (it must stay untouched).  P is built component by component along a float64
  sweep so that the value that gets clipped, W[i, t] - grad / G[t, t], is a drawn target with 0.05 <= |target| <= 2: negative (the
  update clips to 0) for ~40 % of the entries with kind 'mixed' and for every entry with kind 'clip'.  That keeps every update
  MIN_MARGIN away from the clip, so 'exactly 0 where float64 is 0' is a fair demand of any float32 summation order."""
  rng = np.random.RandomState(SWEEP_SEED + 1000 * n + k)
  m = 40
  H = np.abs(rng.randn(m, k)) / np.sqrt(m)
  if k >= 2:
    H[:, k // 2] = 0.0
  G = (H.T @ H).astype(np.float32)                     # symmetric, diagonal ~ 1
  W = np.abs(rng.randn(n, k))
  W[rng.rand(n, k) < 0.3] = 0.0
  W = W.astype(np.float32)
  target = rng.uniform(0.05, 2.0, size=(n, k))
  target[rng.rand(n, k) < (0.4 if kind == 'mixed' else 2.0)] *= -1.0
  G64, cur, P = G.astype(np.float64), W.astype(np.float64), np.zeros((n, k))
  for t in range(k):
    # target = cur_t - (-P_t + cur G[t, :]) / G[t, t]
    P[:, t] = cur @ G64[t, :] + G64[t, t] * (target[:, t] - cur[:, t]) if G64[t, t] != 0 else rng.randn(n)
    P[:, t] = P[:, t].astype(np.float32)
    if G64[t, t] != 0:
      cur[:, t] = np.maximum(cur[:, t] - (-P[:, t] + cur @ G64[t, :]) / G64[t, t], 0)
  return W, G, P.astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep_family():
  """{(n, k, kind): (W, G, P, W64, v64)} and the yardstick: delta_W, delta_v = the largest deviation of the float32 oracle (fresh
  form) from the float64 oracle over the family, for W and for the violation.  Also asserts the condition that makes 'exactly 0
  where float64 is 0' a fair demand: no float64 update comes closer to the clip than MIN_MARGIN, a hundred times delta_W."""
  cases, delta_w, delta_v, margin = {}, 0.0, 0.0, np.inf
  for n in SWEEP_N:
    for k in SWEEP_K:
      for kind in ('mixed', 'clip'):
        W, G, P = sweep_case(n, k, kind)
        W64, v64, mg = sweep(W, G, P, np.float64, want_margin=True)
        W32, v32 = sweep(W, G, P, np.float32)
        delta_w = max(delta_w, float(np.abs(W32.astype(np.float64) - W64).max()))
        delta_v = max(delta_v, abs(v32 - v64))
        margin = min(margin, mg)
        cases[(n, k, kind)] = (W, G, P, W64, v64)
  assert margin > MIN_MARGIN > 100 * delta_w, (margin, delta_w)
  return cases, delta_w, delta_v
