"""Record the whole-fit fixtures of tests/test_nmf_gpu.py with sklearn on a CPU: tests/golden/nmf_fit_<name>.npz.

  python tools/record_nmf_fixtures.py

Each fixture holds float32 inputs (X dense, or as (row, col, value) for the sparse case; the custom init W0, H0), the tolerance, and
sklearn's result in float64 (W, H, n_iter, reconstruction_err) together with the float32 oracle's own deviation from it (dev_W,
dev_H, dev_err): the GPU test allows 8 x that.  sklearn.decomposition.NMF(init='custom', solver='cd') runs on the float64 copies of
the float32 inputs, so the device sees the same numbers.

The tolerance is chosen, not fixed: the fit stops when violation_it / violation_1 <= tol, and a float32 run must stop at the same
iteration, so tol is put in the MIDDLE of a step of the ratio sequence -- the geometric mean of two consecutive ratios of the
float64 oracle.  Conditions (asserted here, they are not measurements): both neighbouring ratios lie at least 2 % from tol, the
float32 oracle stops at the same iteration, that iteration is 20 or more, and sklearn agrees with the float64 oracle to 1e-12."""
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sp
from sklearn.decomposition import NMF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import nmf_oracle as O  # noqa: E402

K = 4
MIN_ITER = 20
MIN_GAP = 1.02


def inputs(name):
  rng = np.random.RandomState({'sparse': 3, 'dense': 4, 'rect': 5}[name])
  if name == 'sparse':
    X = sp.random(60, 60, density=0.1, random_state=rng, format='csr').toarray()
    X[5, :] = 0.0                                     # one empty row, one empty column
    X[:, 9] = 0.0
  elif name == 'dense':
    X = np.abs(rng.randn(60, 5)) @ np.abs(rng.randn(5, 60)) + 0.05 * np.abs(rng.randn(60, 60))
  else:
    X = np.abs(rng.randn(40, 3)) @ np.abs(rng.randn(3, 25)) + 0.05 * np.abs(rng.randn(40, 25))
  X = X.astype(np.float32)
  avg = np.sqrt(X.mean() / K)
  W0 = (avg * np.abs(rng.randn(X.shape[0], K))).astype(np.float32)
  H0 = (avg * np.abs(rng.randn(K, X.shape[1]))).astype(np.float32)
  return X, W0, H0


def choose_tol(ratios):
  """(tol, it): the first iteration it >= MIN_ITER whose ratio step leaves MIN_GAP on both sides of the geometric mean."""
  for it in range(MIN_ITER, len(ratios) + 1):
    before, here = ratios[it - 2], ratios[it - 1]
    tol = float(np.sqrt(before * here))
    if here * MIN_GAP <= tol <= before / MIN_GAP and min(ratios[:it - 1]) >= tol * MIN_GAP:
      return tol, it
  raise AssertionError('no step of the ratio sequence is wide enough')


def record(name):
  X, W0, H0 = inputs(name)
  X64, W64, H64 = X.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64)
  ratios = O.fit(X64, W64, H64, 300, 0.0)[3]
  tol, it = choose_tol(ratios)
  assert it >= MIN_ITER and ratios[it - 1] * MIN_GAP <= tol <= ratios[it - 2] / MIN_GAP
  Wo, Ho, it_o, _ = O.fit(X64, W64, H64, 300, tol)
  model = NMF(n_components=K, init='custom', solver='cd', max_iter=300, tol=tol)
  with warnings.catch_warnings():
    warnings.simplefilter('error')
    Ws = model.fit_transform(sp.csr_matrix(X64) if name == 'sparse' else X64, W=W64.copy(), H=H64.copy())
  Hs = model.components_
  assert model.n_iter_ == it_o == it, (model.n_iter_, it_o, it)
  assert np.abs(Ws - Wo).max() <= 1e-12 and np.abs(Hs - Ho).max() <= 1e-12
  err = float(model.reconstruction_err_)
  assert abs(O.reconstruction_err(X64, Ws, Hs) - err) <= 1e-10 * max(1.0, err)
  W32, H32, it32, _ = O.fit(X, W0, H0, 300, tol, np.float32)
  assert it32 == it, (it32, it)
  dev = dict(dev_W=np.abs(W32 - Ws).max(), dev_H=np.abs(H32 - Hs).max(), dev_err=abs(O.reconstruction_err(X, W32, H32, np.float32) - err))
  out = dict(W0=W0, H0=H0, tol=np.float64(tol), n_iter=np.int64(it), W=Ws, H=Hs, reconstruction_err=np.float64(err),
             ratio_before=np.float64(ratios[it - 2]), ratio_at=np.float64(ratios[it - 1]), **{k: np.float64(v) for k, v in dev.items()})
  if name == 'sparse':
    row, col = np.nonzero(X)
    out.update(row=row.astype(np.int64), col=col.astype(np.int64), value=X[row, col], shape=np.array(X.shape, dtype=np.int64))
  else:
    out['X'] = X
  path = os.path.join(ROOT, 'tests', 'golden', 'nmf_fit_%s.npz' % name)
  np.savez(path, **out)
  print('%-6s n_iter %3d  tol %.6g  (ratios %.6g -> %.6g)  err %.6g  float32 oracle: dW %.2e dH %.2e derr %.2e  -> %s'
        % (name, it, tol, ratios[it - 2], ratios[it - 1], err, dev['dev_W'], dev['dev_H'], dev['dev_err'], os.path.relpath(path, ROOT)))


if __name__ == '__main__':
  for name in ('sparse', 'dense', 'rect'):
    record(name)
