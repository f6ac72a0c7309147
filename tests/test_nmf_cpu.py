"""NMF compression of positional encodings, everything that needs no device: the oracle (nmf_oracle.py) against sklearn and against
itself, the refusals of `gnpde_amd.pos_enc_factorisation.NMF`, the argument errors of the C entry point, and the C ABI."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
from gnpde_amd.pos_enc_factorisation import NMF
import nmf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4


def _inputs(kind, seed=3):
  rng = np.random.RandomState(seed)
  if kind == 'sparse':
    import scipy.sparse as sp
    X = sp.random(60, 60, density=0.1, random_state=rng, format='csr').toarray()
  else:
    X = np.abs(rng.randn(60, 5)) @ np.abs(rng.randn(5, 60)) + 0.05 * np.abs(rng.randn(60, 60))
  avg = np.sqrt(X.mean() / K)
  return X, avg * np.abs(rng.randn(60, K)), avg * np.abs(rng.randn(K, 60))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ('sparse', 'dense'))
@pytest.mark.parametrize('tol', (1e-2, 1e-3))
def test_float64_oracle_equals_sklearn(kind, tol):
  sk = pytest.importorskip('sklearn.decomposition')
  import scipy.sparse as sp
  X, W0, H0 = _inputs(kind)
  model = sk.NMF(n_components=K, init='custom', solver='cd', max_iter=500, tol=tol)
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    Ws = model.fit_transform(sp.csr_matrix(X) if kind == 'sparse' else X, W=W0.copy(), H=H0.copy())
  W, H, n_iter, _ = O.fit(X, W0, H0, 500, tol)
  print('%s tol %g: n_iter %d / %d, max |dW| %.2e |dH| %.2e' % (kind, tol, n_iter, model.n_iter_, np.abs(W - Ws).max(),
                                                             np.abs(H - model.components_).max()))
  assert n_iter == model.n_iter_ and n_iter < 500
  assert np.abs(W - Ws).max() <= 1e-12 and np.abs(H - model.components_).max() <= 1e-12
  assert abs(O.reconstruction_err(X, W, H) - model.reconstruction_err_) <= 1e-10


@pytest.mark.parametrize('kind', ('sparse', 'dense'))
def test_incremental_form_equals_fresh_form(kind):
  X, W0, H0 = _inputs(kind)
  a = O.fit(X, W0, H0, 30, 0.0)
  b = O.fit(X, W0, H0, 30, 0.0, incremental=True)
  assert np.abs(a[0] - b[0]).max() <= 1e-12 and np.abs(a[1] - b[1]).max() <= 1e-12
  assert np.allclose(a[3], b[3], rtol=1e-10, atol=0)
  for key in ((130, 65, 'mixed'), (7, 256, 'mixed'), (130, 17, 'clip')):
    W, Gm, P = O.sweep_family()[0][key][:3]
    Wf, vf = O.sweep(W, Gm, P)
    Wi, vi = O.sweep(W, Gm, P, incremental=True)
    assert np.abs(Wf - Wi).max() <= 1e-12 and abs(vf - vi) <= 1e-12 * vf


@pytest.mark.parametrize('kind', ('sparse', 'dense'))
def test_objective_never_increases(kind):
  X, W0, H0 = _inputs(kind)
  W, Ht = W0.copy(), H0.T.copy()
  last = np.linalg.norm(X - W @ Ht.T)
  for _ in range(20):
    W, _ = O.sweep(W, Ht.T @ Ht, X @ Ht)
    now = np.linalg.norm(X - W @ Ht.T)
    assert now <= last * (1 + 1e-14)
    Ht, _ = O.sweep(Ht, W.T @ W, X.T @ W)
    last = np.linalg.norm(X - W @ Ht.T)
    assert last <= now * (1 + 1e-14)
    assert (W >= 0).all() and (Ht >= 0).all()


def test_gram_identity_error_equals_the_residual_norm():
  for kind in ('sparse', 'dense'):
    X, W0, H0 = _inputs(kind)
    for W, H in ((W0, H0), O.fit(X, W0, H0, 15, 0.0)[:2]):
      assert abs(O.reconstruction_err(X, W, H) - np.linalg.norm(X - W @ H)) <= 1e-10


def test_sweep_family_covers_the_branches():
  cases, delta_w, delta_v = O.sweep_family()
  print('delta_W %.3e delta_v %.3e' % (delta_w, delta_v))
  assert 0 < delta_w < 1e-3 and 0 < delta_v
  assert len(cases) == 2 * len(O.SWEEP_N) * len(O.SWEEP_K)
  for (n, k, kind), (W, Gm, P, W64, v64) in cases.items():
    assert (W == 0).any() or n * k < 8
    if k >= 2:
      assert Gm[k // 2, k // 2] == 0 and np.array_equal(W64[:, k // 2], W[:, k // 2].astype(np.float64))
    live = np.ones(k, dtype=bool)
    if k >= 2:
      live[k // 2] = False
    if kind == 'clip':
      assert (W64[:, live] == 0).all()
    elif n * k >= 64:
      assert (W64[:, live] == 0).any() and (W64[:, live] > 0).any()


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', (dict(solver='mu'), dict(beta_loss='kullback-leibler'), dict(alpha_W=0.1), dict(alpha_H=0.0),
                                dict(l1_ratio=0.5), dict(shuffle=True), dict(init='nndsvd'), dict(init=None), dict(random_state=None)))
def test_unsupported_arguments_are_refused_by_name(kw):
  name = next(iter(kw))
  with pytest.raises(NotImplementedError, match='NMF: %s = ' % name):
    NMF(4, **kw)


def test_defaults_are_accepted_and_a_cpu_tensor_is_refused():
  model = NMF(4, init='random', solver='cd', beta_loss='frobenius', tol=1e-4, max_iter=200, random_state=0, alpha_W=0.0, alpha_H='same',
              l1_ratio=0.0, verbose=0, shuffle=False)
  assert model.n_components == 4 and model.components_ is None and model.n_iter_ is None and model.reconstruction_err_ is None
  x = torch.rand(6, 6)
  with pytest.raises(G.GnpdeError, match='no CPU fallback'):
    model.fit_transform(x)
  with pytest.raises(G.GnpdeError, match='no CPU fallback'):
    model.fit_transform((torch.zeros(2, 3, dtype=torch.int64), torch.ones(3), (6, 6)))
  with pytest.raises(G.GnpdeError, match='no CPU fallback'):
    ops.nmf(x, 2)
  with pytest.raises(G.GnpdeError, match='no CPU fallback'):
    ops.nmf_cd_sweep(torch.rand(6, 2), torch.eye(2), torch.rand(6, 2))
  with pytest.raises(ValueError, match="init = 'custom' needs both W and H"):
    NMF(2, init='custom').fit_transform(x, W=torch.rand(6, 2))
  with pytest.raises(ValueError, match="init = 'random'"):
    model.fit_transform(x, W=torch.rand(6, 4), H=torch.rand(4, 6))
  with pytest.raises(G.GnpdeError, match='n_components = 257'):
    ops.nmf(x, 257)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
C_TYPES = {'float*': _lib.c_vp, 'const float*': _lib.c_vp, 'double*': _lib.c_vp, 'void*': _lib.c_vp, 'int64_t': ctypes.c_int64,
           'int32_t': ctypes.c_int32, 'size_t': ctypes.c_size_t, 'int': ctypes.c_int}


def test_declaration_and_ctypes_signature_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  L = G.lib()
  for name in ('gnpde_nmf_cd_sweep_workspace_bytes', 'gnpde_nmf_cd_sweep'):
    m = re.search(r'^(\w+)\s+%s\(([^)]*)\);' % name, header, re.M)
    assert m, name + ' is not declared in gnpde.h'
    args = [' '.join(a.split()[:-1]) for a in m.group(2).replace('\n', ' ').split(',')]
    res, argtypes = _lib.PROTOTYPES[name]
    assert res is C_TYPES[m.group(1)], name
    assert [C_TYPES[a] for a in args] == list(argtypes), (name, args)
    assert hasattr(L, name), name + ' is not exported by the library'
    assert name in open(os.path.join(ROOT, 'INTEGRATION.md')).read(), name + ' is not in INTEGRATION.md'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 17 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION


def test_entry_point_rejects_bad_arguments_before_any_launch():
  """Limits, null pointers, strides, aliasing and the workspace size return an error code and a message; nothing touches a device."""
  L = G.lib()
  n, k = 8, 4
  buf = torch.zeros(n, 3 * k)
  W, P, Gm, v = torch.zeros(n, k), torch.zeros(n, k), torch.zeros(k, k), torch.zeros(1, dtype=torch.float64)
  need = L.gnpde_nmf_cd_sweep_workspace_bytes(n)
  assert need >= 8 * n + 8 and L.gnpde_nmf_cd_sweep_workspace_bytes(0) == 0 and L.gnpde_nmf_cd_sweep_workspace_bytes(2 ** 31) == 0
  ws = torch.zeros(need + 256, dtype=torch.uint8)
  off = (-ws.data_ptr()) % 256
  wsp = ctypes.c_void_p(ws.data_ptr() + off)
  p = _lib.ptr

  def call(W=W, ldw=k, Gm=Gm, P=P, ldp=k, n=n, k=k, v=v, wsp=wsp, nbytes=need):
    return L.gnpde_nmf_cd_sweep(p(W), ldw, p(Gm), p(P), ldp, n, k, p(v), wsp, nbytes, None)

  for kw, code, text in ((dict(k=0), -2, 'k = 0 outside 1 .. 256'), (dict(k=257), -2, 'k = 257 outside'), (dict(n=0), -2, 'n = 0 outside'),
                         (dict(n=2 ** 31), -2, 'INT32_MAX'), (dict(W=None), -1, 'null pointer'), (dict(v=None), -1, 'null pointer'),
                         (dict(ldw=k - 1), -1, 'row strides'), (dict(ldp=3), -1, 'row strides'), (dict(P=W), -1, 'W and P alias'),
                         (dict(W=buf[:, :k], ldw=3 * k, P=buf[:, k:2 * k], ldp=3 * k), -1, 'W and P alias'),
                         (dict(Gm=W), -1, 'W and G alias'), (dict(nbytes=need - 1), -3, 'workspace'),
                         (dict(wsp=ctypes.c_void_p(ws.data_ptr() + off + 8)), -3, '256-byte aligned'), (dict(wsp=None), -3, 'workspace')):
    assert call(**kw) == code, kw
    assert text in L.gnpde_last_error().decode(), (kw, L.gnpde_last_error().decode())
