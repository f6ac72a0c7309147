"""Matrix factorisation of the positional encoding required for arxiv-ogbn (reference src/pos_enc_factorisation.py): the GDC encoding
X [n, n] is compressed to W [n, dim] with X ~ W H, W, H >= 0, and W replaces the cached encoding.

`NMF` has the surface of sklearn.decomposition.NMF that the reference uses -- solver 'cd', Frobenius loss, no regularisation,
shuffle off -- on the native coordinate-descent sweep (`ops.nmf`, csrc/nmf.hip; include/gnpde.h has the definition).  sklearn is
not imported.  Differences: X is a float32 device tensor or a sparse triple (edge_index, weight, (n, n)), never a CPU array;
init='random' draws from a torch.Generator on the device, so equal `random_state` gives equal factors here but not sklearn's; every
other argument of sklearn's constructor is refused unless it is given at its default.

`compress_pos_encodings(data, opt)` is the reference script's `main` without the dataset loading and without its two broken writes
(`with opt(out_path, 'wb')` calls a dict, `opt['out_path']` is a key the parser never sets): it finds or makes the GDC encoding
(`graph_rewiring.apply_beltrami`), factorises it and writes W over `<data_dir>/pos_encodings/<dataset>_<pos_enc_type>.pkl`, as the
reference's last statement does."""
import os
import pickle
import time

import torch

from . import ops

# sklearn's constructor arguments that select something the native sweep does not have, with the only value each may take
_FIXED = (('solver', 'cd'), ('beta_loss', 'frobenius'), ('alpha_W', 0.0), ('alpha_H', 'same'), ('l1_ratio', 0.0), ('shuffle', False))


class NMF(object):
  """sklearn.decomposition.NMF(n_components, init, random_state, max_iter, tol, verbose) on the device: `fit_transform(X, W=None,
  H=None)` returns W [n, n_components] and leaves `components_` (H), `n_iter_` and `reconstruction_err_`."""

  def __init__(self, n_components, *, init='random', solver='cd', beta_loss='frobenius', tol=1e-4, max_iter=200, random_state=0,
               alpha_W=0.0, alpha_H='same', l1_ratio=0.0, verbose=0, shuffle=False):
    given = dict(solver=solver, beta_loss=beta_loss, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio, shuffle=shuffle)
    for name, only in _FIXED:
      if given[name] != only:
        raise NotImplementedError('NMF: %s = %r is not built (only %s = %r: coordinate descent on the Frobenius loss without '
                                  'regularisation, components in order)' % (name, given[name], name, only))
    if init not in ('random', 'custom'):
      raise NotImplementedError("NMF: init = %r is not built (only init = 'random' and init = 'custom')" % (init,))
    if random_state is None or isinstance(random_state, bool) or not isinstance(random_state, int):
      raise NotImplementedError('NMF: random_state = %r is not built (only an int: it seeds a torch.Generator on the device)' % (random_state,))
    self.n_components = int(n_components)
    self.init = init
    self.random_state = random_state
    self.max_iter = int(max_iter)
    self.tol = float(tol)
    self.verbose = verbose
    self.components_ = None
    self.n_iter_ = None
    self.reconstruction_err_ = None

  @torch.no_grad()
  def fit_transform(self, X, y=None, W=None, H=None):
    if self.init == 'custom' and (W is None or H is None):
      raise ValueError("NMF: init = 'custom' needs both W and H")
    if self.init == 'random' and (W is not None or H is not None):
      raise ValueError("NMF: W and H are given but init = 'random' (sklearn ignores them; pass init = 'custom')")
    for t in (tuple(X) if isinstance(X, (tuple, list)) else (X,)) + (W, H):
      if isinstance(t, torch.Tensor) and not t.is_cuda:
        raise ops._lib.GnpdeError('NMF: got a %s tensor; the factorisation runs only on a HIP device, there is no CPU fallback' % t.device.type)
    W, H, self.n_iter_, err = ops.nmf(X, self.n_components, W=W, H=H, max_iter=self.max_iter, tol=self.tol, seed=self.random_state)
    self.components_ = H
    self.reconstruction_err_ = float(err)
    if self.verbose:
      print('NMF: %d iterations, reconstruction error %.6g' % (self.n_iter_, self.reconstruction_err_))
    return W


def compress_pos_encodings(data, opt, data_dir='../data'):
  """The reference script's main() on `data`: the GDC encoding -- the cached pickle, or `apply_gdc(type='pos_encoding')` cached as
  `graph_rewiring.apply_beltrami` caches it -- factorised by NMF(n_components=opt['embedding_dim'], init='random', random_state=0,
  max_iter=opt['max_iter'], tol=opt['tol']) (defaults 100 and 0.002, the script's); W [n, embedding_dim] is written over the
  encoding's pickle as a CPU tensor and returned."""
  from .graph_rewiring import apply_beltrami
  if opt['pos_enc_type'] != 'GDC':
    raise ValueError('compress_pos_encodings: positional encoding type %r is not GDC' % (opt['pos_enc_type'],))
  start = time.time()
  model = NMF(n_components=opt['embedding_dim'], init='random', random_state=0, max_iter=opt.get('max_iter', 100), tol=opt.get('tol', 0.002),
              verbose=1)
  x = torch.as_tensor(apply_beltrami(data, {key: v for key, v in opt.items() if key != 'gnpde_pos_enc_nmf_dim'}, data_dir))
  if not x.is_cuda and torch.cuda.is_available():
    x = x.cuda()
  print('encodings ready after %.1f s, factorising' % (time.time() - start))
  W = model.fit_transform(x.to(torch.float32).contiguous()).to(torch.device('cpu'))
  print('compressed to %d columns after %.1f s' % (W.shape[1], time.time() - start))
  with open(os.path.join(data_dir, 'pos_encodings', '%s_%s.pkl' % (opt['dataset'], opt['pos_enc_type'])), 'wb') as f:
    pickle.dump(W, f)
  return W
