"""DeepWalk positional encodings, everything that needs no device: self-checks of the oracle (deepwalk_oracle.py), the documented
difference from PyG's literal fp32 loss, the use condition on the oracle trainer, the symbols and the ABI number, argument errors of
the C entry points and of the Python surface, and the option table of `apply_beltrami`."""
import os
import pickle
import re
import types

import numpy as np
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops
from gnpde_amd import deepwalk_embeddings as DW
import deepwalk_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_random_walks', 'gnpde_negative_walks', 'gnpde_random_permutation', 'gnpde_random_permutation_workspace_bytes',
           'gnpde_deepwalk_step_workspace_bytes', 'gnpde_deepwalk_step')


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def test_oracle_walks_follow_edges_and_stay_at_the_sink_and_the_isolated_node():
  ei, n = O.odd_graph()
  rowptr, col = O.csr(ei, n)
  assert col[rowptr[0]:rowptr[1]].tolist() == [1, 1, 3]                 # multiplicity kept, ascending
  starts = np.tile(np.arange(n), 400)
  rw = O.random_walks(rowptr, col, starts, 7, 11, 16, 0)
  assert (rw[:, 0] == starts).all()
  edges = set(zip(ei[0].tolist(), ei[1].tolist()))
  counts = np.zeros((n, n), dtype=np.int64)
  np.add.at(counts, (rw[:, :-1].reshape(-1), rw[:, 1:].reshape(-1)), 1)
  for u in range(n):
    for v in np.nonzero(counts[u])[0]:
      assert (u, int(v)) in edges or (u == v and rowptr[u + 1] == rowptr[u]), (u, v)
  for stay in (5, 7):                                                    # the sink and the isolated node: every transition stays
    assert counts[stay, stay] == counts[stay].sum() > 0
  assert (rw[rw[:, 0] == 7] == 7).all()
  assert 1.6 < counts[0, 1] / counts[0, 3] < 2.5                         # the duplicated edge 0 -> 1 is taken twice as often
  assert counts[2, 2] > 0 and counts[2, 4] > 0                           # the self-loop is an edge like any other


def test_oracle_negative_walks_and_permutation():
  neg = O.negative_walks(1000, np.arange(50), 9, 5, 17, 2)
  assert (neg[:, 0] == np.arange(50)).all() and neg.min() >= 0 and neg.max() < 1000 and len(np.unique(neg[:, 1:])) > 300
  assert (O.negative_walks(1, np.zeros(4, dtype=np.int64), 5, 5, 17, 2) == 0).all()
  for n in (1, 2, 257):
    p = O.random_permutation(n, 3, 18, 0)
    assert np.array_equal(np.sort(p), np.arange(n))
  assert not np.array_equal(O.random_permutation(257, 3, 18, 0), O.random_permutation(257, 3, 18, 1))
  # batches of one epoch draw from disjoint counter ranges: walks 5.. of a call are the walks 0.. of a call that starts at first_walk = 5
  a = O.walk_words(12, 6, 9, 16, 0, 0)
  assert np.array_equal(a[5:], O.walk_words(7, 6, 9, 16, 0, 5))


@pytest.mark.parametrize('L,C', O.GRID_LC + ((6, 2), (7, 7)))
def test_pair_set_equals_the_pairs_of_pygs_windows(L, C):
  rw = torch.arange(L + 1).reshape(1, -1)                                # node id = position
  J = 1 + L + 1 - C
  win = torch.cat([rw[:, j:j + C] for j in range(J)], dim=0)
  pyg = sorted((int(r[0]), int(x)) for r in win for x in r[1:])
  assert pyg == sorted(O.window_pairs(L, C)) and len(pyg) == J * (C - 1)
  touched = {p for ab in pyg for p in ab}
  assert touched == set(range(L + 1))                                    # every walk position takes part in a pair


def test_literal_fp32_form_saturates_where_the_stable_form_does_not():
  """PyG's log(1 - sigmoid(x) + EPS): in fp32 1 - sigmoid(x) is exactly 0 once x > ~17, so the term is log(EPS) = 34.5 and its
  gradient vanishes; -log(sigmoid(-x) + EPS) is x there.  This is the documented difference."""
  x = torch.tensor([5.0, 18.0, 30.0, 50.0])
  literal = -torch.log(1 - torch.sigmoid(x) + O.EPS)
  stable = -torch.log(torch.sigmoid(-x) + O.EPS)
  exact = -torch.log(torch.sigmoid(-x.double()) + O.EPS)
  assert float((stable.double() - exact).abs().max()) < 1e-5
  assert torch.allclose(literal[1:], torch.full((3,), 34.5388), atol=1e-3) and abs(float(literal[0]) - float(exact[0])) < 1e-4
  # on a whole step: the case with rows scaled by 3 has scores beyond +-50; the fp32 run of the stable form tracks float64, the literal
  # form is off by whole units
  w, batches = O.case_inputs('large-scores')
  emb64 = torch.nn.Embedding.from_pretrained(w.double())
  scores = O.pair_scores(emb64, batches[0][1], O.CASES['large-scores']['C'])
  assert float(scores.max()) > 50 and float(scores.min()) < -50
  emb32 = torch.nn.Embedding.from_pretrained(w)
  ref = float(O.loss_of(emb64, *batches[0], 16))
  assert abs(float(O.loss_of(emb32, *batches[0], 16)) - ref) < 1e-4
  assert abs(float(O.loss_of(emb32, *batches[0], 16, literal=True)) - ref) > 0.1
  assert O.case_result('large-scores').d32 < 1e-4


def test_tolerances_come_from_the_oracle_alone():
  for name in ('grid-L20C16-d64-k1', 'collide-n7', 'sparse-n300'):
    r = O.case_result(name)
    assert 0 < r.d32 < 1e-3 and r.tol == 8 * r.d32 and np.isfinite(r.losses).all()
  assert [n for n in O.CASES if O.case_refused(n)] == ['grid-L80C2-d256-k1', 'grid-L80C2-d256-k2']


def test_use_condition_on_the_oracle_trainer():
  n = O.USE['n']
  before = O.community_cosines(O.initial_weights(n, O.USE['d'], 0), n)
  same, different = O.community_cosines(O.use_result(0), n)
  print('cosines before %+.3f / %+.3f, after %+.3f / %+.3f' % (before + (same, different)))
  assert abs(before[0]) < 0.05 and abs(before[1]) < 0.05
  assert same > 0 and different < 0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_number_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  declared = set(re.findall(r'\b(gnpde_[a-z_0-9]+)\s*\(', header))
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  L = G.lib()
  for name in SYMBOLS:
    assert name in declared, name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name), name + ' is not exported by the library'
    assert name in doc, name + ' is not in INTEGRATION.md'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 15 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION
  for name, value in (('GNPDE_DEEPWALK_BAD_START', _lib.DEEPWALK_BAD_START), ('GNPDE_DEEPWALK_BAD_GRAPH', _lib.DEEPWALK_BAD_GRAPH),
                      ('GNPDE_DEEPWALK_BAD_WALK', _lib.DEEPWALK_BAD_WALK)):
    assert int(re.search(r'#define\s+%s\s+(\d+)' % name, header).group(1)) == value
  # the trainer's stream ids are not the ones graph_rewiring's edge sampling draws from
  assert {ops.STREAM_POS_WALKS, ops.STREAM_NEG_WALKS, ops.STREAM_EPOCH_ORDER} == {O.STREAM_POS, O.STREAM_NEG, O.STREAM_ORDER}
  assert not {0, 1} & {ops.STREAM_POS_WALKS, ops.STREAM_NEG_WALKS, ops.STREAM_EPOCH_ORDER}


def test_entry_points_reject_bad_arguments_before_any_launch():
  """Shapes outside the limits, null pointers, strides, the step count and the workspace size return an error code and a message;
  nothing touches a device (this test runs without one)."""
  L = G.lib()
  i64 = torch.zeros(64, dtype=torch.int64)
  i32 = torch.zeros(64, dtype=torch.int32)
  f = torch.zeros(64, 8)
  p = _lib.ptr

  def walks(rowptr=i32, col=i32, e=4, n=3, starts=i64, ns=2, R=2, wl=4, out=i32, flag=i32):
    return L.gnpde_random_walks(p(rowptr), p(col), e, n, p(starts), ns, R, wl, 0, 16, 0, 0, p(out), p(flag), None)
  assert walks(n=0) == -1 and b'random_walks' in L.gnpde_last_error()
  assert walks(R=-1) == -1 and walks(flag=None) == -1 and walks(starts=None) == -1 and walks(out=None) == -1 and walks(ns=0) == -1
  assert walks(rowptr=None) == -1 and walks(e=-1) == -1 and walks(col=None) == -1 and walks(e=2 ** 31) == -1
  assert walks(wl=0) == -2 and walks(wl=128) == -2 and b'walk_length' in L.gnpde_last_error()
  assert walks(R=2 ** 31) == -2
  assert walks(R=0, starts=None, out=None) == 0                          # nothing to walk: no launch, no error

  def negative(n=3, starts=i64, ns=2, R=2, wl=4, out=i32, flag=i32):
    return L.gnpde_negative_walks(n, p(starts), ns, R, wl, 0, 17, 0, 0, p(out), p(flag), None)
  assert negative(n=0) == -1 and b'negative_walks' in L.gnpde_last_error()
  assert negative(wl=128) == -2 and negative(out=None) == -1 and negative(flag=None) == -1 and negative(R=0) == 0

  assert L.gnpde_random_permutation_workspace_bytes(0) == 0 and L.gnpde_random_permutation_workspace_bytes(2 ** 31) == 0
  need = L.gnpde_random_permutation_workspace_bytes(16)
  assert L.gnpde_random_permutation(0, 0, 18, 0, p(i64), p(i64), 512, None) == -1 and b'random_permutation' in L.gnpde_last_error()
  assert L.gnpde_random_permutation(16, 0, 18, 0, None, p(i64), 512, None) == -1
  rc = L.gnpde_random_permutation(16, 0, 18, 0, p(i64), p(i64), 8, None)
  assert rc == (-3 if need else -4)

  def step(emb=f, ld=8, m=f, v=f, ld_mv=8, n=64, d=8, t=1, pos=i32, rp=2, neg=i32, rn=2, wl=4, C=3, lr=0.01, b1=0.9, b2=0.999, eps=1e-8,
           loss=f, flag=i32, ws=f, ws_bytes=8):
    return L.gnpde_deepwalk_step(p(emb), ld, p(m), p(v), ld_mv, n, d, t, p(pos), rp, p(neg), rn, wl, C, lr, b1, b2, eps, p(loss), p(flag), p(ws),
                                 ws_bytes, None)
  for kw, text in ((dict(d=6), b'multiple of 4'), (dict(d=260, ld=260, ld_mv=260), b'multiple of 4'), (dict(d=0), b'multiple of 4'),
                   (dict(wl=128), b'walk_length'), (dict(wl=0), b'walk_length'), (dict(C=5), b'context_size'), (dict(C=1), b'context_size'),
                   (dict(wl=80, C=2, d=256, ld=256, ld_mv=256), b'64 KiB of LDS'), (dict(wl=127, C=64, d=128, ld=128, ld_mv=128), b'64 KiB of LDS'),
                   (dict(rp=2 ** 31, wl=20), b'INT32_MAX')):
    assert step(**kw) == -2 and b'deepwalk_step' in L.gnpde_last_error() and text in L.gnpde_last_error(), (kw, L.gnpde_last_error())
    sizes = dict(dict(rp=2, rn=2, wl=4, C=3, d=8), **{k: v for k, v in kw.items() if k in ('rp', 'rn', 'wl', 'C', 'd')})
    assert L.gnpde_deepwalk_step_workspace_bytes(sizes['rp'], sizes['rn'], sizes['wl'], sizes['C'], sizes['d']) == 0
  for kw in (dict(rp=0), dict(rn=0), dict(emb=None), dict(m=None), dict(v=None), dict(pos=None), dict(neg=None), dict(loss=None), dict(flag=None),
             dict(n=0), dict(ld=4), dict(ld_mv=4), dict(ld=10), dict(t=0), dict(lr=-1.0), dict(b1=1.0), dict(b2=-0.1), dict(eps=-1.0)):
    assert step(**kw) == -1 and b'deepwalk_step' in L.gnpde_last_error(), kw
  assert step(emb=f.reshape(-1)[1:]) == -1 and b'aligned' in L.gnpde_last_error()
  need = L.gnpde_deepwalk_step_workspace_bytes(2, 2, 4, 3, 8)
  rc = step()
  if need == 0:                        # the sort's temporary-storage query needs a device (as gnpde_edge_union's)
    assert rc == -4 and b'query failed' in L.gnpde_last_error()
  else:
    assert need >= 2 * 20 * 8 + 20 * 8 * 4 and rc == -3 and b'workspace' in L.gnpde_last_error()


def test_python_surface_argument_errors():
  ei = torch.tensor([[0, 1], [1, 0]])
  with pytest.raises(NotImplementedError, match='p = q = 1'):
    DW.DeepWalk(ei, 2, p=0.5)
  with pytest.raises(NotImplementedError, match='p = q = 1'):
    DW.DeepWalk(ei, 2, q=2)
  for kw, text in ((dict(embedding_dim=6), 'multiple of 4'), (dict(embedding_dim=260), 'multiple of 4'), (dict(walk_length=128), 'walk_length'),
                   (dict(walk_length=10, context_size=11), 'context_size'), (dict(walks_per_node=0), 'walks_per_node'),
                   (dict(num_negative_samples=0), 'num_negative_samples'), (dict(walk_length=80, context_size=2, embedding_dim=256), '64 KiB')):
    with pytest.raises(G.GnpdeError, match=text):
      DW.DeepWalk(ei, 2, **kw)
  with pytest.raises(G.GnpdeError, match='num_nodes'):
    DW.DeepWalk(ei, 0)
  host = torch.zeros(2, dtype=torch.int64)
  with pytest.raises(G.GnpdeError, match='HIP'):       # no CPU fallback
    ops.random_walks(ei, 2, host, 3, 0, 16, 0)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.negative_walks(2, host, 3, 0, 17, 0)
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.random_permutation(4, 0, 18, 0, device='cpu')
  with pytest.raises(G.GnpdeError, match='HIP'):
    ops.deepwalk_step(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(4, 8), 1, torch.zeros(2, 5, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64), 3)
  with pytest.raises(G.GnpdeError, match='vector'):
    ops.negative_walks(2, torch.zeros(2, 2, dtype=torch.int64), 3, 0, 17, 0)
  with pytest.raises(G.GnpdeError, match='stream'):
    ops.random_permutation(4, 0, 2 ** 32, 0)
  if not torch.cuda.is_available():
    with pytest.raises(G.GnpdeError, match='HIP'):
      DW.DeepWalk(ei, 2, embedding_dim=8, walk_length=4, context_size=3)


def test_pickle_name_is_the_reference_scripts():
  opt = dict(DW.DEFAULTS, dataset='Cora')
  assert DW.pickle_name(opt) == 'DW_Cora_emb_128_wl_020_cs_16_wn_16_epochs_100.pickle'
  assert DW.node_classification_accuracy(torch.zeros(3, 2), types.SimpleNamespace(y=None)) == 0.0


# ---- apply_beltrami --------------------------------------------------------------------------------------------------------------
class _FakeDeepWalk(object):
  made = []

  def __init__(self, edge_index, num_nodes, **kw):
    self.kw = dict(kw, num_nodes=num_nodes)
    self.embedding = torch.full((num_nodes, kw['embedding_dim']), 0.5)
    _FakeDeepWalk.made.append(self)

  def fit(self, epochs, batch_size=128):
    self.kw.update(epochs=epochs, batch_size=batch_size)
    return [0.0] * epochs


def test_apply_beltrami_option_table(tmp_path, monkeypatch):
  monkeypatch.setattr(DW, 'DeepWalk', _FakeDeepWalk)
  del _FakeDeepWalk.made[:]
  data = types.SimpleNamespace(edge_index=torch.tensor([[0, 1], [1, 0]]), num_nodes=2)
  base = {'dataset': 'Synthetic', 'pos_enc_type': 'DW64'}
  beltrami = lambda opt: G.graph_rewiring.apply_beltrami(data, opt, data_dir=str(tmp_path))
  # nothing changes without the opt-in, and HYP* raises with it too
  for opt in (base, dict(base, gnpde_generate_pos_enc=False), dict(base, gnpde_generate_pos_enc=0),
              dict(base, pos_enc_type='HYPS16'), dict(base, pos_enc_type='HYPS16', gnpde_generate_pos_enc=True)):
    with pytest.raises(FileNotFoundError):
      beltrami(opt)
  assert not _FakeDeepWalk.made and not os.path.exists(tmp_path / 'pos_encodings')
  with pytest.raises(ValueError, match='DW<d>'):
    beltrami(dict(base, pos_enc_type='DWx', gnpde_generate_pos_enc=True))
  # the opt-in: the script's defaults, 100 epochs and seed 0 unless the options say otherwise
  enc = beltrami(dict(base, gnpde_generate_pos_enc=True))
  assert _FakeDeepWalk.made.pop().kw == dict(num_nodes=2, embedding_dim=64, walk_length=20, context_size=16, walks_per_node=16, num_negative_samples=1,
                                             seed=0, epochs=100, batch_size=128)
  with open(tmp_path / 'pos_encodings' / 'Synthetic_DW64.pkl', 'rb') as f:
    stored = pickle.load(f)
  assert sorted(stored) == ['acc', 'data'] and stored['acc'] == 0.0 and torch.equal(stored['data'], enc) and enc.shape == (2, 64)
  assert torch.equal(beltrami(base), enc) and not _FakeDeepWalk.made           # a cached pickle is loaded, option or not
  beltrami(dict(base, pos_enc_type='DW32', gnpde_generate_pos_enc=1, gnpde_dw_epochs=3, seed=7))
  kw = _FakeDeepWalk.made.pop().kw
  assert (kw['embedding_dim'], kw['epochs'], kw['seed']) == (32, 3, 7)
  assert sorted(os.listdir(tmp_path / 'pos_encodings')) == ['Synthetic_DW32.pkl', 'Synthetic_DW64.pkl']
