"""k-nearest-neighbour rewiring, everything that needs no device: the two symbols and the ABI number in header / library /
bindings / INTEGRATION.md, argument checks of the C entry point, the drop-in's `graph_rewiring`, and the in-test oracle itself
(knn_oracle.py), including the cap on entries the rounding band leaves undetermined."""
import ctypes
import os
import re
import sys
import types

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, dropin
import knn_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_knn', 'gnpde_knn_workspace_bytes')


def test_symbols_and_abi_number_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  declared = set(re.findall(r'\b(gnpde_[a-z_0-9]+)\s*\(', header))
  L = G.lib()
  for name in SYMBOLS:
    assert name in declared, name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name), name + ' is not exported by the library'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 9 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION


def test_integration_doc_names_both_symbols():
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for name in SYMBOLS:
    assert name in doc
  assert 'graph_rewiring.py:120-126' in doc


def test_entry_point_rejects_bad_arguments_before_any_launch():
  """Outside 1 <= k <= min(n, 128) the C entry point returns an error code and a message; nothing touches a device (this
  test runs without one)."""
  L = G.lib()
  x = torch.zeros(10, 4)
  idx = torch.zeros(10, 4, dtype=torch.int64)
  ws = torch.zeros(4096, dtype=torch.uint8)
  call = lambda n, d, ld, k: L.gnpde_knn(_lib.ptr(x), n, d, ld, k, _lib.ptr(idx), None, _lib.ptr(ws), ws.numel(), None)
  assert call(10, 4, 4, 0) == -2 and b'knn' in L.gnpde_last_error()
  assert call(10, 4, 4, 11) == -2
  assert call(1000, 4, 4, 129) == -2
  assert call(10, 4, 3, 2) == -1        # row stride under the width
  assert call(0, 4, 4, 1) == -1
  assert L.gnpde_knn(None, 10, 4, 4, 2, _lib.ptr(idx), None, _lib.ptr(ws), ws.numel(), None) == -1
  assert L.gnpde_knn(_lib.ptr(x), 10, 4, 4, 2, _lib.ptr(idx), None, _lib.ptr(ws), 8, None) == -3
  assert L.gnpde_knn_workspace_bytes(10, 4, 0) == 0 and L.gnpde_knn_workspace_bytes(10, 4, 11) == 0
  assert L.gnpde_knn_workspace_bytes(10, 4, 2) >= 40


def test_column_split_knob_changes_the_workspace():
  """gnpde_tune(19, S): S partial lists of n k keys live in the workspace, S = 1 needs the norms alone."""
  L = G.lib()
  try:
    G.ops.tune(_lib.TUNE_KNN_SPLITS, 1)
    one = L.gnpde_knn_workspace_bytes(5000, 16, 32)
    G.ops.tune(_lib.TUNE_KNN_SPLITS, 3)
    three = L.gnpde_knn_workspace_bytes(5000, 16, 32)
  finally:
    G.ops.tune(_lib.TUNE_KNN_SPLITS, 0)
  assert one < 5000 * 32 * 8 and three >= one + 3 * 5000 * 32 * 8


def test_python_surface_refuses_host_and_double_tensors():
  with pytest.raises(G.GnpdeError):
    G.ops.knn(torch.zeros(8, 3), 2)
  with pytest.raises(G.GnpdeError):
    G.graph_rewiring.KNN(torch.zeros(8, 3), {'rewire_KNN_k': 2, 'rewire_KNN_T': 'raw', 'rewire_KNN_sym': False})


STUB = '''
MARK = 'from the stub'
def KNN(x, opt):
  return 'stub KNN'
def apply_KNN(data, pos_encoding, model, opt):
  return KNN(data, opt)
def unrelated():
  return MARK
'''


@pytest.fixture
def clean_dropin():
  dropin.uninstall()
  saved = list(sys.path)
  yield
  dropin.uninstall()
  sys.path[:] = saved
  sys.modules.pop('graph_rewiring', None)


def test_dropin_serves_graph_rewiring_with_the_native_search(tmp_path, monkeypatch, clean_dropin):
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  served = dropin.install(native_knn=True)
  assert 'graph_rewiring' in served
  import graph_rewiring
  ours = sys.modules['gnpde_amd.graph_rewiring']
  assert graph_rewiring.KNN is ours.KNN
  assert graph_rewiring.unrelated() == 'from the stub' and graph_rewiring.MARK == 'from the stub'
  assert graph_rewiring.__gnpde_reference__ == str(tmp_path / 'graph_rewiring.py')
  # the stub's apply_KNN looks KNN up when it is called: it must reach ours
  seen = []
  monkeypatch.setattr(ours, 'KNN', lambda x, opt: seen.append((x, opt)) or 'native KNN')
  dropin.uninstall()
  dropin.install(native_knn=True)
  import graph_rewiring as again
  assert again.apply_KNN('data', None, None, {'o': 1}) == 'native KNN' and seen == [('data', {'o': 1})]
  dropin.uninstall()
  assert 'graph_rewiring' not in sys.modules and '_reference_graph_rewiring' not in sys.modules
  assert not dropin.installed()


def test_dropin_graph_rewiring_without_a_reference_file_is_ours(clean_dropin):
  dropin.install(native_knn=True)
  import graph_rewiring
  ours = sys.modules['gnpde_amd.graph_rewiring']
  assert graph_rewiring.KNN is ours.KNN and graph_rewiring.apply_KNN is ours.apply_KNN
  assert graph_rewiring.__gnpde_reference__ is None


def test_dropin_without_the_flag_serves_what_it_served(tmp_path, clean_dropin):
  """install() without native_knn: the names of the parent commit, `graph_rewiring` stays the path's own file."""
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  served = dropin.install()
  assert served == sorted(dropin.MODULES) + ['base_classes']
  assert dropin.install(native_gnn=True) == sorted(list(dropin.MODULES) + ['GNN']) + ['base_classes']
  import graph_rewiring
  assert graph_rewiring.KNN(None, None) == 'stub KNN' and not hasattr(graph_rewiring, '__gnpde_reference__')


def test_oracle_orders_by_distance_then_index():
  """Six points on a line, 0 0 1 3 3 -1: distances from point 2 (at 1) are 1 1 0 4 4 4 -> order 2, 0, 1, 3, 4, 5 (ties by
  ascending index); from point 0: 0 0 1 9 9 1 -> 0, 1, 2, 5, 3, 4."""
  x = torch.tensor([[0.], [0.], [1.], [3.], [3.], [-1.]])
  idx, dist = O.knn_oracle(x, 6)
  assert idx[2].tolist() == [2, 0, 1, 3, 4, 5] and dist[2].tolist() == [0, 1, 1, 4, 4, 4]
  assert idx[0].tolist() == [0, 1, 2, 5, 3, 4] and dist[0].tolist() == [0, 0, 1, 1, 9, 9]
  assert idx[3].tolist()[:3] == [3, 4, 2] and idx[4].tolist()[:3] == [3, 4, 2]
  idx2, _ = O.knn_oracle(x, 2)
  assert torch.equal(idx2, idx[:, :2])


@pytest.mark.parametrize('case', range(len(O.REAL_SHAPES)))
def test_band_leaves_few_entries_undetermined(case):
  """The inclusion test of the real-valued cases decides all but <= 1 % of the n k entries (counted on the oracle alone)."""
  n, d, k = O.REAL_SHAPES[case]
  band = O.real_band(case)
  open_ = band.undetermined()
  print('case %s: %d undetermined entries of %d (%.4f %%)' % ((n, d, k), open_, n * k, 100.0 * open_ / (n * k)))
  assert open_ <= O.CAP_SHARE * n * k
  # the oracle's own answer passes the inclusion rule
  band.check(O.knn_oracle(O.real_input(case), k)[0])


def test_to_undirected_matches_a_set_construction():
  ei = torch.tensor([[0, 0, 1, 2, 2, 3], [0, 1, 0, 3, 1, 2]])
  out = G.graph_rewiring.to_undirected(ei, 4)
  want = sorted({(a, b) for a, b in zip(*ei.tolist())} | {(b, a) for a, b in zip(*ei.tolist())})
  assert [tuple(c) for c in out.t().tolist()] == want


def test_gnn_knn_refuses_fa_layer():
  from helpers import Data
  opt = dict(fa_layer=True)
  with pytest.raises(NotImplementedError, match='fa_layer'):
    G.GNN_KNN(opt, G.DummyDataset(Data(torch.zeros(4, 3), torch.zeros(2, 0, dtype=torch.long)), 2), torch.device('cpu'))
