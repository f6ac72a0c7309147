"""Edge-sampling rewiring and the fully-adjacent layer, everything that needs no device: the in-test oracle itself
(edge_sampling_oracle.py: the Philox known answers, union / selection against set constructions, the share of draws its band
leaves open, the clearance of the model test's threshold), the option table of graph_rewiring (what is accepted, what is refused
and with which words), the ABI number, the drop-in's new flag, and the device errors of the new entry points."""
import os
import re
import sys

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, dropin, graph_rewiring as GR
import edge_sampling_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_philox_words', 'gnpde_random_nodes', 'gnpde_node_importance', 'gnpde_sample_nodes', 'gnpde_sample_nodes_workspace_bytes',
           'gnpde_edge_union', 'gnpde_edge_union_workspace_bytes', 'gnpde_select_edges', 'gnpde_select_edges_workspace_bytes',
           'gnpde_full_adjacency')
CPU = torch.device('cpu')


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', range(3))
def test_oracle_passes_the_philox_known_answers(case):
  counter, key, want = O.KNOWN_ANSWERS[case]
  assert O.known_answer(counter, key) == want


def test_oracle_word_layout():
  """Word i of a stream is word i & 3 of block i >> 2; the key is the seed's two words, the counter (block, stream, call)."""
  seed = (0x299f31d0 << 32) | 0xa4093822
  w = O.words(seed, 0x13198a2e, 0x03707344, (0x85a308d3 << 32) | 0x243f6a88, 6)
  assert tuple(int(v) for v in w[:4]) == O.KNOWN_ANSWERS[2][2]
  nxt = O.known_answer((0x243f6a89, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
  assert (int(w[4]), int(w[5])) == nxt[:2]
  assert not (O.words(1, 0, 0, 0, 8) == O.words(1, 1, 0, 0, 8)).all() and not (O.words(1, 0, 0, 0, 8) == O.words(1, 0, 1, 0, 8)).all()


def test_oracle_random_nodes_stay_in_range():
  for n in (1, 2, 3, 1000, 2 ** 31 - 1):
    v = O.random_nodes(n, 1000, 5, 0, 0)
    assert int(v.min()) >= 0 and int(v.max()) < n
  assert int(O.random_nodes(2 ** 31 - 1, 1000, 5, 0, 0).max()) > 2 ** 30


# five nodes; duplicates inside a ((0,1) twice), inside b ((3,4) twice) and across both ((2,2), (0,1))
A5 = torch.tensor([[0, 4, 0, 2, 1], [1, 0, 1, 2, 3]])
B5 = torch.tensor([[3, 2, 3, 0, 4], [4, 2, 4, 1, 4]])


def test_oracle_union_and_selection_match_set_constructions():
  want = sorted(set(zip(*A5.tolist())) | set(zip(*B5.tolist())))
  assert [tuple(c) for c in O.edge_union(A5, B5).t().tolist()] == want and len(want) == 6
  score = torch.tensor([0.25, 0.5, 0.25, 1.0, 0.125])
  kept, thr = O.select_edges(A5, score, 0.5)
  assert float(thr) == 0.25                                   # the median; two scores tie with it and stay
  assert [tuple(c) for c in kept.t().tolist()] == [c for c, s in zip(zip(*A5.tolist()), score.tolist()) if s >= 0.25]
  assert kept.shape[1] == 4
  assert [tuple(c) for c in O.to_undirected(A5).t().tolist()] == sorted(set(zip(*A5.tolist())) | set(zip(*A5.flip(0).tolist())))
  assert torch.equal(O.full_adjacency(3), torch.tensor([[0, 0, 0, 1, 1, 1, 2, 2, 2], [0, 1, 2, 0, 1, 2, 0, 1, 2]]))


def test_oracle_multinomial_exact_weights():
  """Logits from {0, -200}: weights exactly 2^32 or 0, so a node of weight 0 is never drawn and the draw is uniform over the
  others."""
  logits = torch.tensor([0.0, -200.0] * 32 + [0.0])
  w, _ = O.logit_weights(logits.numpy())
  assert set(w) == {0, 2 ** 32}
  draws = O.sample_nodes(logits.numpy(), 10000, 9, 0, 0)
  assert int((draws % 2).sum()) == 0 and len(set(draws.tolist())) == 33


@pytest.mark.parametrize('case', range(len(O.REAL_CASES)))
def test_band_leaves_few_draws_undetermined(case):
  band = O.real_band(case)
  open_ = band.undetermined()
  print('case %s: %d undetermined draws of %d' % (O.REAL_CASES[case], open_, O.REAL_DRAWS))
  assert open_ <= O.CAP_SHARE * O.REAL_DRAWS
  band.check(O.sample_nodes(O.real_logits(case).numpy(), O.REAL_DRAWS, *O.REAL_STREAM))


CLEARANCE_CASES = [dict(edge_sampling_sym=False), dict(edge_sampling_sym=True)] + [
  dict(function=fn, edge_sampling_seed=seed, **O.E2E_FIRST_SOLVE) for fn, seed in sorted(O.E2E_SEEDS.items())]


@pytest.mark.parametrize('case', CLEARANCE_CASES, ids=lambda c: '-'.join('%s' % v for v in c.values()))
def test_model_threshold_stands_clear_of_every_mean_attention(case):
  """The kept sets of the GPU model tests (edge_sampling on a model: rk4 first solve, with and without sym; GNN_FA end to end:
  euler first solve, both functions) are decided by comparisons with the quantile: on the oracle, no mean attention lies within
  MARGIN (ten times the attention tests' tolerance, relative to the largest) of it."""
  model, data, opt = O.make_model(CPU, edge_sampling_rmv=0.32, **case)
  model.eval()
  first = model.odeblock.odefunc.edge_index
  M = int(first.shape[1] * opt['edge_sampling_add'])
  added = O.edge_union(first, O.random_pairs(O.N, M, opt['edge_sampling_seed'], 0))
  res = O.restated_forward(model, data.x, first, added)
  clearance = O.threshold_clearance(res['mean_att'], res['threshold'])
  print('clearance %.3e (margin %.1e), kept %d of %d' % (clearance, O.MARGIN, res['kept'].shape[1], added.shape[1]))
  assert clearance > O.MARGIN
  assert 0 < res['kept'].shape[1] < added.shape[1]


# ---- the option table -----------------------------------------------------------------------------------------------------------
class _Block(object):
  def __init__(self):
    self.odefunc = type('F', (), {'edge_index': torch.zeros(2, 10, dtype=torch.int64), 'attention_weights': None})()
    self.reg_odefunc = type('R', (), {'odefunc': type('F', (), {'edge_index': None})()})()


class _Model(object):
  """What graph_rewiring reads on a model."""

  def __init__(self, **opt):
    self.opt = dict(block='attention', function='laplacian', reweight_attention=False)
    self.opt.update(opt)
    self.num_nodes, self.device, self.odeblock = 5, CPU, _Block()


def sampling_opt(**over):
  opt = dict(edge_sampling_add_type='random', edge_sampling_add=0.64, edge_sampling_rmv=0.32, edge_sampling_sym=False,
             edge_sampling_space='attention', edge_sampling_T='T0')
  opt.update(over)
  return opt


@pytest.mark.parametrize('kind', ['random', 'importance', 'n2_radius'])
@pytest.mark.parametrize('block,function,rmv', [('attention', 'laplacian', 0.32), ('attention', 'transformer', 0.32),
                                                ('attention', 'laplacian', 0), ('constant', 'transformer', 0)])
def test_supported_options_are_accepted(kind, block, function, rmv):
  GR.check_edge_sampling_supported(_Model(block=block, function=function), sampling_opt(edge_sampling_add_type=kind, edge_sampling_rmv=rmv))


@pytest.mark.parametrize('kind', ['anchored', 'degree'])
def test_broken_add_types_are_refused(kind):
  with pytest.raises(NotImplementedError, match=kind + ".*reference's add_edges crashes"):
    GR.add_edges(_Model(), sampling_opt(edge_sampling_add_type=kind))
  with pytest.raises(ValueError, match='edge_sampling_add_type'):
    GR.add_edges(_Model(), sampling_opt(edge_sampling_add_type='elsewhere'))


@pytest.mark.parametrize('space', ['pos_distance', 'z_distance', 'pos_distance_QK', 'z_distance_QK'])
def test_distance_spaces_are_refused(space):
  with pytest.raises(NotImplementedError, match=space + '.*SpGraphTransAttentionLayer does not have'):
    GR.edge_sampling(_Model(), None, sampling_opt(edge_sampling_space=space))


def test_options_with_arrays_of_the_old_length_are_refused():
  with pytest.raises(NotImplementedError, match='reweight_attention.*edge_weights keep the length'):
    GR.add_edges(_Model(reweight_attention=True), sampling_opt())
  with pytest.raises(NotImplementedError, match="'laplacian' on block 'constant'.*edge_weight"):
    GR.add_edges(_Model(block='constant', function='laplacian'), sampling_opt())


@pytest.mark.parametrize('block', ['constant', 'hard_attention', 'rewire_attention'])
def test_removal_needs_a_fitting_get_attention_weights(block):
  with pytest.raises(NotImplementedError, match='get_attention_weights reads odefunc.edge_index.*%s' % block):
    GR.edge_sampling(_Model(block=block, function='transformer'), None, sampling_opt())
  # adding alone is not refused on the grounds of the block
  GR.check_edge_sampling_supported(_Model(block=block, function='transformer'), sampling_opt(edge_sampling_rmv=0))


@pytest.mark.parametrize('rmv', [0, 0.32])
def test_mixed_block_is_refused(rmv):
  """MixedODEblock adds odefunc.edge_weight, of the original length, to the attention of the changed edge set."""
  with pytest.raises(NotImplementedError, match="block 'mixed'.*edge_weight keeps the length"):
    GR.add_edges(_Model(block='mixed'), sampling_opt(edge_sampling_rmv=rmv))
  with pytest.raises(NotImplementedError, match="block 'mixed'"):
    GR.check_edge_sampling_supported(_Model(block='mixed'), sampling_opt(edge_sampling_rmv=rmv))


def test_importance_without_new_edges_returns_the_tensor_itself():
  m = _Model()
  assert GR.add_edges(m, sampling_opt(edge_sampling_add_type='importance', edge_sampling_add=0.0)) is m.odeblock.odefunc.edge_index


def test_set_edge_index_keeps_the_regularised_twin_in_step():
  m = _Model()
  ei = torch.zeros(2, 3, dtype=torch.int64)
  assert GR.set_edge_index(m, ei) is ei and m.odeblock.odefunc.edge_index is ei and m.odeblock.reg_odefunc.odefunc.edge_index is ei


def test_seed_is_read_once_and_calls_count_up():
  m = _Model(edge_sampling_seed=77)
  assert GR._sampling_stream(m) == (77, 0)
  m.opt['edge_sampling_seed'] = 78
  assert GR._sampling_stream(m) == (77, 1) and GR._sampling_stream(m) == (77, 2)
  assert GR._sampling_stream(_Model())[0] == torch.initial_seed()


# ---- argument checks of the Python surface (no launch) --------------------------------------------------------------------------
def test_negative_counts_and_ranges_are_refused():
  with pytest.raises(G.GnpdeError, match='count = -1 is negative'):
    G.ops.random_nodes(10, -1, 0, 0, 0)
  with pytest.raises(G.GnpdeError, match='count = -3 is negative'):
    G.ops.philox_words(0, 0, 0, 0, -3)
  with pytest.raises(G.GnpdeError, match='outside 1 .. INT32_MAX'):
    G.ops.random_nodes(0, 4, 0, 0, 0)
  with pytest.raises(G.GnpdeError, match='outside 1 .. INT32_MAX'):
    G.ops.random_nodes(2 ** 31, 4, 0, 0, 0)
  with pytest.raises(G.GnpdeError, match='stream'):
    G.ops.random_nodes(10, 4, 0, 2 ** 32, 0)
  with pytest.raises(G.GnpdeError, match='edge positions are int32'):
    G.ops.full_adjacency(46341)


def test_python_surface_refuses_host_tensors():
  ei = torch.zeros(2, 4, dtype=torch.int64)
  f = torch.zeros(4)
  for call in (lambda: G.ops.node_importance(ei, f, 3), lambda: G.ops.sample_nodes(f, 2, 0, 0, 0), lambda: G.ops.edge_union(ei, ei, 3),
               lambda: G.ops.select_edges(ei, f, 0.5), lambda: G.ops.full_adjacency(3, device='cpu'),
               lambda: G.ops.random_nodes(3, 2, 0, 0, 0, device='cpu'), lambda: G.ops.philox_words(0, 0, 0, 0, 4, device='cpu')):
    with pytest.raises(G.GnpdeError, match='HIP device'):
      call()


def test_entry_points_reject_bad_arguments_before_any_launch():
  L = G.lib()
  buf = torch.zeros(64, dtype=torch.int64)
  p = _lib.ptr(buf)
  assert L.gnpde_random_nodes(0, 4, 0, 0, 0, p, None) == -1 and b'random_nodes' in L.gnpde_last_error()
  assert L.gnpde_random_nodes(5, -1, 0, 0, 0, p, None) == -1
  assert L.gnpde_random_nodes(5, 0, 0, 0, 0, None, None) == 0                # nothing to draw: no launch, no error
  assert L.gnpde_philox_words(0, 0, 0, 0, -1, p, None) == -1
  assert L.gnpde_philox_words(0, 0, 0, 0, 0, None, None) == 0
  assert L.gnpde_sample_nodes(p, 0, 4, 0, 0, 0, p, p, p, 512, None) == -1
  # the workspace includes the scan's / sort's own temporary storage, whose size query needs a device: without one the size
  # is reported as 0 and the entry point says so (GNPDE_ESTATE) instead of accepting a workspace that is too small
  assert L.gnpde_sample_nodes_workspace_bytes(0) == 0 and L.gnpde_edge_union_workspace_bytes(-1, 0) == 0
  need = L.gnpde_sample_nodes_workspace_bytes(1000)
  rc = L.gnpde_sample_nodes(p, 8, 4, 0, 0, 0, p, p, p, 8, None)
  if need == 0:
    assert rc == -4 and b'sample_nodes' in L.gnpde_last_error() and b'query failed' in L.gnpde_last_error()
  else:
    assert need >= 16000 and rc == -3 and b'sample_nodes' in L.gnpde_last_error()
  assert L.gnpde_edge_union(p, -1, p, 2, 5, p, p, p, p, 512, None) == -1
  need = L.gnpde_edge_union_workspace_bytes(1000, 24)
  rc = L.gnpde_edge_union(p, 2, p, 2, 5, p, p, p, p, 8, None)
  if need == 0:
    assert rc == -4 and b'edge_union' in L.gnpde_last_error() and b'query failed' in L.gnpde_last_error()
  else:
    assert need >= 3 * 8 * 1024 and rc == -3
  assert L.gnpde_select_edges(p, p, -1, p, p, p, p, 512, None) == -1
  assert L.gnpde_select_edges(p, p, 100000, p, p, p, p, 4, None) == -3
  assert L.gnpde_full_adjacency(0, p, None) == -1
  assert L.gnpde_node_importance(None, p, p, p, None) == -1


# ---- ABI, drop-in, classes ------------------------------------------------------------------------------------------------------
def test_symbols_and_abi_number_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  declared = set(re.findall(r'\b(gnpde_[a-z_0-9]+)\s*\(', header))
  L = G.lib()
  for name in SYMBOLS:
    assert name in declared, name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name), name + ' is not exported by the library'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 13 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION


def test_integration_doc_names_the_symbols_and_the_flag():
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for name in SYMBOLS + ('--native-edge-sampling', 'GNN_FA'):
    assert name in doc, name


STUB = '''
MARK = 'from the stub'
def add_edges(model, opt):
  return 'stub add_edges'
def edge_sampling(model, z, opt):
  return 'stub edge_sampling'
def unrelated():
  return MARK
'''
NAMES = ('add_edges', 'add_outgoing_attention_edges', 'edge_sampling', 'apply_edge_sampling')


@pytest.fixture
def clean_dropin():
  dropin.uninstall()
  saved = list(sys.path)
  yield
  dropin.uninstall()
  sys.path[:] = saved
  for name in ('graph_rewiring', 'GNN_KNN'):
    sys.modules.pop(name, None)


def test_dropin_serves_the_four_functions_and_the_class(tmp_path, clean_dropin):
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  served = dropin.install(native_edge_sampling=True)
  assert 'graph_rewiring' in served and 'GNN_KNN' in served
  import graph_rewiring
  import GNN_KNN
  for name in NAMES:
    assert getattr(graph_rewiring, name) is getattr(GR, name), name
  assert graph_rewiring.unrelated() == 'from the stub'
  assert GNN_KNN.GNN_KNN is G.GNN_FA
  dropin.uninstall()
  assert 'GNN_KNN' not in sys.modules and 'graph_rewiring' not in sys.modules


def test_dropin_flags_compose(clean_dropin):
  dropin.install(native_knn=True, native_gdc=True, native_posdist=True, native_edge_sampling=True)
  import graph_rewiring
  for name in NAMES + ('KNN', 'apply_gdc', 'GDCWrapper', 'apply_pos_dist_rewire'):
    assert getattr(graph_rewiring, name) is getattr(GR, name), name


def test_dropin_without_the_flag_leaves_the_names_alone(tmp_path, clean_dropin):
  (tmp_path / 'graph_rewiring.py').write_text(STUB)
  sys.path.insert(0, str(tmp_path))
  served = dropin.install(native_knn=True)
  assert 'GNN_KNN' not in served and 'GNN_KNN' not in sys.modules
  import graph_rewiring
  assert graph_rewiring.add_edges(None, None) == 'stub add_edges' and graph_rewiring.edge_sampling(None, None, None) == 'stub edge_sampling'
  assert not hasattr(graph_rewiring, 'apply_edge_sampling')
  dropin.uninstall()
  assert dropin.install() == sorted(dropin.MODULES) + ['base_classes']


def test_dropin_usage_names_every_flag():
  with pytest.raises(SystemExit) as info:
    dropin.main(['--no-such-flag'])
  for flag in ('--native-gnn', '--native-knn', '--native-gdc', '--native-posdist', '--native-edge-sampling'):
    assert flag in str(info.value)


def test_gnn_knn_still_refuses_fa_layer_and_points_at_gnn_fa():
  from helpers import Data
  dataset = G.DummyDataset(Data(torch.zeros(4, 3), torch.zeros(2, 0, dtype=torch.long)), 2)
  with pytest.raises(NotImplementedError, match='fa_layer.*GNN_FA'):
    G.GNN_KNN(dict(fa_layer=True), dataset, CPU)
  assert issubclass(G.GNN_FA, G.GNN_KNN)


def test_gnn_fa_on_cpu_tensors_fails_with_the_device_error():
  model, data, opt = O.make_model(CPU)
  model.eval()
  with pytest.raises(G.GnpdeError, match='HIP device'):
    model(data.x, None)
  with pytest.raises(G.GnpdeError, match='HIP device'):
    model.forward_ODE(data.x, None)
  with pytest.raises(G.GnpdeError, match='HIP device'):
    GR.add_edges(model, opt)
  assert model.odeblock.odefunc.edge_index is not None and opt['method'] == 'rk4' and opt['time'] == 2.0
