"""Row attention of a GRAND-nl evaluation in ONE launch, the hub rows normalised by the aggregation's chunk items (gnpde_tune(21, .),
csrc/attention.hip row_attention_sd_one_kernel, csrc/spmm.hip HubDefer): bitwise parity with the two-launch form, a complete weight
buffer, replay == eager, and the shapes that keep the two launches.  The launch decision is read from gnpde_one_launch_evaluations()."""
import ctypes
import functools

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops

pytestmark = pytest.mark.gpu

N = 3000
# entries per row, self-loop included: both sides of every class boundary (16 | 17 entries: a quarter of a wave | a wave per row; 32 | 33 and
# 64: passes of the wave-per-row body; 512 | 513: one wave | chunks), two chunks with the second nearly empty (513) and full (1024), three
# chunks (1025), one hub of six
SHORT = [1, 2, 15, 16, 17, 31, 32, 33, 64, 511, 512]
HUBS = [513, 1024, 1025, 2600]
TUNE_ROW_FUSION_NEVER = 2


@functools.lru_cache(maxsize=None)
def _edges(hubs):
  """Seeded edge list: the special rows spread over the id range, every other row 1..16 entries, a self-loop in every row."""
  g = torch.Generator().manual_seed(20 + int(hubs))
  lens = torch.randint(1, 17, (N,), generator=g)
  special = SHORT + (HUBS if hubs else [])
  rows = torch.linspace(5, N - 7, len(special)).long()
  lens[rows] = torch.tensor(special)
  src, dst = [], []
  for i in range(N):
    m = int(lens[i]) - 1
    others = torch.randperm(N - 1, generator=g)[:m]
    others = others + (others >= i).long()          # distinct columns, none of them i
    src.append(torch.full((m + 1,), i))
    dst.append(torch.cat([torch.tensor([i]), others]))
  ei = torch.stack([torch.cat(src), torch.cat(dst)])
  return ei[:, torch.randperm(ei.size(1), generator=g)].long(), lens


@functools.lru_cache(maxsize=None)
def _graph(hubs, dev):
  ei, lens = _edges(hubs)
  graph = G.CSRGraph(ei.to(dev), N)
  assert graph.struct.n_long_rows == (len(HUBS) if hubs else 0)
  assert graph.struct.n_long_chunks == (sum((v + 511) // 512 for v in HUBS) if hubs else 0)
  assert 2 * graph.struct.n_bin16 >= N              # mostly short rows: the row-pair aggregation kernel at d = 68..128
  return graph


def _desc(graph, d, h, A, dev, norm_idx=0, square_plus=False, seed=0):
  g = torch.Generator().manual_seed(100 + seed)
  x = (torch.randn(N, d, generator=g) * 0.5).to(dev)
  W = (torch.randn(2 * A, d, generator=g) / d ** 0.5).to(dev)
  b = (torch.randn(2 * A, generator=g) * 0.1).to(dev)
  transposed = graph.transposed_positions() if norm_idx == 1 else None
  st = ops.attention_struct(_lib.ATT_SCALED_DOT, h, A, norm_idx, square_plus, transposed=transposed)
  alpha, beta = torch.tensor(0.2, device=dev), torch.tensor(0.1, device=dev)
  x0 = x.clone()
  desc = ops.RhsDescriptor(_lib.RHS_TRANSFORMER, graph, d, x.stride(0), alpha, beta, x0, True, proj_w=W, proj_b=b, att=st)
  desc.keep += [st, transposed]
  return desc, x


def _count():
  return int(_lib.lib().gnpde_one_launch_evaluations())


class _Tune(object):
  def __init__(self, *pairs):
    self.pairs = pairs

  def __enter__(self):
    for k, v in self.pairs:
      ops.tune(k, v)

  def __exit__(self, *exc):
    for k, _ in self.pairs:
      ops.tune(k, 0)


def _solve(desc, x, method, two_launches, use_graph=True, gather=None, fusion_off=True):
  """(state after 2 steps, evaluations that took the one-launch form)."""
  pairs = [(_lib.TUNE_ATT_ONE_LAUNCH, 1 if two_launches else 0)]
  if fusion_off:      # a small graph without hub rows would attend inside the aggregation kernel (attn_spmm_kernel): not the subject here
    pairs.append((_lib.TUNE_ROW_FUSION, TUNE_ROW_FUSION_NEVER))
  with _Tune(*pairs):
    s = ops.FixedStepSolver(desc, method, [0.5, 0.25], x.device)
    if gather is not None:
      s.set_gather(gather)
    c0 = _count()
    y = s.run(x.clone(), use_graph=use_graph).clone()
    torch.cuda.synchronize()
    return y, _count() - c0


# the aggregation kernel decides: d = 128 and d = 96 run the row-pair kernel on these graphs (whole and partial last lane group), whose
# hub-chunk items take the deferred weights; d = 256 runs the wide-row kernel, which keeps the two launches
@pytest.mark.parametrize('h,A', [(4, 16), (4, 32), (4, 64), (2, 8)])
@pytest.mark.parametrize('d', [128, 256, 96])
def test_solve_equals_the_two_launch_form_bitwise(dev, d, h, A):
  claims = d in (128, 96)
  for hubs in (True, False):
    graph = _graph(hubs, str(dev))
    desc, x = _desc(graph, d, h, A, dev, seed=d + A)
    for method in ('rk4', 'euler'):
      y1, n1 = _solve(desc, x, method, two_launches=False)
      y2, n2 = _solve(desc, x, method, two_launches=True)
      what = 'd=%d h=%d A=%d hubs=%s %s' % (d, h, A, hubs, method)
      assert n2 == 0, what
      assert (n1 > 0) == claims, '%s: %d evaluations in the one-launch form' % (what, n1)
      assert torch.isfinite(y1).all() and not torch.equal(y1, x), what
      assert torch.equal(y1, y2), '%s: max |diff| %g' % (what, float((y1 - y2).abs().max()))


def test_weight_buffer_is_complete_after_the_aggregation(dev):
  """One evaluation through gnpde_rhs_eval: the [e] head-mean weights in its workspace -- short rows written by the attention launch, hub
  entries by the aggregation's chunk items -- are those of ops.edge_attention on the projection the evaluation wrote, bit for bit."""
  d, h, A = 128, 4, 16
  graph = _graph(True, str(dev))
  desc, x = _desc(graph, d, h, A, dev, seed=7)
  L = _lib.lib()
  off_w = _lib_align(N * 2 * A * 4) + _lib_align(L.gnpde_spmm_workspace_bytes(graph.ref(), d))
  out = {}
  for two in (False, True):
    # (key 14: q||k interleaved [n, 2A] in the workspace, so that the direct call below can be handed the very same projection)
    with _Tune((_lib.TUNE_ATT_ONE_LAUNCH, int(two)), (14, 1)):
      ws = graph.workspace('rhs%d_%d' % (desc.struct.kind, d), L.gnpde_rhs_workspace_bytes(desc.ref()))
      ws.zero_()
      c0 = _count()
      f = ops.rhs_eval(desc, x).clone()
      torch.cuda.synchronize()
      assert _count() - c0 == (0 if two else 1)
      w = ws[off_w:off_w + 4 * graph.e].view(torch.float32).clone()
      qk = ws[:N * 2 * A * 4].view(torch.float32).view(N, 2 * A).clone()
    out[two] = (f, w, qk)
  assert torch.equal(out[False][0], out[True][0]) and torch.equal(out[False][2], out[True][2])
  assert torch.equal(out[False][1], out[True][1])
  qk = out[False][2]
  st = ops.attention_struct(_lib.ATT_SCALED_DOT, h, A, 0, False, q=qk, k=qk[:, A:], ldqk=2 * A)
  c0 = _count()
  w_ref, _, _ = ops.edge_attention(graph, st, like=x)
  torch.cuda.synchronize()
  assert _count() == c0                             # the direct call returns its weights straight away: two launches
  w = out[False][1]
  assert torch.equal(w, w_ref[:graph.e])
  # every row is a softmax: the hub entries were written (the buffer was zeroed) and sum to 1 with the others
  rows = graph.t['rowptr'].long()
  sums = torch.zeros(N, device=dev, dtype=torch.float64).index_add_(0, torch.repeat_interleave(torch.arange(N, device=dev), rows[1:] - rows[:-1]),
                                                                    w.double())
  assert float((sums - 1).abs().max()) < 1e-5


def _lib_align(v, a=256):
  return (int(v) + a - 1) // a * a


def test_replay_equals_eager(dev):
  graph = _graph(True, str(dev))
  desc, x = _desc(graph, 128, 4, 16, dev, seed=3)
  for method in ('rk4', 'euler'):
    eager, n_e = _solve(desc, x, method, two_launches=False, use_graph=False)
    assert n_e > 0
    with _Tune((_lib.TUNE_ROW_FUSION, TUNE_ROW_FUSION_NEVER)):
      s = ops.FixedStepSolver(desc, method, [0.5, 0.25], dev)
      c0 = _count()
      g1 = s.run(x.clone(), use_graph=True).clone()
      g2 = s.run(x.clone(), use_graph=True).clone()       # the captured graph replayed: nothing of the first solve may be left in the partials
      assert _count() > c0
    assert torch.equal(eager, g1) and torch.equal(eager, g2), method


@pytest.mark.parametrize('case', ['squareplus', 'norm_idx1', 'bf16', 'small_graph_row_fusion'])
def test_other_modes_keep_their_launches(dev, case):
  """Squareplus, the column normaliser, the bf16 gather operand and the attention inside the aggregation kernel (small graphs without hub
  rows) never take the one-launch form: the key changes nothing."""
  hubs = case != 'small_graph_row_fusion'
  graph = _graph(hubs, str(dev))
  desc, x = _desc(graph, 128, 4, 16, dev, norm_idx=1 if case == 'norm_idx1' else 0, square_plus=case == 'squareplus', seed=11)
  kw = dict(gather='bf16') if case == 'bf16' else {}
  if case == 'small_graph_row_fusion':
    kw['fusion_off'] = False
  y1, n1 = _solve(desc, x, 'rk4', two_launches=False, **kw)
  y2, n2 = _solve(desc, x, 'rk4', two_launches=True, **kw)
  assert n1 == 0 and n2 == 0
  assert torch.isfinite(y1).all() and torch.equal(y1, y2)
