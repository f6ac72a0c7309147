"""Hub rows of the row-pair aggregation folded INSIDE the aggregation launch by the last chunk item of each row to arrive (csrc/spmm.hip
fold_ticket / fold_long_row): every result is compared bit for bit with the same call under gnpde_agg_fold_launch(1), which keeps
spmm_long_reduce4_kernel in a launch of its own.  The launch decision is read from gnpde_in_kernel_fold_launches()."""
import functools

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops

pytestmark = pytest.mark.gpu

N = 4096
# entries of the three hub rows: two chunks with a one-entry second chunk, exactly two full chunks, ten chunks (the fold's eight-at-a-time loop
# and its remainder)
HUBS = [513, 1024, 4609]
TUNE_ROW_FUSION_NEVER = 2


def _make_edges(n, hub_lens, seed, hub_is_frequent_column):
  """Seeded edge list: every row 1..16 entries but the hub rows (spread over the id range); distinct columns in a row, a self-loop in every
  row.  hub_is_frequent_column: the first hub row is also the column of one row in two."""
  g = torch.Generator().manual_seed(seed)
  rows = torch.linspace(7, n - 9, len(hub_lens)).long()
  hot = int(rows[0])
  is_hub = torch.zeros(n, dtype=torch.bool)
  is_hub[rows] = True
  # short rows: the self-loop, up to 14 random columns (duplicates are dropped below) and, for one row in two, the frequent column
  extra = torch.randint(0, 15, (n,), generator=g)
  extra[is_hub] = 0
  src = [torch.arange(n), torch.repeat_interleave(torch.arange(n), extra)]
  dst = [torch.arange(n), torch.randint(0, n, (int(extra.sum()),), generator=g)]
  if hub_is_frequent_column:
    even = torch.arange(0, n, 2)
    even = even[~is_hub[even]]
    src.append(even)
    dst.append(torch.full_like(even, hot))
  key = torch.unique(torch.cat(src) * n + torch.cat(dst))
  src, dst = [key // n], [key % n]
  # hub rows: exactly the given number of entries, the row itself among them (a row may be longer than n: columns repeat, as multi-edges do)
  for r, m in zip(rows.tolist(), hub_lens):
    src.append(torch.full((m - 1,), r))
    dst.append(torch.randint(0, n, (m - 1,), generator=g))
  ei = torch.stack([torch.cat(src), torch.cat(dst)])
  lens = torch.bincount(ei[0], minlength=n)
  assert lens[rows].tolist() == list(hub_lens) and int(lens[~is_hub].max()) <= 16 and int(lens.min()) >= 1
  return ei[:, torch.randperm(ei.size(1), generator=g)].long(), rows


@functools.lru_cache(maxsize=None)
def _graph(dev):
  ei, rows = _make_edges(N, HUBS, 31, True)
  graph = G.CSRGraph(ei.to(dev), N)
  assert graph.struct.n_long_rows == len(HUBS)
  assert graph.struct.n_long_chunks == sum((v + 511) // 512 for v in HUBS) == 14
  assert 2 * graph.struct.n_bin16 >= N              # mostly short rows: the row-pair kernel at d = 68..128
  return graph, rows


def _folds():
  return int(_lib.lib().gnpde_in_kernel_fold_launches())


AGG_FOLD = 'agg_fold_launch'      # not a gnpde_tune key: ops.agg_fold_launch(1) keeps the fold launch


def _set(key, value):
  if key == AGG_FOLD:
    ops.agg_fold_launch(value)
  else:
    ops.tune(key, value)


class _Tune(object):
  def __init__(self, *pairs):
    self.pairs = pairs

  def __enter__(self):
    for k, v in self.pairs:
      _set(k, v)

  def __exit__(self, *exc):
    for k, _ in self.pairs:
      _set(k, 0)


def _tickets(graph, dev):
  nbytes = int(_lib.lib().gnpde_spmm_ticket_bytes(graph.ref()))
  assert nbytes == 4 * graph.struct.n_long_rows
  return torch.zeros(max(nbytes // 4, 1), dtype=torch.int32, device=dev)


@functools.lru_cache(maxsize=None)
def _operands(d, dev, other=False):
  """other: a second set (other state, other weights), so that a launch with it leaves OTHER partials in the graph's cached workspace."""
  g = torch.Generator().manual_seed(500 + d + (1000 if other else 0))
  graph, _ = _graph(dev)
  mk = lambda: (torch.randn(N, d, generator=g) * 0.5).to(dev)
  w = (torch.rand(graph.e, generator=g) / 8).to(dev)
  return dict(w=w, u=mk(), x0=mk(), y=mk(), k1=mk())


STAGES = ['RK1C', 'RK2C', 'RK3C', 'RK4C', 'EULER']


def _stage_call(graph, t, stage, with_x0, in_place, tickets, dev, sync=True):
  """One aggregation launch with the stage's epilogue; returns out_y."""
  y = t['y'].clone()
  out = y if in_place else torch.full_like(y, float('nan'))
  kw = dict(stage=getattr(_lib, 'STAGE_' + stage), dt=0.37, out_y=out)
  if stage in ('EULER', 'RK2C', 'RK4C'):
    kw['y'] = y
  if stage in ('RK3C', 'RK4C'):
    kw['k1'] = t['k1']
  alpha, beta = torch.tensor(0.3, device=dev), torch.tensor(0.2, device=dev)
  ops.spmm_rhs(graph, t['w'], t['u'], alpha, beta if with_x0 else None, t['x0'] if with_x0 else None, tickets=tickets, **kw)
  if sync:
    torch.cuda.synchronize()
  return out


@pytest.mark.parametrize('d', [128, 96])
def test_every_stage_equals_the_fold_launch_bitwise(dev, d):
  """The partials live in a workspace the graph caches per width, and depend on (u, w) alone: between the reference and the launch under
  test a launch with ANOTHER state and other weights runs (fold-launch form: plain stores), with no synchronisation before the launch
  under test -- a consumer that read a partial too early or from a stale line would find the other set's value, not its own from before."""
  graph, hub_rows = _graph(str(dev))
  t, t_other = _operands(d, str(dev)), _operands(d, str(dev), other=True)
  tickets = _tickets(graph, dev)
  cases = [(s, x0, False) for s in STAGES for x0 in (True, False)] + [('RK4C', True, True), ('RK4C', False, True)]
  for stage, with_x0, in_place in cases:
    what = 'd=%d %s x0=%s in_place=%s' % (d, stage, with_x0, in_place)
    with _Tune((AGG_FOLD, 1)):
      c0 = _folds()
      ref = _stage_call(graph, t, stage, with_x0, in_place, tickets, dev)
      assert _folds() == c0, what
    with _Tune((AGG_FOLD, 1)):
      other = _stage_call(graph, t_other, stage, with_x0, False, tickets, dev, sync=False)
    c0 = _folds()
    got = _stage_call(graph, t, stage, with_x0, in_place, tickets, dev)
    assert _folds() == c0 + 1, what
    assert torch.isfinite(ref).all() and torch.isfinite(other).all(), what
    assert not any(torch.equal(other[r], ref[r]) for r in hub_rows.tolist()), what       # the other set's hub rows ARE other values
    assert torch.equal(got, ref), '%s: max |diff| %g, hub rows %s' % (what, float((got - ref).abs().max()),
                                                                      [bool(torch.equal(got[r], ref[r])) for r in hub_rows.tolist()])
    assert int(tickets.abs().sum()) == 0, what      # every last arriver put its ticket back


def _desc(graph, d, h, A, dev, seed=0):
  g = torch.Generator().manual_seed(100 + seed)
  x = (torch.randn(N, d, generator=g) * 0.5).to(dev)
  W = (torch.randn(2 * A, d, generator=g) / d ** 0.5).to(dev)
  b = (torch.randn(2 * A, generator=g) * 0.1).to(dev)
  st = ops.attention_struct(_lib.ATT_SCALED_DOT, h, A, 0, False)
  alpha, beta = torch.tensor(0.2, device=dev), torch.tensor(0.1, device=dev)
  desc = ops.RhsDescriptor(_lib.RHS_TRANSFORMER, graph, d, x.stride(0), alpha, beta, x.clone(), True, proj_w=W, proj_b=b, att=st)
  desc.keep += [st]
  return desc, x


STEPS = [0.5, 0.25, 0.25]


def _solve(desc, x, method, fold_launch, use_graph, replays=1):
  """(states after a solve of 3 steps: one per run of the same solver, launches folded in the kernel, one-launch attention evaluations).
  Every run integrates the SAME buffer in place (refilled from x), so a captured solve is captured once and replayed after that."""
  with _Tune((AGG_FOLD, 1 if fold_launch else 0), (_lib.TUNE_ROW_FUSION, TUNE_ROW_FUSION_NEVER)):
    s = ops.FixedStepSolver(desc, method, STEPS, x.device)
    c0, a0 = _folds(), int(_lib.lib().gnpde_one_launch_evaluations())
    y = torch.empty_like(x)
    ys = []
    for _ in range(replays):
      y.copy_(x)
      ys.append(s.run(y, use_graph=use_graph).clone())
    torch.cuda.synchronize()
    return ys, _folds() - c0, int(_lib.lib().gnpde_one_launch_evaluations()) - a0


@pytest.mark.parametrize('d', [128, 96])
def test_deferred_hub_weights_solve_equals_the_fold_launch_bitwise(dev, d):
  """(h, A) = (4, 16): the chunk items also form their entries' weights (DEFER instantiation of the row-pair kernel)."""
  graph, _ = _graph(str(dev))
  desc, x = _desc(graph, d, 4, 16, dev, seed=d)
  for method, evals in (('rk4', 12), ('euler', 3)):
    (ref,), n_ref, one_ref = _solve(desc, x, method, True, True)
    (got,), n_got, one_got = _solve(desc, x, method, False, True)
    assert n_ref == 0 and n_got == evals, (method, n_ref, n_got)       # the fold launch was not taken, in any evaluation
    assert one_ref == evals and one_got == evals, (method, one_ref, one_got)
    assert torch.isfinite(ref).all() and not torch.equal(ref, x)
    assert torch.equal(got, ref), '%s d=%d: max |diff| %g' % (method, d, float((got - ref).abs().max()))


def test_twenty_replays_equal_eager(dev):
  """One capture, nineteen replays of it (the launch counter moves at enqueue time only: 12 / 3 launches for 20 runs).  The memset node
  zeroes the tickets in every replay; that the last arrivers put them back is what the back-to-back launches below rely on."""
  graph, _ = _graph(str(dev))
  desc, x = _desc(graph, 128, 4, 16, dev, seed=3)
  for method, evals in (('rk4', 12), ('euler', 3)):
    (eager,), n_e, _ = _solve(desc, x, method, False, False)
    (ref,), n_r, _ = _solve(desc, x, method, True, False)
    assert n_e > 0 and n_r == 0 and torch.equal(eager, ref)
    ys, n_g, _ = _solve(desc, x, method, False, True, replays=20)
    assert len(ys) == 20 and n_g == evals, (method, n_g)                # captured once: every later run replayed the graph
    for i, y in enumerate(ys):
      assert torch.equal(y, eager), '%s replay %d: max |diff| %g' % (method, i, float((y - eager).abs().max()))


def test_routes_that_keep_the_fold_launch(dev):
  """The wide-row kernel (d = 256) and the plain aggregation keep spmm_long_reduce4_kernel, tickets or not, and their results."""
  graph, _ = _graph(str(dev))
  tickets = _tickets(graph, dev)
  t = _operands(256, str(dev))
  outs = []
  for tk, knob in ((tickets, 0), (None, 0), (tickets, 1)):
    with _Tune((AGG_FOLD, knob)):
      c0 = _folds()
      outs.append(_stage_call(graph, t, 'RK4C', True, False, tk, dev))
      assert _folds() == c0
  assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
  assert int(tickets.abs().sum()) == 0
  t = _operands(128, str(dev))
  plain = []
  for knob in (0, 1):
    with _Tune((AGG_FOLD, knob)):
      c0 = _folds()
      plain.append(ops.spmm(graph, t['w'], t['u']).clone())
      torch.cuda.synchronize()
      assert _folds() == c0
  assert torch.equal(plain[0], plain[1])
  # the plain aggregation is the sum the stages build on: against float64 on the hub rows (entries of one sign scale: 4609 products of
  # |w| <= 1/8 and |u| ~ 0.5 summed in fp32 in a fixed order, error <= 4609 * 2^-24 * sum |w u| ~ 1e-2 at the very worst; seen far smaller)
  rowptr, col = graph.t['rowptr'].long(), graph.t['colidx'].long()
  for r in _graph(str(dev))[1].tolist():
    e0, e1 = int(rowptr[r]), int(rowptr[r + 1])
    ref = (t['w'][e0:e1].double()[:, None] * t['u'][col[e0:e1]].double()).sum(0)
    assert float((plain[0][r].double() - ref).abs().max()) < 1e-3


# ---- the hand-off under uneven load -------------------------------------------------------------------------------------------------

N_BIG, HUBS_BIG, LAUNCHES = 16384, 256, 100


@functools.lru_cache(maxsize=None)
def _big_graph(dev):
  g = torch.Generator().manual_seed(77)
  hub_lens = torch.randint(513, 4097, (HUBS_BIG,), generator=g).tolist()
  ei, rows = _make_edges(N_BIG, hub_lens, 78, False)
  graph = G.CSRGraph(ei.to(dev), N_BIG)
  assert graph.struct.n_long_rows == HUBS_BIG and 2 * graph.struct.n_bin16 >= N_BIG
  return graph, rows


def test_hand_off_under_uneven_load_every_word(dev):
  """256 hub rows of 513..4096 entries (2..8 chunks, arriving at very different times) among 16 128 rows of 1..16 entries; 100 launches back
  to back on one stream with nothing between them, each into its own slice of one buffer.  The launches ALTERNATE between two operand sets
  (state, source and weights), so the partial buffer -- one per graph and width, shared by all of them -- holds the OTHER set's partials
  when a launch starts, and the L1 / L2 of the consumers are warm with those lines: a partial read before its producer published it, a
  stale line, or a fold started early on a ticket that was not put back gives a wrong hub row, which the same values left by the
  previous launch would hide.  Every word of every launch is compared with the fold launch's result for its set."""
  d = 128
  graph, rows = _big_graph(str(dev))
  rows = rows.to(dev)
  g = torch.Generator().manual_seed(79)
  alpha, beta = torch.tensor(0.3, device=dev), torch.tensor(0.2, device=dev)
  tickets = _tickets(graph, dev)
  sets, refs = [], []
  for _ in range(2):
    u = (torch.randn(N_BIG, d, generator=g) * 0.5).to(dev)
    x0 = (torch.randn(N_BIG, d, generator=g) * 0.5).to(dev)
    w = (torch.rand(graph.e, generator=g) / 8).to(dev)
    sets.append((u, x0, w))
    with _Tune((AGG_FOLD, 1)):
      ref = torch.empty(N_BIG, d, device=dev)
      ops.spmm_rhs(graph, w, u, alpha, beta, x0, out=ref, tickets=tickets)
      torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    refs.append(ref)
  assert int((refs[0][rows] == refs[1][rows]).sum()) <= 4               # (random floats: all but a chance few of the 32 768 hub words differ)
  outs = torch.full((LAUNCHES, N_BIG, d), float('nan'), device=dev)
  c0 = _folds()
  for i in range(LAUNCHES):
    u, x0, w = sets[i % 2]
    ops.spmm_rhs(graph, w, u, alpha, beta, x0, out=outs[i], tickets=tickets)
  torch.cuda.synchronize()
  assert _folds() == c0 + LAUNCHES
  for k in range(2):
    got, ref = outs[k::2], refs[k]
    bad = (got[:, rows] != ref[rows][None]).sum(dim=(1, 2))             # NaN != anything: an unwritten word counts
    assert int(bad.sum()) == 0, 'set %d: mismatching hub words per launch: %s' % (k, bad.nonzero().flatten().tolist()[:20])
    assert int((got != ref[None]).sum()) == 0                           # ... and every other row
  assert int(tickets.abs().sum()) == 0
