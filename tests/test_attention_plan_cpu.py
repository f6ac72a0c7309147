"""The row attention's launch plan (gnpde_attention_plan, plan_attention in csrc/attention.hip): which route, template line of the row
kernels, sweeps, grids and hub handling a call takes -- the decision launch_planned carries out, asked without a device.
tests/test_attention_dispatch_gpu.py runs every line against float64 and cannot see a wrong line that still computes the right
numbers; this file pins the lines, the ones no GPU test reaches through gnpde_edge_attention included (a forked stream, the one-launch
form and what refuses it, the hub rows alone, single passes, the A/B keys).

The expected values are literal tables, written from the dispatch code as it stood before the plan existed (edge_attention_impl's
chain of launchers: launch_sd_with_hubs, launch_sd_one, launch_rows_any, launch_hub_a_any, launch_rows_sd_mode's lane mapping and
grids, the squareplus sweep pair, the general passes), not taken from the planner.

Host graphs (tests/row_cases.py: the staircase graphs of the GPU test); operand addresses are constants and nothing is dereferenced."""
import ctypes
import functools

import pytest

import gnpde_amd as G
from gnpde_amd import _lib, ops
import row_cases as RC

BASE = 1 << 20          # operand addresses: only their alignment (and being non-null) is read
WS = 3 * BASE
NONE, IN_ROWS, DEFERRED, OWN, OWN_FORKED, LONG_STATS = range(6)          # GNPDE_ATT_HUBS_*
QUARTER, LANES, WHOLE_WAVE = 1, 2, 3                                      # GNPDE_ATT_ROWS16_*
PER_WAVE, SLOTS_FOLD, ATOMIC = 1, 2, 3                                    # GNPDE_ATT_GMAX_*

# rows of <= 16 entries per workgroup of row_attention_sd_kernel<H, DK4, GL16, RI16, P16, ..>: 4 waves x (64 / GL16) rows a wave x RI16
# interleaved -- (heads, d_k): 16 H lanes a row (a quarter wave at 4 heads, d_k 4 and 16), 4 rows interleaved at d_k 4 and 2 at 8 / 16
# where one pass covers 16 entries x H, 2 on the quarter waves, 1 at 8 heads
SD_ROWS16 = {(1, 4): 64, (1, 8): 32, (1, 16): 32, (2, 4): 32, (2, 8): 16, (2, 16): 16, (4, 4): 32, (4, 8): 8, (4, 16): 32,
             (8, 4): 4, (8, 8): 4, (8, 16): 4}
WHOLE_WAVE_ROWS16 = {(4, 4): 16, (4, 16): 8}       # gnpde_tune(17, 9): a wave a row, 4 (d_k 4) / 2 rows interleaved
GENERIC_ROWS16 = {1: 16, 2: 8, 4: 4, 8: 4}         # row_attention_kernel<TYPE, H, GL16, P16>: 4 waves x (64 / min(16 H, 64)) rows


def cdiv(a, b):
  return (a + b - 1) // b


@functools.lru_cache(maxsize=None)
def host_graph(name, row_begin=0):
  ei, lens, side = RC.graph_edges(name)
  g = G.CSRGraph(ei, lens.numel(), device='cpu')
  if row_begin:
    g.set_row_range(row_begin, g.n)
  return g


def bins(name):
  """(n_bin16, n_bin64, hub rows, hub chunks) of the side of the graph that carries the staircase."""
  return RC.expected_bins(RC.graph_edges(name)[1])


def struct(c, graph, q=BASE, **over):
  A = c.h * c.dk
  gat = c.att_type == 'gat'
  st = ops.attention_struct(_lib.ATT_GAT if gat else _lib.ATT_TYPES[c.att_type], c.h, A, c.norm_idx, c.sqp, ldqk=(A if gat else 2 * A) + c.ld_pad,
                            leaky_slope=c.slope, transposed=graph.transposed_positions() if c.norm_idx == 1 else None)
  st.q, st.k = q, (q if (gat or q is None) else q + 4 * A)                # k = the table's columns [A, 2A), as the GPU test hands them
  st.gat_a = BASE if gat else None
  st.output_var = st.lengthscale = BASE
  st.edge_w_csr = BASE if c.reweight else None
  for name, v in over.items():
    setattr(st, name, v)
  return st


def plan(c, graph=None, tune=(), **kw):
  graph = host_graph(c.graph) if graph is None else graph
  over = {k: kw.pop(k) for k in ('q', 'k', 'n_key_rows', 'gat_a', 'output_var', 'lengthscale', 't_from_csr', 'type', 'norm_idx', 'heads', 'ldqk')
          if k in kw}
  st = struct(c, graph, **over)
  want_all = c.outputs == 'all'
  kw.setdefault('ws_addr', WS)
  try:
    for key, v in tune:
      ops.tune(key, v)
    return ops.attention_plan(graph, st, kw.pop('want_w_mean', True), kw.pop('want_att', want_all), kw.pop('want_prods', want_all), **kw)
  finally:
    for key, v in tune:
      ops.tune(key, 0)


def expected_line(c, generic):
  """(route, MODE per sweep, SCATTER, dk4, gmax, hubs, gat_terms) of a case of row_cases.CASES, by the part of the GPU test's table."""
  route = RC.intended(c, generic)
  hubs_there = bins(c.graph)[2] > 0
  gat = c.att_type == 'gat'
  if route == RC.GENERAL:
    # every long segment of the normalised side has its two statistics launches; squareplus: atomic maxima in scores_kernel
    return (route, (), 0, 0, ATOMIC if c.sqp else 0, LONG_STATS if hubs_there else NONE, int(gat))
  if route == RC.ROWS:
    # row_attention_kernel per class (no d_k in its template line) + the hub launches in line
    return (route, (0,), 0, 0, 0, OWN if hubs_there else NONE, int(gat))
  modes = {1: (0,), 2: (2, 1), 3: (2, 1) if c.sqp else (0,), 4: (4,), 5: (3,), 8: (2, 1) if c.sqp else (0,)}[c.part]
  gmax = 0 if len(modes) == 1 else (SLOTS_FOLD if hubs_there else PER_WAVE)
  return (route, modes, int(c.norm_idx == 1), 1 if gat else c.dk // 4, gmax, IN_ROWS if hubs_there else NONE, 2 if gat else 0)


def line(p):
  return (p.route_name, p.modes, p.scatter, p.dk4, p.gmax, p.hubs, p.gat_terms)


@pytest.mark.parametrize('generic', [0, 1], ids=['specialised', 'generic'])
@pytest.mark.parametrize('c', RC.CASES, ids=RC.case_id)
def test_route_and_template_line(c, generic):
  p = plan(c, tune=((_lib.TUNE_ATT_GENERIC_ROWS, generic),))
  assert line(p) == expected_line(c, generic)
  assert p.h == c.h and p.swapped == p.scatter
  assert p.vec4 == int(c.dk % 4 == 0 and c.ld_pad == 0)
  n16, n64, n_long, n_chunks = bins(c.graph)
  if p.route_name == RC.GENERAL:
    assert (p.passes, p.seg_stats_heads, p.n_sweeps, p.rows16) == (7, int(c.h in (1, 2, 4, 8)), 0, 0)
    assert (p.n_long, p.max_chunks) == (n_long, cdiv(int(RC.graph_edges(c.graph)[1].max()), RC.LONG_ROW))
    assert p.launches == 3 + 2 * (n_long > 0) + (c.att_type == 'gat')
  else:
    assert p.n_hub == n_chunks and p.passes == 0
  if p.route_name == RC.SD:
    quarter = c.h == 4 and p.dk4 in (1, 4)
    assert p.rows16 == (QUARTER if quarter else LANES)
    # squareplus without hub rows: one word per wave of the maximum sweep; with hub rows the slots, a memset and the fold launch
    if c.sqp:
      waves = 4 * (cdiv(n16, SD_ROWS16[c.h, c.dk]) + cdiv(n64, 4))
      assert (p.gmax, p.gmax_count) == ((PER_WAVE, waves) if c.graph == 'nohubs' else (SLOTS_FOLD, 0))
    assert p.launches == sum(g > 0 for pair in p.grids for g in pair) + (p.gmax == SLOTS_FOLD) + (p.gat_terms != 0)


SWEEPS = {False: (0,), True: (2, 1)}


@pytest.mark.parametrize('name', ['hubs', 'nohubs'])
@pytest.mark.parametrize('h,dk', RC.SD_PAIRS)
def test_grids_of_both_row_classes(name, h, dk):
  n16, n64, n_long, n_hub = bins(name)
  for sqp in (False, True):
    p = plan(RC._case(0, name, 'scaled_dot', h, dk, sqp=sqp))
    assert p.route_name == RC.SD and p.modes == SWEEPS[sqp] and p.n_hub == n_hub
    rows16 = SD_ROWS16[h, dk]
    want = tuple((cdiv(n16, rows16) + n_hub, cdiv(n64, 4) + (0 if mode == 2 else n_hub)) for mode in SWEEPS[sqp])
    assert p.grids == want
    assert all(g > 0 for pair in want for g in pair)
  # the generic row kernels: a launch per class without hub blocks, the hub rows in two launches of their own
  p = plan(RC._case(0, name, 'scaled_dot', h, dk), tune=((_lib.TUNE_ATT_GENERIC_ROWS, 1),))
  assert (p.route_name, p.dk4, p.rows16) == (RC.ROWS, 0, LANES)
  assert p.grids == ((cdiv(n16, GENERIC_ROWS16[h]), cdiv(n64, 4)),) and p.launches == 2 + 2 * (n_hub > 0)


@pytest.mark.parametrize('h,dk', [(4, 4), (8, 16)])
def test_a_launch_of_hub_blocks_only(h, dk):
  for name in ('no16', 'no64'):
    n16, n64, n_long, n_hub = bins(name)
    assert n_hub == 4 and (n16 == 0) == (name == 'no16') and (n64 == 0) == (name == 'no64')
    p = plan(RC._case(8, name, 'scaled_dot', h, dk))
    assert p.grids == ((cdiv(n16, SD_ROWS16[h, dk]) + 4, cdiv(n64, 4) + 4),) and 4 in p.grids[0] and p.launches == 2
    # squareplus: the maximum sweep has no hub phase 1, so its second launch has no block at all where no row has 17..512 entries
    p = plan(RC._case(8, name, 'scaled_dot', h, dk, sqp=True))
    assert p.grids == ((cdiv(n16, SD_ROWS16[h, dk]) + 4, cdiv(n64, 4)), (cdiv(n16, SD_ROWS16[h, dk]) + 4, cdiv(n64, 4) + 4))
    assert p.launches == (4 if name == 'no16' else 3) + 1 and p.gmax == SLOTS_FOLD


PLAIN = [RC._case(1, 'hubs', 'scaled_dot', h, dk) for h, dk in RC.SD_PAIRS]


@pytest.mark.parametrize('name', ['hubs', 'nohubs'])
def test_forked_stream_keeps_the_sd_row_kernels_without_hub_blocks(name):
  """The line no GPU test of gnpde_edge_attention reaches: with a second stream the hub rows run as a branch of their own launches and
  the rows keep row_attention_sd_kernel, no hub block in front."""
  n16, n64, n_long, n_hub = bins(name)
  for h, dk in RC.SD_PAIRS:
    p = plan(RC._case(1, name, 'scaled_dot', h, dk), fork=True)
    assert (p.route_name, p.modes, p.scatter, p.dk4, p.gmax) == (RC.ROWS, (0,), 0, dk // 4, 0)
    assert p.hubs == (OWN_FORKED if n_hub else NONE) and p.n_hub == n_hub
    assert p.grids == ((cdiv(n16, SD_ROWS16[h, dk]), cdiv(n64, 4)),) and p.launches == 2 + 2 * (n_hub > 0)
  # every other type has no such line: its generic row kernels, forked hubs
  p = plan(RC._case(4, name, 'exp_kernel', 4, 4), fork=True)
  assert (p.route_name, p.dk4, p.hubs) == (RC.ROWS, 0, OWN_FORKED if n_hub else NONE)
  p = plan(RC._case(5, name, 'gat', 4, 4), fork=True)
  assert (p.route_name, p.dk4, p.hubs, p.gat_terms) == (RC.ROWS, 0, OWN_FORKED if n_hub else NONE, 1)
  # squareplus / columns leave their fast path for the general passes
  assert plan(RC._case(2, name, 'scaled_dot', 4, 4, sqp=True), fork=True).route_name == RC.GENERAL


def test_one_launch_where_the_aggregation_can_take_the_hub_rows():
  n16, n64, n_long, n_hub = bins('hubs')
  for c in PLAIN:
    p = plan(c, defer=True)
    if c.h == 8:          # 8 heads keep the two launches
      assert (p.route_name, p.hubs, p.launches) == (RC.SD, IN_ROWS, 2)
      continue
    assert (p.route_name, p.hubs, p.modes, p.dk4, p.launches) == ('sd_one', DEFERRED, (0,), c.dk // 4, 1)
    assert p.grids == ((n_hub + cdiv(n64, 4) + cdiv(n16, SD_ROWS16[c.h, c.dk]), 0),)
    assert p.rows16 == (QUARTER if (c.h == 4 and c.dk != 8) else LANES)
  p = plan(RC._case(1, 'nohubs', 'scaled_dot', 4, 4), defer=True)
  assert (p.route_name, p.hubs, p.launches) == ('sd_one', NONE, 1)


def test_one_launch_refused():
  c = RC._case(1, 'hubs', 'scaled_dot', 4, 4)
  plain = plan(c)
  assert line(plain) == (RC.SD, (0,), 0, 1, 0, IN_ROWS, 0)
  same = lambda p: (line(p), p.grids, p.launches) == (line(plain), plain.grids, plain.launches)     # noqa: E731
  assert same(plan(RC._case(1, 'hubs', 'scaled_dot', 4, 4, reweight=True), defer=True))             # edge weights
  assert same(plan(c, defer=True, n_key_rows=host_graph('hubs').n + 8))                              # halo rows
  assert same(plan(c, defer=True, tune=((_lib.TUNE_ATT_ONE_LAUNCH, 1),)))                            # key 21
  # key 17 (any value: the one kernel has the quarter-wave mapping alone); 9 also moves the plain call to whole waves
  assert same(plan(c, defer=True, tune=((_lib.TUNE_ATT_ROWS16, 1),)))
  whole = plan(c, defer=True, tune=((_lib.TUNE_ATT_ROWS16, 9),))
  assert (whole.route_name, whole.rows16) == (RC.SD, WHOLE_WAVE)
  # key 4: no specialised row kernel at all
  p = plan(c, defer=True, tune=((_lib.TUNE_ATT_GENERIC_ROWS, 1),))
  assert (p.route_name, p.dk4, p.hubs) == (RC.ROWS, 0, OWN)
  # a row sub-range: the two launches over the rows from row_begin
  p = plan(c, graph=host_graph('hubs', 8), defer=True)
  assert same(p)
  # a second stream
  assert plan(c, defer=True, fork=True).route_name == RC.ROWS
  # other types, other normalisers
  assert plan(RC._case(4, 'hubs', 'exp_kernel', 4, 4), defer=True).route_name == RC.SD
  assert plan(RC._case(2, 'hubs', 'scaled_dot', 4, 4, sqp=True), defer=True).route_name == RC.SD
  assert plan(RC._case(6, 'hubs', 'scaled_dot', 4, 12), defer=True).route_name == RC.ROWS


def test_hub_rows_alone():
  n_hub = bins('hubs')[3]
  for c in PLAIN + [RC._case(6, 'hubs', 'scaled_dot', 4, 12), RC._case(4, 'hubs', 'exp_kernel', 2, 8)]:
    p = plan(c, hubs_only=True)
    assert (p.route_name, p.hubs, p.n_hub, p.launches, p.n_sweeps, p.grids) == ('hubs_only', OWN, n_hub, 2, 0, ())
  p = plan(RC._case(5, 'hubs', 'gat', 4, 4), hubs_only=True)
  assert (p.route_name, p.hubs, p.gat_terms, p.launches) == ('hubs_only', OWN, 1, 3)
  p = plan(RC._case(1, 'nohubs', 'scaled_dot', 4, 4), hubs_only=True)
  assert (p.route_name, p.hubs, p.launches) == ('hubs_only', NONE, 0)


def test_single_passes_and_the_backward_s_request():
  n_long = bins('hubs')[2]
  for c in (RC._case(1, 'hubs', 'scaled_dot', 4, 4), RC._case(2, 'hubs', 'scaled_dot', 4, 4, sqp=True), RC._case(7, 'hubs', 'scaled_dot', 3, 4)):
    heads = int(c.h in (1, 2, 4, 8))
    p = plan(c, want_w_mean=False, stats_only=True)
    assert (p.route_name, p.passes, p.hubs, p.launches, p.seg_stats_heads) == (RC.GENERAL, 3, LONG_STATS, 4, heads)
    assert p.gmax == (ATOMIC if c.sqp else 0) and (p.n_long, p.max_chunks) == (n_long, 3)
    for pass_, launches, hubs in ((1, 1, NONE), (2, 3, LONG_STATS), (3, 1, NONE)):
      p = plan(c, want_w_mean=pass_ == 3, pass_=pass_)
      assert (p.route_name, p.passes, p.hubs, p.launches) == (RC.GENERAL, 1 << (pass_ - 1), hubs, launches)
      assert p.gmax == (ATOMIC if (c.sqp and pass_ == 1) else 0)       # the maximum is cleared in front of pass 1 alone


def test_ab_keys():
  n16, n64, n_long, n_hub = bins('hubs')
  # key 17 = 9: a whole wave per row of <= 16 entries -- at 4 heads, d_k 4 and 16, the row softmax (MODE 0) without SCATTER only
  for h, dk in RC.SD_PAIRS:
    p = plan(RC._case(1, 'hubs', 'scaled_dot', h, dk), tune=((_lib.TUNE_ATT_ROWS16, 9),))
    if (h, dk) in WHOLE_WAVE_ROWS16:
      assert p.rows16 == WHOLE_WAVE and p.grids == ((cdiv(n16, WHOLE_WAVE_ROWS16[h, dk]) + n_hub, cdiv(n64, 4) + n_hub),)
    else:
      assert p.rows16 == LANES and p.grids == ((cdiv(n16, SD_ROWS16[h, dk]) + n_hub, cdiv(n64, 4) + n_hub),)
  t16, t64, _, t_hub = bins('hubs_t')
  others = [RC._case(4, 'hubs', 'exp_kernel', 4, 4), RC._case(2, 'hubs', 'scaled_dot', 4, 4, sqp=True), RC._case(5, 'hubs', 'gat', 4, 4),
            RC._case(3, 'hubs_t', 'scaled_dot', 4, 4, norm_idx=1)]
  for c in others:
    p = plan(c, tune=((_lib.TUNE_ATT_ROWS16, 9),))
    a, b, hubs = (t16, t64, t_hub) if c.norm_idx else (n16, n64, n_hub)
    assert p.route_name == RC.SD and p.rows16 == QUARTER and p.grids[-1] == (cdiv(a, 32) + hubs, cdiv(b, 4) + hubs), RC.case_id(c)
  # ... and on the forked line
  p = plan(RC._case(1, 'hubs', 'scaled_dot', 4, 16), fork=True, tune=((_lib.TUNE_ATT_ROWS16, 9),))
  assert (p.route_name, p.rows16, p.grids) == (RC.ROWS, WHOLE_WAVE, ((cdiv(n16, 8), cdiv(n64, 4)),))
  # key 16: a small grid without hub rows keeps the slots, the memset and the fold launch
  c = RC._case(2, 'nohubs', 'scaled_dot', 4, 4, sqp=True)
  assert (plan(c).gmax, plan(c).launches) == (PER_WAVE, 4)
  p = plan(c, tune=((_lib.TUNE_GMAX_SMALL, 1),))
  assert (p.gmax, p.gmax_count, p.launches) == (SLOTS_FOLD, 0, 5)
  # key 11 = 2 is reported (hub_normalise_body folds straight from memory)
  assert plan(PLAIN[0]).hub_fold == 0 and plan(PLAIN[0], tune=((_lib.TUNE_HUB_FOLD, 2),)).hub_fold == 2
  assert plan(PLAIN[0], tune=((_lib.TUNE_HUB_FOLD, 1),)).hub_fold == 0


def test_row_sub_range():
  g = host_graph('hubs', 8)
  assert plan(RC._case(1, 'hubs', 'scaled_dot', 4, 4), graph=g).route_name == RC.SD
  assert plan(RC._case(6, 'hubs', 'cosine_sim', 4, 4), graph=g).route_name == RC.ROWS
  for c in (RC._case(2, 'hubs', 'scaled_dot', 4, 4, sqp=True), RC._case(7, 'hubs', 'scaled_dot', 3, 4), RC._case(7, 'hubs', 'scaled_dot', 4, 4, outputs='all')):
    with pytest.raises(_lib.GnpdeError, match='error -1.*a row sub-range needs the fused row path'):
      plan(c, graph=g)
  with pytest.raises(_lib.GnpdeError, match='error -1.*a row sub-range'):
    plan(RC._case(1, 'hubs', 'scaled_dot', 4, 4), graph=g, want_w_mean=False, stats_only=True)


def test_an_empty_graph_launches_nothing():
  import torch
  g = G.CSRGraph(torch.zeros(2, 0, dtype=torch.long), 5, device='cpu')
  p = plan(RC._case(1, 'hubs', 'scaled_dot', 4, 4), graph=g, ws_addr=0)
  assert (p.route_name, p.launches, p.grids) == ('none', 0, ())


def test_refusals_come_before_any_launch():
  """Every check of the launch, in its order, with its code: the plan refuses what the launch refuses."""
  L = _lib.lib()
  c = RC._case(1, 'hubs', 'scaled_dot', 4, 4)
  g = host_graph('hubs')
  # the first check: a null graph, a null attention descriptor
  out = _lib.AttentionLaunchStruct()
  st = struct(c, g)
  for gref, aref in ((None, ctypes.byref(st)), (g.ref(), None), (None, None)):
    assert L.gnpde_attention_plan(gref, aref, _lib.ATT_PLAN_W_MEAN, 0, WS, ctypes.byref(out)) == -1
    assert b'null descriptor' in L.gnpde_last_error()
    assert L.gnpde_edge_attention(gref, aref, ctypes.c_void_p(BASE), None, None, ctypes.c_void_p(WS), 1 << 40, None) == -1
  assert L.gnpde_attention_plan(g.ref(), ctypes.byref(st), _lib.ATT_PLAN_W_MEAN, 0, WS, None) == -1       # (and nowhere to write the plan)
  refused = [
    ('no output requested', dict(want_w_mean=False)),
    ('must be a factor', dict(heads=3)),
    ('bad type', dict(type=5)),
    ('attention_norm_idx must be 0 or 1', dict(norm_idx=2)),
    ('bad q/k', dict(q=None)), ('bad q/k', dict(k=None)), ('bad q/k', dict(ldqk=15)),
  ]
  for msg, kw in refused:
    with pytest.raises(_lib.GnpdeError, match='error -1.*%s' % msg):
      plan(c, **kw)
  with pytest.raises(_lib.GnpdeError, match='error -1.*GAT needs the vector a'):
    plan(RC._case(5, 'hubs', 'gat', 4, 4), gat_a=None)
  for name in ('output_var', 'lengthscale'):
    with pytest.raises(_lib.GnpdeError, match='error -1.*exp_kernel needs output_var and lengthscale'):
      plan(RC._case(4, 'hubs', 'exp_kernel', 4, 4), **{name: None})
  # the graph's own arrays
  for field, msg, cc in (('cscptr', 'norm_idx=1 needs the CSC view', RC._case(3, 'hubs_t', 'scaled_dot', 4, 4, norm_idx=1)),
                         ('rowidx', 'graph lacks rowidx/perm', c), ('perm', 'graph lacks rowidx/perm', c)):
    gg = host_graph(cc.graph)
    kept = getattr(gg.struct, field)
    try:
      setattr(gg.struct, field, None)
      with pytest.raises(_lib.GnpdeError, match='error -1.*%s' % msg):
        plan(cc)
    finally:
      setattr(gg.struct, field, kept)
  # the workspace: null is GNPDE_EWS (its size is not the plan's question), then its alignment
  with pytest.raises(_lib.GnpdeError, match='error -3.*workspace'):
    plan(c, ws_addr=0)
  with pytest.raises(_lib.GnpdeError, match='error -1.*workspace must be 16-byte aligned'):
    plan(c, ws_addr=WS + 8)
  with pytest.raises(_lib.GnpdeError, match='error -1.*pass outside 0..3'):
    plan(c, pass_=4)
  # the order: an earlier check answers first
  with pytest.raises(_lib.GnpdeError, match='no output requested'):
    plan(c, want_w_mean=False, heads=3, ws_addr=0)
  with pytest.raises(_lib.GnpdeError, match='error -3'):
    plan(c, graph=host_graph('hubs', 8), want_att=True, ws_addr=0)
  # the launch itself refuses the same with host operands, so nothing can have been launched
  st = struct(c, g, q=None)
  assert L.gnpde_edge_attention(g.ref(), ctypes.byref(st), ctypes.c_void_p(BASE), None, None, ctypes.c_void_p(WS), 1 << 40, None) == -1
  st = struct(c, g)
  assert L.gnpde_edge_attention(g.ref(), ctypes.byref(st), None, None, None, ctypes.c_void_p(WS), 1 << 40, None) == -1
  assert L.gnpde_edge_attention(g.ref(), ctypes.byref(st), ctypes.c_void_p(BASE), None, None, ctypes.c_void_p(WS), 16, None) == -3
  assert L.gnpde_edge_attention_pass(g.ref(), ctypes.byref(st), 3, None, ctypes.c_void_p(WS), 1 << 40, None) == -1
