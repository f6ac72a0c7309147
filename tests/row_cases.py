"""Row attention judged row by row: the staircase graphs, the per-segment metric, the float64 references and the list of cases that
tests/test_row_cases_cpu.py (input validity, on the CPU) and tests/test_attention_dispatch_gpu.py (every dispatch line of
csrc/attention.hip, on the device) share.  A plain helper module, not a conftest.

Why per segment: helpers.assert_parity divides the largest error by the largest reference value of the WHOLE tensor.  The head-mean
weight of a one-entry row is 1.0, those of a 1100-entry hub row about 1e-3: a hub row wrong by 1 % in every entry has a global relative
error of about 1e-5 and passes.  Hub rows run code of their own (chunk partials, hub_normalise_body, the deferred fold of the
aggregation's chunk items), so the metric here divides by the largest reference value of the SEGMENT the entry is normalised in (a row
for attention_norm_idx = 0, a column for 1).

The references are float64: oracle/restate.py is dtype-generic, and it is handed the very fp32 table the kernel reads, upcast, behind
identity projections -- neither the oracle's own fp32 rounding nor the projection's is part of a comparison."""
import collections
import functools

import torch

from oracle import restate as R

# entries per segment, self-loop included: both sides of every class boundary of the row kernels (16 | 17 entries: the two lane mappings;
# 32 | 33, 64 | 65, 128 | 129: passes and batches of the wave-per-row body; 512 | 513: one wave | chunks), two chunks with the second
# nearly empty (513) and full (1024), three chunks (1025, 1100)
SHORT = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512]
HUBS = [513, 1024, 1025, 1100]
N = 1200
LONG_ROW = 512            # GNPDE_LONG_ROW
DUP_LEN = 20              # entries of the row that lists one column twice
WAVE, WAVES_PER_BLOCK = 64, 4
GMAX_PART_CAP = 8192      # kGmaxPartCap of csrc/attention.hip


def sd_rows_per_block16(h, dk4):
  """Rows of <= 16 entries per workgroup of row_attention_sd_kernel (the constexpr of the same name in csrc/attention.hip)."""
  quarter = h == 4 and dk4 in (1, 4)
  gl16 = 16 if quarter else min(16 * h, WAVE)
  p16 = (16 * h + gl16 - 1) // gl16
  ri16 = 2 if quarter else (4 if (dk4 == 1 and p16 == 1) else (2 if p16 == 1 else 1))
  return (WAVE // gl16) * ri16 * WAVES_PER_BLOCK


SD_PAIRS = [(h, dk) for h in (1, 2, 4, 8) for dk in (4, 8, 16)]
ROWS_PER_BLOCK16 = sorted({sd_rows_per_block16(h, dk // 4) for h, dk in SD_PAIRS})      # [4, 8, 16, 32, 64]


def sd_sweep_waves(h, dk4, n16, n64):
  """Waves of the two launches of a squareplus maximum sweep without hub blocks (sd_sweep_waves of csrc/attention.hip)."""
  rpb = sd_rows_per_block16(h, dk4)
  return ((n16 + rpb - 1) // rpb * WAVES_PER_BLOCK if n16 else 0) + ((n64 + WAVES_PER_BLOCK - 1) // WAVES_PER_BLOCK * WAVES_PER_BLOCK if n64 else 0)


def staircase_graph(n, short=SHORT, hubs=HUBS, seed=0, transpose=False, empty=3, dup_row=True, fill=(1, 16)):
  """(edge list [2, E] int64 in shuffled order, lens [n]): every ordinary row has fill[0]..fill[1] entries (1..16 by default) with a
  self-loop, the lengths listed in `short` and `hubs` are spread over the id range, the columns of a row are distinct, `empty` rows have
  no entry at all, and (dup_row) one more row of DUP_LEN entries lists one column twice.  transpose=True swaps the two index rows, so
  that the COLUMNS carry the staircase (attention_norm_idx = 1); lens are the lengths of the staircase side either way."""
  g = torch.Generator().manual_seed(seed)
  lens = torch.randint(fill[0], fill[1] + 1, (n,), generator=g)
  special = list(short) + list(hubs)
  taken = set()
  if special:
    rows = torch.linspace(5, n - 7, len(special)).long()
    assert rows.unique().numel() == len(special) and max(special) <= n
    lens[rows] = torch.tensor(special)
    taken = set(rows.tolist())
  free = [i for i in torch.randperm(n, generator=g).tolist() if i not in taken]
  assert len(free) >= empty + int(dup_row)
  for i in free[:empty]:
    lens[i] = 0
  dup = free[empty] if dup_row else -1
  if dup_row:
    lens[dup] = DUP_LEN
  src, dst = [], []
  for i in range(n):
    m = int(lens[i])
    if m == 0:
      continue
    k = m - 1 - int(i == dup)
    others = torch.randperm(n - 1, generator=g)[:k]
    others = others + (others >= i).long()          # distinct columns, none of them i
    cols = [torch.tensor([i]), others]
    if i == dup:
      cols.append(others[:1])                       # ... but for this one
    src.append(torch.full((m,), i))
    dst.append(torch.cat(cols))
  ei = torch.stack([torch.cat(src), torch.cat(dst)])
  ei = ei[:, torch.randperm(ei.size(1), generator=g)].long()
  return (ei.flip(0).contiguous() if transpose else ei), lens


# name -> arguments of staircase_graph.  empty = 5: with n = 1200 the <= 16-entry class has 1178 (hubs) / 1182 (no hubs) rows, a multiple
# of none of ROWS_PER_BLOCK16, and the 17..512 class 13 rows, no multiple of 4: the masked tail slots (live[r], the re-read of the
# class's last record) run for every (heads, d_k).  The two tiny graphs have no row of one class at all -- a launch there consists of
# hub blocks only and the n_rows == 0 clamp of row_attention_sd_rows is live.
GRAPHS = {
  'hubs': dict(n=N, seed=31, empty=5),
  'nohubs': dict(n=N, hubs=[], seed=32, empty=5),
  'hubs_t': dict(n=N, seed=33, empty=5, transpose=True),
  'nohubs_t': dict(n=N, hubs=[], seed=34, empty=5, transpose=True),
  'no16': dict(n=640, short=[], hubs=[513, 640], seed=35, empty=600, dup_row=False, fill=(17, 40)),
  'no64': dict(n=640, short=[], hubs=[513, 640], seed=36, empty=560, dup_row=False, fill=(1, 16)),
}


@functools.lru_cache(maxsize=None)
def graph_edges(name):
  """(ei, lens, side): side = the index row that carries the staircase (0: rows, 1: columns)."""
  kw = GRAPHS[name]
  ei, lens = staircase_graph(**kw)
  return ei, lens, int(bool(kw.get('transpose', False)))


def expected_bins(lens):
  """(n_bin16, n_bin64, n_long, n_long_chunks) of segments of these lengths."""
  n16 = int(((lens >= 1) & (lens <= 16)).sum())
  n64 = int(((lens > 16) & (lens <= LONG_ROW)).sum())
  hub = lens[lens > LONG_ROW]
  return n16, n64, int(hub.numel()), int(((hub + LONG_ROW - 1) // LONG_ROW).sum())


# ------------------------------------------------------------------------------------------------
# the metric
# ------------------------------------------------------------------------------------------------
def per_segment_error(got, ref64, seg):
  """For every segment, the largest |got - ref| over its entries (and heads) divided by the largest |ref| in that segment.  got, ref64:
  [E] or [E, h] in one order, seg [E] the segment id of every entry in that order.  Returns the vector [max id + 1] (float64; segments
  without entries: 0)."""
  got = got.detach().double().cpu().reshape(got.shape[0], -1)
  ref = ref64.detach().double().cpu().reshape(ref64.shape[0], -1)
  seg = seg.detach().long().cpu()
  assert got.shape == ref.shape and seg.shape[0] == got.shape[0]
  n = int(seg.max()) + 1 if seg.numel() else 0
  err = torch.zeros(n, dtype=torch.float64).scatter_reduce_(0, seg, (got - ref).abs().amax(dim=1), 'amax', include_self=True)
  top = torch.zeros(n, dtype=torch.float64).scatter_reduce_(0, seg, ref.abs().amax(dim=1), 'amax', include_self=True)
  return err / top.clamp_min(1e-300)


CLASSES = (('<=16', 1, 16), ('17..512', 17, LONG_ROW), ('>512', LONG_ROW + 1, 1 << 62))


def class_errors(err, lens):
  """{length class: worst per-segment error} (classes without a segment are left out)."""
  lens = lens.long().cpu()[:err.numel()]
  out = {}
  for name, lo, hi in CLASSES:
    m = (lens >= lo) & (lens <= hi)
    if bool(m.any()):
      out[name] = float(err[m].max())
  return out


def assert_rows(got, ref64, seg, lens, tol, what=''):
  """The output is finite and every segment's error is <= tol; a failure names the worst segment, its length and the worst error of
  every length class.  lens [n]: entries per segment id.  Returns the per-class errors."""
  assert got.shape == ref64.shape, '%s: shape %s vs %s' % (what, tuple(got.shape), tuple(ref64.shape))
  assert bool(torch.isfinite(got).all()), '%s: non-finite output' % what
  err = per_segment_error(got, ref64, seg)
  per_class = class_errors(err, lens)
  if err.numel():
    worst = int(err.argmax())
    assert float(err[worst]) <= tol, '%s: segment %d (%d entries) rel err %.3e > %.1e; worst per length class: %s' % (
      what, worst, int(lens[worst]), float(err[worst]), tol, ', '.join('%s %.3e' % kv for kv in per_class.items()))
  return per_class


# ------------------------------------------------------------------------------------------------
# the cases of tests/test_attention_dispatch_gpu.py
# ------------------------------------------------------------------------------------------------
# part: the case number of the module docstring there; A = heads * d_k; ld_pad: columns added to the table's row stride; outputs: 'w' =
# head-mean weights only, 'all' = att [E,h] and prods [E,h] as well
Case = collections.namedtuple('Case', 'part graph att_type h dk norm_idx sqp reweight slope ld_pad outputs')


def _case(part, graph, att_type, h, dk, norm_idx=0, sqp=False, reweight=False, slope=0.2, ld_pad=0, outputs='w'):
  return Case(part, graph, att_type, h, dk, norm_idx, sqp, reweight, slope, ld_pad, outputs)


def case_id(c):
  return '%d-%s-%s-h%d-dk%d-n%d%s%s%s%s%s' % (c.part, c.graph, c.att_type, c.h, c.dk, c.norm_idx, '-sqp' if c.sqp else '', '-rw' if c.reweight else '',
                                             '-slope%g' % c.slope if c.att_type == 'gat' else '', '-ld+%d' % c.ld_pad if c.ld_pad else '',
                                             '-all' if c.outputs == 'all' else '')


def _cases():
  out = []
  for h, dk in SD_PAIRS:
    out += [_case(1, 'hubs', 'scaled_dot', h, dk), _case(1, 'hubs', 'scaled_dot', h, dk, reweight=True)]
    out += [_case(2, 'nohubs', 'scaled_dot', h, dk, sqp=True), _case(2, 'hubs', 'scaled_dot', h, dk, sqp=True)]
    out += [_case(3, 'hubs_t', 'scaled_dot', h, dk, norm_idx=1), _case(3, 'hubs_t', 'scaled_dot', h, dk, norm_idx=1, sqp=True)]
    out += [_case(4, 'hubs', 'exp_kernel', h, dk)]
  out += [_case(3, 'hubs_t', 'scaled_dot', 4, 4, norm_idx=1, reweight=True)]
  out += [_case(4, 'hubs', 'exp_kernel', 2, 12)]
  for h in (1, 2, 4, 8):
    out += [_case(5, 'hubs', 'gat', h, 4), _case(5, 'hubs', 'gat', h, 16, slope=0.05)]
  out += [_case(5, 'hubs', 'gat', 3, 4), _case(5, 'hubs', 'gat', 4, 4, reweight=True), _case(5, 'hubs', 'gat', 2, 16, reweight=True, slope=0.05)]
  for att_type in ('cosine_sim', 'pearson'):
    out += [_case(6, 'hubs', att_type, h, dk) for h in (1, 2, 4, 8) for dk in (4, 8)]
  out += [_case(6, 'hubs', 'scaled_dot', 4, 12), _case(6, 'hubs', 'scaled_dot', 2, 32), _case(6, 'hubs', 'scaled_dot', 8, 12), _case(6, 'hubs', 'scaled_dot', 1, 32)]
  for norm_idx, graph in ((0, 'hubs'), (1, 'hubs_t')):
    out += [_case(7, graph, 'scaled_dot', 4, 2, norm_idx), _case(7, graph, 'scaled_dot', 3, 4, norm_idx),
            _case(7, graph, 'scaled_dot', 4, 4, norm_idx, ld_pad=1), _case(7, graph, 'scaled_dot', 3, 4, norm_idx, sqp=True, outputs='all')]
    out += [_case(7, graph, 'scaled_dot', h, 4, norm_idx, outputs='all') for h in (1, 2, 4, 8)]
    out += [_case(7, graph, 'scaled_dot', 4, 4, norm_idx, sqp=True, outputs='all')]
  for graph in ('no16', 'no64'):
    out += [_case(8, graph, 'scaled_dot', h, dk, sqp=sqp) for h, dk in ((4, 4), (8, 16)) for sqp in (False, True)]
  assert len(set(out)) == len(out)
  return out


CASES = _cases()
OUTPUT_VAR = 1.2

# the routes of gnpde_attention_plan (_lib.ATT_ROUTES) that gnpde_edge_attention reaches: the scaled-dot row kernels with the hub chunks in
# their first blocks, a row kernel per class + hub launches, the three general passes
SD, ROWS, GENERAL = 'sd_rows', 'rows', 'general'


def intended(c, generic):
  """The route a case is there to run (the table of tests/test_attention_dispatch_gpu.py's docstring), generic =
  gnpde_tune(TUNE_ATT_GENERIC_ROWS, .)."""
  if c.part in (1, 4):
    return ROWS if (generic or c.dk == 12) else SD
  if c.part in (2, 3):
    return GENERAL if (generic or c.reweight) else SD
  if c.part == 5:
    return GENERAL if c.h == 3 else (ROWS if (generic or c.reweight) else SD)
  if c.part == 6:
    return ROWS
  if c.part == 7:
    return GENERAL
  return SD if not generic else (GENERAL if c.sqp else ROWS)


def lengthscale(dk):
  """|q - k|^2 of standard-normal head vectors is about 2 d_k: a lengthscale of 0.8 sqrt(d_k) keeps the exp kernel's scores O(1) apart,
  so that the row softmax over them is not flat and an error in a score shows in the weights."""
  return 0.8 * dk ** 0.5


@functools.lru_cache(maxsize=None)
def case_inputs(c):
  """Seeded fp32 inputs of a case, on the CPU: table [n, ld] (q||k, columns [0, A) and [A, 2A); for GAT the projected features wx
  [n, A]), the GAT vector a [2 d_k], edge weights [E] in edge order (or None).  Standard-normal tables, drawn directly."""
  ei, lens, side = graph_edges(c.graph)
  n = lens.numel()
  A = c.h * c.dk
  width = A if c.att_type == 'gat' else 2 * A
  g = torch.Generator().manual_seed(1000 + CASES.index(c))
  table = torch.zeros(n, width + c.ld_pad)
  table[:, :width] = torch.randn(n, width, generator=g)
  # (GAT scores a . [wx_i || wx_j] of unit variance, like the scaled dot products: with a standard-normal `a` they reach 20 at d_k = 16
  #  and the fp32 oracle's own rounding of them, 1.5e-5 per segment, would be larger than the tolerance)
  a = torch.randn(2 * c.dk, generator=g) / (2 * c.dk) ** 0.5 if c.att_type == 'gat' else None
  ew = torch.rand(ei.size(1), generator=g) + 0.5 if c.reweight else None
  return table, a, ew


def reference(c, dtype=torch.float64):
  """att [E, h] and prods [E, h] (None for GAT) of oracle/restate.py in `dtype`, in edge order, from the case's own fp32 table upcast:
  identity projections, so the table is all the oracle sees."""
  ei, lens, side = graph_edges(c.graph)
  table, a, ew = case_inputs(c)
  A = c.h * c.dk
  eye = torch.eye(A, dtype=dtype)
  if c.att_type == 'gat':
    assert not c.sqp
    att, _ = R.gat_attention(table[:, :A].to(dtype), ei, eye, a.to(dtype).view(-1, 1, 1), c.h, c.slope, c.norm_idx)
    if ew is not None:     # (the library's edge weights multiply the GAT scores too; the reference layer has none: softmax of e * w)
      x = table[:, :A].to(dtype).view(-1, c.h, c.dk)
      av = a.to(dtype)
      e_ = torch.nn.functional.leaky_relu((x[ei[0]] * av[:c.dk]).sum(-1) + (x[ei[1]] * av[c.dk:]).sum(-1), c.slope)
      att = R.segment_softmax(e_ * ew.to(dtype).unsqueeze(1), ei[c.norm_idx], lens.numel())
    return att, None
  zero = torch.zeros(A, A, dtype=dtype)
  return R.transformer_attention(table[:, :2 * A].to(dtype), ei, torch.cat([eye, zero], dim=1), None, torch.cat([zero, eye], dim=1), None, c.h,
                                 attention_type=c.att_type, norm_idx=c.norm_idx, square_plus=c.sqp,
                                 edge_weights=None if ew is None else ew.to(dtype), reweight=ew is not None,
                                 output_var=torch.tensor([OUTPUT_VAR], dtype=dtype), lengthscale=torch.tensor([lengthscale(c.dk)], dtype=dtype))


@functools.lru_cache(maxsize=None)
def reference64(c):
  """The float64 reference of a case, computed once per (graph, type, heads, d_k, ...) and shared by every run of it."""
  return reference(c, torch.float64)
