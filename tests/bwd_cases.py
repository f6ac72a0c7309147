"""The attention backward judged row by row: inputs, float64 references, tolerances and the lists of cases that
tests/test_bwd_cases_cpu.py (validity of inputs and bounds, on the CPU) and tests/test_bwd_dispatch_gpu.py (every launch line of
csrc/backward.hip, on the device) share.  A plain helper module, not a conftest; it builds on tests/row_cases.py (the staircase graphs,
the per-segment metric, the length classes).

What is differentiated: L = sigmoid(alpha) sum_e r_e w_e with w = the head mean of the row softmax of s_eh = q_i,h . k_j,h / sqrt(d_k)
[* edge_w_e], e = (i, j).  Then, with a = softmax_row(s) and c_ih = sum_{e in row i} a_eh r_e,
  ds_eh = sigmoid(alpha) (a_eh / H) (r_e - c_ih) [* edge_w_e]              d L / d (q_i,h . k_j,h / sqrt d_k)
  d q_i  = (1 / sqrt d_k) sum_{e in row i}    ds_e,head k_j                a sum over the ROWS of the graph
  d k_j  = (1 / sqrt d_k) sum_{e in column j} ds_e,head q_i                a sum over its COLUMNS = the rows of the transposed graph
The references are float64: oracle/restate.py behind identity projections on the case's own fp32 table, upcast (as row_cases.reference);
ds by the formula above from the oracle's attention, d q and d k by float64 autograd of L through the oracle -- two derivations that
tests/test_bwd_cases_cpu.py holds against each other.

The graph side matters.  ds and d q are sums over rows: they run on the graphs whose ROWS carry the staircase 1, 2, 15, 16, 17, ..., 512 |
513, 1024, 1025, 1100 (hubs, nohubs, no16, no64).  The columns of those graphs have at most about 25 entries, so d k there would run the
<= 16 class alone: d k runs on the transposed staircases (hubs_t, nohubs_t), whose COLUMNS carry the staircase; the kernel walks the rows
of graph.transposed_positions()[0] and reads ds through t_from_csr.

Tolerance, per segment: max(helpers.TOL, 3 x the error the oracle itself makes for that length class of that case when it is evaluated in
fp32) -- measured against the float64 reference on the CPU, never against a kernel (the rule of _grad_close in this suite).  A segment
whose reference is zero (largest entry below 1e-6 of the tensor's largest: the one-entry rows, where a = 1 and r - c = 0 identically) has
no scale of its own and is judged absolutely, at TOL x the tensor's largest entry."""
import collections
import functools
import math

import torch

from oracle import restate as R
import row_cases as RC
from helpers import TOL

ALPHA = 0.4                                   # the epilogue's alpha: the kernels scale by sigmoid(alpha)
DEGENERATE = 1e-6                             # a segment below this fraction of the tensor's maximum is judged absolutely

AB_PAIRS = list(RC.SD_PAIRS)                                                   # the 12 GNPDE_AB lines: heads in {1,2,4,8} x d_k in {4,8,16}
DQ_PAIRS = [(h, dk) for h, dk in AB_PAIRS if h * dk <= 32]                      # the 9 pairs whose kernel can also form d q
HR_PAIRS = [(h, dk) for h, dk in AB_PAIRS if h * dk <= 32]                      # the 9 GNPDE_HR lines: heads * d_k / 4 <= 8
assert len(AB_PAIRS) == 12 and len(DQ_PAIRS) == 9 and DQ_PAIRS == [(1, 4), (1, 8), (1, 16), (2, 4), (2, 8), (2, 16), (4, 4), (4, 8), (8, 4)]

RefCase = collections.namedtuple('RefCase', 'graph h dk reweight')
Ref = collections.namedtuple('Ref', 'att ds dq dk')        # att, ds [E, h] in edge order; dq, dk [n, A]


def ref_id(c):
  return '%s-h%d-dk%d%s' % (c.graph, c.h, c.dk, '-rw' if c.reweight else '')


MAX_DRAWS = 32


def _draw(c, attempt):
  ei, lens, side = RC.graph_edges(c.graph)
  A = c.h * c.dk
  g = torch.Generator().manual_seed(7000 + 1000 * sorted(RC.GRAPHS).index(c.graph) + 40 * c.h + 2 * c.dk + int(c.reweight) + 100003 * attempt)
  table = torch.randn(lens.numel(), 2 * A, generator=g)
  r = torch.randn(ei.size(1), generator=g)
  ew = torch.rand(ei.size(1), generator=g) + 0.5 if c.reweight else None
  return table, r, ew


def ds_from_att(ei, att, r, ew, n):
  """The formula's ds [E, h] from an attention [E, h] (row softmax), r [E] and edge weights [E] or None, in the dtype of att."""
  s = torch.sigmoid(torch.tensor(ALPHA, dtype=att.dtype))
  cc = R.scatter_sum(att * r.unsqueeze(1), ei[0], n)[ei[0]]
  ds = s * (att / att.shape[1]) * (r.unsqueeze(1) - cc)
  return ds if ew is None else ds * ew.unsqueeze(1)


def _reference(c, draw, dtype):
  ei, lens, side = RC.graph_edges(c.graph)
  table, r, ew = draw
  n, A = lens.numel(), c.h * c.dk
  q = table[:, :A].to(dtype).clone().requires_grad_(True)
  k = table[:, A:].to(dtype).clone().requires_grad_(True)
  eye, zero = torch.eye(A, dtype=dtype), torch.zeros(A, A, dtype=dtype)
  rr = r.to(dtype)
  eww = None if ew is None else ew.to(dtype)
  att, _ = R.transformer_attention(torch.cat([q, k], dim=1), ei, torch.cat([eye, zero], dim=1), None, torch.cat([zero, eye], dim=1), None, c.h,
                                   attention_type='scaled_dot', norm_idx=0, square_plus=False, edge_weights=eww, reweight=ew is not None)
  s = torch.sigmoid(torch.tensor(ALPHA, dtype=dtype))
  loss = s * (rr * att.mean(dim=1)).sum()
  dq, dk = torch.autograd.grad(loss, (q, k))
  a = att.detach()
  return Ref(a, ds_from_att(ei, a, rr, eww, n), dq, dk)


def _fp32_errors(c, r64, r32):
  ei, lens, side = RC.graph_edges(c.graph)
  rows, cols = segment_lens(c.graph, False), segment_lens(c.graph, True)
  out = {'ds': segment_error(r32.ds, r64.ds, ei[0]) + (rows,)}
  for name, lens_ in (('dq', rows), ('dk', cols)):
    g, keep = node_rows(getattr(r32, name), lens_)
    out[name] = segment_error(g, getattr(r64, name)[keep], keep) + (lens_,)
  return out


@functools.lru_cache(maxsize=None)
def _case(c):
  """(inputs, float64 reference, fp32-oracle errors, draws taken) of a case.  A draw is kept only if the oracle ITSELF, evaluated in fp32
  on it, stays within TOL of float64 in every segment of ds, d q and d k; otherwise the next seed is drawn.  What is turned away is an
  ill-conditioned draw, decided by the reference alone: in a two-entry row ds = +- a (1 - a) (r_1 - r_2), formed as r_1 - c, so its relative
  error is eps |r| / |r_1 - r_2| -- among the ~150 two-entry rows of a staircase graph the closest pair of standard-normal r's is about
  1 / 150 apart, which puts fp32 at 1e-5 in about every second draw.  (By the tolerance rule such a draw would only widen the device
  bound to 3 x that error; turning it away keeps the bound at TOL.)"""
  for attempt in range(MAX_DRAWS):
    draw = _draw(c, attempt)
    r64 = _reference(c, draw, torch.float64)
    errs = _fp32_errors(c, r64, _reference(c, draw, torch.float32))
    if max(float(e[0].max()) for e in errs.values()) <= TOL:
      return draw, r64, errs, attempt + 1
  raise AssertionError('%s: no well-conditioned draw among %d seeds' % (ref_id(c), MAX_DRAWS))


def inputs(c):
  """Seeded fp32 inputs of a case, on the CPU, drawn directly: the table q||k [n, 2A] and r [E] standard normal, edge weights [E] in
  [0.5, 1.5) (or None), all in edge order."""
  return _case(c)[0]


def reference(c, dtype=torch.float64):
  """Ref(att, ds, dq, dk) of the case in `dtype` from the oracle (see the module docstring)."""
  return _reference(c, inputs(c), dtype)


def reference64(c):
  """The float64 reference of a case, computed once and shared."""
  return _case(c)[1]


def head_sums(ei, ds, table, h, dk, by_column):
  """The formula's d q (by_column False) / d k (True) from ds [E, h] and the table, by index_add in the dtype of ds."""
  A = h * dk
  n = table.shape[0]
  head = torch.arange(A) // dk
  seg, other = (ei[1], ei[0]) if by_column else (ei[0], ei[1])
  feat = (table[:, :A] if by_column else table[:, A:2 * A]).to(ds.dtype)
  return torch.zeros(n, A, dtype=ds.dtype).index_add_(0, seg, ds[:, head] * feat[other]) / math.sqrt(dk)


# ------------------------------------------------------------------------------------------------
# the metric: row_cases.per_segment_error, with the zero segments judged absolutely
# ------------------------------------------------------------------------------------------------
def segment_lens(graph, by_column=False):
  """Entries per row (per column) of the graph's edge list."""
  ei, lens, side = RC.graph_edges(graph)
  return torch.bincount(ei[int(by_column)], minlength=lens.numel())


def segment_error(got, ref64, seg):
  """(err [n], degenerate [n] bool): row_cases.per_segment_error, but for the segments whose reference is zero (see DEGENERATE) the largest
  |got - ref| divided by the TENSOR's largest |ref|."""
  err = RC.per_segment_error(got, ref64, seg)
  g2 = got.detach().double().cpu().reshape(got.shape[0], -1)
  r2 = ref64.detach().double().cpu().reshape(ref64.shape[0], -1)
  seg = seg.detach().long().cpu()
  n = err.numel()
  top = torch.zeros(n, dtype=torch.float64).scatter_reduce_(0, seg, r2.abs().amax(dim=1), 'amax', include_self=True)
  dif = torch.zeros(n, dtype=torch.float64).scatter_reduce_(0, seg, (g2 - r2).abs().amax(dim=1), 'amax', include_self=True)
  present = torch.zeros(n, dtype=torch.bool)
  present[seg] = True
  whole = float(r2.abs().max()) if r2.numel() else 0.0
  degenerate = present & (top < DEGENERATE * whole)
  return torch.where(degenerate, dif / max(whole, 1e-300), err), degenerate


def node_rows(t, lens):
  """A per-node tensor [n, A] as segments of one row each: (the rows with entries, their ids).  Rows without entries are not written by
  the row kernels and are left out of every comparison."""
  keep = (lens > 0).nonzero().flatten()
  return t[keep.to(t.device)], keep


def class_tolerances(err32, lens):
  """{length class: max(TOL, 3 x the fp32 oracle's worst per-segment error in that class)}."""
  return {name: max(TOL, 3.0 * e) for name, e in RC.class_errors(err32, lens).items()}


def assert_segments(got, ref64, seg, lens, tol, what=''):
  """row_cases.assert_rows with a tolerance per length class (tol: a dict of row_cases.CLASSES names, or one number) and the zero
  segments judged absolutely: the output is finite and every segment's error is within its class's tolerance; a failure names the worst
  segment, its length and the worst error of every length class.  Returns the per-class errors."""
  assert got.shape == ref64.shape, '%s: shape %s vs %s' % (what, tuple(got.shape), tuple(ref64.shape))
  assert bool(torch.isfinite(got).all()), '%s: non-finite output' % what
  err, _ = segment_error(got, ref64, seg)
  lens = lens.long().cpu()
  per_class = RC.class_errors(err, lens)
  if not isinstance(tol, dict):
    tol = {name: float(tol) for name, _, _ in RC.CLASSES}
  tolv = torch.full((err.numel(),), TOL, dtype=torch.float64)
  for name, lo, hi in RC.CLASSES:
    if name in tol:
      tolv[(lens[:err.numel()] >= lo) & (lens[:err.numel()] <= hi)] = tol[name]
  if err.numel():
    worst = int((err / tolv).argmax())
    assert float(err[worst]) <= float(tolv[worst]), '%s: segment %d (%d entries) rel err %.3e > %.1e; worst per length class: %s' % (
      what, worst, int(lens[worst]), float(err[worst]), float(tolv[worst]), ', '.join('%s %.3e' % kv for kv in per_class.items()))
  return per_class


def oracle_fp32_errors(c):
  """Per-segment error of the fp32 oracle against the float64 one, {'ds' | 'dq' | 'dk': (err [n], degenerate [n], lens [n])}: ds and d q
  by rows, d k by columns."""
  return _case(c)[2]


def tolerances(c, what):
  """The tolerance per length class of the case's ds / dq / dk (section "Tolerance" of the module docstring)."""
  err, _, lens = oracle_fp32_errors(c)[what]
  return class_tolerances(err, lens)


# ------------------------------------------------------------------------------------------------
# the cases of tests/test_bwd_dispatch_gpu.py
# ------------------------------------------------------------------------------------------------
HUB_FORMS = ('chunks', 'block')          # hub_ws given: three chunk kernels; hub_ws NULL: one 1024-thread block per hub row

# attention backward, ds: (RefCase, hub form, variant).  variant: '' | 'rpos' (r in the transposed graph's order, read through
# csr_positions) | 'noscale' (scale NULL) | 'raw' (a raw scale, no sigmoid)
DsCase = collections.namedtuple('DsCase', 'ref hubs variant')
RAW_SCALE = 0.7
RPOS_PAIRS = [(1, 4), (2, 8), (4, 16), (8, 4)]        # one pair per head count


def _ds_cases():
  out = []
  for h, dk in AB_PAIRS:
    out += [DsCase(RefCase('hubs', h, dk, rw), hubs, '') for rw in (False, True) for hubs in HUB_FORMS]
  for graph in ('no16', 'no64'):
    out += [DsCase(RefCase(graph, h, dk, False), hubs, '') for h, dk in ((4, 4), (8, 16)) for hubs in HUB_FORMS]
  out += [DsCase(RefCase('nohubs', 4, 4, False), 'chunks', '')]                  # no hub launch at all
  out += [DsCase(RefCase('hubs', h, dk, False), HUB_FORMS[i % 2], 'rpos') for i, (h, dk) in enumerate(RPOS_PAIRS)]
  out += [DsCase(RefCase('hubs', 4, 8, False), 'chunks', 'noscale'), DsCase(RefCase('hubs', 2, 4, True), 'block', 'raw')]
  assert len(set(out)) == len(out)
  return out


# fused d q: (RefCase, hub form)
DqCase = collections.namedtuple('DqCase', 'ref hubs')


def _dq_cases():
  out = [DqCase(RefCase('hubs', h, dk, False), hubs) for h, dk in DQ_PAIRS for hubs in HUB_FORMS]
  out += [DqCase(RefCase('hubs', 4, 4, True), 'chunks'), DqCase(RefCase('hubs', 8, 4, True), 'block')]
  out += [DqCase(RefCase(graph, 4, 4, False), 'chunks') for graph in ('no16', 'no64', 'nohubs')]
  return out


# head_rowsum: (RefCase, side, hub form).  side 'dq': the rows of the graph, pos NULL, feat = k; 'dk': the rows of the transposed graph,
# pos = t_from_csr, feat = q
HrCase = collections.namedtuple('HrCase', 'ref side hubs')


def _hr_cases():
  out = []
  for h, dk in HR_PAIRS:
    out += [HrCase(RefCase('hubs', h, dk, False), 'dq', hubs) for hubs in HUB_FORMS]
    out += [HrCase(RefCase('hubs_t', h, dk, False), 'dk', hubs) for hubs in HUB_FORMS]
  for graph in ('no16', 'no64'):
    out += [HrCase(RefCase(graph, h, dk, False), 'dq', hubs) for h, dk in ((4, 4), (8, 4)) for hubs in HUB_FORMS]
  out += [HrCase(RefCase('nohubs', 4, 4, False), 'dq', 'chunks'), HrCase(RefCase('nohubs_t', 4, 4, False), 'dk', 'chunks')]
  out += [HrCase(RefCase('hubs_t', 4, 4, True), 'dk', 'chunks')]
  return out


# gnpde_softmax_rows_bwd: heads 1, 2, 4, 8 (compile-time) and 3 (the run-time loop), d_k = 4
SB_CASES = [RefCase('hubs', h, 4, rw) for h in (1, 2, 4, 8, 3) for rw in (False, True)]

# gnpde_head_spmm: (heads, d_k, aligned) -> the line.  The float4 kernel head_spmm_kernel<A/4, 64, true> for A/4 in {1, ..., 64}; the
# generic head_spmm_any_kernel<VW, CPL>: VW = 2 when d_k is even and the operands allow 8-byte rows, CPL = ceil((A / VW) / 64).
# (1, 2) needs 65..128 scalar columns and (1, 3) 129..192: an odd d_k, so that no two-wide load applies -- A = 75 = 3 x 25 and
# A = 165 = 5 x 33; neither is reached by the SHAPES of tests/test_head_shapes_gpu.py.
HS_VEC4 = [(1, 4), (2, 4), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32)]
HS_ANY = {(4, 2): (2, 1), (8, 30): (2, 2), (3, 3): (1, 1), (3, 25): (1, 2), (5, 33): (1, 3), (7, 35): (1, 4)}


def head_spmm_line(h, dk):
  """What gnpde_head_spmm switches on for an aligned q||k table [n, 2A] (feat = one half, out = a half of a [n, 2A] table):
  ('vec4', A / 4) or ('any', VW, CPL)."""
  A = h * dk
  a4 = A // 4
  if dk % 4 == 0 and a4 <= 64 and a4 & (a4 - 1) == 0:      # (d_k % 4 == 0: ld = 2A is a multiple of 4 and both halves are 16-byte aligned)
    return ('vec4', a4)
  vw = 2 if dk % 2 == 0 else 1          # (d_k even: A is even, ld = 2A is even and both halves are 8-byte aligned; d_k odd: scalar columns)
  av = A // vw
  shift = 0
  while (1 << shift) < av and shift < 6:
    shift += 1
  return ('any', vw, (av + (1 << shift) - 1) >> shift)


HsCase = collections.namedtuple('HsCase', 'h dk by_column')
HS_CASES = [HsCase(h, dk, bc) for h, dk in HS_VEC4 + list(HS_ANY) for bc in (False, True)]


@functools.lru_cache(maxsize=None)
def head_spmm_inputs(c):
  """(graph name, ds [E, h] in edge order, table [n, 2A]): standard normal, drawn directly.  Rows on `hubs`, columns on `hubs_t`, whose
  columns carry the staircase."""
  graph = 'hubs_t' if c.by_column else 'hubs'
  ei, lens, side = RC.graph_edges(graph)
  g = torch.Generator().manual_seed(9000 + 300 * c.h + c.dk)
  return graph, torch.randn(ei.size(1), c.h, generator=g), torch.randn(lens.numel(), 2 * c.h * c.dk, generator=g)


@functools.lru_cache(maxsize=None)
def head_spmm_reference(c):
  """(float64 reference [n, A], tolerance per length class, lens): feat = the k half for rows (d q), the q half for columns (d k)."""
  graph, ds, table = head_spmm_inputs(c)
  ei, lens, side = RC.graph_edges(graph)
  ref = head_sums(ei, ds.double(), table, c.h, c.dk, c.by_column)
  f32 = head_sums(ei, ds, table, c.h, c.dk, c.by_column)
  g, keep = node_rows(f32, lens)
  err, _ = segment_error(g, ref[keep], keep)
  return ref, class_tolerances(err, lens), lens


DS_CASES, DQ_CASES, HR_CASES = _ds_cases(), _dq_cases(), _hr_cases()


def ds_id(c):
  return 'ds-%s-%s%s' % (ref_id(c.ref), c.hubs, '-' + c.variant if c.variant else '')


def dq_id(c):
  return 'dq-%s-%s' % (ref_id(c.ref), c.hubs)


def hr_id(c):
  return 'hr-%s-%s-%s' % (c.side, ref_id(c.ref), c.hubs)


def sb_id(c):
  return 'sb-' + ref_id(c)


def hs_id(c):
  return 'hs-h%d-dk%d-%s' % (c.h, c.dk, 'cols' if c.by_column else 'rows')


def ref_cases():
  """Every RefCase some device case compares with, once."""
  out = []
  for c in [x.ref for x in DS_CASES + DQ_CASES + HR_CASES] + SB_CASES:
    if c not in out:
      out.append(c)
  return out


REF_CASES = ref_cases()
