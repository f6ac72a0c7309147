"""The aggregation (csrc/spmm.hip) judged row by row: the graphs, the operands, the float64 references, the expected launch lines and the
list of launches that tests/test_agg_cases_cpu.py (input validity, on the CPU) and tests/test_spmm_dispatch_gpu.py (every dispatch line
and every stage, on the device) share.  A plain helper module, not a conftest.

Why per row: helpers.assert_parity divides the largest error by the largest value of the WHOLE [n, d] tensor.  With weights of one scale
the aggregate of a 1-entry row is about 30 times smaller than that of an 1100-entry row, so an error of 1e-4 of its own size in a short
row passes a global 1e-5.  Short rows, hub rows and empty rows run different code (two rows per wave / one row per wave / chunk items and
a fold / nothing but the epilogue), so the metric here divides every row's largest error by that row's largest reference value
(row_cases.per_segment_error with one segment per row).

The references are float64: oracle/restate.py's spmm on the very fp32 operands of the launch, upcast, and the eleven stages written out
from include/gnpde.h (gnpde_epilogue_t) and torchdiffeq's tables -- one formula per stage, no association order taken from
csrc/epilogue.h."""
import functools

import torch

from oracle import restate as R
import row_cases as RC

# ------------------------------------------------------------------------------------------------
# the graphs
# ------------------------------------------------------------------------------------------------
# Entries per row, both sides of every length at which a kernel changes what it does: 8- and 16-entry batches (7 | 8 | 9, 15 | 16 | 17),
# 32 (rows(8,1,4)'s batch; own row | shared row in the row-pair kernel), 64 (one coalesced index load per wave), 128, 512 (row | chunks)
STAIRS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512]
# two chunks with a one-entry second chunk, two full chunks, three chunks, and ten chunks: the fold's eight-at-a-time loop AND its remainder
HUBS = [513, 1024, 1025, 1100]
MULTI = 4609              # longer than the graph is wide: its columns repeat, as multi-edges do
EMPTY = 6                 # rows without an entry (besides those of the pair block)
DUP_LEN = 20              # entries of the row that lists one column twice
LONG_ROW = RC.LONG_ROW
# Rows (2i, 2i + 1) of the pair block: what a half-wave of spmm_pair_kernel does depends on the PARTNER row -- both <= 32 entries (own rows),
# one > 32 (both halves share each row in turn), a hub partner (have = false), an empty partner.  Two hub rows come early so that a row
# range can begin behind them and still inside the block.
PAIRS = [(0, 0), (0, 5), (513, 3), (600, 0), (5, 0), (1, 1), (16, 17), (17, 16), (15, 31), (32, 32), (32, 33), (33, 32), (33, 1), (0, 33),
         (40, 0), (512, 3), (3, 512), (3, 513), (513, 1024), (16, 16), (31, 32), (64, 65)]
# 8 * 151: under the contiguous deal every XCD takes exactly 151 rows -- an odd share, so the last pair of EVERY XCD has no second row
# (xcd_row_of returns -1) -- and the pair block (44 rows <= 151, at even ids) lies in XCD 0's share; under the hashed deal (blocks of 16
# rows, an even size) the same rows are still pairs.
N = 1208
XCDS = 8
GRAPHS = {'short': dict(fill=(1, 16), seed=41),       # 2 n_bin16 >= n: the row-pair line for 17..32 16-byte lanes
          'long': dict(fill=(17, 40), seed=42)}       # 2 n_bin16 <  n: the wide-row line
KINDS = tuple(GRAPHS)
ROW_RANGE_BEGIN = 21      # odd, inside the pair block, behind the hub rows 4 (513 entries) and 6 (600)


def agg_graph(n, fill, seed):
  """(edge list [2, E] int64 in shuffled order, lens [n]): rows [0, 2 len(PAIRS)) have the prescribed pair lengths, STAIRS + HUBS + [MULTI] are
  spread over the other ids, EMPTY more rows have no entry, one row of DUP_LEN entries lists a column twice, every other row has
  fill[0]..fill[1] entries.  A row's columns are distinct (but for the dup row and the MULTI row) and contain the row itself."""
  g = torch.Generator().manual_seed(seed)
  lens = torch.randint(fill[0], fill[1] + 1, (n,), generator=g)
  block = 2 * len(PAIRS)
  lens[:block] = torch.tensor(PAIRS).flatten()
  special = STAIRS + HUBS + [MULTI]
  rows = torch.linspace(block + 3, n - 7, len(special)).long()
  assert rows.unique().numel() == len(special) and int(rows.min()) >= block
  lens[rows] = torch.tensor(special)
  taken = set(range(block)) | set(rows.tolist())
  free = [i for i in torch.randperm(n, generator=g).tolist() if i not in taken]
  for i in free[:EMPTY]:
    lens[i] = 0
  dup = free[EMPTY]
  lens[dup] = DUP_LEN
  src, dst = [], []
  for i in range(n):
    m = int(lens[i])
    if m == 0:
      continue
    if m > n:
      cols = [torch.tensor([i]), torch.randint(0, n, (m - 1,), generator=g)]
    else:
      others = torch.randperm(n - 1, generator=g)[:m - 1 - int(i == dup)]
      others = others + (others >= i).long()          # distinct columns, none of them i
      cols = [torch.tensor([i]), others] + ([others[:1]] if i == dup else [])
    src.append(torch.full((m,), i))
    dst.append(torch.cat(cols))
  ei = torch.stack([torch.cat(src), torch.cat(dst)])
  ei = ei[:, torch.randperm(ei.size(1), generator=g)].long()
  assert torch.equal(torch.bincount(ei[0], minlength=n), lens)
  return ei, lens


@functools.lru_cache(maxsize=None)
def graph_edges(kind):
  """(ei [2, E], lens [n], edge weights [E] in edge order: rand * 0.3 + 0.01)"""
  kw = GRAPHS[kind]
  ei, lens = agg_graph(N, kw['fill'], kw['seed'])
  w = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(kw['seed'] + 100)) * 0.3 + 0.01
  return ei, lens, w


def xcd_lists(n, row_begin, shift):
  """Host restatement of xcd_row_of (csrc/common.h): the row list of each of the 8 XCDs, -1 = no row.  shift < 0: contiguous eighths;
  else blocks of 2^shift rows, eight consecutive blocks a group, the XCDs taking the blocks of group j rotated by a hash of j."""
  rn = n - row_begin
  if shift < 0:
    per = (rn + XCDS - 1) // XCDS
    return [[row_begin + x * per + r if row_begin + x * per + r < n else -1 for r in range(per)] for x in range(XCDS)]
  nb = (rn + (1 << shift) - 1) >> shift
  per = ((nb + XCDS - 1) // XCDS) << shift
  out = []
  for x in range(XCDS):
    rows = []
    for r in range(per):
      j, i = r >> shift, r & ((1 << shift) - 1)
      rot = ((j * 2654435761) & 0xffffffff) >> 29
      row = row_begin + ((j * XCDS + ((x + rot) & (XCDS - 1))) << shift) + i
      rows.append(row if row < n else -1)
    out.append(rows)
  return out


# ------------------------------------------------------------------------------------------------
# widths and the line each takes (width_class of csrc/spmm.hip; the literal table of tests/test_spmm_plan_cpu.py)
# ------------------------------------------------------------------------------------------------
# widths by lane type; the comment gives (lanes per row -> line of the table)
LANES16 = [24,    # 6: rows (8, 1, 4)
           64,    # 16: rows (16, 1, 4)
           80, 100, 128,   # 20, 25, 32 (128: no column predicate): row pairs on the short-row graph, wide L = 32 on the long-row graph
           200, 256,       # 50, 64 (256: no column predicate): wide L = 64
           300,   # 75: rows (64, 2, 2)     -- from here on the fold's column loop takes a second pass (d > 256)
           520,   # 130: rows (64, 3, 1)
           800]   # 200: rows (64, 4, 1)
LANES8 = [6, 30, 50, 90, 162, 302, 402]     # 3, 15, 25, 45, 81, 151, 201 lanes: rows (8,1,4) (16,1,4) (16,2,4) (32,2,4) (64,2,2) (64,3,1) (64,4,1)
LANES4 = [7, 15, 31, 63, 127, 191, 255]     # the same seven lines on 4-byte lanes
WIDTHS = LANES16 + LANES8 + LANES4
_SEVEN = [(8, 1, 4), (16, 1, 4), (16, 2, 4), (32, 2, 4), (64, 2, 2), (64, 3, 1), (64, 4, 1)]
_ROWS16 = {24: (8, 1, 4), 64: (16, 1, 4), 300: (64, 2, 2), 520: (64, 3, 1), 800: (64, 4, 1)}


def lane_bytes(d):
  return 16 if d in LANES16 else 8 if d in LANES8 else 4


def rows_line(slots):
  """The rows (L, K, U) line of a row covered by `slots` lanes where neither the row-pair nor the wide-row kernel runs."""
  return _SEVEN[[i for i, top in enumerate((8, 16, 32, 64, 128, 192, 256)) if slots <= top][0]]


def intended(kind, d, lanes=None, quad=False):
  """(lane bytes, kernel family, L, K, U) a contiguous, aligned call of width d is there to run; lanes: the demoted lane type of an
  unaligned call; quad: the bf16 operand under gnpde_tune(18, 2)."""
  lanes = lane_bytes(d) if lanes is None else lanes
  if lanes < 16:
    return (lanes, 'rows') + rows_line((d + lanes // 4 - 1) // (lanes // 4))
  if d in _ROWS16:
    return (16, 'rows') + _ROWS16[d]
  if d <= 128:
    if kind == 'short':
      return (16, 'quad_lo', 16, 1, 16) if quad and d % 8 == 0 else (16, 'pair', 32, 1, 16)
    return (16, 'wide', 32, 1, 8)
  return (16, 'wide', 64, 1, 8)


def plan_line(p):
  return (p.lane_bytes, p.kernel, p.L, p.K, p.U)


# ------------------------------------------------------------------------------------------------
# the launches
# ------------------------------------------------------------------------------------------------
STAGES = ['RHS', 'EULER', 'RK1', 'RK2', 'RK3', 'RK4', 'RK1C', 'RK2C', 'RK3C', 'RK4C', 'LINCOMB']
PREFETCHABLE = ['RHS', 'EULER', 'RK1C', 'RK2C', 'RK3C', 'RK4C']       # stage_prefetchable: fold_stage / epilogue_pre; the others: epilogue<>
# what a stage reads besides u and x0, and what it writes (gnpde_epilogue_t); p0, p1: LINCOMB's earlier derivatives prev[0], prev[1]
READS = {'RHS': (), 'EULER': ('y',), 'RK1': ('y',), 'RK2': ('y', 'k1'), 'RK3': ('y', 'k1', 'k2'), 'RK4': ('y', 'k1', 'k2', 'k3'),
         'RK1C': (), 'RK2C': ('y',), 'RK3C': ('k1',), 'RK4C': ('y', 'k1'), 'LINCOMB': ('y', 'p0', 'p1')}
WRITES = {'RHS': ('out_k',), 'EULER': ('out_y',), 'RK1': ('out_k', 'out_y'), 'RK2': ('out_k', 'out_y'), 'RK3': ('out_k', 'out_y'),
          'RK4': ('out_y',), 'RK1C': ('out_y',), 'RK2C': ('out_y',), 'RK3C': ('out_y',), 'RK4C': ('out_y',), 'LINCOMB': ('out_k', 'out_y')}
OPERANDS = ('u', 'x0', 'y', 'k1', 'k2', 'k3', 'p0', 'p1')


def f32(v):
  """the value a float argument has once it is an fp32 field of gnpde_epilogue_t or an fp32 device scalar"""
  return float(torch.tensor(v, dtype=torch.float32))


ALPHA, BETA, DT = f32(0.3), f32(-0.7), f32(0.7)
COEF = (f32(0.31), f32(-0.45), f32(0.62))     # LINCOMB with n_prev = 2: the weights of prev[0], prev[1] and k
VARIANT_WIDTHS = (100, 50, 31)                # one width per lane type also runs without a source term and with alpha taken as it is

PLAIN = ('plain', True, True)                 # a launch: (stage name or 'plain', with x0, alpha through the sigmoid)


def launches(d, stages=STAGES, variants=None):
  variants = d in VARIANT_WIDTHS if variants is None else variants
  out = [PLAIN] + [(s, True, True) for s in stages]
  if variants:
    out += [(s, False, True) for s in stages] + [(s, True, False) for s in stages]
  return out


def launch_id(launch):
  return '%s%s%s' % (launch[0], '' if launch[1] else '-nox0', '' if launch[2] else '-rawalpha')


def fold_kind(kind, d, launch, tickets=False, lanes=None, lo=False):
  """The hub-row fold of a launch over the whole graph: spmm_long_reduce4_kernel on 16-byte lanes, the scalar spmm_long_reduce_kernel on
  narrower ones, and the last chunk item of the row-pair kernel where tickets are given and fold_stage states the stage."""
  line = intended(kind, d, lanes)
  if line[0] < 16:
    return 'scalar'
  if lo:
    return 'reduce4_lo'
  return 'in_kernel' if (tickets and line[1] == 'pair' and launch[0] in PREFETCHABLE) else 'reduce4'


@functools.lru_cache(maxsize=64)
def operands(kind, d, bf16=False):
  """{name: fp32 [n, d]} seeded standard-normal tensors, a different one for every operand.  bf16: u is rounded to bfloat16 and widened
  again, so that the bf16 shadow of u holds u exactly.  The caller must not write to them."""
  g = torch.Generator().manual_seed(7000 + 3 * d + KINDS.index(kind))
  t = {name: torch.randn(N, d, generator=g) for name in OPERANDS}
  if bf16:
    t['u'] = t['u'].to(torch.bfloat16).float()
  return t


# ------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------
def aggregate(kind, d, dtype, bf16=False):
  ei, lens, w = graph_edges(kind)
  return R.spmm(ei, w.to(dtype), N, operands(kind, d, bf16)['u'].to(dtype))


@functools.lru_cache(maxsize=None)
def aggregate64(kind, d, bf16=False):
  """A u in float64 from the upcast fp32 operands: computed once per (graph, d) and shared by every launch of it; left unchanged."""
  return aggregate(kind, d, torch.float64, bf16)


def stage_reference(launch, ax, t):
  """{output name: [n, d]} of a launch in the dtype of ax: ax = A u, t = the operands in the same dtype."""
  stage, with_x0, sigmoid = launch
  if stage == 'plain':
    return {'out': ax}
  a = torch.tensor(ALPHA, dtype=ax.dtype)
  a = torch.sigmoid(a) if sigmoid else a
  k = a * (ax - t['u'])
  if with_x0:
    k = k + BETA * t['x0']
  u, y, k1, k2, k3 = t['u'], t['y'], t['k1'], t['k2'], t['k3']
  if stage == 'RHS':
    return {'out_k': k}
  if stage == 'EULER':
    return {'out_y': y + DT * k}
  if stage == 'RK1':                       # the 3/8 rule: y + dt k1 / 3
    return {'out_k': k, 'out_y': y + DT * k / 3}
  if stage == 'RK2':                       # y + dt (k2 - k1 / 3)
    return {'out_k': k, 'out_y': y + DT * (k - k1 / 3)}
  if stage == 'RK3':                       # y + dt (k1 - k2 + k3)
    return {'out_k': k, 'out_y': y + DT * (k1 - k2 + k)}
  if stage == 'RK4':                       # y + dt (k1 + 3 k2 + 3 k3 + k4) / 8
    return {'out_y': y + DT * (k1 + 3 * k2 + 3 * k3 + k) / 8}
  if stage == 'RK1C':                      # the compact forms: the same step through the previous stage INPUTS (u == y here)
    return {'out_y': u + DT * k / 3}
  if stage == 'RK2C':                      # u == u2
    return {'out_y': 2 * y - u + DT * k}
  if stage == 'RK3C':                      # u == u3, field k1 holds u2
    return {'out_y': 2 * k1 - u + DT * k}
  if stage == 'RK4C':                      # u == u4, field k1 holds u3
    return {'out_y': (6 * k1 + 3 * u - y + DT * k) / 8}
  assert stage == 'LINCOMB'
  return {'out_k': k, 'out_y': y + COEF[0] * t['p0'] + COEF[1] * t['p1'] + COEF[2] * k}


def reference(kind, d, launch, dtype=torch.float64, bf16=False):
  ax = aggregate64(kind, d, bf16) if dtype == torch.float64 else aggregate(kind, d, dtype, bf16)
  return stage_reference(launch, ax, {k: v.to(dtype) for k, v in operands(kind, d, bf16).items()})


# ------------------------------------------------------------------------------------------------
# the metric
# ------------------------------------------------------------------------------------------------
ROWS = torch.arange(N)


def row_errors(got, ref64, rows=slice(None)):
  """per row: largest |got - ref| of the row / largest |ref| of the row"""
  return RC.per_segment_error(got[rows], ref64[rows], torch.arange(ref64[rows].shape[0]))


def class_errors(got, ref64, lens, rows=slice(None)):
  return RC.class_errors(row_errors(got, ref64, rows), lens[rows])


def assert_rows(got, ref64, lens, tol, what='', rows=slice(None)):
  """Every row of `rows` (a slice) is finite and within tol of the reference by its own scale -- hub, empty and pair-block rows included;
  returns the worst error per length class.  Empty rows are a class of their own here ('0': their output is the epilogue of ax = 0)."""
  got, ref64, lens = got[rows], ref64[rows], lens[rows]
  per_class = RC.assert_rows(got, ref64, torch.arange(ref64.shape[0]), lens, tol, what)
  empty = lens == 0
  if bool(empty.any()):
    per_class['0'] = float(RC.per_segment_error(got[empty], ref64[empty], torch.arange(int(empty.sum()))).max())
  return per_class


def worst(into, per_class):
  for k, v in per_class.items():
    into[k] = max(into.get(k, 0.0), v)
  return into
