"""The case table of the projection's dispatch tests (csrc/linear.hip: plan_next / plan_tile choose among 36 kernel instantiations).

A case is (n, d, m, x view, W view, out view, relu, bias) and the line or lines ops.linear must take for it, in launch order.
test_linear_dispatch_cpu.py checks the table against gnpde_linear_plan without a GPU (addresses are modelled: only their alignment
is read); test_linear_dispatch_gpu.py builds the same operands on the device, asserts the same plan and runs them.

Views
  x    'dense'  ldx = d                          'pad4'  ldx = d + 4 (padded rows, still 16-byte aligned when d % 4 == 0)
       'col1'   columns 1 .. d of [n, d + 4]: the pointer is 4 bytes past 16-byte alignment
       'ld1'    ldx = d + 1: rows lose 16-byte alignment
  W    'dense'  or 'off1': a contiguous [m, d] matrix that starts 4 bytes past 16-byte alignment
  out  None     a fresh [n, m] tensor (ldo = m), or (extra, c0): columns c0 .. c0 + m of a NaN-filled [n + 1, m + extra] buffer

Which line a shape takes (the rules of plan_next / plan_tile, restated here only as a reading aid for the table):
  * n <= 32 768, aligned operands, d % 16 == 0 and m % 16 == 0: small<2> (m % 32 == 0) or small<1>, one launch.
  * otherwise columns go left to right in launches of 8, 4, 2 or 1 column tiles by the tiles still to go, so a launch of ONE complete
    column tile (persistent<1,.>, staged<1,.>, tile<1,1,1>) only ever ends an m % 16 == 0 product -- which the small rule takes up to
    32 768 rows.  Those nine lines therefore have their short case at n = 32 769 (2 049 row tiles, the last of one row) and none at
    n = 1 / 201; every other line has both.
"""
import collections

Case = collections.namedtuple('Case', 'id n d m xv wv ov relu bias lines tall att_dim')

BASE = 1 << 20          # modelled allocation address: the allocator's alignment (>= 256 bytes) is all that matters

ALL_LINES = (['small<1>', 'small<2>', 'staged2<4>', 'staged2<8>'] +
             ['staged<%d,%d>' % (mt, kb) for mt in (1, 2) for kb in (4, 8)] +
             ['persistent<%d,%d>' % (mt, kb) for mt in (1, 2) for kb in (1, 2, 3, 5, 6, 7)] +
             ['lds<%d,%d>' % (mt, dmax) for mt in (4, 8) for dmax in (128, 256)] +
             ['tile<%d,%s>' % (mt, af) for mt in (1, 2, 4, 8) for af in ('1,1', '1,0', '0,0')])
SPLIT_LINES = ['staged2<4>+split', 'staged2<8>+split']
assert len(ALL_LINES) == 36 and len(set(ALL_LINES)) == 36

RAG = ['tile<1,1,0>']       # the ragged last column tile of an aligned product
# (d, m, x view, W view, out view of BOTH variants or None, lines): each runs at n = 1 and n = 201
SHORT_SHAPES = [
  (48, 48, None, None, None, ['small<1>']),
  (64, 64, None, None, None, ['small<2>']),
  (272, 16, None, None, None, ['small<1>']),                # K batches of 8 blocks: 17 blocks = 2 full batches + 1
  (144, 96, None, None, None, ['small<2>']),
  (64, 34, None, None, None, ['staged2<4>'] + RAG),         # even ldo, even column base, 8-byte aligned out (B: window (6, 2))
  (128, 34, None, None, None, ['staged2<8>'] + RAG),
  (64, 33, None, None, None, ['staged<2,4>'] + RAG),        # odd ldo (A: 33, B: 39)
  (128, 33, None, None, None, ['staged<2,8>'] + RAG),       # A: odd ldo; B: even ldo 40 but c0 = 3, out 4 bytes off 8-byte alignment
  (128, 34, None, None, (6, 1), ['staged<2,8>'] + RAG),     # even ldo 40, c0 = 1
  (16, 33, None, None, None, ['persistent<2,1>'] + RAG),
  (32, 33, None, None, None, ['persistent<2,2>'] + RAG),
  (48, 33, None, None, None, ['persistent<2,3>'] + RAG),
  (80, 33, None, None, None, ['persistent<2,5>'] + RAG),
  (96, 33, None, None, None, ['persistent<2,6>'] + RAG),
  (112, 33, None, None, None, ['persistent<2,7>'] + RAG),
  (16, 72, None, None, None, ['lds<4,128>'] + RAG),         # nkb = 1 against KU = 4
  (32, 72, None, None, None, ['lds<4,128>'] + RAG),         # nkb = 2
  (128, 72, None, None, None, ['lds<4,128>'] + RAG),        # nkb = 8: the widest DMAX = 128
  (48, 136, None, None, None, ['lds<8,128>'] + RAG),        # nkb = 3
  (80, 136, None, None, None, ['lds<8,128>'] + RAG),        # nkb = 5
  (128, 136, None, None, None, ['lds<8,128>'] + RAG),
  (144, 72, None, None, None, ['lds<4,256>'] + RAG),        # nkb = 9: the narrowest DMAX = 256
  (176, 72, None, None, None, ['lds<4,256>'] + RAG),        # nkb = 11
  (256, 72, None, None, None, ['lds<4,256>'] + RAG),
  (176, 136, None, None, None, ['lds<8,256>'] + RAG),
  (256, 136, None, None, None, ['lds<8,256>'] + RAG),       # nkb = 16
  (144, 33, None, None, None, ['tile<2,1,1>'] + RAG),       # d > 128
  (272, 72, None, None, None, ['tile<4,1,1>'] + RAG),       # d > 256
  (272, 136, None, None, None, ['tile<8,1,1>'] + RAG),
  (20, 136, None, None, None, ['tile<8,1,0>'] + RAG),       # ragged K on 16-byte loads
  (20, 72, None, None, None, ['tile<4,1,0>'] + RAG),
  (20, 40, None, None, None, ['tile<2,1,0>'] + RAG),
  (100, 40, None, None, None, ['tile<2,1,0>'] + RAG),       # 6 K blocks + 4: a full batch, then a ragged one
  (64, 17, None, None, None, ['tile<2,1,0>']),              # ragged columns only
  (30, 136, None, None, None, ['tile<8,0,0>', 'tile<1,0,0>']),   # ldx = 30 / 34, ldw = 30: scalar loads
  (30, 72, None, None, None, ['tile<4,0,0>', 'tile<1,0,0>']),
  (30, 40, None, None, None, ['tile<2,0,0>', 'tile<1,0,0>']),
  (64, 32, 'col1', None, None, ['tile<2,0,0>']),            # x starts at column 1
  (64, 48, None, 'off1', None, ['tile<2,0,0>', 'tile<1,0,0>']),  # W 4 bytes off
  (64, 16, 'ld1', None, None, ['tile<1,0,0>']),             # ldx % 4 != 0
]

# n = 32 769: the first row count past the small rule -- the only way to a launch of one complete column tile
MID_SHAPES = [(16 * kb, 48, (6, 2), ['persistent<2,%d>' % kb, 'persistent<1,%d>' % kb]) for kb in (1, 2, 3, 5, 6, 7)] + [
  (64, 48, (6, 2), ['staged2<4>', 'staged<1,4>']),
  (128, 48, (7, 2), ['staged<2,8>', 'staged<1,8>']),        # odd ldo 55
  (144, 48, (5, 3), ['tile<2,1,1>', 'tile<1,1,1>']),
  (48, 240, (6, 2), ['lds<8,128>', 'lds<4,128>', 'persistent<2,3>', 'persistent<1,3>']),   # 8, 4, 2, 1 column tiles to go
]
MID_N = 32769

# tall: every wave runs two row tiles and waves 0..5 a third, the very last tile ragged (7 rows).  n = 16 (2 waves + 5) + 7 with
# waves = grid.x * (block / 64) of the line's launch; the CPU test derives the same from the plan's grid.
TALL_SHAPES = [
  (98391, 16, 16, (6, 2), ['persistent<1,1>']),
  (98391, 112, 32, (5, 3), ['persistent<2,7>']),
  (98391, 128, 16, (6, 2), ['staged<1,8>']),
  (98391, 64, 32, (7, 2), ['staged<2,4>']),                 # odd ldo 39
  (131159, 64, 32, (6, 2), ['staged2<4>']),
  (131159, 128, 32, (6, 2), ['staged2<8>']),
  (262231, 80, 64, (5, 3), ['lds<4,128>']),                 # nkb = 5: a full K batch and a guarded one, in every tile
  (131159, 48, 128, (6, 2), ['lds<8,128>']),                # nkb = 3 < KU
  (131159, 176, 64, (6, 2), ['lds<4,256>']),
  (65623, 256, 128, (5, 3), ['lds<8,256>']),
]
SPLIT_SHAPES = [(131159, 64, ['staged2<4>+split']), (131159, 128, ['staged2<8>+split'])]     # ops.qk_tables, att_dim = 16


def _cases():
  out = []
  for i, (d, m, xv, wv, ov, lines) in enumerate(SHORT_SHAPES):
    tag = 'd%d-m%d-%s' % (d, m, lines[0]) + ('' if ov is None else '-c%d' % ov[1]) + ('' if xv is None else '-' + xv) + ('' if wv is None else '-' + wv)
    # A: one row, plain operands, no bias.  B: 13 row tiles with a 9-row last one, padded x rows, out a window of a NaN buffer.
    out.append(Case('n1-' + tag, 1, d, m, xv or 'dense', wv or 'dense', ov, False, False, lines, False, 0))
    if ov is None:
      window = {('staged2<4>',): (6, 2), ('staged2<8>',): (6, 2), ('staged<2,4>',): (6, 2), ('staged<2,8>',): (7, 3)}.get(
        (lines[0],), (5, 3) if i % 4 < 2 else (6, 2))
    else:
      window = ov
    out.append(Case('n201-' + tag, 201, d, m, xv or 'pad4', wv or 'dense', window, i % 2 == 0, True, lines, False, 0))
  for d, m, ov, lines in MID_SHAPES:
    out.append(Case('n%d-d%d-m%d-%s' % (MID_N, d, m, lines[-1]), MID_N, d, m, 'pad4', 'dense', ov, False, True, lines, False, 0))
  for n, d, m, ov, lines in TALL_SHAPES:
    out.append(Case('tall-n%d-d%d-m%d-%s' % (n, d, m, lines[0]), n, d, m, 'pad4', 'dense', ov, False, True, lines, True, 0))
  for n, d, lines in SPLIT_SHAPES:
    out.append(Case('tall-n%d-d%d-%s' % (n, d, lines[0]), n, d, 32, 'dense', 'dense', None, False, True, lines, True, 16))
  return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)


def geometry(c):
  """(ldx, x offset, ldw, W offset, ldo, out offset) of a case's operands, offsets in floats from an aligned allocation."""
  ldx, xoff = {'dense': (c.d, 0), 'pad4': (c.d + 4, 0), 'col1': (c.d + 4, 1), 'ld1': (c.d + 1, 0)}[c.xv]
  woff = {'dense': 0, 'off1': 1}[c.wv]
  ldo, ooff = (c.m, 0) if c.ov is None else (c.m + c.ov[0], c.ov[1])
  assert ooff + c.m <= ldo
  return ldx, xoff, c.d, woff, ldo, ooff


def takes_padded_copies(n, d, ldx, ldw):
  """ops.linear's rule for running on zero-padded copies of both operands (no case of the table may meet it: the table is about the
  operands as given)."""
  return n >= 4096 and (d % 16 != 0 or ldx % 4 != 0 or ldw % 4 != 0)


def modelled_launches(L, struct, n, d, m, ldx=None, xoff=0, woff=0, ldo=None, ooff=0):
  """gnpde_linear_plan for operands at modelled addresses (no device)."""
  ldx = d if ldx is None else ldx
  ldo = m if ldo is None else ldo
  args = (BASE + 4 * xoff, n, d, ldx, BASE + 4 * woff, m, d, BASE + 4 * ooff, ldo)
  count = L.gnpde_linear_plan(*args, None, 0)
  assert count >= 0, L.gnpde_last_error()
  plan = (struct * max(count, 1))()
  assert L.gnpde_linear_plan(*args, plan, count) == count
  return list(plan[:count])
