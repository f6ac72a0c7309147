"""The projection's launch decision (gnpde_linear_plan: the function the launchers of csrc/linear.hip switch on) against the case table
of linear_cases.py, without a GPU: every case takes the lines the table says, the table reaches all 36 instantiations and both split
forms, the tall cases make every wave run a second row tile and some a third, and the decision turns where the rules say it does."""
import ctypes

import pytest

from gnpde_amd import _lib
import linear_cases as LC


def launches(n, d, m, **kw):
  return LC.modelled_launches(_lib.lib(), _lib.LinearLaunchStruct, n, d, m, **kw)


def lines(n, d, m, **kw):
  return [l.line for l in launches(n, d, m, **kw)]


def case_launches(c):
  if c.att_dim:
    one = _lib.LinearLaunchStruct()
    rc = _lib.lib().gnpde_linear_split_plan(LC.BASE, c.n, c.d, c.d, LC.BASE, c.m, c.d, LC.BASE, LC.BASE + 4 * c.n * c.att_dim, c.att_dim,
                                            ctypes.byref(one))
    assert rc == 1, _lib.lib().gnpde_last_error()
    return [one]
  ldx, xoff, ldw, woff, ldo, ooff = LC.geometry(c)
  assert not LC.takes_padded_copies(c.n, c.d, ldx, ldw), 'the table is about operands as given'
  return launches(c.n, c.d, c.m, ldx=ldx, xoff=xoff, woff=woff, ldo=ldo, ooff=ooff)


@pytest.mark.parametrize('c', LC.CASES, ids=lambda c: c.id)
def test_case_takes_the_lines_of_the_table(c):
  plan = case_launches(c)
  assert [l.line for l in plan] == c.lines
  # the launches tile the output columns left to right, each on a grid that covers every row tile at least once per stride
  col = 0
  tiles = (c.n + 15) // 16
  for l in plan:
    assert l.col_base == col and 1 <= l.cols <= (c.m if l.line.startswith('small') else 16 * l.mt)
    assert l.block in (256, 512) and 1 <= l.grid_x <= (tiles + l.block // 64 - 1) // (l.block // 64)
    assert l.grid_y == (c.m // (16 * l.mt) if l.line.startswith('small') else 1)
    col += l.cols
  assert col == c.m


def test_table_reaches_every_instantiation():
  seen = {line for c in LC.CASES for line in c.lines}
  assert seen == set(LC.ALL_LINES) | set(LC.SPLIT_LINES), (sorted(set(LC.ALL_LINES) - seen), sorted(seen - set(LC.ALL_LINES)))
  # n = 1 and n = 201 at every line a short product can reach (see linear_cases: a single complete column tile needs n > 32 768)
  needs_mid = {l for l in LC.ALL_LINES if l.startswith(('persistent<1,', 'staged<1,')) or l == 'tile<1,1,1>'}
  for n in (1, 201):
    assert {line for c in LC.CASES if c.n == n for line in c.lines} == set(LC.ALL_LINES) - needs_mid
  assert needs_mid <= {line for c in LC.CASES if c.n == LC.MID_N for line in c.lines}
  # each family once with relu on the A operand and once without a bias
  for fam in _lib.LINEAR_FAMILIES:
    of = [c for c in LC.CASES if any(l.startswith(fam + '<') for l in c.lines)]
    assert any(c.relu for c in of) and any(not c.bias for c in of) and any(c.bias and not c.relu for c in of), fam
  # tall: one per family and MT of the grid-stride kernels, and both split forms
  tall = {line for c in LC.CASES if c.tall for line in c.lines}
  assert tall == {'persistent<1,1>', 'persistent<2,7>', 'staged<1,8>', 'staged<2,4>', 'staged2<4>', 'staged2<8>', 'lds<4,128>', 'lds<8,128>',
                  'lds<4,256>', 'lds<8,256>'} | set(LC.SPLIT_LINES)
  # out windows at even and odd ldo and c0
  wins = {(LC.geometry(c)[4] % 2, LC.geometry(c)[5] % 2) for c in LC.CASES if c.ov is not None}
  assert wins == {(0, 0), (0, 1), (1, 0), (1, 1)}


@pytest.mark.parametrize('c', [c for c in LC.CASES if c.tall], ids=lambda c: c.id)
def test_tall_case_strides(c):
  """Every wave of the launch runs two row tiles, waves 0..5 a third, and the last -- ragged -- tile is one of those third iterations."""
  (l,) = case_launches(c)
  waves = l.grid_x * (l.block // 64)
  tiles = (c.n + 15) // 16
  assert tiles >= 2 * waves + 6
  assert c.n % 16 != 0 and (tiles - 1) // waves == 2
  assert tiles <= 2 * waves + 16, 'no larger than the stride condition needs'


def test_small_rule_ends_at_32768_rows():
  assert lines(32768, 64, 32) == ['small<2>'] and lines(32768, 64, 48) == ['small<1>']
  assert lines(32769, 64, 32) == ['staged2<4>'] and lines(32769, 64, 48) == ['staged2<4>', 'staged<1,4>']
  assert lines(32768, 272, 256) == ['small<2>'] and lines(32769, 272, 256) == ['tile<8,1,1>', 'tile<8,1,1>']
  small = launches(32768, 64, 96)[0]
  assert (small.grid_x, small.grid_y, small.block, small.cols) == (512, 3, 256, 96)
  # the rule wants aligned operands, complete K blocks and complete column tiles
  assert lines(201, 64, 32, xoff=1, ldx=68) == ['tile<2,0,0>']
  assert lines(201, 60, 32) == ['tile<2,1,0>'] and lines(201, 64, 31) == ['tile<2,1,0>']


def test_width_boundaries():
  n = 40000
  assert lines(n, 128, 32) == ['staged2<8>'] and lines(n, 144, 32) == ['tile<2,1,1>']
  assert lines(n, 112, 16) == ['persistent<1,7>'] and lines(n, 128, 16) == ['staged<1,8>'] and lines(n, 144, 16) == ['tile<1,1,1>']
  assert lines(n, 128, 64) == ['lds<4,128>'] and lines(n, 144, 64) == ['lds<4,256>']
  assert lines(n, 128, 128) == ['lds<8,128>'] and lines(n, 144, 128) == ['lds<8,256>']
  assert lines(n, 256, 64) == ['lds<4,256>'] and lines(n, 272, 64) == ['tile<4,1,1>']
  assert lines(n, 256, 128) == ['lds<8,256>'] and lines(n, 272, 128) == ['tile<8,1,1>']
  # grids: 3 / 4 workgroups of 256 per CU for the register / paired kernels, 512-thread workgroups for the LDS ones, capped by the tiles
  tiles = (n + 15) // 16
  assert [launches(n, d, m)[0].grid_x for d, m in ((112, 32), (128, 32), (128, 64), (128, 128), (256, 64), (256, 128), (272, 64))] == \
         [(tiles + 3) // 4, (tiles + 3) // 4, (tiles + 7) // 8, (tiles + 7) // 8, (tiles + 7) // 8, 256, (tiles + 3) // 4]
  assert [launches(200000, d, m)[0].grid_x for d, m in ((112, 32), (128, 32), (128, 64), (128, 128), (256, 64), (256, 128))] == \
         [768, 1024, 1024, 512, 512, 256]
  assert [launches(200000, d, m)[0].block for d, m in ((112, 32), (128, 32), (128, 64), (272, 64))] == [256, 256, 512, 256]


def test_column_tiles_still_to_go():
  """8, 4, 2 or 1 column tiles by what is left; a ragged last tile takes the guarded kernel at the width of what is left."""
  n = 40000
  plan = launches(n, 48, 240)
  assert [(l.line, l.col_base, l.cols) for l in plan] == [('lds<8,128>', 0, 128), ('lds<4,128>', 128, 64), ('persistent<2,3>', 192, 32),
                                                          ('persistent<1,3>', 224, 16)]
  assert lines(n, 48, 256) == ['lds<8,128>', 'lds<8,128>']
  assert lines(n, 48, 128 + 16) == ['lds<8,128>', 'persistent<1,3>']
  assert lines(n, 48, 112) == ['lds<4,128>', 'persistent<2,3>', 'persistent<1,3>']        # 7 tiles: 4 + 2 + 1
  assert [(l.line, l.col_base, l.cols) for l in launches(n, 48, 120)] == [('tile<8,1,0>', 0, 120)]     # 8 tiles to go, the eighth ragged
  assert lines(n, 48, 50) == ['tile<4,1,0>']                                                # 4 tiles to go, the fourth ragged
  assert lines(n, 48, 33) == ['persistent<2,3>', 'tile<1,1,0>'] and lines(n, 48, 17) == ['tile<2,1,0>'] and lines(n, 48, 5) == ['tile<1,1,0>']


def test_paired_stores_want_an_even_aligned_out():
  n = 40000
  for d, kb in ((64, 4), (128, 8)):
    assert lines(n, d, 32) == ['staged2<%d>' % kb]
    assert lines(n, d, 32, ldo=33) == ['staged<2,%d>' % kb]                 # odd ldo: odd rows would start 4 bytes off
    assert lines(n, d, 32, ldo=34, ooff=1) == ['staged<2,%d>' % kb]         # out itself 4 bytes off
    assert lines(n, d, 32, ldo=34, ooff=2) == ['staged2<%d>' % kb]
    assert lines(n, d, 64, ldo=65) == ['lds<4,128>']                        # only the 32-column launch has a paired form
    assert lines(n, d, 96, ldo=97) == ['lds<4,128>', 'staged<2,%d>' % kb] and lines(n, d, 96) == ['lds<4,128>', 'staged2<%d>' % kb]


def test_operand_alignment():
  n = 40000
  assert lines(n, 64, 32, ldx=68) == ['staged2<4>']                         # padded rows keep 16-byte loads
  assert lines(n, 64, 32, ldx=65) == ['tile<2,0,0>']                        # ldx % 4 != 0
  assert lines(n, 64, 32, ldx=68, xoff=1) == ['tile<2,0,0>']                # x starts at column 1
  assert lines(n, 64, 32, woff=1) == ['tile<2,0,0>']
  assert lines(n, 62, 32) == ['tile<2,0,0>']                                # ldw = d = 62
  assert lines(n, 64, 240, xoff=2, ldx=68) == ['tile<8,0,0>', 'tile<4,0,0>', 'tile<2,0,0>', 'tile<1,0,0>']
  assert lines(n, 60, 240) == ['tile<8,1,0>', 'tile<4,1,0>', 'tile<2,1,0>', 'tile<1,1,0>']    # ragged K on aligned operands


def test_split_plan_follows_linear_split_supported():
  L = _lib.lib()
  one = _lib.LinearLaunchStruct()
  for d, kb in ((64, 4), (128, 8)):
    assert L.gnpde_linear_split_plan(LC.BASE, 40000, d, d, LC.BASE, 32, d, LC.BASE, LC.BASE + 64 * 40000, 16, ctypes.byref(one)) == 1
    assert (one.line, one.split, one.cols, one.grid_x, one.grid_y, one.block) == ('staged2<%d>+split' % kb, 1, 32, 625, 1, 256)
  assert L.gnpde_linear_split_plan(LC.BASE, 200000, 64, 64, LC.BASE, 32, 64, LC.BASE, LC.BASE + 64 * 200000, 16, ctypes.byref(one)) == 1
  assert one.grid_x == 1024
  for bad in (dict(n=32768), dict(d=48), dict(m=64), dict(split=8), dict(ldx=65), dict(q=LC.BASE + 4)):
    a = dict(n=40000, d=64, m=32, split=16, ldx=64, q=LC.BASE)
    a.update(bad)
    rc = L.gnpde_linear_split_plan(LC.BASE, a['n'], a['d'], max(a['ldx'], a['d']), LC.BASE, a['m'], a['d'], a['q'], LC.BASE + 64 * a['n'],
                                   a['split'], ctypes.byref(one))
    assert rc < 0 and b'linear_split_plan' in L.gnpde_last_error(), bad
    assert bool(L.gnpde_linear_split_supported(ctypes.c_void_p(LC.BASE), a['n'], a['d'], max(a['ldx'], a['d']), ctypes.c_void_p(LC.BASE), a['m'],
                                               a['d'], a['split'])) == ('q' in bad)


def test_plan_counts_and_cap():
  L = _lib.lib()
  args = (LC.BASE, 40000, 48, 48, LC.BASE, 240, 48, LC.BASE, 240)
  assert L.gnpde_linear_plan(*args, None, 0) == 4
  two = (_lib.LinearLaunchStruct * 3)()
  two[2].family = 77
  assert L.gnpde_linear_plan(*args, two, 2) == 4                        # the count, however many fit
  assert [two[0].line, two[1].line] == ['lds<8,128>', 'lds<4,128>'] and two[2].family == 77
  assert L.gnpde_linear_plan(LC.BASE, 0, 48, 48, LC.BASE, 240, 48, LC.BASE, 240, None, 0) == 0     # n = 0 launches nothing


def test_the_bound_tells_a_wrong_entry_from_rounding():
  """The GPU test's entry-by-entry bound on the CPU: fp32 BLAS and a sequential fp32 chain pass it; one dropped product, a neighbour's
  bias, a neighbour's row or a NaN in ONE entry of 300 x 32 do not."""
  import torch
  from test_linear_dispatch_gpu import assert_within_bound
  g = torch.Generator().manual_seed(3)
  x, W, b = torch.randn(300, 112, generator=g), torch.randn(32, 112, generator=g) / 112 ** 0.5, torch.randn(32, generator=g)
  good = torch.nn.functional.linear(x, W, b)
  assert_within_bound(good, x, W, b, 112, False, 'BLAS')
  chain = torch.zeros(300, 32)
  for k in range(112):
    chain += x[:, k:k + 1] * W[:, k]
  assert_within_bound(chain + b, x, W, b, 112, False, 'chain')
  assert_within_bound(torch.nn.functional.linear(torch.relu(x), W), x, W, None, 112, True, 'relu')
  k = int((x[17] * W[5]).abs().argmax())
  wrong = [good.clone() for _ in range(4)]
  wrong[0][17, 5] -= x[17, k] * W[5, k]
  wrong[1][3, 7] += b[8] - b[7]
  wrong[2][200] = good[199]
  wrong[3][299, 31] = float('nan')
  for bad in wrong:
    with pytest.raises(AssertionError, match='past the bound'):
      assert_within_bound(bad, x, W, b, 112, False, 'wrong')
