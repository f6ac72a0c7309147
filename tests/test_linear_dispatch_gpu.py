"""Every line of the projection's dispatch table (csrc/linear.hip: 36 kernel instantiations and the two-table form of staged2) on the
device, over the case table of linear_cases.py, against float64 on the CPU.

Per case: the plan is what the table says (ops.linear_plan -- the decision the launcher itself switches on), then

  * entry by entry  |out - ref| <= gamma (|x| |W|^T + |b|) + d 2^-126,  gamma = k u / (1 - k u), k = d + 1, u = 2^-24: the standard bound
    of a length-d fp32 dot product in ANY summation order plus the bias add (Higham, Accuracy and Stability of Numerical Algorithms,
    section 3.1), with the smallest normal number per product for underflow.  Nothing in it is tuned; a dropped product, a wrong row,
    a neighbour's bias or a stale K block exceed it by orders of magnitude.  For relu cases x is relu(x) on both sides.
  * bit identity (d % 16 == 0): the first 16 floor(m / 16) columns equal, bit for bit, ops.linear of the same rows in chunks of
    <= 32 768 rows on contiguous operands, which take the small<.> line -- the "same MFMA sequence and k order" contract of the file.
  * nothing outside the [n, m] window of a NaN-filled out buffer (one spare row, spare columns on both sides) is written, and the
    padding columns of x hold NaN, so a read past a row's d floats poisons the result.
"""
import math

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
import linear_cases as LC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float('nan')


def host_operands(c, seed):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(c.n, c.d, generator=g)                       # mixed sign: relu has something to do
  W = torch.randn(c.m, c.d, generator=g) / math.sqrt(c.d)
  b = torch.randn(c.m, generator=g) if c.bias else None
  return x, W, b


def device_views(c, x, W, b, dev):
  """The case's operands on the device in the views the table names (geometry of linear_cases)."""
  ldx, xoff, ldw, woff, ldo, ooff = LC.geometry(c)
  xd = torch.full((c.n, ldx), NAN, device=dev)[:, xoff:xoff + c.d]         # whatever of a row is not x holds NaN
  xd.copy_(x)
  assert xd.stride(0) == ldx and xd.stride(1) == 1 and xd.data_ptr() % 16 == 4 * xoff
  wflat = torch.full((c.m * c.d + 4,), NAN, device=dev)
  Wd = wflat[woff:woff + c.m * c.d].view(c.m, c.d)
  Wd.copy_(W)
  assert Wd.is_contiguous() and Wd.data_ptr() % 16 == 4 * woff
  bd = None if b is None else b.to(dev)
  if c.ov is None:
    return xd, Wd, bd, None, None
  buf = torch.full((c.n + 1, ldo), NAN, device=dev)
  out = buf[:c.n, ooff:ooff + c.m]
  assert out.stride(0) == ldo and out.data_ptr() % 8 == (4 * ooff) % 8
  return xd, Wd, bd, out, buf


def assert_within_bound(res, x, W, b, d_true, relu, what):
  """Entry by entry against float64 (the bound of the module docstring, at the TRUE d for zero-padded operands)."""
  x64 = (torch.relu(x) if relu else x).double()
  W64 = W.double()
  ref = x64 @ W64.t()
  mag = x64.abs() @ W64.abs().t()
  if b is not None:
    ref += b.double()
    mag += b.double().abs()
  k = d_true + 1
  bound = (k * U / (1 - k * U)) * mag + d_true * 2.0 ** -126
  got = res.detach().cpu().double()
  assert got.shape == ref.shape
  err = (got - ref).abs()
  err[torch.isnan(err)] = float('inf')
  ratio = err / bound
  worst = int(ratio.argmax())
  print('%s: worst |err| / bound = %.3g at (%d, %d), max |err| = %.3g' % (what, float(ratio.flatten()[worst]), worst // ref.shape[1],
                                                                        worst % ref.shape[1], float(err.max())))
  bad = err > bound
  assert not bool(bad.any()), '%s: %d entries past the bound, first at %s, worst err / bound %.3g' % (
    what, int(bad.sum()), tuple(int(v) for v in bad.nonzero()[0]), float(ratio.max()))


def assert_bits_of_small(res, xd, Wd, bd, relu, what):
  """The complete column tiles equal the small<.> kernel's result on the same rows bit for bit."""
  n, d = xd.shape
  mc = Wd.shape[0] // 16 * 16
  if d % 16 != 0 or mc == 0:
    return
  fresh = lambda t: torch.empty(t.shape, dtype=t.dtype, device=t.device).copy_(t)     # a new, aligned, contiguous allocation
  Wc = fresh(Wd[:mc])
  bc = None if bd is None else fresh(bd[:mc])
  for r0 in range(0, n, 32768):
    xc = fresh(xd[r0:r0 + 32768])
    assert ops.linear_plan(xc, Wc) == ['small<%d>' % (2 if mc % 32 == 0 else 1)]
    ref = ops.linear(xc, Wc, bc, relu_input=relu)
    got = res[r0:r0 + 32768, :mc]
    if not torch.equal(got, ref):
      diff = got != ref
      raise AssertionError('%s: %d of %d entries of rows %d.. differ in bits from small<.>, first at %s, max |diff| %.3g' % (
        what, int(diff.sum()), diff.numel(), r0, tuple(int(v) for v in diff.nonzero()[0]), float((got - ref).abs().max())))


@pytest.mark.parametrize('idx', range(len(LC.CASES)), ids=[c.id for c in LC.CASES])
def test_dispatch_line(dev, idx):
  c = LC.CASES[idx]
  x, W, b = host_operands(c, 5000 + idx)
  if c.att_dim:
    return check_split(dev, c, x, W, b)
  xd, Wd, bd, out, buf = device_views(c, x, W, b, dev)
  assert ops.linear_plan(xd, Wd, out=out) == c.lines
  res = ops.linear(xd, Wd, bd, out=out, relu_input=c.relu)
  assert res.shape == (c.n, c.m) and (out is None or res.data_ptr() == out.data_ptr())
  assert_within_bound(res, x, W, b, c.d, c.relu, c.id)
  if buf is not None:
    assert int(torch.isnan(buf).sum()) == buf.numel() - c.n * c.m, '%s: a write outside the [n, m] window of out' % c.id
  assert_bits_of_small(res, xd, Wd, bd, c.relu, c.id)


def check_split(dev, c, x, W, b):
  """gnpde_linear_split through ops.qk_tables: two tables [n, A] that equal the interleaved columns bit for bit."""
  A = c.att_dim
  xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
  big = torch.full((c.n * c.m + 64,), NAN, device=dev)
  assert ops.qk_tables_plan(xd, Wd, A, out=big[32:32 + c.n * c.m]) == c.lines
  q, k, ld, _ = ops.qk_tables(xd, Wd, bd, A, out=big[32:32 + c.n * c.m])
  assert ld == A and q.shape == k.shape == (c.n, A) and q.is_contiguous() and k.is_contiguous()
  assert bool(torch.isnan(big[:32]).all()) and bool(torch.isnan(big[-32:]).all()) and not bool(torch.isnan(big[32:-32]).any())
  res = torch.cat([q, k], dim=1)
  assert_within_bound(res, x, W, b, c.d, False, c.id)
  assert ops.linear_plan(xd, Wd) == [c.lines[0].replace('+split', '')]
  assert torch.equal(res, ops.linear(xd, Wd, bd)), 'the two tables differ from the interleaved columns'
  assert_bits_of_small(res, xd, Wd, bd, False, c.id)


def test_padded_operand_cache(dev):
  """ops.linear's zero-padded operand copies (n >= 4096 with a K or a stride the 16-byte loads do not cover; _PAD_X, _PAD_W): a second
  x of the same shape, a weight changed in place, relu on a padded operand, and more shapes than the cache holds."""
  ops._PAD_X.clear()
  ops._PAD_W.clear()
  g = torch.Generator().manual_seed(77)

  def run(x, W, b, relu, lines, xd=None, Wd=None):
    xd = x.to(dev) if xd is None else xd
    Wd = W.to(dev) if Wd is None else Wd
    assert ops.linear_plan(xd, Wd) == lines
    out = ops.linear(xd, Wd, None if b is None else b.to(dev), relu_input=relu)
    assert_within_bound(out, x, W, b, x.shape[1], relu, 'padded n=%d d=%d' % tuple(x.shape))

  n, d, m = 4100, 30, 40
  lines = ['persistent<2,2>', 'tile<1,1,0>']          # K padded to 32, aligned copies
  x1, x2 = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
  W = torch.randn(m, d, generator=g) / math.sqrt(d)
  b = torch.randn(m, generator=g)
  run(x1, W, b, False, lines)
  assert len(ops._PAD_X) == 1 and len(ops._PAD_W) == 1
  run(x2, W, b, False, lines)                         # another x of the same shape: the kept buffer is refilled
  assert len(ops._PAD_X) == 1
  Wd = W.to(dev)
  run(x2, W, b, False, lines, Wd=Wd)
  Wd.mul_(-1.5)                                       # the weight changes in place between two calls
  run(x2, W * -1.5, b, False, lines, Wd=Wd)
  run(x1, W, None, True, lines)                       # relu on a padded operand, no bias
  # rows that lose 16-byte alignment (ldx = d + 1) with complete K blocks: a copy at the same K
  x3 = torch.randn(n, 64, generator=g)
  W3 = torch.randn(32, 64, generator=g) / 8

  x3d = torch.full((n, 65), NAN, device=dev)[:, :64]
  x3d.copy_(x3)
  run(x3, W3, b[:32], True, ['small<2>'], xd=x3d)
  # more shapes than the cache holds (4 of x): it is cleared and refilled, and the first shape still computes
  for i, (dn, dd) in enumerate(((1, 30), (2, 22), (3, 50), (4, 81), (5, 17))):
    xs = torch.randn(n + dn, dd, generator=g)
    Ws = torch.randn(m, dd, generator=g) / math.sqrt(dd)
    kb = (dd + 15) // 16
    run(xs, Ws, b, i % 2 == 1, ['persistent<2,%d>' % kb if kb != 4 else 'staged2<4>', 'tile<1,1,0>'])
    assert 1 <= len(ops._PAD_X) <= 4
  assert (n, d, 32, str(dev)) not in ops._PAD_X
  run(x1, W, b, False, lines)
  run(x2, W, b, True, lines)


def test_out_is_checked_before_any_launch(dev):
  x = torch.randn(40, 64, device=dev)
  W = torch.randn(32, 64, device=dev)
  for what, out in (('float32', torch.empty(40, 32, device=dev, dtype=torch.float64)),
                    ('is on', torch.empty(40, 32)),
                    ('the product is', torch.empty(40, 31, device=dev)),
                    ('the product is', torch.empty(41, 32, device=dev)),
                    ('the product is', torch.empty(40 * 32, device=dev)),
                    ('unit column stride', torch.empty(32, 40, device=dev).t()),
                    ('unit column stride', torch.empty(40, 64, device=dev)[:, ::2])):
    with pytest.raises(G.GnpdeError, match=what):
      ops.linear(x, W, out=out)
    with pytest.raises(G.GnpdeError, match=what):
      ops.linear_plan(x, W, out=out)
  out = torch.zeros(41, 40, device=dev)[:40, 3:35]          # a column window is fine
  assert ops.linear(x, W, out=out).data_ptr() == out.data_ptr() and bool((out != 0).any())
