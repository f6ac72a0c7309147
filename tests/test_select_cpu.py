"""csrc/select.h states once the selection primitives of the rewiring kernels.  Its plain-C++ part is compiled here with the host
compiler into tests/select_probe.cpp, which prints what it computes with its inputs; every value is compared for equality with a
Python statement of the same thing: the order-preserving float key and its inverse, the histogram bin that holds a rank (against a
cumulative sum) and the column-split rule (against the two rules it replaced, transcribed below as they stood in knn.hip and
posdist.hip)."""
import importlib
import os
import shutil
import struct
import subprocess

import pytest

O = importlib.import_module('gnpde_amd.ops')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(O.__file__)), 'csrc')


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  """The probe's output lines, split into words, by their first word."""
  cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
  assert cxx is not None, 'no host C++ compiler'
  exe = tmp_path_factory.mktemp('select') / 'probe'
  res = subprocess.run([cxx, '-std=c++17', '-O1', '-fno-builtin', '-Wall', '-Werror', '-I', CSRC,
                        os.path.join(ROOT, 'tests', 'select_probe.cpp'), '-o', str(exe), '-lm'], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-3000:]
  out = subprocess.run([str(exe)], capture_output=True, text=True)
  assert out.returncode == 0, out.stderr[-3000:]
  lines = {}
  for line in out.stdout.splitlines():
    w = line.split()
    lines.setdefault(w[0], []).append(w[1:])
  return lines


def _f(bits):
  return struct.unpack('<f', struct.pack('<I', bits))[0]


def _bits(x):
  return struct.unpack('<I', struct.pack('<f', x))[0]


def test_ordered_key_is_strictly_monotone_and_inverted(probe):
  rows = [[int(v, 16) for v in w] for w in probe['key']]
  values = [_f(r[0]) for r in rows]
  flt_max, tiny = _f(0x7f7fffff), _f(1)
  # the list holds what it must: both zeros, denormals of both signs, +-FLT_MAX, neighbouring floats
  have = {r[0] for r in rows}
  assert {_bits(0.0), _bits(-0.0), _bits(tiny), _bits(-tiny), _bits(flt_max), _bits(-flt_max)} <= have
  assert {0x3f7fffff, 0x3f800000, 0x3f800001, 0xbf7fffff, 0xbf800000, 0xbf800001} <= have
  # ascending as floats, -0 before +0
  for a, b in zip(values, values[1:]):
    assert a < b or (a == 0.0 and b == 0.0 and str(a) == '-0.0' and str(b) == '0.0'), (a, b)
  keys = [r[1] for r in rows]
  assert all(a < b for a, b in zip(keys, keys[1:])), keys
  for bits, key, back in rows:
    assert back == bits, (hex(bits), hex(key), hex(back))
    assert key == ((~bits & 0xffffffff) if bits & 0x80000000 else (bits | 0x80000000))


def test_rank_bin_equals_a_cumulative_sum(probe):
  hists = {int(w[0]): [int(v) for v in w[1:]] for w in probe['hist']}
  assert any(c > 2 ** 32 for h in hists.values() for c in h)
  seen = set()
  for w in probe['rank']:
    h, begin, end, rank, bin_, rest = (int(v) for v in w)
    counts = hists[h][begin:end]
    cum, want = 0, None
    for b, c in enumerate(counts):
      if rank < cum + c:
        want = (begin + b, rank - cum)
        break
      cum += c
    assert want is not None and (bin_, rest) == want, (w, want)
    total = sum(counts)
    seen.update((h, begin, end, name) for name, r in (('first', 0), ('last', total - 1)) if rank == r)
    # an empty bin is never the answer; empty bins lie before and after hits
    assert hists[h][bin_] > 0
  ranges = {(int(w[0]), int(w[1]), int(w[2])) for w in probe['rank']}
  assert all((r + ('first',)) in seen and (r + ('last',)) in seen for r in ranges)
  # both sides of every edge between two occupied stretches: each occupied bin of each range is hit at its first and last rank
  for h, begin, end in ranges:
    hit = {}
    for w in probe['rank']:
      if (int(w[0]), int(w[1]), int(w[2])) == (h, begin, end):
        hit.setdefault(int(w[4]), set()).add(int(w[5]))
    for b in range(begin, end):
      c = hists[h][b]
      assert (c == 0 and b not in hit) or {0, c - 1} <= hit[b], (h, begin, end, b)
  assert any(hists[h][begin] == 0 and hists[h][end - 1] == 0 for h, begin, end in ranges)
  assert len(ranges) >= 8


def _choose_splits(n, k, cus, forced):
  """knn.hip's choose_splits as it stood: kTM = 64, kMaxSplits = 32, kMaxMergeKeys = 4096 (integer arithmetic)."""
  tiles = (n + 63) // 64
  s = forced
  if s <= 0:
    s = 1 if tiles >= cus else (cus + tiles - 1) // tiles
  if s > 32:
    s = 32
  if s > 4096 // k:
    s = 4096 // k
  if s > tiles:
    s = tiles
  if s < 1:
    s = 1
  per = (tiles + s - 1) // s          # splits that would get no column tile are dropped
  return (tiles + per - 1) // per


def _radius_splits(n, cus, forced):
  """posdist.hip's radius_splits as it stood: two workgroups per CU, kMaxRadiusSplits = 32."""
  tiles = (n + 63) // 64
  s = forced
  if s <= 0:
    s = 1 if tiles >= 2 * cus else (2 * cus + tiles - 1) // tiles
  if s > 32:
    s = 32
  if s > tiles:
    s = tiles
  if s < 1:
    s = 1
  per = (tiles + s - 1) // s
  return (tiles + per - 1) // per


def test_column_splits_equals_the_two_rules_it_replaced(probe):
  seen = set()
  for w in probe['splits']:
    n, k, cus, forced, got = (int(v) for v in w[1:])
    want = _choose_splits(n, k, cus, forced) if w[0] == 'knn' else _radius_splits(n, cus, forced)
    assert got == want, (w, want)
    seen.add((w[0], n, k, cus, forced))
  grid = {(n, cus, forced) for n in (1, 64, 65, 2708, 169343) for cus in (1, 256) for forced in (0, 1, 3, 64)}
  assert seen == {('knn', n, k, c, f) for n, c, f in grid for k in (1, 32, 128)} | {('radius', n, 0, c, f) for n, c, f in grid}
