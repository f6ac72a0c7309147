"""csrc/embedded_pair.h is the one native statement of the embedded pairs, of the step-size controller and of the host's batch
rule.  Its plain-C++ part is compiled here with the host compiler into tests/embedded_pair_probe.cpp, which prints what it
states; every value is compared for EXACT equality with the Python statement of the same thing: the tableaux with
odeint._TABLEAUS, the decision with the controller lines of odeint._solve_dopri5 (restated below with math.pow, the libm
function the compiled program calls), the batch rule with dt (10^m - 1) / 9 < t1 - t in exact rationals."""
import importlib
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

O = importlib.import_module('gnpde_amd.odeint')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(O.__file__)), 'csrc')

RATIOS = [0.0, 1e-30, 0.5, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 7.0, 1e30]


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  """The probe's output lines, split into words, by their first word."""
  cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
  assert cxx is not None, 'no host C++ compiler'
  exe = tmp_path_factory.mktemp('embedded_pair') / 'probe'
  # (-fno-builtin: pow is libm's at run time, as math.pow's, not the compiler's constant folding)
  res = subprocess.run([cxx, '-std=c++17', '-O1', '-fno-builtin', '-Wall', '-Werror', '-I', CSRC,
                        os.path.join(ROOT, 'tests', 'embedded_pair_probe.cpp'), '-o', str(exe), '-lm'], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-3000:]
  out = subprocess.run([str(exe)], capture_output=True, text=True)
  assert out.returncode == 0, out.stderr[-3000:]
  lines = {}
  for line in out.stdout.splitlines():
    w = line.split()
    lines.setdefault(w[0], []).append(w[1:])
  return lines


def _padded(values, n):
  return list(values) + [0.0] * (n - len(values))


def test_tableaux_are_bit_equal_to_the_python_ones(probe):
  heads = {w[0]: [int(v) for v in w[1:]] for w in probe['tableau']}
  assert sorted(heads) == sorted(O._TABLEAUS)
  for name, tab in O._TABLEAUS.items():
    S = len(tab['beta'])
    assert heads[name] == [S, int(tab['fsal']), tab['order']]
    a = {(int(w[1]), int(w[2])): float.fromhex(w[3]) for w in probe['a'] if w[0] == name}
    assert len(a) == 36
    for r in range(6):
      row = _padded(tab['beta'][r], 6) if r < S else [0.0] * 6
      for j in range(6):
        assert a[(r, j)].hex() == float(row[j]).hex(), (name, r, j)
    c = {int(w[1]): [float.fromhex(v) for v in w[2:]] for w in probe['c'] if w[0] == name}
    assert len(c) == 7
    for j in range(7):
      want = [_padded(tab[k], 7)[j] for k in ('c_sol', 'c_err', 'c_mid')]
      assert [v.hex() for v in c[j]] == [float(v).hex() for v in want], (name, j)


def _decide(t, dt, t1, ratio32, order, safety=0.9, ifactor=10.0, dfactor=0.2):
  """odeint._solve_dopri5: accept, the end-point test of its loop, the interpolation fraction, the controller (lines
  `if ratio == 0: ...  factor = clamp(safety / r ** (1 / order), min=lo, max=ifactor)`), on Python floats (float64)."""
  ratio = float(ratio32)
  accept = ratio <= 1
  done, x, t_next = False, 0.0, t
  if accept:
    t_next = t + dt
    if not t1 > t_next:                       # `while tt[i] > t_cur` ends
      x = float(np.float32((t1 - t) / (t_next - t)))
      done = True
  if ratio == 0:
    dt_next = dt * ifactor
  else:
    lo = 1.0 if ratio < 1 else dfactor
    factor = min(max(safety / math.pow(ratio, 1.0 / order), lo), ifactor)
    dt_next = dt * factor
  return int(accept), int(done), x, t_next, dt_next


def test_step_decide_equals_the_python_controller(probe):
  rows = probe['decide']
  seen_ratios, seen_orders, seen_ends = set(), set(), set()
  for w in rows:
    order = int(w[0])
    ratio, t, dt, t1 = (float.fromhex(v) for v in w[1:5])
    assert float(np.float32(ratio)) == ratio
    got = (int(w[5]), int(w[6])) + tuple(float.fromhex(v) for v in w[7:10])
    want = _decide(t, dt, t1, np.float32(ratio), order)
    assert got[:2] == want[:2] and [v.hex() for v in got[2:]] == [v.hex() for v in want[2:]], (w, want)
    seen_ratios.add(ratio)
    seen_orders.add(order)
    seen_ends.add((t + dt > t1) - (t + dt < t1))
  assert seen_ratios == {float(np.float32(r)) for r in RATIOS} and seen_orders == {2, 5} and seen_ends == {-1, 0, 1}
  assert len(rows) == len(RATIOS) * 2 * 8
  # t + dt one ulp below / at / one ulp above t1, on an accepted step: not done, done, done
  for w in rows:
    ratio, t, dt, t1 = (float.fromhex(v) for v in w[1:5])
    if ratio <= 1 and (t, dt) == (0.25, 0.125) and t1 != 1.0:
      assert int(w[6]) == int(t1 <= 0.375)


def test_plan_batch_is_the_reach_rule(probe):
  rows = probe['plan']
  assert len(rows) == 3 * 2 * 2 * 9
  seen = set()
  for w in rows:
    tps, have = int(w[0]), int(w[1])
    t, dt, t1 = (Fraction(float.fromhex(v)) for v in w[2:5])
    # m trial steps, each accepted with the largest growth (x 10), cover dt (10^m - 1) / 9: another one is queued while that stays
    # short of t1; one trial step before the first read of the record
    m = 1
    while have and m < tps and dt * (10 ** m - 1) / 9 < t1 - t:
      m += 1
    assert int(w[5]) == m, w
    seen.add((tps, have, (t1 - t) / dt))
  assert {s[0] for s in seen} == {1, 3, 8} and {s[1] for s in seen} == {0, 1}
  assert min(s[2] for s in seen) == Fraction(1, 2) and max(s[2] for s in seen) == 2000
