"""csrc/fixed_grid.h states once the stage schedule of the fixed-grid methods (euler, midpoint, compact 3/8-rule rk4): which
GNPDE_STAGE_* evaluation j of a step is and which buffers are its y, k1 and out_y.  The header is plain C++; it is compiled here
with the host compiler into tests/fixed_grid_probe.cpp, which runs the table over five dummy buffers and prints every evaluation.
Every printed line is compared for equality with the tables as they stood, written out by hand, in solver.hip, sharded.hip and
adjoint.hip (transcribed below), the weights with numpy.float32 in the operation order the adjoint sweeps used; and the stage
formulas of include/gnpde.h, applied in float64 to the operands the table names, must give each method's growth factor on
u' = lambda u -- a swapped operand gives a consistent solver of lower order, which a short-horizon parity test can miss."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

O = importlib.import_module('gnpde_amd.ops')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(os.path.dirname(os.path.abspath(O.__file__)), 'csrc')

EULER, RK4, MIDPOINT = 0, 1, 2                   # GNPDE_METHOD_*
ST_EULER, ST_RK1C, ST_RK2C, ST_RK3C, ST_RK4C, ST_LINCOMB = 1, 6, 7, 8, 9, 10     # GNPDE_STAGE_*
# evaluation j -> (stage, input, y, k1, out_y) as positions in u[]; -1: the stage does not read it
TABLE = {
  EULER: [(ST_EULER, 0, 0, -1, 1)],
  MIDPOINT: [(ST_LINCOMB, 0, 0, -1, 1), (ST_LINCOMB, 1, 0, -1, 2)],
  RK4: [(ST_RK1C, 0, -1, -1, 1), (ST_RK2C, 1, 0, -1, 2), (ST_RK3C, 2, -1, 1, 3), (ST_RK4C, 3, 0, 2, 4)],
}
DTS = [np.float32(0.5), np.float32(0.2), np.float32(1.0), np.float32(0.1), np.float32(0.3), np.float32(2.2) / np.float32(7.0)]


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  """The probe's output lines, split into words, by their first word."""
  cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
  assert cxx is not None, 'no host C++ compiler'
  exe = tmp_path_factory.mktemp('fixed_grid') / 'probe'
  res = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', 'fixed_grid_probe.cpp'), '-o', str(exe)], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-3000:]
  out = subprocess.run([str(exe)], capture_output=True, text=True)
  assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-3000:])
  lines = {}
  for line in out.stdout.splitlines():
    w = line.split()
    lines.setdefault(w[0], []).append(w[1:])
  return lines


def _evals(probe):
  """(method, dt) -> the step's evaluations in order: (j, stage, input, y, k1, out_y, e.dt, coef[0], weight)."""
  steps = {}
  for w in probe['eval']:
    key = (int(w[0]), np.float32(float.fromhex(w[1])))
    steps.setdefault(key, []).append(tuple(int(v) for v in w[2:8]) + tuple(float.fromhex(v) for v in w[8:11]))
  return steps


def test_schedule_equals_the_hand_written_tables(probe):
  assert sorted(probe['method']) == sorted([[str(EULER), '1', '2'], [str(MIDPOINT), '2', '2'], [str(RK4), '4', '4']])
  steps = _evals(probe)
  assert set(steps) == {(m, dt) for m in TABLE for dt in DTS}
  for (m, dt), evals in steps.items():
    assert len(evals) == len(TABLE[m])
    for j, (got, want) in enumerate(zip(evals, TABLE[m])):
      assert got[0] == j and got[1:6] == want, (m, dt, got, want)
      assert np.float32(got[6]) == dt and got[6] == float(dt)
      # midpoint: y_mid = y + f(y) * (dt / 2), then y + dt * f(y_mid); nobody else sets a coefficient
      coef = (np.float32(0.5) * dt if j == 0 else dt) if m == MIDPOINT else np.float32(0.0)
      assert got[7] == float(coef), (m, dt, j, got[7], coef)
      if m == EULER:
        assert got[8] == float(dt)
      if m == RK4:
        c8 = np.float64(dt) * 0.125
        weight = np.float32(c8) if j in (0, 3) else np.float32(3.0 * c8)
        assert got[8] == float(weight), (dt, j, got[8], weight)
  # everything else is the caller's: alpha, beta, x0, alpha_sigmoid pass through, and the first non-zero status ends the step
  assert sorted(probe['base']) == sorted([[str(m), str(j), '1'] for m in TABLE for j in range(len(TABLE[m]))])
  assert probe['status'] == [['7', '2']]


def _apply(stage, dt, coef, u, k, y, a):
  """out_y of include/gnpde.h's stage formulas for the stage input u and k = f(u).  Operands the table does not name are None."""
  if stage == ST_EULER:
    return y + dt * k
  if stage == ST_LINCOMB:
    return y + coef * k
  if stage == ST_RK1C:
    return u + dt * k * (1.0 / 3.0)
  if stage == ST_RK2C:
    return (2.0 * y - u) + dt * k
  if stage == ST_RK3C:
    return (2.0 * a - u) + dt * k
  assert stage == ST_RK4C
  return ((6.0 * a + 3.0 * u - y) + dt * k) * 0.125


def test_one_step_has_the_growth_factor_of_its_method(probe):
  steps = _evals(probe)
  growth = {EULER: lambda z: 1 + z, MIDPOINT: lambda z: 1 + z + z ** 2 / 2,
            RK4: lambda z: 1 + z + z ** 2 / 2 + z ** 3 / 6 + z ** 4 / 24}
  checked = 0
  for (m, dt), evals in steps.items():
    for lam in (-1.3, 0.7, 2.0, -0.05):
      vals = [1.0, None, None, None, None]
      for j, stage, i_in, i_y, i_k1, i_out, e_dt, coef, _ in evals:
        u = vals[i_in]
        y = vals[i_y] if i_y >= 0 else None
        a = vals[i_k1] if i_k1 >= 0 else None
        vals[i_out] = _apply(stage, e_dt, coef, u, lam * u, y, a)
      z = lam * float(dt)
      got, want = vals[len(evals)], growth[m](z)
      assert abs(got - want) <= 1e-14, (m, dt, lam, got, want)
      checked += 1
  assert checked == 3 * len(DTS) * 4
