"""csrc/tape_reverse.h is the one native statement of the reverse walk through a recorded Dormand-Prince solve for a general
right-hand side (the sweep of csrc/adjoint.hip behind GRAND-nl / GAT dopri5 training).  Its plain C++ is compiled here with the host
compiler into tests/tape_reverse_probe.cpp, which drives the walk in double on the scalar ODE y' = theta sin(y) + phi; the gradients
it prints are held against float64 torch autograd through a differentiable replay of the same steps written here (1e-12: both sides
compute in double), and its coefficient tables against oracle/tape_reverse.py."""
import os
import shutil
import subprocess

import pytest
import torch

from oracle import tape_reverse as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'graph-neural-pde_amd', 'csrc')

THETA, PHI, Y0 = 0.83, -0.31, 0.47
STEPS = [0.21, 0.34, 0.18]


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
  cxx = next((c for c in ('g++', 'c++', 'clang++') if shutil.which(c)), None)
  assert cxx is not None, 'no host C++ compiler'
  exe = tmp_path_factory.mktemp('tape_reverse') / 'probe'
  res = subprocess.run([cxx, '-std=c++17', '-O1', '-ffp-contract=off', '-Wall', '-Werror', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                        os.path.join(ROOT, 'tests', 'tape_reverse_probe.cpp'), '-o', str(exe), '-lm'], capture_output=True, text=True)
  assert res.returncode == 0, res.stderr[-3000:]

  def run(*args):
    out = subprocess.run([str(exe)] + [float(a).hex() for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = {}
    for line in out.stdout.splitlines():
      w = line.split()
      lines.setdefault(w[0], []).append(w[1:])
    return lines
  return run


def test_the_tables_are_those_of_the_oracle(probe):
  lines = probe()
  a = {(int(w[0]), int(w[1])): float.fromhex(w[2]) for w in lines['a']}
  assert len(a) == 21
  for r, row in enumerate(TR.A):
    for j, v in enumerate(row):
      assert a[(r, j)].hex() == float(v).hex(), (r, j)
  mid = {int(w[0]): float.fromhex(w[1]) for w in lines['mid']}
  assert [mid[j].hex() for j in range(7)] == [float(v).hex() for v in TR.MID]


def _replay(theta, phi, y0, hs, x):
  """torchdiffeq's accepted steps with GIVEN sizes and its quartic end point, differentiable, float64."""
  f = lambda u: theta * torch.sin(u) + phi      # noqa: E731
  y, k0 = y0, f(y0)
  for h in hs:
    ks = [k0]
    u = y
    for row in TR.A:
      u = y + sum(c * h * kj for c, kj in zip(row, ks))
      ks.append(f(u))
    ya, y, k0 = y, u, ks[6]
  ym = ya + sum(c * h * kj for c, kj in zip(TR.MID, ks))
  fa, fb = ks[0], ks[6]
  ca = 2 * h * (fb - fa) - 8 * (y + ya) + 16 * ym
  cb = h * (5 * fa - 3 * fb) + 18 * ya + 14 * y - 32 * ym
  cc = h * (fb - 4 * fa) - 11 * ya - 5 * y + 16 * ym
  cd = h * fa
  return ya + x * cd + x ** 2 * cc + x ** 3 * cb + x ** 4 * ca


@pytest.mark.parametrize('x', [0.37, 1.0])
@pytest.mark.parametrize('n_steps', [1, 3])
def test_the_walk_gives_autograd_s_gradients(probe, x, n_steps):
  hs = STEPS[:n_steps]
  lines = probe(THETA, PHI, Y0, x, *hs)
  assert int(lines['evals'][0][0]) == 6 * n_steps + 1
  got = [float.fromhex(v) for v in lines['grad'][0]]
  theta, phi, y0 = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (THETA, PHI, Y0))
  out = _replay(theta, phi, y0, [torch.tensor(h, dtype=torch.float64) for h in hs], torch.tensor(x, dtype=torch.float64))
  assert abs(float.fromhex(lines['out'][0][0]) - float(out.detach())) <= 1e-12
  want = [float(g) for g in torch.autograd.grad(out, (y0, theta, phi))]
  for name, g, w in zip(('y0', 'theta', 'phi'), got, want):
    assert abs(g - w) <= 1e-12, (name, g, w)
  assert all(abs(w) > 1e-3 for w in want)       # (none of the three is trivially zero)
