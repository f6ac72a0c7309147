"""A/B of the fixed-grid host code (csrc/fixed_grid.h and its callers) between two builds of the library: the same Python layer over
--lib PATH (default: the library of this tree).

  python tools/fixed_grid_ab.py [--lib PATH] hashes
      one line `name sha256` per output tensor of a seeded list: FixedStepSolver for euler / midpoint / compact rk4 / classic rk4, replayed and
      eager, fp32 and bf16 gather operand, on a laplacian and a scaled-dot transformer problem; the recorded forward + reverse sweep (training
      without the adjoint method) for euler / midpoint / rk4 on two cases of tests/test_tape_gpu.py's FIXED_CASES (state, grad_x, every
      parameter gradient); the continuous adjoint for euler / rk4; a world-1 native sharded solve for euler / rk4.  Two builds that enqueue
      the same launches print the same lines.
  python tools/fixed_grid_ab.py [--lib PATH] time
      one JSON line of host-side costs at the ogbn-arxiv shape: an eager rk4 solve of 20 steps (enqueue_ms: until the last launch is
      enqueued, eager_ms: until the device is done), the first run of a fresh solver with a captured graph (capture_ms) and one recorded
      training step of 8 rk4 steps, forward + reverse sweep (train_ms); medians of --repeats."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gnpde_amd as G  # noqa: E402
from gnpde_amd import _lib, ops  # noqa: E402


def sha(t):
  return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()


def descriptor(block, x):
  """(descriptor over a fresh state buffer, that buffer) as odeint._solve_native builds them"""
  n, d = x.shape
  y, x0 = _lib.alloc_state(n, d, x.device), _lib.alloc_state(n, d, x.device)
  x0.copy_(x)
  return block.odefunc._descriptor(y, x0_override=x0), y


def hashes_solver(dev, out):
  import test_tape_gpu as T
  for kind, d in (('laplacian', 32), ('transformer', 32)):
    block, x = T._fixed_block(dev, kind, 'constant', 1500, d, 4, 16, 61, 'rk4', 2.2, step_size=0.5, hubs=2, hub_deg=700)
    block.eval()
    x = x.to(dev)
    desc, y = descriptor(block, x)
    for method, classic, dts in (('euler', 0, [0.5, 0.5, 0.2]), ('midpoint', 0, [0.5] * 4 + [0.2]), ('rk4', 0, [0.5] * 4 + [0.2]),
                                 ('rk4', 1, [0.5] * 4 + [0.2])):
      ops.tune(_lib.TUNE_RK4_CLASSIC, classic)
      try:
        sol = ops.FixedStepSolver(desc, method, dts, dev)
        for gather in ('fp32', 'bf16'):
          sol.set_gather(gather)
          for use_graph in (True, False):
            y.copy_(x)
            sol.run(y, use_graph=use_graph)
            out('solver %s %s%s %s %s' % (kind, method, '_classic' if classic else '', gather, 'replay' if use_graph else 'eager'), y)
        sol.close()
      finally:
        ops.tune(_lib.TUNE_RK4_CLASSIC, 0)


def hashes_recorded(dev, out):
  import test_tape_gpu as T
  for case in ('l_attention_rk4_hubs', 'nl_hubs_rk4'):
    for method, step in (('euler', 0.5), ('midpoint', 0.5), ('rk4', 1.0)):
      kw = dict(T.FIXED_CASES[case], method=method, step_size=step, time=2.2)
      block, x = T._fixed_block(dev, seed=61, **kw)
      c = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
      z, gx, grads, _ = T._train_once(block, x, dev, c)
      assert str(block.odefunc._last_train_solve).startswith('native recorded fixed-grid'), block.odefunc._last_train_solve
      out('recorded %s %s z' % (case, method), z)
      out('recorded %s %s grad_x' % (case, method), gx)
      for k in sorted(grads):
        if grads[k] is not None:
          out('recorded %s %s grad %s' % (case, method, k), grads[k])


def hashes_adjoint(dev, out):
  import test_adjoint_native_gpu as A
  from helpers import random_graph
  n = 1500
  ei = random_graph(n, 5, seed=31, hubs=2, hub_deg=700).to(dev)
  x = torch.randn(n, 32, generator=torch.Generator().manual_seed(32)).to(dev)
  for function in ('transformer', 'laplacian'):
    for method, step in (('euler', 0.5), ('rk4', 1.0)):
      opt = A._opt(function=function, method=method, step_size=step, adjoint_method=method, adjoint_step_size=step, time=2.2)
      z, gx, grads, native, _ = A._run(dev, opt, ei, x, 33, host=False)
      assert native, 'the adjoint solve did not run natively'
      out('adjoint %s %s z' % (function, method), z)
      out('adjoint %s %s grad_x' % (function, method), gx)
      for k in sorted(grads):
        out('adjoint %s %s grad %s' % (function, method, k), grads[k])


def hashes_sharded(dev, out):
  import test_sharded_gpu as S
  D = S.D
  for kind in ('transformer', 'laplacian'):
    n, d, ei, x, p, alpha, beta, _ = S._problem(kind, seed=5)
    sh = D.PartitionPlan(ei, n, 1).shard(0)
    be = D.NativeBackend(sh, d, dev, kind, p, alpha, beta, True)
    x_own = D.scatter_rows(x, sh).to(dev)
    for method, T in (('euler', 3.0), ('rk4', 2.0)):
      solver = D.NativeShardedSolver(sh, be, T, 1.0, method)
      with torch.no_grad():
        z = solver.integrate(x_own, x_own)
      out('sharded world-1 %s %s' % (kind, method), z)


def run_hashes(dev):
  def out(name, t):
    assert torch.isfinite(t).all(), name
    print('%-90s %s' % (name.replace(' ', '_'), sha(t)), flush=True)
  hashes_solver(dev, out)
  hashes_recorded(dev, out)
  hashes_adjoint(dev, out)
  hashes_sharded(dev, out)


def run_time(dev, repeats):
  from gather_dtype_ab import make_block
  block, x, n, e, d = make_block('arxiv', 'transformer', 20, dev)
  desc, y = descriptor(block, x)
  dts = [1.0] * 20
  sol = ops.FixedStepSolver(desc, 'rk4', dts, dev)
  enq, eager = [], []
  for i in range(repeats + 1):
    y.copy_(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol.run(y, use_graph=False)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if i > 0:
      enq.append((t1 - t0) * 1e3)
      eager.append((t2 - t0) * 1e3)
  sol.close()
  cap = []
  for i in range(repeats + 1):
    sol = ops.FixedStepSolver(desc, 'rk4', dts, dev)
    y.copy_(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sol.run(y, use_graph=True)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    sol.close()
    if i > 0:
      cap.append((t1 - t0) * 1e3)
  del sol, desc, block
  block, x, n, e, d = make_block('arxiv', 'transformer', 8, dev)
  c = torch.randn(x.shape, generator=torch.Generator().manual_seed(7)).to(dev)
  train = []
  for i in range(repeats + 2):
    for p in block.parameters():
      p.grad = None
    block.train()
    xin = x.clone().requires_grad_(True)
    block.set_x0(xin)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z = block(xin)
    (z * c).sum().backward()
    torch.cuda.synchronize()
    if i > 1:
      train.append((time.perf_counter() - t0) * 1e3)
  assert str(block.odefunc._last_train_solve).startswith('native recorded fixed-grid'), block.odefunc._last_train_solve
  med = statistics.median
  print(json.dumps(dict(lib=_lib.LIB_PATH, enqueue_ms=round(med(enq), 4), eager_ms=round(med(eager), 4), capture_ms=round(med(cap), 4),
                        train_ms=round(med(train), 4), repeats=repeats)), flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('what', choices=['hashes', 'time'])
  ap.add_argument('--lib', default=None, help='libgnpde_hip.so to load instead of this tree\'s')
  ap.add_argument('--repeats', type=int, default=5)
  args = ap.parse_args()
  if args.lib is not None:
    _lib.LIB_PATH = os.path.abspath(args.lib)     # before the first call into the library
  assert torch.cuda.is_available(), 'needs a HIP device'
  dev = torch.device('cuda:0')
  assert G.lib().gnpde_abi_version() == _lib.ABI_VERSION
  mapped = {line.split()[-1] for line in open('/proc/self/maps') if 'libgnpde_hip.so' in line}
  assert mapped == {os.path.realpath(_lib.LIB_PATH)}, mapped     # the one library asked for, and no other build beside it
  if args.what == 'hashes':
    run_hashes(dev)
  else:
    run_time(dev, args.repeats)


if __name__ == '__main__':
  main()
