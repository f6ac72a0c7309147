"""Record tests/golden/gatmix_constant_*.npz: whole no-grad solves of the reference's GAT function with mix_features
(src/function_GAT_attention.py:32-38, f = alpha (A(x) (x W) Wout - x) + beta x0) inside its own ConstantODEblock, on the CPU.

Needs the reference tree (oracle/ref_env.py); the tests that read the fixtures do not.  Same inputs as the block fixtures of
oracle/gen_golden.py: make_graph(150, 6, 21), x from seed 22 [150, 24], parameters randomise(block, 777).

  gatmix_constant_rk4        rk4, time 2.3, step 1.0 (short last step)
  gatmix_constant_euler_h05  euler, time 2.2, step 0.5
  gatmix_constant_dopri5     dopri5, time 2.0, tol_scale 100

The names do not start with `block_`: the CPU tests that walk every block_* fixture restate a GAT block WITHOUT Wout.
Every fixture also holds `ref_dev`: the deviation of the reference's float32 solve from its own float64 solve (same parameters,
same graph), relative to the largest entry -- the noise floor a float32 implementation is compared against -- and `nfe64`.

Usage:  python tools/record_gat_mix_fixtures.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import make_graph, randomise, data_of, save, BASE  # noqa: E402  (activates the reference environment)
from function_GAT_attention import ODEFuncAtt  # noqa: E402
from block_constant import ConstantODEblock  # noqa: E402

CASES = {
  'gatmix_constant_rk4': dict(method='rk4', time=2.3, step_size=1.0),
  'gatmix_constant_euler_h05': dict(method='euler', time=2.2, step_size=0.5),
  'gatmix_constant_dopri5': dict(method='dopri5', time=2.0, tol_scale=100.0),
}


def solve(opt, ei, x, dtype):
  t = torch.tensor([0, opt['time']])
  block = ConstantODEblock(ODEFuncAtt, [], opt, data_of(ei, x.float()), torch.device('cpu'), t=t)
  randomise(block, 777)
  block = block.to(dtype)
  for f in (block.odefunc, block.reg_odefunc.odefunc):        # the GAT layer's tensors follow the module
    f.edge_index = f.edge_index.long()
  block.eval()
  xs = x.to(dtype)
  block.set_x0(xs)
  with torch.no_grad():
    z = block(xs)
  return block, z


def main():
  n, d = 150, 24
  ei = make_graph(n, 6, 21)
  x = torch.randn(n, d, generator=torch.Generator().manual_seed(22))
  for name, over in CASES.items():
    opt = {**BASE, 'function': 'GAT', 'block': 'constant', 'mix_features': True, **over}
    block, z = solve(opt, ei, x, torch.float32)
    block64, z64 = solve(opt, ei, x, torch.float64)
    dev = float((z.double() - z64).abs().max() / z64.abs().max())
    lay = block.odefunc.multihead_att_layer
    norm = float(torch.linalg.matrix_norm(lay.W.detach() @ lay.Wout.detach(), 2))
    print('%-28s float32 vs float64 %.3e   nfe %d / %d   |W Wout|_2 %.2f   max|z| %.2f' %
          (name, dev, block.odefunc.nfe, block64.odefunc.nfe, norm, float(z.abs().max())))
    save(name, opt, {'edge_index': ei, 'x': x, 'z': z, 'nfe': np.int64(block.odefunc.nfe), 'ref_dev': np.float64(dev),
                     'nfe64': np.int64(block64.odefunc.nfe)}, block)


if __name__ == '__main__':
  main()
