"""tests/golden/nltrain_*.npz (tools/record_nl_dopri5_fixtures.py): the reference's GRAND-nl / GAT block in training mode with
opt['adjoint'] = False and method dopri5, loss.backward() through torchdiffeq's loop.  The oracle's right-hand side under this
package's differentiable host loop `_solve_dopri5` with torch CPU autograd reproduces output, evaluation count and every gradient
(the asserts and tolerances of test_oracle_golden.py::test_training_without_the_adjoint_method), and the recorded error ratios keep
clear of 1, so a float32 solve on other hardware takes the same accept / reject sequence."""
import importlib

import numpy as np
import pytest
import torch

from helpers import Fixture, fixtures, assert_parity
from nl_dopri5_oracle import oracle_rhs

O = importlib.import_module('gnpde_amd.odeint')
NAMES = fixtures('nltrain_')
BAND = (0.85, 1.2)


def test_the_fixtures_are_there():
  assert len(NAMES) == 7 and sum('rejects' in n for n in NAMES) == 2 and any('gat' in n for n in NAMES)


@pytest.mark.parametrize('name', NAMES)
def test_error_ratios_keep_clear_of_one(name):
  fx = Fixture(name)
  ratios = np.asarray(fx.arr['ratios'], dtype=np.float64)
  assert ratios.size >= 2 and int(fx.arr['nfe']) == 2 + 6 * ratios.size
  assert not np.any((ratios > BAND[0]) & (ratios < BAND[1])), ratios
  assert bool(np.any(ratios > 1.0)) == ('rejects' in name)
  assert fx.opt['method'] == 'dopri5' and not fx.opt['adjoint'] and fx.opt['function'] in ('transformer', 'GAT')


@pytest.mark.parametrize('name', NAMES)
def test_training_without_the_adjoint_method(name):
  fx = Fixture(name)
  opt = fx.opt
  p = {k: v.clone().requires_grad_(True) for k, v in fx.params.items()}
  x = fx.t('x').clone().requires_grad_(True)
  calls = [0]
  rhs = oracle_rhs(opt, p, fx.t('edge_index'), fx.t('x'), calls)
  z = O._solve_dopri5(rhs, x, torch.tensor([0, opt['time']]), opt['tol_scale'] * 1e-9, opt['tol_scale'] * 1e-7)[1]
  assert calls[0] == int(fx.arr['nfe']) == int(fx.arr['nfe_after_backward'])       # the backward evaluates nothing
  assert_parity(z, fx.t('z'), 1e-5, name + ' z')
  (z * fx.t('c')).sum().backward()
  assert_parity(x.grad, fx.t('grad_x'), 1e-4, name + ' grad_x')
  # (errors are measured against the largest gradient of the same module: a gradient that is zero in exact arithmetic -- K.bias under
  #  a softmax over rows -- is rounding noise on both sides)
  keys = [k for k in fx.arr if k.startswith('grad/')]
  scale = {}
  for k in keys:
    mod = k[5:].rsplit('.', 2)[0] if 'multihead' in k else k
    scale[mod] = max(scale.get(mod, 0.0), float(fx.t(k).abs().max()))
  for k in keys:
    got = p[k[5:]].grad
    assert got is not None, k
    mod = k[5:].rsplit('.', 2)[0] if 'multihead' in k else k
    err = float((got.reshape(fx.arr[k].shape) - fx.t(k)).abs().max())
    assert err <= 1e-4 * scale[mod], '%s %s: abs err %.3e against module scale %.3e' % (name, k, err, scale[mod])
