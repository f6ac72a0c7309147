"""The BLEND split kernel on the native VJP stage, everything that needs no device: the chain-rule entry gnpde_split_kernel_grads in
header / library / bindings / INTEGRATION.md, the ABI number, the argument checks of the C entry point (an error code before any
launch), and the shape rule that sends the split kernel -- and the plain exp kernel up to width 256 -- to the native stage."""
import importlib
import os
import re
import types

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('gnpde_split_kernel_grads', 'gnpde_split_kernel_grad_floats')
O = importlib.import_module('gnpde_amd.odeint')


def test_symbols_and_abi_number_agree():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  declared = set(re.findall(r'\b(gnpde_[a-z_0-9]+)\s*\(', header))
  L = G.lib()
  for name in SYMBOLS:
    assert name in declared, name + ' is not declared in gnpde.h'
    assert name in _lib.PROTOTYPES, name + ' has no ctypes prototype'
    assert hasattr(L, name), name + ' is not exported by the library'
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 10 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION      # (9 before this entry existed)
  assert 'function_transformer_attention.py:133-171' in header


def test_integration_doc_names_the_entry():
  doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
  for name in SYMBOLS:
    assert name in doc


def test_entry_point_rejects_bad_arguments_before_any_launch():
  """Null pointers, a width the stage does not take and feature + positional columns beyond the state width return GNPDE_EINVAL with a
  message; nothing touches a device (this test runs without one, on host tensors that a launch could not read)."""
  L = G.lib()
  h, dk, d, f0, p0 = 2, 4, 10, 5, 3
  A = h * dk
  g = torch.zeros(4 * A * d + 4 * A + 2)
  w = torch.zeros(4 * A, d)
  b = torch.zeros(4 * A)
  s = torch.ones(4)
  out = torch.zeros(2 * A * (d + 2) + 4)
  assert L.gnpde_split_kernel_grad_floats(h, dk, d) == out.numel()
  assert L.gnpde_split_kernel_grad_floats(0, dk, d) == 0
  P = _lib.ptr

  def call(g_=g, w_=w, b_=b, lx=s[0:1], lp=s[1:2], ox=s[2:3], op=s[3:4], h_=h, dk_=dk, d_=d, f0_=f0, p0_=p0, out_=out):
    return L.gnpde_split_kernel_grads(P(g_), P(w_), P(b_), P(lx), P(lp), P(ox), P(op), h_, dk_, d_, f0_, p0_, P(out_), None)
  assert call(f0_=8) == -1 and b'split_kernel_grads' in L.gnpde_last_error()      # 8 + 3 > 10
  assert call(p0_=11) == -1
  assert call(p0_=0) == -1
  assert call(f0_=-1) == -1
  assert call(h_=0) == -1 and call(dk_=0) == -1 and call(d_=0) == -1
  assert call(h_=8, dk_=64) == -1                                                  # attention_dim 512
  for name in ('g_', 'w_', 'b_', 'lx', 'lp', 'ox', 'op', 'out_'):
    assert call(**{name: None}) == -1, name
  assert float(out.abs().max()) == 0.0


def _func(attention_type, beltrami, A, h, mix=False):
  lay = types.SimpleNamespace(attention_dim=A, h=h, d_k=A // h, split_kernel=bool(beltrami and attention_type == 'exp_kernel'))
  lay.kernel_att_dim = 2 * A if lay.split_kernel else A
  return types.SimpleNamespace(multihead_att_layer=lay, opt=dict(mix_features=mix, attention_type=attention_type))


@pytest.mark.parametrize('beltrami,A,h,ok', [
  (True, 16, 2, True), (True, 32, 2, True), (True, 128, 8, True),      # kernel widths 32, 64, 256
  (True, 256, 8, False),                                               # kernel width 512
  (True, 24, 2, False),                                                # kernel width 48: 48 / 4 is no power of two
  (True, 8, 4, True),                                                  # d_k = 2: heads of width 4
  (True, 4, 4, False),                                                 # d_k = 1: heads of width 2
  (False, 16, 4, True), (False, 128, 8, True), (False, 256, 8, True),  # the plain exp kernel up to width 256
  (False, 256, 16, False), (False, 512, 8, False)])
def test_stage_shape_rule(beltrami, A, h, ok):
  assert O._transformer_stage_native(_func('exp_kernel', beltrami, A, h)) == ok
  assert not O._transformer_stage_native(_func('exp_kernel', beltrami, A, h, mix=True))


def test_other_scores_keep_their_rule():
  assert O._transformer_stage_native(_func('scaled_dot', False, 20, 5))
  assert O._transformer_stage_native(_func('scaled_dot', True, 256, 8))          # beltrami without the exp kernel is no split kernel
  assert not O._transformer_stage_native(_func('scaled_dot', False, 260, 4))
  assert O._transformer_stage_native(_func('pearson', False, 32, 4))
  assert not O._transformer_stage_native(_func('cosine_sim', False, 128, 4))     # d_k = 32
