"""The C ABI of the optional bf16 gather operand, as far as it can be checked without a GPU: the five exports with the header's
prototypes, and the host-side size query."""
import ctypes
import os
import re

import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C parameter type -> ctypes type of gnpde_amd._lib.PROTOTYPES
C_TYPES = {'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t, 'int': ctypes.c_int}
EXPORTS = ['gnpde_to_bf16', 'gnpde_spmm_lo', 'gnpde_spmm_rhs_lo', 'gnpde_solver_gather_bytes', 'gnpde_solver_set_gather']


def _ctype_of(param):
  param = param.strip()
  if '*' in param:
    base = param.replace('const', '').split('*')[0].strip()
    return {'gnpde_graph_t': ctypes.POINTER(_lib.GraphStruct), 'gnpde_epilogue_t': ctypes.POINTER(_lib.EpilogueStruct),
            'gnpde_rhs_t': ctypes.POINTER(_lib.RhsStruct)}.get(base, ctypes.c_void_p)
  return C_TYPES[param.rsplit(' ', 1)[0].strip()]


def test_the_five_exports_exist_with_the_headers_prototypes():
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  lib = ctypes.CDLL(_lib.LIB_PATH)
  for name in EXPORTS:
    m = re.search(r'^(int|size_t)\s+' + name + r'\(([^;]*?)\);', header, flags=re.M | re.S)
    assert m, '%s is not declared in gnpde.h' % name
    assert hasattr(lib, name), 'libgnpde_hip.so does not export %s' % name
    restype, argtypes = _lib.PROTOTYPES[name]
    assert restype is C_TYPES[m.group(1)], name
    want = [_ctype_of(p) for p in m.group(2).replace('\n', ' ').split(',')]
    assert list(argtypes) == want, '%s: ctypes prototype %s, header %s' % (name, argtypes, want)
  assert int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1)) >= 8


def _laplacian_descriptor(d, ld, padded=False):
  """A host-only descriptor: gnpde_solver_gather_bytes reads shapes and flags, never the device arrays."""
  n = 40
  ei = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
  graph = G.CSRGraph(ei, n)
  alpha = torch.tensor(0.1)
  w = torch.ones(n)
  return ops.RhsDescriptor(_lib.RHS_LAPLACIAN, graph, d, ld, alpha, None, None, True, w_csr=w, padded_rows=padded), n


def test_gather_bytes_by_shape():
  L = _lib.lib()
  desc, n = _laplacian_descriptor(128, 128)
  state = (n * 128 * 2 + 255) // 256 * 256
  assert L.gnpde_solver_gather_bytes(desc.ref(), _lib.METHOD_EULER) == 2 * state
  assert L.gnpde_solver_gather_bytes(desc.ref(), _lib.METHOD_MIDPOINT) == 2 * state
  assert L.gnpde_solver_gather_bytes(desc.ref(), _lib.METHOD_RK4) == 4 * state
  # d = 22 unpadded: out of scope, 0 with a message
  desc22, _ = _laplacian_descriptor(22, 22)
  assert L.gnpde_solver_gather_bytes(desc22.ref(), _lib.METHOD_RK4) == 0
  msg = L.gnpde_last_error().decode()
  assert 'solver_gather_bytes' in msg and '16-byte lanes' in msg and 'd=22' in msg
  # the same width with padded rows is covered by the kernels
  desc24, _ = _laplacian_descriptor(22, 24, padded=True)
  assert L.gnpde_solver_gather_bytes(desc24.ref(), _lib.METHOD_RK4) > 0
  assert L.gnpde_solver_gather_bytes(desc.ref(), 7) == 0 and 'bad method' in L.gnpde_last_error().decode()


def test_option_value_is_validated_without_a_device():
  import importlib
  O = importlib.import_module('gnpde_amd.odeint')      # (the package attribute of that name is the function)

  class F(object):
    opt = {}
  f = F()
  assert O.gather_dtype_requested(f) in ('fp32', 'bf16')
  f.opt = {'gnpde_gather_dtype': 'bf16'}
  assert O.gather_dtype_requested(f) == 'bf16'
  f.opt = {'gnpde_gather_dtype': 'half'}
  try:
    O.gather_dtype_requested(f)
  except ValueError as e:
    assert 'gnpde_gather_dtype' in str(e)
  else:
    raise AssertionError('a bad value was accepted')
