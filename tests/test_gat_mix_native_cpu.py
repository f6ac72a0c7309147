"""GNPDE_RHS_MIX_FEATURES without a device: ABI version and struct mirror, the workspace layout of flagged and unflagged GAT
descriptors (totals computed from the layout rule of csrc/solver.hip rhs_layout, written out here), and what check_rhs refuses."""
import ctypes
import os
import re

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESHAPE, EINVAL = -2, -1


def last_error():
  return _lib.lib().gnpde_last_error().decode(errors='replace')


def align_up(v, a=256):
  return (v + a - 1) // a * a


def host_graph(n, m, hubs=()):
  src, dst = [], []
  for i in range(n):
    k = hubs[i] if i < len(hubs) else m
    src.append(torch.full((k,), i))
    dst.append((torch.arange(k) + i) % n)
  return G.CSRGraph(torch.stack([torch.cat(src), torch.cat(dst)]).long(), n)


def descriptor(graph, d, A, heads, mix, ld=None):
  """A GAT descriptor over host tensors (nothing is dereferenced by the size and check entry points)."""
  ld = d if ld is None else ld
  alpha, beta = torch.zeros(1), torch.zeros(1)
  x0 = torch.zeros(graph.n, ld)
  gat_a = torch.zeros(2 * (A // heads))
  att = ops.attention_struct(_lib.ATT_GAT, heads, A, 0, False, leaky_slope=0.2, gat_a=gat_a)
  desc = ops.RhsDescriptor(_lib.RHS_GAT, graph, d, ld, alpha, beta, x0, True, proj_w=torch.zeros(A, d), att=att,
                           out_w=torch.zeros(d, A) if mix else None)
  desc.keep += [gat_a]
  return desc


def test_abi_version_and_struct_mirror():
  text = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  header = int(re.search(r'#define GNPDE_ABI_VERSION (\d+)', text).group(1))
  assert header == _lib.ABI_VERSION == _lib.lib().gnpde_abi_version() and header >= 25
  assert int(re.search(r'#define GNPDE_RHS_MIX_FEATURES (\d+)', text).group(1)) == _lib.RHS_MIX_FEATURES == 2
  names = [f[0] for f in _lib.RhsStruct._fields_]
  assert names[-2:] == ['out_w', 'out_ld'] and names[-3] == 'att'
  # appended: every earlier field keeps its offset, the struct grows by one pointer and one padded int
  assert _lib.RhsStruct.out_w.offset == _lib.RhsStruct.att.offset + ctypes.sizeof(_lib.AttentionStruct)
  assert _lib.RhsStruct.out_ld.offset == _lib.RhsStruct.out_w.offset + 8
  assert ctypes.sizeof(_lib.RhsStruct) == _lib.RhsStruct.out_w.offset + 16
  assert hasattr(_lib.lib(), 'gnpde_linear_epilogue')


@pytest.mark.parametrize('n,d,A,heads,hubs', [(150, 24, 16, 4, ()), (150, 24, 32, 4, ()), (600, 24, 64, 4, (513, 600, 0)),
                                             (600, 80, 16, 2, (513, 600, 0))])
def test_workspace_layout(n, d, A, heads, hubs):
  """rhs_layout: projection [n, A], aggregation scratch, head-mean weights [e], attention scratch, (flagged: z [n, A]), tickets; every
  region rounded up to 256 bytes.  Without the flag the total is today's sum; with it the total grows by the z region and by whatever
  the aggregation scratch grows when A > d (it is sized for the wider of the two gathers)."""
  L = _lib.lib()
  g = host_graph(n, 5, hubs)
  plain, mix = descriptor(g, d, A, heads, False), descriptor(g, d, A, heads, True)
  att_bytes = L.gnpde_attention_workspace_bytes(g.ref(), ctypes.byref(plain.struct.att))
  spmm = lambda w: align_up(L.gnpde_spmm_workspace_bytes(g.ref(), w))       # noqa: E731
  tickets = align_up(L.gnpde_spmm_ticket_bytes(g.ref()))
  unflagged = align_up(n * A * 4) + spmm(d) + align_up(g.e * 4) + align_up(att_bytes) + tickets
  assert L.gnpde_rhs_workspace_bytes(plain.ref()) == unflagged
  flagged = unflagged + align_up(n * A * 4) + (spmm(max(d, A)) - spmm(d))
  assert L.gnpde_rhs_workspace_bytes(mix.ref()) == flagged
  if hubs and A > d:
    assert spmm(A) > spmm(d)
  if not hubs:
    assert spmm(d) == 0 and tickets == 0 and flagged - unflagged == align_up(n * A * 4)
  # the solvers' workspaces carry the same growth
  for method in (_lib.METHOD_EULER, _lib.METHOD_RK4, _lib.METHOD_MIDPOINT):
    assert (L.gnpde_solver_workspace_bytes(mix.ref(), method) - L.gnpde_solver_workspace_bytes(plain.ref(), method)) == flagged - unflagged


def test_check_rhs_refusals():
  L = _lib.lib()
  g = host_graph(150, 5)
  size = lambda desc: L.gnpde_rhs_workspace_bytes(desc.ref())        # noqa: E731  (0 with gnpde_last_error set when check_rhs refuses)
  ok = descriptor(g, 24, 16, 4, True)
  assert size(ok) > 0
  # another kind
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.kind, bad.struct.proj_m = _lib.RHS_TRANSFORMER, 32
  assert size(bad) == 0 and 'GAT' in last_error()
  lap = descriptor(g, 24, 16, 4, True)
  lap.struct.kind = _lib.RHS_LAPLACIAN
  lap.struct.w_csr = lap.struct.proj_w
  assert size(lap) == 0 and 'GAT' in last_error()
  # no table
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.out_w = None
  assert size(bad) == 0 and 'out_w' in last_error()
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.out_ld = 12
  assert size(bad) == 0 and 'out_ld' in last_error()
  # partitioned descriptors
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.proj_row_begin, bad.struct.proj_row_end = 0, 64
  assert size(bad) == 0 and 'partitioned' in last_error()
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.n_state_rows = 158
  assert size(bad) == 0 and 'partitioned' in last_error()
  # shapes outside the kernel's rule
  for d, A, heads in [(260, 16, 4), (24, 6, 3), (24, 260, 4)]:
    assert size(descriptor(g, d, A, heads, True)) == 0 and 'attention_dim' in last_error(), (d, A)
    assert size(descriptor(g, d, A, heads, False)) > 0
  # error codes: the kind is an argument error, partition and shape are shape errors (read from an entry point that returns them)
  h = ctypes.c_void_p()
  dts = (ctypes.c_float * 1)(1.0)
  create = lambda desc: L.gnpde_solver_create(ctypes.byref(h), desc.ref(), _lib.METHOD_EULER, dts, 1, None, 0)      # noqa: E731
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.kind, bad.struct.proj_m = _lib.RHS_TRANSFORMER, 32
  assert create(bad) == EINVAL
  bad = descriptor(g, 24, 16, 4, True)
  bad.struct.proj_row_end = 64
  assert create(bad) == ESHAPE
  assert create(descriptor(g, 260, 16, 4, True)) == ESHAPE
  # the objects that differentiate or shard refuse before they look at anything else
  assert L.gnpde_adjoint_create(ctypes.byref(h), ok.ref(), None, None, None, None, _lib.METHOD_RK4, dts, 1, None, 0) == ESHAPE
  assert 'mix_features' in last_error()
  assert L.gnpde_adjoint_adaptive_create(ctypes.byref(h), ok.ref(), None, None, _lib.ADAPTIVE_DOPRI5, 1e-5, 1e-7, None, 0) == ESHAPE
  assert L.gnpde_solver_gather_bytes(ok.ref(), _lib.METHOD_RK4) == 0


def test_python_predicate_and_signature():
  """ODEFuncAtt._has_native_rhs is the one rule the route rule and forward consult; the descriptor signature sees the table."""
  from helpers import Data
  n = 50
  ei = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n]).long()
  base = dict(heads=4, attention_dim=16, attention_norm_idx=0, leaky_relu_slope=0.2, self_loop_weight=1, max_nfe=1000, add_source=False,
              no_alpha_sigmoid=False, mix_features=True)
  for d, A, heads, ok in [(24, 16, 4, True), (256, 256, 8, True), (260, 16, 4, False), (24, 6, 3, False), (24, 260, 4, False)]:
    x = torch.zeros(n, d)
    f = G.ODEFuncAtt(d, d, dict(base, attention_dim=A, heads=heads, hidden_dim=d), Data(x, ei), torch.device('cpu'))
    assert f._has_native_rhs(x) == ok, (d, A)
    plain = G.ODEFuncAtt(d, d, dict(base, attention_dim=A, heads=heads, hidden_dim=d, mix_features=False), Data(x, ei), torch.device('cpu'))
    assert plain._has_native_rhs(x)
    if not ok:
      with pytest.raises(NotImplementedError):
        f._descriptor(x)
