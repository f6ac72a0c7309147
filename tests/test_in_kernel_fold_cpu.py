"""Host side of the in-kernel hub-row fold (gnpde_agg_fold_launch): the ticket size export, the refusal of a ticket buffer that is too small
(before anything is launched), the switch that keeps the fold launch, the launch counter and the register budget recorded in profiles/kernel_resources.txt."""
import ctypes
import os
import re

import torch

import gnpde_amd as G
from gnpde_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_graph(n=600, hubs=(513, 600, 0)):
  """Rows of 3 entries but the first len(hubs) rows, which have the given lengths (0: an empty row)."""
  src, dst = [], []
  for i in range(n):
    m = hubs[i] if i < len(hubs) else 3
    src.append(torch.full((m,), i))
    dst.append((torch.arange(m) + i) % n)
  return G.CSRGraph(torch.stack([torch.cat(src), torch.cat(dst)]).long(), n)


def test_ticket_bytes_is_one_word_per_long_row():
  L = _lib.lib()
  g = _host_graph()
  assert g.n_long_rows == 2
  assert L.gnpde_spmm_ticket_bytes(g.ref()) == 4 * g.n_long_rows == 8
  assert L.gnpde_spmm_ticket_bytes(_host_graph(hubs=()).ref()) == 0
  assert L.gnpde_spmm_ticket_bytes(None) == 0
  # the partials' size keeps its meaning: one row of d floats (padded to 4) per chunk
  assert L.gnpde_spmm_workspace_bytes(g.ref(), 126) == g.n_long_chunks * 128 * 4 == 4 * 128 * 4


def test_too_small_tickets_are_refused_before_any_launch():
  L = _lib.lib()
  g = _host_graph()
  d = 128
  u, out = torch.zeros(g.n, d), torch.zeros(g.n, d)
  w = torch.zeros(g.e)
  alpha = torch.zeros(1)
  epi = ops.make_epilogue(alpha, None, None, True, stage=_lib.STAGE_RHS, out_k=out)
  ws = torch.zeros(L.gnpde_spmm_workspace_bytes(g.ref(), d), dtype=torch.uint8)
  tickets = torch.zeros(2, dtype=torch.int32)
  p = lambda t: ctypes.c_void_p(t.data_ptr())
  for nbytes in (0, 4, 7):
    rc = L.gnpde_spmm_rhs_tickets(g.ref(), p(w), p(u), d, d, ctypes.byref(epi), p(ws), ws.numel(), p(tickets), nbytes, None)
    assert rc == -3, (nbytes, rc)                    # GNPDE_EWS
    assert 'tickets' in L.gnpde_last_error().decode()
  # ticket bytes without a ticket pointer: a bad argument, not "no tickets"
  assert L.gnpde_spmm_rhs_tickets(g.ref(), p(w), p(u), d, d, ctypes.byref(epi), p(ws), ws.numel(), None, 8, None) == -1


def test_switch_counter_and_abi():
  L = _lib.lib()
  try:
    ops.agg_fold_launch(1)
  finally:
    ops.agg_fold_launch(0)
  assert L.gnpde_agg_fold_launch(2) == -1 and L.gnpde_agg_fold_launch(-1) == -1      # GNPDE_EINVAL
  assert L.gnpde_tune(22, 0) == -1                              # the switch is an entry of its own, not a tune key: 22 stays past the last
  assert L.gnpde_in_kernel_fold_launches() >= 0
  header = open(os.path.join(ROOT, 'include', 'gnpde.h')).read()
  in_header = int(re.search(r'#define\s+GNPDE_ABI_VERSION\s+(\d+)', header).group(1))
  assert in_header >= 21 and L.gnpde_abi_version() == in_header == _lib.ABI_VERSION
  for name in ('gnpde_spmm_ticket_bytes', 'gnpde_spmm_rhs_tickets', 'gnpde_in_kernel_fold_launches', 'gnpde_agg_fold_launch'):
    assert name in header


def test_row_pair_kernel_keeps_three_waves_per_simd_with_the_fold_inside():
  rows = {}
  for line in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')):
    m = re.match(r'^(\S+\.hip)\s+(.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$', line)
    if m:
      vgpr, agpr, sgpr, scratch, spills, lds, occ = (int(v) for v in m.groups()[2:])
      rows[m.group(2).replace('gnpde::', '')] = dict(vgpr=vgpr, scratch=scratch, spills=spills, occ=occ)
  for full in ('true', 'false'):
    for defer in ('true', 'false'):
      r = rows['spmm_pair_kernel<4, %s, false, %s>' % (full, defer)]
      assert r['occ'] >= 3 and r['vgpr'] <= 168 and r['scratch'] == 0 and r['spills'] == 0, (full, defer, r)
  # the wide-row kernels do not carry the fold: the registers and occupancy they had
  wide = {'spmm_wide_kernel<4, 32, 8, false, false>': (84, 5), 'spmm_wide_kernel<4, 32, 8, true, false>': (86, 5),
          'spmm_wide_kernel<4, 64, 8, false, false>': (84, 5), 'spmm_wide_kernel<4, 64, 8, true, false>': (80, 6)}
  for name, (vgpr, occ) in wide.items():
    assert (rows[name]['vgpr'], rows[name]['occ'], rows[name]['scratch'], rows[name]['spills']) == (vgpr, occ, 0, 0), (name, rows[name])
