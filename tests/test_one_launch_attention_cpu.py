"""Compile-time side of the one-launch row attention (gnpde_tune(21, .)): the register budget of the new and the changed kernels as
tools/kernel_resources.py recorded it in profiles/kernel_resources.txt, the tune key and the launch-decision counter."""
import os
import re

import gnpde_amd as G
from gnpde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources():
  rows = {}
  for line in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')):
    m = re.match(r'^(\S+\.hip)\s+(.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$', line)
    if m:
      vgpr, agpr, sgpr, scratch, spills, lds, occ = (int(v) for v in m.groups()[2:])
      rows[m.group(2).replace('gnpde::', '')] = dict(vgpr=vgpr, scratch=scratch, spills=spills, lds=lds, occ=occ)
  return rows


def test_merged_attention_kernel_and_deferred_aggregation_fit_their_budgets():
  rows = _resources()
  merged = {k: v for k, v in rows.items() if k.startswith('row_attention_sd_one_kernel<')}
  assert len(merged) == 9                                      # 1, 2, 4 heads x d_k 4, 8, 16
  for name, r in merged.items():
    assert r['scratch'] == 0 and r['spills'] == 0, (name, r)
  head = merged['row_attention_sd_one_kernel<4, 1, 16, 2, 4, 4, 8>']      # the headline: 4 heads, d_k = 4
  assert head['occ'] >= 8 and head['vgpr'] <= 64, head
  for full in ('true', 'false'):
    plain = rows['spmm_pair_kernel<4, %s, false, false>' % full]
    defer = rows['spmm_pair_kernel<4, %s, false, true>' % full]
    assert (plain['vgpr'], plain['occ'], plain['scratch'], plain['spills']) == (136, 3, 0, 0), plain
    assert defer['occ'] == plain['occ'] and defer['scratch'] == 0 and defer['spills'] == 0, defer
  # the wide-row kernel is not touched: the registers and occupancy it had
  wide = {'spmm_wide_kernel<4, 32, 8, false, false>': (84, 5), 'spmm_wide_kernel<4, 32, 8, true, false>': (86, 5),
          'spmm_wide_kernel<4, 64, 8, false, false>': (84, 5), 'spmm_wide_kernel<4, 64, 8, true, false>': (80, 6)}
  for name, (vgpr, occ) in wide.items():
    assert (rows[name]['vgpr'], rows[name]['occ'], rows[name]['scratch'], rows[name]['spills']) == (vgpr, occ, 0, 0), (name, rows[name])
  # the two launches the other modes keep did not lose a wave per SIMD to the shared row body
  for name in ('row_attention_sd_kernel<4, 1, 16, 2, 4, 1, 0, false>', 'row_attention_sd_kernel<4, 1, 64, 1, 4, 8, 0, false>'):
    assert rows[name]['occ'] >= 8 and rows[name]['scratch'] == 0 and rows[name]['spills'] == 0, (name, rows[name])


def test_tune_key_and_decision_counter():
  L = _lib.lib()
  assert _lib.TUNE_ATT_ONE_LAUNCH == 21
  src = open(os.path.join(ROOT, 'graph-neural-pde_amd', 'csrc', 'common.h')).read()
  assert re.search(r'GNPDE_TUNE_ATT_ONE_LAUNCH\s*=\s*21\b', src) and re.search(r'GNPDE_TUNE_COUNT\s*=\s*22\b', src)
  try:
    G.ops.tune(_lib.TUNE_ATT_ONE_LAUNCH, 1)
  finally:
    G.ops.tune(_lib.TUNE_ATT_ONE_LAUNCH, 0)
  assert L.gnpde_tune(22, 0) == -1                              # GNPDE_EINVAL: past the last key
  assert L.gnpde_one_launch_evaluations() >= 0
