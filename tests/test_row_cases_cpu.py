"""The helpers of tests/row_cases.py on the CPU: the staircase builder gives exactly the rows it promises and the host graph builder
bins them as the cases of tests/test_attention_dispatch_gpu.py assume; the per-segment metric catches a hub row that the whole-tensor
metric lets pass; and the inputs of every case are valid -- the fp32 oracle itself, on the same table, stays under TOL / 2 per segment
against the float64 one, so a kernel line over TOL there is the kernel's doing.

Measured maximum of the fp32 oracle's per-segment error over the 143 cases (n = 1200, standard-normal tables): 2.9e-6 on att [E,h]
(2-nohubs-scaled_dot-h8-dk4-n0-sqp), 2.3e-6 on the head mean (2-hubs-scaled_dot-h1-dk4-n0-sqp), both squareplus; the row softmax
(scaled_dot, exp_kernel, GAT, cosine_sim, pearson) stays <= 1.6e-6.  Head mean by length class: <=16 2.2e-6, 17..512 2.3e-6, >512 1.6e-6."""
import pytest
import torch

import gnpde_amd as G
import row_cases as RC
from helpers import TOL, assert_parity


@pytest.mark.parametrize('name', sorted(RC.GRAPHS))
def test_staircase_builder(name):
  kw = RC.GRAPHS[name]
  ei, lens, side = RC.graph_edges(name)
  n = kw['n']
  assert ei.dtype == torch.int64 and ei.shape[0] == 2 and lens.numel() == n
  assert torch.equal(torch.bincount(ei[side], minlength=n), lens)                  # exact lengths
  special = list(kw.get('short', RC.SHORT)) + list(kw.get('hubs', RC.HUBS))
  rest = sorted(lens.tolist())
  for v in special:
    rest.remove(v)                                                                 # every listed length is there
  assert int((lens == 0).sum()) == kw['empty']
  lo, hi = kw.get('fill', (1, 16))
  dup = kw.get('dup_row', True)
  ordinary = [v for v in rest if v != 0]
  if dup:
    ordinary.remove(RC.DUP_LEN)
  assert ordinary and all(lo <= v <= hi for v in ordinary)
  # a self-loop in every row that has entries; columns distinct but for ONE repeated entry in the dup row
  loops = torch.zeros(n, dtype=torch.bool)
  loops[ei[side][ei[0] == ei[1]]] = True
  assert torch.equal(loops, lens > 0)
  key = ei[side] * n + ei[1 - side]
  uniq, counts = torch.unique(key, return_counts=True)
  assert int((counts > 1).sum()) == int(dup) and int(counts.max()) == (2 if dup else 1)
  if dup:
    assert int(lens[int(uniq[counts > 1]) // n]) == RC.DUP_LEN
  # shuffled: the entries of the first rows are not stored together
  assert not torch.equal(ei[side], torch.sort(ei[side]).values)

  # the host builder bins the staircase side as intended (for a transposed staircase: the transposed graph, which the column
  # normaliser's fast path walks, and the long columns of the graph itself, which the general passes walk)
  graph = G.CSRGraph(ei, n, device='cpu')
  view = graph.transposed() if side else graph
  n16, n64, n_long, n_chunks = RC.expected_bins(lens)
  assert (view.n_bin16, view.n_bin64, view.n_long_rows, view.n_long_chunks) == (n16, n64, n_long, n_chunks)
  assert n_chunks == sum((v + 511) // 512 for v in lens.tolist() if v > 512)
  assert view.max_row_len == int(lens.max())
  if side:
    assert graph.n_long_cols == n_long and graph.max_col_len == int(lens.max())
    if n_long:
      assert (graph.max_col_len + 511) // 512 == 3                                 # seg_stats_long_* with max_chunks = 3
  if name in ('hubs', 'nohubs', 'hubs_t', 'nohubs_t'):
    assert n == 1200 and (11000 if 'nohubs' in name else 14000) <= ei.shape[1] <= 16000
    assert n_long == (0 if 'nohubs' in name else len(RC.HUBS))
    # the masked tail slots run: neither class fills its last workgroup, for any (heads, d_k)
    assert RC.ROWS_PER_BLOCK16 == [4, 8, 16, 32, 64]
    assert all(n16 % rpb != 0 for rpb in RC.ROWS_PER_BLOCK16), n16
    assert n64 % RC.WAVES_PER_BLOCK != 0, n64
    for h, dk in RC.SD_PAIRS:                                                      # squareplus without hubs: the per-wave-maxima sweep
      assert RC.sd_sweep_waves(h, dk // 4, n16, n64) <= RC.GMAX_PART_CAP
  if name == 'no16':
    assert n16 == 0 and n64 > 0 and n_long == 2
  if name == 'no64':
    assert n64 == 0 and n16 > 0 and n_long == 2


def test_per_segment_error_is_per_segment():
  ref = torch.tensor([[1.0, 2.0], [4.0, 0.5], [1e-3, 2e-3], [1e-3, 1e-3]], dtype=torch.float64)
  got = ref.clone()
  got[1, 1] += 0.04          # segment 0: 0.04 / 4
  got[3, 0] -= 1e-5          # segment 2: 1e-5 / 2e-3
  err = RC.per_segment_error(got.float(), ref, torch.tensor([0, 0, 2, 2]))
  assert err.shape == (3,) and float(err[1]) == 0.0
  assert abs(float(err[0]) - 0.01) < 1e-6 and abs(float(err[2]) - 5e-3) < 1e-6
  one = RC.per_segment_error(got[:, 0].float(), ref[:, 0], torch.tensor([0, 0, 2, 2]))     # [E] as well as [E, h]
  assert float(one[0]) == 0.0 and abs(float(one[2]) - 1e-2) < 1e-6
  classes = RC.class_errors(err, torch.tensor([2, 0, 600]))
  assert set(classes) == {'<=16', '>512'} and classes['>512'] == float(err[2])
  with pytest.raises(AssertionError, match='non-finite'):
    RC.assert_rows(torch.tensor([float('nan')]), torch.tensor([1.0], dtype=torch.float64), torch.tensor([0]), torch.tensor([1]), TOL, 'nan')


def test_a_hub_row_wrong_by_one_percent_passes_the_global_metric_and_fails_the_row_metric():
  """The motive, pinned: every entry of the 1100-entry hub row 1 % too large.  The whole-tensor metric misses it where the hub row is flat
  (entries of about 1 / 1100, an error of 9e-6 of the largest weight, 1.0) and the tensor has as many rows as the graphs of
  tests/test_kernels_gpu.py (3000 - 5000; here 6000: the 2-norm of the error, 3e-4, over that of ~6000 short rows, ~36).  On the
  1200-row graphs of the dispatch cases with their standard-normal tables the same planted error reads 7.7e-5 globally: the per-row
  metric is needed for what is ten times smaller than that."""
  n, h, A = 6000, 4, 16
  ei, lens = RC.staircase_graph(n, seed=41)
  table = torch.randn(n, 2 * A, generator=torch.Generator().manual_seed(42)) * 0.05
  eye, zero = torch.eye(A, dtype=torch.float64), torch.zeros(A, A, dtype=torch.float64)
  att, _ = RC.R.transformer_attention(table.double(), ei, torch.cat([eye, zero], dim=1), None, torch.cat([zero, eye], dim=1), None, h)
  ref = att.mean(dim=1)
  hub = int((lens == 1100).nonzero())
  planted = ref.clone()
  planted[ei[0] == hub] *= 1.01
  assert_parity(planted.float(), ref, tol=TOL, what='planted hub error, global metric')          # passes: the gap
  with pytest.raises(AssertionError, match=r'segment %d \(1100 entries\)' % hub) as info:
    RC.assert_rows(planted.float(), ref, ei[0], lens, TOL, 'planted hub error')
  assert '>512 9.' in str(info.value) or '>512 1.0' in str(info.value)                             # about 1e-2, named per class
  RC.assert_rows(ref.float(), ref, ei[0], lens, TOL, 'the reference itself in fp32')


@pytest.mark.parametrize('c', RC.CASES, ids=RC.case_id)
def test_inputs_are_valid_the_fp32_oracle_stays_under_half_the_tolerance(c):
  ei, lens, side = RC.graph_edges(c.graph)
  assert side == c.norm_idx
  att64, prods64 = RC.reference64(c)
  att32, _ = RC.reference(c, torch.float32)
  assert att64.dtype == torch.float64 and att32.dtype == torch.float32 and att64.shape == (ei.shape[1], c.h)
  seg = ei[c.norm_idx]
  sums = torch.zeros(lens.numel(), c.h, dtype=torch.float64).index_add_(0, seg, att64)
  assert float((sums[lens > 0] - 1).abs().max()) < 1e-12                                         # every segment is normalised
  err = RC.per_segment_error(att32, att64, seg)
  err_mean = RC.per_segment_error(att32.mean(dim=1), att64.mean(dim=1), seg)
  print('fp32 oracle per segment: att %.3e, head mean %.3e' % (float(err.max()), float(err_mean.max())))
  assert float(err.max()) <= TOL / 2 and float(err_mean.max()) <= TOL / 2
