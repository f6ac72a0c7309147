"""Every line of the aggregation's dispatch table (width_class in csrc/spmm.hip) once, against the CPU oracle.

The table is keyed by the lane type (16-, 8- or 4-byte lanes: contiguous rows, so ld = d decides it), the number of lanes that cover a
row, and -- for rows of 17..32 16-byte lanes -- by whether at least half of the graph's rows have <= 16 entries (two rows per wave) or
not (one row per wave).  Two graphs of 400 rows, one of each kind, both with two hub rows (> 512 entries) that run as chunk items and
are folded by the 16-byte reduce kernel (d % 4 == 0) or the generic one."""
import pytest
import torch

import gnpde_amd as G
from gnpde_amd import ops
from oracle import restate as R
from helpers import assert_parity, random_graph

pytestmark = pytest.mark.gpu

N = 400
GRAPHS = {'short': dict(avg_deg=6, seed=11), 'long': dict(avg_deg=24, seed=12)}

# widths by lane type; the comment gives (lanes per row -> line of the table)
LANES16 = [24,    # 6: rows (8, 1, 4)
           64,    # 16: rows (16, 1, 4)
           80, 100, 128,   # 20, 25, 32 (128: no column predicate): row pairs on the short-row graph, wide L = 32 on the long-row graph
           200, 256,       # 50, 64 (256: no column predicate): wide L = 64
           300,   # 75: rows (64, 2, 2)
           520,   # 130: rows (64, 3, 1)
           800]   # 200: rows (64, 4, 1)
LANES8 = [6, 30, 50, 90, 162, 302, 402]     # 3, 15, 25, 45, 81, 151, 201 lanes: rows (8,1,4) (16,1,4) (16,2,4) (32,2,4) (64,2,2) (64,3,1) (64,4,1)
LANES4 = [7, 15, 31, 63, 127, 191, 255]     # the same seven lines on 4-byte lanes


@pytest.fixture(scope='module')
def graphs(dev):
  out = {}
  for kind, kw in GRAPHS.items():
    ei = random_graph(N, kw['avg_deg'], seed=kw['seed'], hubs=2, hub_deg=600)
    g = torch.Generator().manual_seed(kw['seed'] + 100)
    w = torch.rand(ei.size(1), generator=g) * 0.3 + 0.01
    graph = G.CSRGraph(ei.to(dev), N)
    out[kind] = (ei, w, graph, ops.edge_to_csr_mean(graph, w.to(dev)))
  # a change of the generator must not quietly move a case to another line of the table
  assert 2 * out['short'][2].n_bin16 >= N and out['short'][2].n_long_rows >= 2
  assert 2 * out['long'][2].n_bin16 < N and out['long'][2].n_long_rows >= 2
  return out


@pytest.mark.parametrize('kind', ['short', 'long'])
@pytest.mark.parametrize('d', LANES16 + LANES8 + LANES4)
def test_dispatch_line(dev, graphs, kind, d):
  ei, w, graph, w_csr = graphs[kind]
  g = torch.Generator().manual_seed(1000 + d)
  x = torch.randn(N, d, generator=g)
  x0 = torch.randn(N, d, generator=g)
  alpha, beta = torch.tensor(0.3), torch.tensor(-0.7)
  xd = x.to(dev)
  assert xd.stride(0) == d
  out = ops.spmm_rhs(graph, w_csr, xd, alpha.to(dev), beta.to(dev), x0.to(dev), True)
  assert_parity(out, R.rhs_laplacian(x, ei, w, alpha, beta, x0, no_alpha_sigmoid=False, add_source=True), what='spmm_rhs %s d=%d' % (kind, d))
  assert_parity(ops.spmm(graph, w_csr, xd), R.spmm(ei, w, N, x), what='spmm %s d=%d' % (kind, d))


def test_width_past_the_table_is_a_shape_error(dev, graphs):
  ei, w, graph, w_csr = graphs['short']
  x = torch.zeros(N, 257, device=dev)      # 257 4-byte lanes: one more than the widest line
  with pytest.raises(G.GnpdeError, match='too large'):
    ops.spmm(graph, w_csr, x)
  with pytest.raises(G.GnpdeError, match='too large'):
    ops.spmm_rhs(graph, w_csr, x, torch.tensor(0.3).to(dev), torch.tensor(-0.7).to(dev), x, True)
