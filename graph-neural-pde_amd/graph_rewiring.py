"""k-nearest-neighbour rewiring in feature space (BLEND's `--rewire_KNN`; reference src/graph_rewiring.py:116-147): `KNN` and
`apply_KNN` under the reference's names and signatures.  The search is the native kernel behind `ops.knn` (the reference uses a
pykeops LazyTensor.argKmin); making the edge set undirected is torch device ops (once per rewiring).

Tie order is a definition of this package (KeOps leaves it unspecified): a node's neighbours are ascending by the computed
distance, equal distances by ascending node index; a node is its own first neighbour (distance exactly 0)."""
import torch

from . import ops


def to_undirected(edge_index, num_nodes):
  """Both directions of every edge, duplicates removed, sorted by (row, col): what torch_geometric.utils.to_undirected returns for
  an index without edge attributes."""
  row = torch.cat([edge_index[0], edge_index[1]])
  col = torch.cat([edge_index[1], edge_index[0]])
  key = torch.unique(row * int(num_nodes) + col)     # sorted
  return torch.stack([torch.div(key, int(num_nodes), rounding_mode='floor'), key % int(num_nodes)], dim=0)


def KNN(x, opt):
  """edge_index [2, n k] int64: row 0 is every node repeated k times, row 1 its k nearest neighbours in squared Euclidean
  distance (the reference's layout, graph_rewiring.py:127-129); with opt['rewire_KNN_sym'] the undirected edge set."""
  k = opt['rewire_KNN_k']
  print(f"Rewiring with KNN: t={opt['rewire_KNN_T']}, k={opt['rewire_KNN_k']}")
  ind = ops.knn(x, k)
  n = ind.shape[0]
  src = torch.arange(n, dtype=torch.int64, device=ind.device).repeat_interleave(k)
  ei = torch.stack([src, ind.reshape(-1)], dim=0)
  if opt['rewire_KNN_sym']:
    ei = to_undirected(ei, n)
  return ei


@torch.no_grad()
def apply_KNN(data, pos_encoding, model, opt):
  if opt['rewire_KNN_T'] == "raw":
    ei = KNN(data.x, opt)  # rewiring on raw features here
  elif opt['rewire_KNN_T'] == "T0":
    ei = KNN(model.forward_encoder(data.x, pos_encoding), opt)
  elif opt['rewire_KNN_T'] == 'TN':
    ei = KNN(model.forward_ODE(data.x, pos_encoding), opt)
  else:
    raise Exception("Need to set rewire_KNN_T")
  return ei
