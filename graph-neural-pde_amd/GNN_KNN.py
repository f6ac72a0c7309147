"""The model of BLEND's k-nearest-neighbour rewiring runs (reference src/GNN_KNN.py): `GNN` plus the two partial forwards that
`graph_rewiring.apply_KNN` searches in -- `forward_encoder` (the encoder output, `rewire_KNN_T = 'T0'`) and `forward_ODE` (the
diffused state, 'TN').  `forward(x, pos_encoding)` is the parent's.

`opt['fa_layer']` (the extra diffusion over `add_edges` / `edge_sampling` edge sets, reference GNN_KNN.py:65-83) raises
NotImplementedError HERE: the layer lives in the subclass `GNN_FA` (GNN_FA.py), which the drop-in serves under the name `GNN_KNN`
with `--native-edge-sampling`.  There is no `GNNKNNEarly`; the early-stopping variant is the natural follow-up."""
import torch
import torch.nn.functional as F

from .GNN import GNN


FA_LAYER_REFUSAL = ("opt['fa_layer'] (add_edges / edge_sampling diffusion of GNN_KNN) is not implemented in this class: "
                    "use gnpde_amd.GNN_FA")


class GNN_KNN(GNN):
  def __init__(self, opt, dataset, device=torch.device('cpu')):
    if opt.get('fa_layer', False):
      raise NotImplementedError(FA_LAYER_REFUSAL)
    super(GNN_KNN, self).__init__(opt, dataset, device)
    self.data_edge_index = dataset.data.edge_index.to(device)

  def forward(self, x, pos_encoding=None):
    if self.opt.get('fa_layer', False):
      raise NotImplementedError(FA_LAYER_REFUSAL)
    return super(GNN_KNN, self).forward(x, pos_encoding)

  def forward_encoder(self, x, pos_encoding=None):
    """The encoder with NO dropout, whatever the mode (reference GNN_KNN.py:106-146); on ogbn-arxiv the positional encoding
    bypasses `mp`, as there.  The same layers run in both modes (no test-time kernel swap), so the tensor that is searched does not
    depend on the mode the rewiring step finds the model in."""
    opt = self.opt
    y = None
    if opt['use_labels']:
      y = x[:, -self.num_classes:]
      x = x[:, :-self.num_classes]
    if opt['beltrami']:
      x = self.mx(x)
      p = pos_encoding if opt.get('dataset') == 'ogbn-arxiv' else self.mp(pos_encoding)
      x = torch.cat([x, p], dim=1)
    else:
      x = self.m1(x)
    if opt['use_mlp']:
      x = x + self.m11(F.relu(x))
      x = x + self.m12(F.relu(x))
    if y is not None:
      x = torch.cat([x, y], dim=-1)
    if opt['batch_norm']:
      x = self.bn_in(x)
    if opt['augment']:
      x = torch.cat([x, torch.zeros(x.shape).to(self.device)], dim=1)
    return x

  def forward_ODE(self, x, pos_encoding=None):
    """Encoder -> ODE block -> the `augment` split (reference GNN_KNN.py:148-182)."""
    if self.opt.get('fa_layer', False):
      raise NotImplementedError(FA_LAYER_REFUSAL)
    x = self.forward_encoder(x, pos_encoding)
    self.odeblock.set_x0(x)
    if self.training and self.odeblock.nreg > 0:
      z, self.reg_states = self.odeblock(x)
    else:
      z = self.odeblock(x)
    if self.opt['augment']:
      z = torch.split(z, x.shape[1] // 2, dim=1)[0]
    return z
