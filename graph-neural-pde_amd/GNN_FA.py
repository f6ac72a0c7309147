"""`GNN_KNN` with the fully-adjacent layer (`opt['fa_layer']`, reference src/GNN_KNN.py:65-83 and :158-176): after the ODE block's
solve, ONE more solve of the same block -- rk4, step 1, over the block's own [0, T] (the blocks read opt['method'] and
opt['step_size'] at forward time but fixed their `t` at construction, so the reference's assignment to opt['time'] has no effect;
neither has it here) -- on an edge set that `graph_rewiring.add_edges` enlarges and, with opt['edge_sampling_rmv'] != 0,
`graph_rewiring.edge_sampling` thins.  Then `odefunc.edge_index` is the data's edge set again.

`GNN_KNN` itself keeps refusing `fa_layer`; this class does not run that refusal.  Differences from the reference: the three
options and `odefunc.edge_index` are restored in a `finally`, and so are the attention and the source term of the
first solve (they belong to the restored state, and the backward of its recorded solve reads them again; the second solve of a training forward takes the differentiable
host loop, because the first one's record still awaits its backward); the regularised twin `reg_odefunc.odefunc` follows every change of
the edge set; the random stream is this package's (graph_rewiring's docstring).  Without opt['fa_layer'] this is `GNN_KNN`.
`GNNKNNEarly` is not built."""
import torch

from .GNN import GNN
from .GNN_KNN import GNN_KNN
from . import graph_rewiring


class GNN_FA(GNN_KNN):
  def __init__(self, opt, dataset, device=torch.device('cpu')):
    GNN.__init__(self, opt, dataset, device)        # not GNN_KNN.__init__: that is where fa_layer is refused
    self.data_edge_index = dataset.data.edge_index.to(device)

  def _solve(self, x):
    if self.training and self.odeblock.nreg > 0:
      z, self.reg_states = self.odeblock(x)
      return z
    return self.odeblock(x)

  def _fa_layer(self, z):
    """The second diffusion (steps 1-7 of the reference, GNN_KNN.py:65-83)."""
    opt = self.opt
    saved = {k: opt[k] for k in ('time', 'method', 'step_size')}
    # what the FIRST solve ran with: the backward of its recorded solve reads the function's attention and source again
    funcs = (self.odeblock.odefunc, self.odeblock.reg_odefunc.odefunc)
    first = [(f.attention_weights, f.x0) for f in funcs]
    try:
      graph_rewiring.check_edge_sampling_supported(self, opt)
      opt['time'], opt['method'], opt['step_size'] = 1, 'rk4', 1
      self.odeblock.set_x0(z)
      graph_rewiring.set_edge_index(self, graph_rewiring.add_edges(self, opt))
      if opt['edge_sampling_rmv'] != 0:
        graph_rewiring.edge_sampling(self, z, opt)
      out = self.odeblock(z)
      return out[0] if isinstance(out, tuple) else out      # the regularisers' integrals are those of the first solve
    finally:
      graph_rewiring.set_edge_index(self, self.data_edge_index)
      for f, (att, x0) in zip(funcs, first):
        f.attention_weights, f.x0 = att, x0
      opt.update(saved)

  def forward(self, x, pos_encoding=None):
    x = self.encode(x, pos_encoding)
    self.odeblock.set_x0(x)
    z = self._solve(x)
    if self.opt.get('fa_layer', False):
      z = self._fa_layer(z)
    return self.decode(z, x.shape[1])

  def forward_ODE(self, x, pos_encoding=None):
    x = self.forward_encoder(x, pos_encoding)
    self.odeblock.set_x0(x)
    z = self._solve(x)
    if self.opt.get('fa_layer', False):
      z = self._fa_layer(z)
    if self.opt['augment']:
      z = torch.split(z, x.shape[1] // 2, dim=1)[0]
    return z
