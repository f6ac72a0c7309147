"""Operator surface kept from the reference's src/base_classes.py so that GNN.py / run_GNN.py can
use these classes unchanged: ODEFunc (:77-95) and ODEblock (:32-74) with the same constructor
signatures, attributes written from outside (edge_index, edge_weight, attention_weights, x0, nfe),
parameter names (alpha_train, beta_train, alpha_sc, beta_sc) and the two-function layout
(`odefunc` + `reg_odefunc.odefunc`) that the reference's state_dicts contain."""
import torch
from torch import nn

from . import _lib
from .graph import graph_of
from .utils import MaxNFEException
from .odeint import odeint, odeint_adjoint


# --------------------------------------------------------------------------------------------------
# Regularisers of the dynamics (reference src/regularized_ODE_function.py:35-81, registry src/base_classes.py:10-29;
# "Adapted from cfinlay/ffjord-rnode" there).  Each maps (x, t, dx, func) -> one value per node that the solver integrates
# next to the state; run_GNN.py adds coeff * mean to the loss (:82-87).  Off in every best_params entry.
# --------------------------------------------------------------------------------------------------
def quadratic_cost(x, t, dx, unused_context):
  """kinetic_energy: 1/2 mean_c dx^2 per node (first order: uses the native backward)."""
  return 0.5 * dx.reshape(dx.shape[0], -1).pow(2).mean(dim=-1)


def directional_derivative(x, t, dx, unused_context):
  """directional_penalty: 1/2 mean_c (J dx)^2 with the vector-Jacobian product grad(dx, x, dx) of the reference (:58-64)."""
  ddx = torch.autograd.grad(dx, x, dx, create_graph=True)[0]
  return 0.5 * ddx.reshape(x.size(0), -1).pow(2).mean(dim=-1)


def total_derivative(x, t, dx, unused_context):
  """total_deriv: needs df/dt; these right-hand sides are autonomous, so -- like the reference (:38-55) -- it raises and
  points at the mathematically equivalent directional_penalty."""
  ddx = torch.autograd.grad(dx, x, dx, create_graph=True)[0]
  try:
    u = torch.full_like(dx, 1 / x.numel(), requires_grad=True)
    tmp = torch.autograd.grad((u * dx).sum(), t, create_graph=True)[0]
    partial_dt = torch.autograd.grad(tmp.sum(), u, create_graph=True)[0]
  except RuntimeError as e:
    if 'One of the differentiated Tensors' in str(e):
      raise RuntimeError('No partial derivative with respect to time. Use mathematically equivalent '
                         '"directional_derivative" regularizer instead')
    raise
  return 0.5 * (ddx + partial_dt).pow(2).reshape(x.size(0), -1).mean(dim=-1)


def jacobian_frobenius_regularization_fn(x, t, dx, context):
  """jacobian_norm2: what the reference computes under that name (:67-81) -- the sum over feature columns i of
  d(sum_nodes dx[:, i]) / dx[:, i], one backward pass per column."""
  total = 0.
  for i in range(x.shape[1]):
    total = total + torch.autograd.grad(dx[:, i].sum(), x, create_graph=True)[0][:, i]
  return total


REGULARIZATION_FNS = {
  'kinetic_energy': quadratic_cost,
  'jacobian_norm2': jacobian_frobenius_regularization_fn,
  'total_deriv': total_derivative,
  'directional_penalty': directional_derivative,
}


def create_regularization_fns(args):
  """(functions, coefficients) of the regularisers switched on in `args` (reference src/base_classes.py:18-29)."""
  fns, coeffs = [], []
  for key, fn in REGULARIZATION_FNS.items():
    if args.get(key) is not None:
      fns.append(fn)
      coeffs.append(args[key])
  return fns, coeffs


def _first_order(fn):
  return getattr(fn, '__name__', '') == 'quadratic_cost'


class RegularizedODEfunc(nn.Module):
  """Reference src/regularized_ODE_function.py:8-33 (state_dict prefix `reg_odefunc.odefunc.`): integrates the
  regularisers' per-node values next to the state.  dx = f(t, x) comes from the native kernels; a regulariser that
  differentiates dx a second time (create_graph) needs a twice-differentiable f, which the kernel-backed autograd
  function is not, so for those evaluations f is the composite of PyTorch device ops (same arithmetic, announced once)."""

  def __init__(self, odefunc, regularization_fns):
    super(RegularizedODEfunc, self).__init__()
    self.odefunc = odefunc
    self.regularization_fns = regularization_fns

  def forward(self, t, state):
    if not isinstance(state, tuple):
      return self.odefunc(t, state)
    with torch.enable_grad():
      x = state[0]
      if not x.requires_grad:
        x.requires_grad_(True)
      if not torch.is_tensor(t):
        t = torch.tensor(float(t), dtype=x.dtype, device=x.device)
      if t.is_floating_point() and not t.requires_grad:
        t = t.detach().requires_grad_(True)
      if len(state) == 1:
        return (self.odefunc(t, x),)
      if all(_first_order(fn) for fn in self.regularization_fns):
        dx = self.odefunc(t, x)
      else:
        from .autograd import twice_differentiable_rhs
        self.odefunc._check_nfe()
        dx = twice_differentiable_rhs(self.odefunc, x)
      reg = tuple(fn(x, t, dx, self.odefunc) for fn in self.regularization_fns)
      return (dx,) + reg


class ODEFunc(nn.Module):
  """Base of the three right-hand sides.  Subclasses implement `_descriptor(x)` (the native
  gnpde_rhs_t for the current attributes); `forward(t, x)` = nfe guard + one native evaluation."""

  def __init__(self, opt, data, device):
    super(ODEFunc, self).__init__()
    self.opt = opt
    self.device = device
    self.edge_index = None
    self.edge_weight = None
    self.attention_weights = None
    self.alpha_train = nn.Parameter(torch.tensor(0.0))
    self.beta_train = nn.Parameter(torch.tensor(0.0))
    self.x0 = None
    self.nfe = 0
    self.alpha_sc = nn.Parameter(torch.ones(1))
    self.beta_sc = nn.Parameter(torch.ones(1))
    self._cache = {}

  # ---- shared plumbing -------------------------------------------------------------------------
  def _graph(self, x):
    if self.edge_index is None:
      raise _lib.GnpdeError('%s.edge_index has not been set' % self.__class__.__name__)
    ei = self.edge_index
    if ei.device != x.device:
      raise _lib.GnpdeError('edge_index is on %s but the state is on %s' % (ei.device, x.device))
    return graph_of(ei, x.shape[0], x.device)

  def _locality_view(self, x, forward_solve=True):
    """graph.LocalityView the fused solves of this function run on (nodes relabelled part by part or by descending row
    length, whichever a timed aggregation prefers; results bit-identical up to the row permutation, which the solver undoes), or
    None.  opt['gnpde_reorder'] / GNPDE_REORDER: 'auto' (default: in evaluation mode, when the state does not fit the L2s and a
    candidate is at least 2 % faster), '1' (the faster candidate, always), 'parts' / 'degree' (that order), '0' (never).
    forward_solve=False: the caller is the BACKWARD (adjoint) solve of a training step -- it takes the decision its forward took
    and never counts as a repeat of the edge set."""
    import os
    mode = str(self.opt.get('gnpde_reorder', os.environ.get('GNPDE_REORDER', 'auto'))).lower()
    if mode == 'auto' and self.training:
      # training forwards may hand over a NEW edge set every step (hard attention, rewiring: reference
      # src/block_transformer_hard_attention.py:55-61) -- a clustering and a timing run per step would cost more than any order
      # can return.  So the automatic rule applies in training only from the SECOND FORWARD solve on the same edge_index tensor
      # (identity and version unchanged: constant / attention blocks, every epoch after the first).  The adjoint solve of a step
      # is not a repeat: with a fresh edge set per step it would otherwise run the probe on every step's backward.
      ei = self.edge_index
      if ei is None:
        return None
      last = self.__dict__.get('_reorder_seen')     # (tensor, version, forward solves seen): holds the tensor, so its id stays unique
      same = last is not None and last[0] is ei and last[1] == ei._version
      if forward_solve:
        count = last[2] + 1 if same else 1
        self.__dict__['_reorder_seen'] = (ei, ei._version, count)
      else:
        count = last[2] if same else 0
      if count < 2:
        return None
    return self._graph(x).locality_view(4 * int(x.shape[1]), mode)

  def _check_nfe(self):
    if self.nfe > self.opt["max_nfe"]:
      raise MaxNFEException
    self.nfe += 1

  # The fused solves count their evaluations in bulk, with the same outcome as _check_nfe once per evaluation: the reference raises at
  # the first evaluation that finds nfe > max_nfe, and nfe then stands at max_nfe + 1 (or where it already stood beyond that).
  def _nfe_room(self):
    """Evaluations the reference would still allow before it raises."""
    return self.opt['max_nfe'] + 1 - self.nfe

  def _charge_fixed_nfe(self, n_evals):
    """Before a fixed-grid solve of n_evals evaluations: raises where the reference would raise inside it, counting the evaluations it
    would have made until then.  A solve that fits is counted by the caller once it has run (`func.nfe += n_evals`)."""
    room = self._nfe_room()
    if n_evals > room:
      self.nfe += max(room, 0)
      raise MaxNFEException

  def _settle_adaptive_nfe(self, room, finished, spent):
    """After an adaptive device solve that was allowed `room` evaluations (_nfe_room() before it ran) and made `spent`."""
    if not finished or spent > room:
      self.nfe += min(spent, room)
      raise MaxNFEException
    self.nfe += spent

  def _needs_grad(self, x):
    if not torch.is_grad_enabled():
      return False
    return x.requires_grad or any(p.requires_grad for p in self.parameters())

  def _has_native_rhs(self, x):
    """Whether `_descriptor(x)` exists for this configuration and state shape: asked by every no-grad native solve (routes.py)
    and by `forward`.  Functions with a configuration outside their kernels' shapes override it (ODEFuncAtt with mix_features)."""
    return True

  def _source(self, x):
    """x0 term of the epilogue (opt['add_source'])."""
    if not self.opt['add_source']:
      return None
    if self.x0 is None:
      raise _lib.GnpdeError('add_source is set but x0 was never assigned (call ODEblock.set_x0)')
    return self.x0

  @staticmethod
  def _match_rows(x0, x):
    """The source term in the row layout of the state (the kernels use ONE leading dimension for every operand)."""
    x0 = _lib.f32rows(x0, 'x0')
    if x0.stride(0) == x.stride(0) or x0.shape != x.shape:
      return x0
    out = _lib.alloc_state(x.shape[0], x.shape[1], x.device) if _lib.is_padded(x) else torch.empty_like(x, memory_format=torch.contiguous_format)
    return out.copy_(x0)

  def _memo(self, key, tensors, make):
    """Cache derived device buffers on (identity, version) of their source tensors."""
    sig = tuple((id(t), t._version) if t is not None else None for t in tensors)
    hit = self._cache.get(key)
    if hit is not None and hit[0] == sig:
      return hit[2]
    val = make()
    self._cache[key] = (sig, tensors, val)  # `tensors` kept alive so that ids stay unique
    return val

  def forward(self, t, x):
    from . import ops
    self._check_nfe()
    if self._needs_grad(x):
      from .autograd import rhs_with_grad
      return rhs_with_grad(self, x)
    with torch.no_grad():
      x = _lib.f32c(x)   # descriptor (leading dimension) and kernels must see the same, contiguous, operand
      return ops.rhs_eval(self._descriptor(x), x)

  def __repr__(self):
    return self.__class__.__name__


class ODEblock(nn.Module):
  def __init__(self, odefunc, regularization_fns, opt, data, device, t):
    super(ODEblock, self).__init__()
    self.opt = opt
    self.t = t
    self.device = device
    self.aug_dim = 2 if opt['augment'] else 1
    self.odefunc = odefunc(self.aug_dim * opt['hidden_dim'], self.aug_dim * opt['hidden_dim'], opt, data, device)
    self.nreg = len(regularization_fns)
    self.reg_odefunc = RegularizedODEfunc(self.odefunc, regularization_fns)
    self.train_integrator = odeint_adjoint if opt['adjoint'] else odeint
    self.test_integrator = None
    self.set_tol()

  def set_x0(self, x0):
    self.odefunc.x0 = x0.clone().detach()
    self.reg_odefunc.odefunc.x0 = x0.clone().detach()

  def set_tol(self):
    self.atol = self.opt['tol_scale'] * 1e-7
    self.rtol = self.opt['tol_scale'] * 1e-9
    if self.opt['adjoint']:
      self.atol_adjoint = self.opt['tol_scale_adjoint'] * 1e-7
      self.rtol_adjoint = self.opt['tol_scale_adjoint'] * 1e-9

  def reset_tol(self):
    self.atol = 1e-7
    self.rtol = 1e-9
    self.atol_adjoint = 1e-7
    self.rtol_adjoint = 1e-9

  def set_time(self, time):
    self.t = torch.tensor([0, time]).to(self.device)

  def _second_function(self, odefunc, opt, data, device):
    """The reference's blocks build a SECOND function object and leave the first inside reg_odefunc
    (state_dicts therefore hold both); same here."""
    width = self.aug_dim * opt['hidden_dim']
    self.odefunc = odefunc(width, width, opt, data, device)

  def _share_graph(self, edge_index, edge_weight, device):
    """Hand the block's normalised adjacency to both function objects."""
    self.odefunc.edge_index = edge_index.to(device)
    self.odefunc.edge_weight = edge_weight.to(device)
    inner = self.reg_odefunc.odefunc
    inner.edge_index, inner.edge_weight = self.odefunc.edge_index, self.odefunc.edge_weight

  def _rw_graph(self, data, opt, device):
    from .utils import get_rw_adj
    ei, ew = get_rw_adj(data.edge_index, edge_weight=data.edge_attr, norm_dim=1, fill_value=opt['self_loop_weight'],
                        num_nodes=data.num_nodes, dtype=data.x.dtype)
    self._share_graph(ei, ew, device)
    return self.odefunc.edge_index, self.odefunc.edge_weight

  def _use_default_integrators(self, opt):
    self.train_integrator = odeint_adjoint if opt['adjoint'] else odeint
    self.test_integrator = odeint
    self.set_tol()

  def trajectory(self, x, times):
    """The state at every entry of `times` (strictly increasing, times[0] the start), [len(times), n, d], from ONE solve: the block's own
    `forward` runs -- attention weights, edge selection and rewiring are prepared as usual -- with `times` in place of `self.t` (the
    reference stitches separate integrations together, GNN_image.forward_plot_path, each restarting the step-size controller).
    No-grad solves of the package's functions run natively (odeint: 'native fixed grid' / 'native device controller')."""
    if self.training and self.nreg > 0:
      raise _lib.GnpdeError('ODEblock.trajectory: not while training with regularisers (their integrals belong to the end time)')
    times = torch.as_tensor(times, dtype=torch.float32) if not torch.is_tensor(times) else times
    if times.dim() != 1 or times.numel() < 2:
      raise ValueError('ODEblock.trajectory: times must be a vector of at least two times')
    # one device tensor per set of values, kept on the block like `self.t`: odeint caches its host reads of the times (grid, plan,
    # end points) per tensor object, so repeated calls with the same times read nothing back
    key = (str(times.dtype), tuple(times.detach().cpu().tolist()))
    kept = self.__dict__.get('_trajectory_kept')
    if kept is None or kept[0] != key:
      kept = self.__dict__['_trajectory_kept'] = (key, times.detach().to(self.device))
    self._trajectory_times = kept[1]
    try:
      return self.forward(x)
    finally:
      self._trajectory_times = None

  def _integrate(self, x, options):
    """Common tail of the block forwards (reference src/block_constant.py:35-70).  Inside `trajectory` the output times are the
    caller's and every output is returned."""
    times = getattr(self, '_trajectory_times', None)
    t = self.t.type_as(x) if times is None else times
    if times is not None and t.dtype != x.dtype:      # (kept per state dtype as well: type_as of another dtype makes a new tensor)
      cast = self.__dict__.setdefault('_trajectory_cast', {})
      hit = cast.get(x.dtype)
      if hit is None or hit[0] is not times:
        hit = cast[x.dtype] = (times, times.type_as(x))
      t = hit[1]
    integrator = self.train_integrator if self.training else self.test_integrator
    regularised = self.training and self.nreg > 0
    kw = dict(method=self.opt['method'], options=options, atol=self.atol, rtol=self.rtol)
    if self.opt['adjoint'] and self.training:
      kw.update(adjoint_method=self.opt['adjoint_method'],
                adjoint_options=dict(step_size=self.opt['adjoint_step_size']),
                adjoint_atol=self.atol_adjoint, adjoint_rtol=self.rtol_adjoint)
    if regularised:   # reference src/block_constant.py:40-43,64-67: (state, one integral per regulariser)
      state = (x,) + tuple(torch.zeros(x.size(0)).to(x) for _ in range(self.nreg))
      state_dt = integrator(self.reg_odefunc, state, t, **kw)
      return state_dt[0][1], tuple(st[1] for st in state_dt[1:])
    state_dt = integrator(self.odefunc, x, t, **kw)
    return state_dt[1] if times is None else state_dt

  def __repr__(self):
    return self.__class__.__name__ + '( Time Interval ' + str(self.t[0].item()) + ' -> ' + str(self.t[1].item()) + ")"
