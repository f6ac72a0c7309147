"""Which solver runs a solve, and why not a faster one: the one route rule of `odeint`, the early-stopping test integrators and the
backward intervals of the adjoint method.  Pure host Python -- no device call, and no device -> host read beyond odeint's cached
`_strictly_increasing`; the callers ask, then dispatch on the name.

  forward(func, y0, t, method, options)                  -> (route, reason)      odeint
  early(func, y0, t, method, host_loop, max_test_steps)  -> (route, reason)      EarlyStopRK4 / EarlyStopDopri5 .integrate
  adjoint(func, y, method, options, params)              -> (route, reason)      one backward interval of _AdjointSolve

`reason` says why the next-faster route was refused (None: the fastest route runs); every reason is one of REASONS.

  route               runner                                         runs
  ------------------  ---------------------------------------------  ----------------------------------------------------------------
  native_fixed        _solve_native                                  euler / midpoint / rk4, whole time loop one captured graph
  sharded             distributed.solve_sharded                      rows partitioned over the ranks (gnpde_shard, two output times)
  recorded_fixed      _solve_fixed_recorded                          differentiated fixed grid: recorded solve + native reverse sweep
  host_fixed          _solve_fixed_host                              fixed grid, one evaluation of f at a time (any callable)
  device_controller   _solve_dopri5_device                           dopri5 / adaptive_heun, step-size controller on the device
  host_stages         _solve_dopri5_native                           dopri5, native stages, controller on the host (eager_stages)
  recorded_dopri5     _solve_dopri5_recorded                         differentiated dopri5: recorded solve + native reverse sweep
  host_loop           _solve_dopri5                                  embedded pair, one evaluation of f at a time (any callable)
  adjoint_native      _adjoint_native                                fixed-grid adjoint interval as one native object
  adjoint_stagewise   _adjoint_fixed_grid                            fixed-grid adjoint interval, one autograd VJP per stage
  adjoint_device      _adjoint_adaptive_native(device_controller=1)  adaptive adjoint on the components, controller on the device
  adjoint_host_pair   _adjoint_adaptive_native                       adaptive adjoint on the components, controller on the host
  adjoint_flat        odeint over the flat augmented vector          everything else (torchdiffeq's own formulation)

Two fallbacks depend on the device and stay in their runners: a recorded dopri5 solve whose accepted steps outgrow the tape
(`_TapeTooLong`: the solve runs again on the host loop), and the free-memory estimate of `_solve_fixed_recorded` (a record that would not
fit runs the host loop).  `adjoint_device` keeps one guard in its runner, the 16-byte row stride of the buffer the runner allocates."""
import os

import torch

from . import _lib
from . import odeint as O

FIXED, ADAPTIVE, ADJOINT_FIXED = ('euler', 'rk4', 'midpoint'), ('dopri5', 'adaptive_heun'), ('euler', 'rk4')
ROUTES = ('native_fixed', 'sharded', 'recorded_fixed', 'host_fixed', 'device_controller', 'host_stages', 'recorded_dopri5', 'host_loop',
          'adjoint_native', 'adjoint_stagewise', 'adjoint_device', 'adjoint_host_pair', 'adjoint_flat')

FOREIGN = 'foreign callable'
STATE = 'state is not a float32 [n, d] tensor on a HIP device'
DIFFERENTIATED = 'differentiated solve'
NO_RHS = 'no native right-hand side for this configuration'
SHARD_OUTPUTS = 'gnpde_shard: the row-partitioned solver has two output times'
NOT_INCREASING = 'output times are not strictly increasing'
TIMES_DTYPE = 'times are not float32'
CALLER_NORM = 'a norm of the caller'
EARLY_OUTPUTS = 'early stopping has two output times'
NO_TRIAL_BUDGET = 'max_test_steps is under one'
WIDE = 'state is wider than 256 columns'
NO_VJP_STAGE = 'no native VJP stage for this function and configuration'
TAPE_BUSY = 'the record of an earlier forward pass still awaits its backward'
ADJOINT_METHOD = 'no native adjoint solve for this method'
NOT_LAPLACIAN = 'native adaptive adjoint covers the Laplacian function only'
SCALAR_PARAMS = 'alpha_train or beta_train is not among the adjoint parameters'
# (a refusal by a switch is reported under the switch's own name)
SWITCHES = ('gnpde_host_outputs', 'gnpde_shard', 'gnpde_host_dopri5_training', 'gnpde_host_fixed_training', 'gnpde_composite_backward',
            'gnpde_host_adjoint', 'gnpde_host_controller_adjoint', 'no_alpha_sigmoid', 'GNPDE_HOST_DOPRI5_TRAINING',
            'GNPDE_HOST_FIXED_TRAINING', 'host_controller', 'eager_stages', 'host_flat')
REASONS = (FOREIGN, STATE, DIFFERENTIATED, NO_RHS, SHARD_OUTPUTS, NOT_INCREASING, TIMES_DTYPE, CALLER_NORM, EARLY_OUTPUTS, NO_TRIAL_BUDGET,
           WIDE, NO_VJP_STAGE, TAPE_BUSY, ADJOINT_METHOD, NOT_LAPLACIAN, SCALAR_PARAMS) + SWITCHES


# --------------------------------------------------------------------------------------------------
# the facts of a solve, each read in one place
# --------------------------------------------------------------------------------------------------
def on_device(y):
  """The state every native route takes: a float32 [n, d] tensor on a HIP device."""
  return y.is_cuda and y.dim() == 2 and y.dtype == torch.float32


def env_switched(name):
  """A `GNPDE_HOST_*` switch of the environment (A/B runs of bench.py); the `gnpde_*` switches are read from func.opt below."""
  return os.environ.get(name, '0') == '1'


def host_outputs_requested(func):
  """opt['gnpde_host_outputs'] (or GNPDE_HOST_OUTPUTS=1): solves with more than two output times keep the host loops (A/B runs, tests)."""
  opt = getattr(func, 'opt', None)
  v = env_switched('GNPDE_HOST_OUTPUTS')
  if hasattr(opt, 'get'):
    v = opt.get('gnpde_host_outputs', v)
  return bool(v)


def shard_requested(func):
  """opt['gnpde_shard'] (or GNPDE_SHARD=1) with an initialised process group (distributed.shard_requested)."""
  from . import distributed as D
  return D.shard_requested(func)


def vjp_stage_native(func):
  """Whether the native VJP stage of csrc/adjoint.hip (recorded solves, fixed-grid adjoint) covers this function: the Laplacian function
  always, GRAND-nl and GAT within the shapes of odeint._transformer_stage_native / _gat_stage_native, nothing else."""
  kind = func.__class__.__name__
  if kind == 'LaplacianODEFunc':
    return True
  if kind == 'ODEFuncTransformerAtt':
    return O._transformer_stage_native(func)
  if kind == 'ODEFuncAtt':
    return O._gat_stage_native(func)
  return False


def tape_busy(func, name):
  """True while the record of an earlier forward pass of this function is still waiting for its backward (the autograd node of that pass
  is alive and has not run): the next differentiated solve then takes the host loop instead of overwriting it -- two forwards before
  one backward (siamese losses, gradient accumulation over two graphs) stay differentiable, as in the reference."""
  ref = func.__dict__.get(name)
  ctx = ref() if ref is not None else None
  return ctx is not None and not getattr(ctx, 'gnpde_consumed', False)


# --------------------------------------------------------------------------------------------------
# refusals: None, or the reason a family of routes cannot take the solve
# --------------------------------------------------------------------------------------------------
def _native_refusal(func, y0):
  """The no-grad native solves (fixed grid, device controller, native stages, row-partitioned)."""
  if not hasattr(func, '_descriptor'):
    return FOREIGN
  if not on_device(y0):
    return STATE
  if func._needs_grad(y0):
    return DIFFERENTIATED
  if not func._has_native_rhs(y0):
    return NO_RHS
  return None


def _outputs_refusal(func, t):
  """More than two output times on a native solve that could take two."""
  if host_outputs_requested(func):
    return 'gnpde_host_outputs'
  if shard_requested(func):
    return SHARD_OUTPUTS
  if not O._strictly_increasing(t):
    return NOT_INCREASING
  return None


def _controller_refusal(t, method, options):
  """The device controller, for a solve the native stages can take."""
  if t.dtype != torch.float32:
    return TIMES_DTYPE
  if options.get('host_controller', False):
    return 'host_controller'
  if method == 'adaptive_heun' and options.get('norm') is not None:
    return CALLER_NORM
  return None


def _recorded_refusal(func, y0, t, method, options):
  """The recorded solve + native reverse sweep of a differentiated two-time solve that is not a foreign callable's and is on the device
  (the Laplacian function swept by csrc/dopri5.hip or csrc/adjoint.hip, GRAND-nl and GAT by the VJP stage of csrc/adjoint.hip)."""
  dopri5 = method == 'dopri5'
  laplacian = func.__class__.__name__ == 'LaplacianODEFunc'
  if y0.shape[1] > 256:
    return WIDE
  if dopri5 and t.dtype != torch.float32:
    return TIMES_DTYPE
  opt = func.opt
  name = 'gnpde_host_dopri5_training' if dopri5 else 'gnpde_host_fixed_training'
  if opt.get(name):
    return name
  if opt.get('gnpde_composite_backward'):
    return 'gnpde_composite_backward'
  if dopri5 and laplacian:        # (the sweep of csrc/dopri5.hip takes alpha' = sigmoid(alpha_train); it runs inside a sharded process too)
    if opt.get('no_alpha_sigmoid'):
      return 'no_alpha_sigmoid'
  elif opt.get('gnpde_shard'):
    return 'gnpde_shard'
  if not vjp_stage_native(func):
    return NO_VJP_STAGE
  name = 'GNPDE_HOST_DOPRI5_TRAINING' if dopri5 else 'GNPDE_HOST_FIXED_TRAINING'
  if env_switched(name):
    return name
  if dopri5 and options:
    if options.get('norm') is not None:
      return CALLER_NORM
    for name in ('host_controller', 'eager_stages'):
      if options.get(name):
        return name
  return None


# --------------------------------------------------------------------------------------------------
# the three rules
# --------------------------------------------------------------------------------------------------
def forward(func, y0, t, method, options):
  """The route of odeint(func, y0, t, method=method, options=options) for a tensor state."""
  if method in FIXED:
    if options.get('step_size', None) is None:
      raise ValueError('fixed-grid methods need options["step_size"]')
    why = _native_refusal(func, y0)
    if len(t) > 2:
      why = why or _outputs_refusal(func, t)
      return ('native_fixed', None) if why is None else ('host_fixed', why)
    if why is None:
      if shard_requested(func):     # one process per GPU, rows partitioned over the ranks
        if method == 'midpoint':
          raise _lib.GnpdeError('gnpde_shard: the row-partitioned solver runs euler, rk4, dopri5 and adaptive_heun; unset gnpde_shard for midpoint')
        return 'sharded', None
      return 'native_fixed', None
    if why is DIFFERENTIATED and torch.is_grad_enabled():      # training without the adjoint method
      why = _recorded_refusal(func, y0, t, method, options)
      if why is None:
        return ('host_fixed', TAPE_BUSY) if tape_busy(func, '_tape_live_fixed') else ('recorded_fixed', None)
    return 'host_fixed', why
  if method not in ADAPTIVE:
    raise ValueError('unsupported method %r (euler, midpoint, rk4, dopri5, adaptive_heun)' % (method,))
  why = _native_refusal(func, y0)
  if why is not FOREIGN and shard_requested(func):
    # rows partitioned over the ranks; the controller runs on every rank over an all-reduced error norm
    if why is None and len(t) == 2:
      return 'sharded', None
    # (a replicated single-GPU solve on every rank would be a silent waste of N - 1 GPUs)
    raise _lib.GnpdeError('gnpde_shard is set but this %s solve cannot run row-partitioned (float32 [n, d] state on a HIP device, two '
                            'output times, no autograd) -- unset gnpde_shard for it' % method)
  if len(t) > 2:
    why = why or _outputs_refusal(func, t) or _controller_refusal(t, method, options)
    if why is None and method == 'dopri5' and options.get('eager_stages', False):
      why = 'eager_stages'
    return ('device_controller', None) if why is None else ('host_loop', why)
  if why is DIFFERENTIATED and torch.is_grad_enabled() and method == 'dopri5':      # training without the adjoint method
    why = _recorded_refusal(func, y0, t, method, options)
    if why is None:
      return ('host_loop', TAPE_BUSY) if tape_busy(func, '_tape_live_dopri5') else ('recorded_dopri5', None)
  why = why or _controller_refusal(t, method, options)
  if why is None and method == 'dopri5' and options.get('eager_stages', False):      # controller on the host, one scalar read per trial step
    return 'host_stages', 'eager_stages'
  return ('device_controller', None) if why is None else ('host_loop', why)


def early(func, y0, t, method, host_loop=False, max_test_steps=None):
  """The route of the early-stopping test integrators (`method` rk4: EarlyStopRK4, dopri5: EarlyStopDopri5 with its host_loop option
  and trial budget)."""
  why = _native_refusal(func, y0)
  if why is None and len(t) != 2:
    why = EARLY_OUTPUTS
  if method == 'rk4':
    return ('native_fixed', None) if why is None else ('host_fixed', why)
  if why is None and t.dtype != torch.float32:
    why = TIMES_DTYPE
  if why is not None:
    return 'host_loop', why
  if host_loop:
    return 'host_stages', 'host_controller'
  if int(max_test_steps) < 1:
    return 'host_stages', NO_TRIAL_BUDGET
  return 'device_controller', None


def adjoint(func, y, method, options, params):
  """The route of one backward interval of the adjoint method from the state `y`: `method` and `options` are the caller's adjoint_method
  and adjoint_options, `params` the parameters the gradients are asked for."""
  if method not in ADJOINT_FIXED and method not in ADAPTIVE:
    return 'adjoint_flat', ADJOINT_METHOD
  fixed = method in ADJOINT_FIXED
  if fixed and options.get('step_size') is None:
    raise ValueError('fixed-grid adjoint methods need adjoint_options["step_size"]')
  if not hasattr(func, '_descriptor'):
    why = FOREIGN
  elif not on_device(y):
    why = STATE
  elif fixed and y.shape[1] > 256:
    why = WIDE
  elif not fixed and func.__class__.__name__ != 'LaplacianODEFunc':
    why = NOT_LAPLACIAN
  else:
    why = None
    for name in ('gnpde_composite_backward', 'gnpde_host_adjoint') + (() if fixed else ('no_alpha_sigmoid',)):
      if func.opt.get(name):
        why = name
        break
  if fixed:
    if why is None and not vjp_stage_native(func):
      why = NO_VJP_STAGE
    return ('adjoint_native', None) if why is None else ('adjoint_stagewise', why)
  if why is None and options.get('host_flat', False):
    why = 'host_flat'
  # (a caller's own adjoint norm -- torchdiffeq's adjoint_options['norm'], e.g. 'seminorm' -- is honoured by the flat loop only: the
  # native controller's norm is the default mixed one)
  if why is None and options.get('norm') is not None:
    why = CALLER_NORM
  if why is not None:
    return 'adjoint_flat', why
  # the device controller (csrc/adjoint_adaptive.hip) integrates g_alpha -- and g_beta where there is a source term -- with the state
  ids = [id(p) for p in params]
  if id(func.alpha_train) not in ids or (func.opt['add_source'] and id(func.beta_train) not in ids):
    return 'adjoint_host_pair', SCALAR_PARAMS
  if func.opt.get('gnpde_host_controller_adjoint'):
    return 'adjoint_host_pair', 'gnpde_host_controller_adjoint'
  if y.shape[1] > 256:
    return 'adjoint_host_pair', WIDE
  return 'adjoint_device', None
