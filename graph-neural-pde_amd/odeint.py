"""Integrator entry point with torchdiffeq's calling convention
(`odeint(func, y0, t, method=, options=, atol=, rtol=)` -> tensor [len(t), *y0.shape]), as used by
the reference's blocks (src/block_constant.py:57-62, src/block_transformer_attention.py:58-63).

Fixed-grid methods (`euler`, `rk4` == torchdiffeq 0.2.1's 3/8-rule rk4_alt_step_func) on one of this
package's ODEFunc objects run as ONE native solver object whose whole time loop is a captured
hipGraph (csrc/solver.hip); dopri5 / adaptive_heun run with the step-size controller on the device (csrc/dopri5.hip).  Both serve
any number of strictly increasing output times (output_plan / output_times below).  Everything else runs the host loops below, which
still evaluate f through the native kernels.  Which runner takes a solve, and why not a faster one, is decided in routes.py (its
docstring lists the routes): `odeint`, the early-stopping integrators and `_AdjointSolve.backward` ask it and dispatch on the name."""
import contextlib
import math
import os

import torch

from . import _lib
from . import routes

_THIRD = 1 / 3
_TRIAL_TRACE = None       # tests / diagnostics: a list that receives (t, dt, error ratio) of every trial step of the host-controlled adaptive solves
_EVALS_PER_STEP = {'euler': 1, 'midpoint': 2, 'rk4': 4}


def time_grid(t, step_size):
  """torchdiffeq FixedGridODESolver grid: niters = ceil((t1 - t0)/h + 1) points t0 + i h, the last
  one replaced by t1 (so the final step may be short).  Computed in t's dtype like the original."""
  t0, t1 = t[0], t[-1]
  niters = int(torch.ceil((t1 - t0) / step_size + 1).item())
  grid = torch.arange(0, niters, dtype=t.dtype, device=t.device) * step_size + t0
  grid[-1] = t1
  return grid


_GRID_CACHE = {}


def _cached_host_read(t, tag, read):
  """read(t) -- a device -> host synchronisation -- kept per (tensor object, version, storage address, dtype, tag); tensors without a
  version counter are read every time."""
  try:
    key = (id(t), t._version, t.data_ptr(), t.dtype, tag)
  except RuntimeError:
    key = None
  hit = _GRID_CACHE.get(key) if key is not None else None
  if hit is not None and hit[0] is t:
    return hit[1]
  val = read(t)
  if key is not None:
    if len(_GRID_CACHE) >= 64:
      _GRID_CACHE.clear()
    _GRID_CACHE[key] = (t, val)        # (holds `t`: its id cannot be handed to another tensor while it is a key)
  return val


def step_sizes(t, step_size):
  """The step sizes of torchdiffeq's fixed grid over `t` as host floats.  The blocks pass the SAME device tensor `block.t` on every forward
  pass: reading it back costs a device -> host synchronisation per solve (~25 us of a 150-us Cora forward), so the result is cached."""
  def read(t):
    grid = time_grid(t.detach().to('cpu'), step_size)
    return tuple((grid[1:] - grid[:-1]).tolist())
  return _cached_host_read(t, float(step_size), read)


def end_points(t):
  """(float(t[0]), float(t[-1])) with the same cache as step_sizes: the adaptive device solves read them once per `block.t`."""
  return _cached_host_read(t, 'ends', lambda t: (float(t[0]), float(t[-1])))


def output_plan(t, step_size):
  """Where the outputs t[1:] of a fixed-grid solve come from, as torchdiffeq's FixedGridODESolver.integrate (and `_solve_fixed_host`)
  decides it: ((step, frac), ...) -- output j + 1 is produced by the first step [ta, tb] of `time_grid` with tb >= t[j + 1] (`step`, 1-based),
  as y_next (frac 1.0), y (frac 0.0) or y + frac (y_next - y) with frac = (t[j + 1] - ta) / (tb - ta) computed in t's dtype.  Host floats,
  cached like step_sizes."""
  def read(t):
    tc = t.detach().to('cpu')
    grid = time_grid(tc, step_size)
    plan, j = [], 1
    for i in range(len(grid) - 1):
      ta, tb = grid[i], grid[i + 1]
      while j < len(tc) and tb >= tc[j]:
        if tc[j] == tb:
          frac = 1.0
        elif tc[j] == ta:
          frac = 0.0
        else:
          frac = float((tc[j] - ta) / (tb - ta))
        plan.append((i + 1, frac))
        j += 1
    return tuple(plan)
  return _cached_host_read(t, ('plan', float(step_size)), read)


def output_times(t):
  """t[1:] as host floats (the output times of an adaptive device solve; float64 of t's values, as the host loop's t.to(float64))."""
  return _cached_host_read(t, 'outs', lambda t: tuple(t.detach().to('cpu', torch.float64)[1:].tolist()))


def _strictly_increasing(t):
  return _cached_host_read(t, 'increasing', lambda t: bool((t[1:] > t[:-1]).all().item()))


def default_trials_per_sync(numel):
  """Trial steps of a device-controlled adaptive solve between two host reads of its record, by the size of the WHOLE state.  Launch-bound
  sizes: keep the queue full between reads; large states: a read per trial step costs nothing next to the evaluations and nothing is
  replayed past the end point."""
  return 8 if numel < (1 << 22) else 1


# --------------------------------------------------------------------------------------------------
# plumbing shared by the native solve paths: every path keeps its solver objects and state-sized buffers on the function object, in a
# slot of its own (func.__dict__[slot] = {key: entry}): _solver_state (fixed-step inference), _dopri5_device (adaptive inference),
# _tape_state / _fixed_tape_state (recorded dopri5 / fixed-grid training), _adjoint_state (fixed-grid adjoint), _dopri5_host (eager
# dopri5 with the host controller), _adjoint_adaptive (adaptive adjoint: host-controlled stages and the device solver)
# --------------------------------------------------------------------------------------------------
def _close_slot(func, slot):
  st = func.__dict__.get(slot)
  if st:
    for old in st.values():
      for name in ('solver', 'sweep'):
        if old.get(name) is not None:
          old[name].close()
    st.clear()


def _entry(func, slot, key, n, d, device, bufs=('y',), siblings=(), view=None):
  """The entry of `key` in the slot.  One live entry per slot: a miss closes what the slot holds -- its solvers' buffers are state-sized
  -- and what the `siblings` hold (an eval that alternates methods must not hold a fixed-step AND a 12-buffer dopri5 workspace), then
  allocates the state buffers named in `bufs`, and `x0` where the function has a source term (rows padded to a multiple of 4 floats
  when the width is not one: 16-byte lanes for d = 162 etc.).  The entry holds `view`, so that the id in the caller's key stays its."""
  st = func.__dict__.setdefault(slot, {})
  ent = st.get(key)
  if ent is None:
    _close_slot(func, slot)
    for name in siblings:
      _close_slot(func, name)
    ent = st[key] = {'solver': None, 'sweep': None, 'sig': None, 'sweep_sig': None, 'view': view, 'extra': {}, 'grads': None}
    for name in bufs:
      ent[name] = _lib.alloc_state(n, d, device)
    ent['x0'] = _lib.alloc_state(n, d, device) if func.opt['add_source'] else None
  return ent


def _solver_for(ent, sig, build, name='solver'):
  """ent[name] ('solver', or the 'sweep' over it), rebuilt by build() when the signature is another one; a sweep over an old solver goes
  with it."""
  sig_name = 'sig' if name == 'solver' else 'sweep_sig'
  if ent[name] is None or ent[sig_name] != sig:
    for old in ('solver', 'sweep') if name == 'solver' else ('sweep',):
      if ent[old] is not None:
        ent[old].close()
        ent[old] = None
    ent[name] = build()
    ent[sig_name] = sig
  return ent[name]


def _order32(view):
  """view.order as an int32 device tensor, kept on the view (the row map the solvers' own copies take); None without a view."""
  if view is None:
    return None
  order32 = view.__dict__.get('order32')
  if order32 is None:
    order32 = view.__dict__['order32'] = view.order.to(torch.int32).contiguous()
  return order32


def _rows_in(view, src, dst):
  """dst = the rows of src in the order the solver runs in (relabelled graph, graph.LocalityView: src[order])."""
  return dst.copy_(src) if view is None else view.enter(src, out=dst)


def _rows_out(view, src, dst):
  """dst = the rows of src back in the caller's order (src[inv])."""
  return dst.copy_(src) if view is None else view.leave(src, out=dst)


def _copy_source(func, dst, view=None):
  """The solver's copy of the source term, refreshed from func.x0."""
  if func.x0 is None:
    raise _lib.GnpdeError('add_source is set but x0 was never assigned (call ODEblock.set_x0)')
  _rows_in(view, func.x0.detach(), dst)


def _weights_t(func, graph, out=None):
  """The Laplacian weights in the entry order of the transposed graph; out: a buffer with a persistent address (captured graphs keep
  the pointer), at least one element long."""
  w_csr = func._weights_csr(graph)
  if graph.e == 0:
    return w_csr if out is None else out
  t_from_csr = graph.transposed_positions()[1]
  if out is None:
    return torch.index_select(w_csr[:graph.e], 0, t_from_csr[:graph.e].long())
  torch.index_select(w_csr[:graph.e], 0, t_from_csr[:graph.e].long(), out=out[:graph.e])
  return out


# --------------------------------------------------------------------------------------------------
# native fixed-step path
# --------------------------------------------------------------------------------------------------
_OUTPUT_REPORTS = {'native_fixed': 'native fixed grid', 'device_controller': 'native device controller'}


def _note_output_solve(func, route, reason):
  if hasattr(func, '_descriptor'):       # the route the last solve with more than two output times took, or why it was the host loop
    func._last_output_solve = _OUTPUT_REPORTS[route] if reason is None else 'host loop (%s)' % reason


def gather_dtype_requested(func):
  """opt['gnpde_gather_dtype'] (or GNPDE_GATHER_DTYPE): 'fp32' (default) or 'bf16' -- the element type of the neighbour rows the
  aggregation gathers in no-grad fixed-step solves ("bf16 gather operand").  Anything else raises ValueError."""
  opt = getattr(func, 'opt', None)
  v = os.environ.get('GNPDE_GATHER_DTYPE', 'fp32')
  if hasattr(opt, 'get'):
    v = opt.get('gnpde_gather_dtype', v)
  v = str(v).lower()
  if v not in _lib.GATHER_DTYPES:
    raise ValueError("gnpde_gather_dtype must be 'fp32' or 'bf16' (got %r)" % (v,))
  return v


_FP32_GATHER_DEPTH = [0]


@contextlib.contextmanager
def _fp32_gather():
  """Solves inside run with the fp32 gather operand whatever the option says (forward solves of the adjoint method)."""
  _FP32_GATHER_DEPTH[0] += 1
  try:
    yield
  finally:
    _FP32_GATHER_DEPTH[0] -= 1


def _note_gather(func, used):
  try:
    func.gather_dtype_used = used       # what the last solve of this function ran with
  except AttributeError:
    pass


def _solve_native(func, y0, t, method, step_size, use_graph=True, evaluator=None):
  from . import ops
  gather = gather_dtype_requested(func)
  if y0.shape[1] % 4 != 0 or _FP32_GATHER_DEPTH[0]:   # widths whose rows this layer pads, and the forward solve of the adjoint
    gather = 'fp32'                                   # method, keep the fp32 operand (scope of the option: INTEGRATION.md)
  dts = list(step_sizes(t, step_size))
  n_evals = len(dts) * _EVALS_PER_STEP[method]
  func._charge_fixed_nfe(n_evals)
  # relabelled graph (graph.LocalityView): the state enters as y0[order] and leaves as y[inv]; the in-graph early-stopping
  # evaluator gets its labels and split masks in the same order (EarlyStopEvaluator.relabelled: shared counters and trace)
  view = func._locality_view(y0) if hasattr(func, '_locality_view') else None
  if evaluator is not None and view is not None:
    evaluator = evaluator.relabelled(view)
  # more than two output times: the plan rides in the solver (snapshot nodes behind the steps that produce an output)
  plan = output_plan(t, step_size) if len(t) > 2 else None
  if plan is not None and evaluator is not None:
    raise _lib.GnpdeError('early stopping inside a fixed-grid solve has two output times')
  key = (method, tuple(dts), tuple(y0.shape), str(y0.device), id(view), gather, plan)
  y0c = y0.detach()
  ent = _entry(func, '_solver_state', key, y0c.shape[0], y0c.shape[1], y0c.device, siblings=('_dopri5_device',), view=view)
  _rows_in(view, y0c, ent['y'])
  if ent['x0'] is not None:
    # the solver's copy of the source term is refreshed only when the caller's tensor is another one or was written to (keyed on
    # the tensor OBJECT, kept alive here so that its address cannot be handed to another tensor, and its version counter)
    src = func.x0
    # (inference tensors have no version counter -- reading it raises -- and writes through .data / set_() do not bump it: the
    #  key also holds the storage address, and anything that cannot be keyed is copied every solve)
    try:
      stamp = None if src is None else (src._version, src.data_ptr())
    except RuntimeError:
      stamp = None
    if stamp is None or ent.get('x0_src') is not src or ent.get('x0_version') != stamp:
      _copy_source(func, ent['x0'], view)
      ent['x0_src'], ent['x0_version'] = src, stamp
  desc = func._descriptor(ent['y'], x0_override=ent['x0'], graph=None if view is None else view.graph)
  _solver_for(ent, func._descriptor_signature(desc), lambda: ops.FixedStepSolver(desc, method, dts, y0.device))
  if getattr(ent['solver'], 'evaluator', None) is not evaluator:
    ent['solver'].set_early_stop(evaluator)     # per-step early-stopping evaluation inside the same hipGraph
  if getattr(ent['solver'], 'gather_dtype', 'fp32') != gather:
    ent['solver'].set_gather(gather)            # raises for a shape the bf16 kernels do not cover: never a silent fp32 run
  if plan is not None:
    order32 = _order32(view)
    if getattr(ent['solver'], 'output_plan', None) != plan or getattr(ent['solver'], '_out_order', None) is not order32:
      # (a buffer with a persistent address: the captured graph holds it; rows land in the caller's order)
      ent['solver'].set_outputs(plan, torch.empty((len(plan),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device), order32)
  ent['solver'].run(ent['y'], use_graph=use_graph)
  _note_gather(func, gather)
  func.nfe += n_evals
  out = torch.empty((len(t),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
  out[0].copy_(y0c)
  if plan is not None:
    out[1:].copy_(ent['solver']._outs)
  else:
    _rows_out(view, ent['y'], out[1])
  return out


# --------------------------------------------------------------------------------------------------
# host loops (any callable)
# --------------------------------------------------------------------------------------------------
def _rk4_38_step(func, t0, dt, t1, y0):
  k1 = func(t0, y0)
  k2 = func(t0 + dt * _THIRD, y0 + dt * k1 * _THIRD)
  k3 = func(t0 + dt * (2 * _THIRD), y0 + dt * (k2 - k1 * _THIRD))
  k4 = func(t1, y0 + dt * (k1 - k2 + k3))
  return (k1 + 3 * (k2 + k3) + k4) * dt * 0.125


def _solve_fixed_host(func, y0, t, method, step_size, on_step=None):
  grid = time_grid(t, step_size)
  out = torch.empty((len(t),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
  out[0] = y0
  j = 1
  y = y0
  for i in range(len(grid) - 1):
    ta, tb = grid[i], grid[i + 1]
    dt = tb - ta
    if method == 'euler':
      dy = dt * func(ta, y)
    elif method == 'midpoint':      # torchdiffeq fixed_grid.py Midpoint._step_func
      half = 0.5 * dt
      dy = dt * func(ta + half, y + func(ta, y) * half)
    else:
      dy = _rk4_38_step(func, ta, dt, tb, y)
    y_next = y + dy
    while j < len(t) and tb >= t[j]:
      if t[j] == tb:
        out[j] = y_next
      elif t[j] == ta:
        out[j] = y
      else:
        out[j] = y + ((t[j] - ta) / (tb - ta)) * (y_next - y)
      j += 1
    y = y_next
    if on_step is not None:
      on_step(y, i + 1)
  return out


# Dormand-Prince 5(4) coefficients (Shampine's error weights), as used by torchdiffeq's dopri5
_DP_A = (1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0)
_DP_B = ((1 / 5,),
         (3 / 40, 9 / 40),
         (44 / 45, -56 / 15, 32 / 9),
         (19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729),
         (9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656),
         (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84))
_DP_E = (35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720,
         -2187 / 6784 + 12231 / 42400, 11 / 84 - 649 / 6300, -1 / 60)
_DP_MID = (6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
           187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2)


_DP_SOL = (35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0.0)

# embedded pairs of torchdiffeq 0.2.1 (dopri5.py, adaptive_heun.py): stage nodes, stage weights, solution and error
# weights, mid-point weights of the quartic interpolant, order; `fsal`: the last stage input is the solution
_TABLEAUS = {
  'dopri5': dict(alpha=_DP_A, beta=_DP_B, c_sol=_DP_SOL, c_err=_DP_E, c_mid=_DP_MID, order=5, fsal=True),
  'adaptive_heun': dict(alpha=(1.0,), beta=((1.0,),), c_sol=(0.5, 0.5), c_err=(0.5, -0.5), c_mid=(0.5, 0.0), order=2,
                        fsal=False),
}


def _rms(v):
  return v.pow(2).mean().sqrt()


def _mixed_norm(shapes):
  """torchdiffeq's default norm of a tuple state (misc.py _mixed_linf_rms_norm): the largest component rms."""
  sizes = [int(torch.Size(sh).numel()) for sh in shapes]

  def norm(v):
    return max(_rms(part) for part in torch.split(v, sizes))
  return norm


def _combine(y0, ks, coeffs, dt):
  """y0 + sum_j (c_j * dt) k_j with the coefficients rounded to the state dtype first, as
  torchdiffeq's k.matmul(beta * dt) does."""
  acc = None
  for kj, c in zip(ks, coeffs):
    if c == 0.0:
      continue
    term = kj * (torch.tensor(c, dtype=kj.dtype, device=kj.device) * dt)
    acc = term if acc is None else acc + term
  return acc if y0 is None else y0 + acc


def _solve_dopri5(func, y0, t, rtol, atol, max_num_steps=2 ** 31 - 1, safety=0.9, ifactor=10.0, dfactor=0.2,
                  on_accept=None, stop_after=None, tableau='dopri5', norm=None, on_reject=None):
  """Adaptive embedded Runge-Kutta (Dormand-Prince 5(4) by default, `adaptive_heun` 2(1)) with torchdiffeq 0.2.1's
  controller: time and step size in float64, state in y0's dtype, rms error norm (or `norm`), the last stage
  derivative reused as the next step's first (rk_common.py: f1 = k[..., -1], also for the non-FSAL Heun pair),
  quartic-interpolated output."""
  tab = _TABLEAUS[tableau]
  order = tab['order']
  nrm = norm if norm is not None else _rms
  dev = y0.device
  f64 = dict(dtype=torch.float64, device=dev)
  rtol_t, atol_t = torch.as_tensor(rtol, **f64), torch.as_tensor(atol, **f64)
  tt = t.to(torch.float64)
  out = torch.empty((len(t),) + tuple(y0.shape), dtype=y0.dtype, device=dev)
  out[0] = y0
  f0 = func(tt[0], y0)
  # initial step (Hairer, Norsett & Wanner), order p = 4
  scale = atol_t + torch.abs(y0) * rtol_t
  d0, d1 = nrm(y0 / scale), nrm(f0 / scale)
  h0 = torch.tensor(1e-6, dtype=y0.dtype, device=dev) if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
  f1 = func(tt[0].to(y0.dtype) + h0, y0 + h0 * f0)
  d2 = nrm((f1 - f0) / scale) / h0
  if d1 <= 1e-15 and d2 <= 1e-15:
    h1 = torch.max(torch.tensor(1e-6, dtype=y0.dtype, device=dev), h0 * 1e-3)
  else:
    h1 = (0.01 / max(d1, d2)) ** (1.0 / order)
  dt = torch.min(100 * h0, h1).to(torch.float64)
  y, f, t_prev, t_cur = y0, f0, tt[0], tt[0]
  interp = None
  for i in range(1, len(t)):
    n_steps = 0
    while tt[i] > t_cur and (stop_after is None or n_steps < stop_after):
      assert n_steps < max_num_steps, 'max_num_steps exceeded'
      assert t_cur + dt > t_cur, 'underflow in dt {}'.format(float(dt))
      dty = dt.to(y.dtype)
      ks = [f]
      yi = None
      for a_i, b_i in zip(tab['alpha'], tab['beta']):
        yi = _combine(y, ks, b_i, dty)
        ks.append(func(t_cur + dt if a_i == 1.0 else t_cur + a_i * dt, yi))
      y1 = yi if tab['fsal'] else _combine(y, ks, tab['c_sol'], dty)
      f1 = ks[-1]
      err = _combine(None, ks, tab['c_err'], dty)
      tol = atol_t + rtol_t * torch.max(y.abs(), y1.abs())
      ratio = nrm(err / tol)
      accept = bool(ratio <= 1)
      if _TRIAL_TRACE is not None:
        _TRIAL_TRACE.append((float(t_cur), float(dt), float(ratio)))
      if accept:
        y_mid = _combine(y, ks, tab['c_mid'], dty)
        interp = (y, y1, y_mid, ks[0], ks[-1], dty, t_cur, t_cur + dt)
        t_prev, t_cur = t_cur, t_cur + dt
        y, f = y1, f1
        if on_accept is not None:
          on_accept(y, float(t_cur))
      elif on_reject is not None:
        on_reject(y, float(t_cur))
      # step-size controller: torchdiffeq 0.2.1 computes the next step size under torch.no_grad (misc.py _optimal_step_size), so a
      # differentiated solve (opt['adjoint'] = False) treats every step size after the first as a constant of the backward pass
      with torch.no_grad():
        if ratio == 0:
          dt = dt * ifactor
        else:
          lo = 1.0 if ratio < 1 else dfactor
          r = ratio.to(torch.float64)
          factor = torch.clamp(safety / r ** (1.0 / order), min=lo, max=ifactor)
          dt = dt * factor
      n_steps += 1
    if stop_after is not None and n_steps >= stop_after:   # EarlyStopDopri5.advance: the state where it stopped
      out[i] = y
      continue
    ya, yb, ym, fa, fb, h, ta, tb = interp
    xfrac = ((tt[i] - ta) / (tb - ta)).to(y0.dtype)
    ca = 2 * h * (fb - fa) - 8 * (yb + ya) + 16 * ym
    cb = h * (5 * fa - 3 * fb) + 18 * ya + 14 * yb - 32 * ym
    cc = h * (fb - 4 * fa) - 11 * ya - 5 * yb + 16 * ym
    cd = h * fa
    total = ya + xfrac * cd
    xp = xfrac
    for coef in (cc, cb, ca):
      xp = xp * xfrac
      total = total + xp * coef
    out[i] = total
  return out


# --------------------------------------------------------------------------------------------------
# the embedded pair with torchdiffeq 0.2.1's controller on the host (one scalar read per trial step) and everything state-sized on the
# device, over a list of components: the eager forward dopri5 is one component, the adaptive adjoint two and a pair of scalars
# --------------------------------------------------------------------------------------------------
class _StageComponent(object):
  """One state-sized component of _solve_pair_host, on native stages: K_j = f(stage input) is ONE right-hand-side launch of `desc`
  whose epilogue also forms the next stage input  y + sign sum_m c_m K_m  (GNPDE_STAGE_LINCOMB; sign -1: the component runs in
  reversed time, the sign applied by negating the coefficients), the scaled rms is a device reduction.  `bufs`: y, y1, two stage
  inputs, stages + 1 derivatives (_component_bufs); `scratch`: the (one-element result, workspace) of the reduction."""

  def __init__(self, desc, sign, bufs, rtol, atol, scratch):
    self.desc, self.sign, self.tols, self.scratch = desc, sign, (float(atol), float(rtol)), scratch
    self.y, self.y1, self.u, self.K = bufs[0], bufs[1], bufs[2:4], list(bufs[4:])
    self.ws = desc.graph.workspace('rhs%d_%d' % (desc.struct.kind, desc.struct.d), _lib.lib().gnpde_rhs_workspace_bytes(desc.ref()))

  def signed(self, coefs):
    return [-c for c in coefs] if self.sign < 0 else list(coefs)

  def stage(self, j, src, dst=None, row=()):
    """K_j = f(src); dst = y + sign sum_m row_m K_m (m < j), the next stage input, in the same launch."""
    from . import ops
    if dst is None:
      ops.rhs_stage(self.desc, src, _lib.STAGE_LINCOMB, ws=self.ws, out_k=self.K[j])
    else:
      ops.rhs_stage(self.desc, src, _lib.STAGE_LINCOMB, ws=self.ws, y=self.y, out_k=self.K[j], out_y=dst, prev=self.K[:j],
                    coef=self.signed(row))

  def scaled_rms(self, terms, coefs, y1=None):
    """rms(sum_j c_j v_j / (atol + rtol max(|y|, |y1|))) in one fused pass, as a one-element tensor (overwritten by the next call)."""
    from . import ops
    return ops.rk_error_ratio(self.y, self.y if y1 is None else y1, terms, coefs, self.tols[0], self.tols[1], *self.scratch)

  def axpys(self, coefs, out):
    """out = y + sign sum_j c_j K_j, zeros skipped (views of padded rows are fine: plain torch ops)"""
    first = True
    for kj, c in zip(self.K, self.signed(coefs)):
      if c == 0.0:
        continue
      if first:
        torch.add(self.y, kj, alpha=c, out=out)
        first = False
      else:
        out.add_(kj, alpha=c)
    if first:
      out.copy_(self.y)
    return out

  def accept(self):
    """The trial step becomes the state; its last derivative is carried over as the next step's first."""
    self.y, self.y1 = self.y1, self.y
    self.K[0], self.K[-1] = self.K[-1], self.K[0]


def _component_bufs(prefix, stages):
  """The names of a component's buffers in an _entry."""
  return tuple(prefix + s for s in ('', '1', 'u0', 'u1')) + tuple('%sk%d' % (prefix, j) for j in range(stages + 1))


def _host_pair_entry(func, slot, key, n, d, device, bufs):
  """_entry of a host-controlled embedded-pair solve; its `extra` also keeps the scratch of the norm reductions between solves."""
  ent = _entry(func, slot, key, n, d, device, bufs)
  if 'ratio_dev' not in ent['extra']:
    ent['extra']['ratio_dev'] = torch.zeros(1, dtype=torch.float32, device=device)
    ent['extra']['err_ws'] = torch.empty(4096, dtype=torch.float32, device=device)
  return ent


def _solve_pair_host(method, comps, T0, T1, check, scalars=None, interp=None, on_accept=None, on_reject=None, stop_after=None,
                     initial_step_only=False, safety=0.9, ifactor=10.0, dfactor=0.2):
  """The embedded pair `method` of _TABLEAUS from T0 to T1 on the components `comps` (the _StageComponent protocol: y, y1, u, K,
  stage, scaled_rms, axpys, accept), with the accept / reject rule, step-size update (float64), carried-over derivative and
  Hairer-Norsett-Wanner initial step of `_solve_dopri5` (which stays the path for foreign callables); time and step size are host
  floats, every coefficient is float(float32(c) * float32(dt)).  The norm is torchdiffeq's mixed one, the largest component's scaled
  rms: one component alone is read straight from its one-element tensor.  `check()` runs once per stage, before its launches.

  scalars: an optional extra component of a few numbers in ONE small tensor -- attributes g (the state), g1, K (stages + 1 slots),
  stage(j, src) -> K_j given every component's stage input, ratio(v, g0, g1) -> the one-element largest |v| / tolerance.
  interp(x, h, c_mid): called before an accepted step that reaches T1 is committed (y, y1, K still those of the step) with the
  end-point fraction, float32(dt) and the mid-point coefficients; the interpolation is the caller's.
  on_accept / on_reject(first component's y, t), stop_after: as in `_solve_dopri5`; every trial step is appended to _TRIAL_TRACE
  when that is a list.  initial_step_only: stop after the initial step (two stages: K[0] holds f(y)).
  Returns (the step size the next trial step would take, trial steps made)."""
  import numpy as np
  f32 = np.float32
  tab = _TABLEAUS[method]
  order, stages = tab['order'], len(tab['alpha'])
  sc = scalars

  def norm(of_comp, of_scalars):
    if len(comps) == 1 and sc is None:
      return float(of_comp(comps[0]).item())
    parts = [of_comp(c).clone() for c in comps]
    return float(torch.cat(parts + ([of_scalars()] if sc is not None else [])).max().item())

  def stage(j, src, dst=None, row=()):
    check()
    for i, c in enumerate(comps):
      c.stage(j, src[i], None if dst is None else dst[i], row)
    if sc is not None:
      sc.K[j] = sc.stage(j, src)

  def lincomb(coefs):
    return sum(sc.K[j] * coefs[j] for j in range(len(coefs)) if coefs[j] != 0.0)

  # initial step (Hairer, Norsett & Wanner), as misc.py _select_initial_step over the mixed norm
  stage(0, [c.y for c in comps])
  d0 = norm(lambda c: c.scaled_rms([c.y], [1.0]), lambda: sc.ratio(sc.g, sc.g, sc.g))
  d1 = norm(lambda c: c.scaled_rms(c.K[:1], [1.0]), lambda: sc.ratio(sc.K[0], sc.g, sc.g))
  h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else float(f32(0.01) * f32(d0) / f32(d1))
  src = [c.axpys([h0], c.u[0]) for c in comps]
  stage(1, src)
  d2 = norm(lambda c: c.scaled_rms([c.K[1], c.K[0]], [1.0, -1.0]), lambda: sc.ratio(sc.K[1] - sc.K[0], sc.g, sc.g)) / h0
  h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else float(f32(f32(0.01) / f32(max(d1, d2))) ** f32(1.0 / order))
  dt = float(min(100 * h0, h1))
  t_cur, n_steps = T0, 0
  while not initial_step_only and T1 > t_cur and (stop_after is None or n_steps < stop_after):
    assert t_cur + dt > t_cur, 'underflow in dt {}'.format(dt)
    dty = f32(dt)
    rows = [[float(f32(b) * dty) for b in row] for row in tab['beta']]
    # first stage input from the derivative carried over (rk_common: f1 = k[..., -1], also for the non-FSAL Heun pair)
    src = [c.axpys(rows[0], c.u[0]) for c in comps]
    for r in range(1, stages + 1):               # K_r at stage input u_r; its epilogue forms u_{r+1}
      if r < stages:
        last = r == stages - 1 and tab['fsal']    # (first-same-as-last: the last stage input IS the solution)
        dst = [c.y1 if last else c.u[r % 2] for c in comps]
        stage(r, src, dst, rows[r])
        src = dst
      else:
        stage(r, src)
    if tab['fsal']:
      sol = rows[stages - 1]
    else:
      sol = [float(f32(c) * dty) for c in tab['c_sol']]
      for c in comps:
        c.axpys(sol, c.y1)
    cerr = [float(f32(e) * dty) for e in tab['c_err']]
    if sc is not None:
      sc.g1 = sc.g + lincomb(sol)
      err_s = lincomb(cerr)
    ratio = norm(lambda c: c.scaled_rms(c.K, cerr, c.y1), lambda: sc.ratio(err_s, sc.g, sc.g1))   # the one host sync of the step
    if _TRIAL_TRACE is not None:
      _TRIAL_TRACE.append((t_cur, dt, ratio))
    if ratio <= 1:
      t_next = t_cur + dt
      if t_next >= T1 and interp is not None:   # the end point lies in this step (torchdiffeq _interp_fit / _interp_evaluate)
        interp(float(f32((T1 - t_cur) / (t_next - t_cur))), float(dty), [float(f32(c) * dty) for c in tab['c_mid']])
      for c in comps:
        c.accept()
      if sc is not None:
        sc.K[0], sc.g = sc.K[stages], sc.g1
      t_cur = t_next
      if on_accept is not None:
        on_accept(comps[0].y, t_cur)
    elif on_reject is not None:
      on_reject(comps[0].y, t_cur)
    if ratio == 0:
      dt = dt * ifactor
    else:
      lo = 1.0 if ratio < 1 else dfactor
      dt = dt * min(ifactor, max(safety / ratio ** (1.0 / order), lo))
    n_steps += 1
  return dt, n_steps


def _solve_dopri5_native(func, y0, t, rtol, atol, on_accept=None, stop_after=None, on_reject=None):
  """dopri5 by _solve_pair_host on ONE native component of sign +1, the end point by the fused quartic interpolation
  (options eager_stages; EarlyStopDopri5's host loop).  Buffers: slot _dopri5_host.  Like the other host-controlled solves it now
  appends its trial steps to _TRIAL_TRACE when that is a list."""
  from . import ops
  names = _component_bufs('y', 6)
  ent = _host_pair_entry(func, '_dopri5_host', (tuple(y0.shape), str(y0.device)), y0.shape[0], y0.shape[1], y0.device, names + ('out',))
  ent['y'].copy_(y0.detach())
  if ent['x0'] is not None:
    _copy_source(func, ent['x0'])
  ex = ent['extra']
  comp = _StageComponent(func._descriptor(ent['y'], x0_override=ent['x0']), 1, [ent[nm] for nm in names], rtol, atol,
                         (ex['ratio_dev'], ex['err_ws']))
  out = torch.empty((2,) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
  out[0].copy_(y0)

  def interp(x, h, c_mid):
    out[1].copy_(ops.dopri5_interp(comp.y, comp.y1, comp.K, c_mid, h, x, ent['out']))
  n_steps = _solve_pair_host('dopri5', [comp], float(t[0]), float(t[-1]), func._check_nfe, interp=interp, on_accept=on_accept,
                             on_reject=on_reject, stop_after=stop_after)[1]
  if stop_after is not None and n_steps >= stop_after:   # EarlyStopDopri5.advance: the state where it stopped
    out[1].copy_(comp.y)
  return out


def _solve_dopri5_device(func, y0, t, rtol, atol, trials_per_sync=None, evaluator=None, stop_after=None, pair='dopri5'):
  """dopri5 with the controller on the device (csrc/dopri5.hip): a trial step is one hipGraph replay; accept / reject, the
  step-size update, the end-point interpolation and the commit are decided by kernels from a record in device memory, which the
  host reads once per `trials_per_sync` trial steps.  Same arithmetic as `_solve_pair_host` with one component (`_solve_dopri5_native`,
  which stays for A/B runs and for callers that hook into every step).  evaluator + stop_after: the early-stopping test integrator -- the decoder / arg-max / split counts run
  as kernels behind every trial step, gated by the controller, and the solve gives up after `stop_after` trial steps
  (gnpde_dopri5_set_early_stop); returns (out, times of the accepted steps) then."""
  from . import ops
  from .utils import MaxNFEException
  room = func._nfe_room()
  if room <= 0:
    raise MaxNFEException
  # Relabelled graph (graph.LocalityView) under the same rule as the fixed-step solves (opt['gnpde_reorder'] / GNPDE_REORDER, 'auto' by
  # default).  The error norm of a trial step is a sum over the rows; its squares are accumulated in double (csrc/misc.hip), so the
  # float32 ratio -- and with it every accept / reject decision and step size -- is the same on the relabelled graph as on the graph as
  # given (the states themselves are bit-identical row by row: the entries of a row keep their order)
  view = func._locality_view(y0) if hasattr(func, '_locality_view') else None
  if evaluator is not None and view is not None:
    evaluator = evaluator.relabelled(view)
  key = (tuple(y0.shape), str(y0.device), float(rtol), float(atol), id(view))
  y0c = y0.detach()
  ent = _entry(func, '_dopri5_device', key, y0c.shape[0], y0c.shape[1], y0c.device, siblings=('_solver_state',), view=view)
  if ent['x0'] is not None:
    _copy_source(func, ent['x0'], view)
  # (ent['y'] only fixes the row stride; the solver owns its buffers)
  desc = func._descriptor(ent['y'], x0_override=ent['x0'], graph=None if view is None else view.graph)
  sol = _solver_for(ent, func._descriptor_signature(desc), lambda: ops.Dopri5Solver(desc, rtol, atol, y0.device))
  if getattr(sol, 'pair', 'dopri5') != pair:      # (`pair`: 'dopri5' or torchdiffeq's 'adaptive_heun' -- the same controller, another trial step)
    sol.set_pair(pair)
  times = output_times(t) if len(t) > 2 else None
  if times is not None and evaluator is not None:
    raise _lib.GnpdeError('early stopping on the device controller has two output times')
  if times is None and getattr(sol, 'out_times', None) is not None:
    sol.set_outputs(None)
  if evaluator is not None:
    if getattr(sol, 'evaluator', None) is not evaluator or getattr(sol, 'max_trial_steps', None) != int(stop_after):
      sol.set_early_stop(evaluator, int(stop_after))
  elif getattr(sol, 'evaluator', None) is not None:
    sol.set_early_stop(None)
  if trials_per_sync is None:
    trials_per_sync = default_trials_per_sync(y0c.numel())
    if os.environ.get('GNPDE_DOPRI5_TRIALS_PER_SYNC'):          # A/B runs
      trials_per_sync = max(1, int(os.environ['GNPDE_DOPRI5_TRIALS_PER_SYNC']))
  out = torch.empty((len(t),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
  out[0].copy_(y0c)
  # relabelled graph: the permutation rides in the solver's own first and last copy (gnpde_dopri5_set_row_order) instead of two
  # index_select launches around it
  order32 = _order32(view)
  if getattr(sol, '_row_order', None) is not order32:
    sol.set_row_order(order32)
  if times is not None and getattr(sol, 'out_times', None) != times:
    # more than two output times: the accepted trial steps write the interior outputs (emit kernel of the captured trial step) into a
    # buffer with a persistent address, kept while the count stays; the last output is the run's own
    buf = getattr(sol, '_outs', None)
    if buf is None or buf.shape[0] != len(times):
      buf = torch.empty((len(times),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
    sol.set_outputs(times, buf)
  t0_, t1_ = end_points(t)
  finished = ent['solver'].run(y0c, t0_, t1_, out[-1], trials_per_sync=trials_per_sync, max_evals=room)
  spent = ent['solver'].stats()['evals']
  func._dopri5_stats = ent['solver'].stats()
  func._settle_adaptive_nfe(room, finished, spent)
  if times is not None:
    out[1:-1].copy_(sol._outs[:-1])
  if evaluator is not None:
    n_acc = ent['solver'].stats()['accepted']
    return out, ent['solver'].times[:n_acc + 1].tolist()
  return out


# --------------------------------------------------------------------------------------------------
# recorded dopri5: training WITHOUT the adjoint method (reference default opt['adjoint'] = False; best_params Cora / Citeseer)
# --------------------------------------------------------------------------------------------------
def _tape_claim(func, name, ctx):
  import weakref
  func.__dict__[name] = weakref.ref(ctx)


_TAPE_GROWTH_CAP_BYTES = 96 << 30     # a recorded dopri5 solve whose tape would outgrow this runs the host loop instead (round-5 advisor item)


class _TapeTooLong(_lib.GnpdeError):
  pass


_TAPE_BUDGET_BYTES = 8 << 30     # first tape allocation (it grows when a solve accepts more steps than it holds)


def _run_recorded_dopri5(func, sol, desc, y0c, t0, t1, out1, room):
  """One recorded run into out1; a tape that is too short doubles (up to _TAPE_GROWTH_CAP_BYTES) and the solve runs again.  Counts the
  evaluations into func.nfe as the host loop would and raises MaxNFEException where it would."""
  n = y0c.shape[0]
  tps = default_trials_per_sync(y0c.numel())
  while True:
    try:
      finished = sol.run(y0c, t0, t1, out1, trials_per_sync=tps, max_evals=room)
      break
    except _lib.GnpdeError as exc:
      if 'do not fit the tape' not in str(exc):
        raise
      torch.cuda.synchronize(y0c.device)
      state_bytes = max(n * desc.struct.ld * 4, 1)
      if 2 * sol.tape_capacity * 6 * state_bytes > _TAPE_GROWTH_CAP_BYTES:
        raise _TapeTooLong('recorded dopri5: %d accepted steps do not fit a tape of %.0f GB' % (sol.tape_capacity, _TAPE_GROWTH_CAP_BYTES / 1e9))
      sol.set_tape(2 * sol.tape_capacity)           # more accepted steps than slots: a longer tape, and the solve again
  stats = sol.stats()
  func._dopri5_stats = dict(stats, recorded=True)
  func._settle_adaptive_nfe(room, finished, stats['evals'])


def _recorded_dopri5_forward(func, y0, t0, t1, rtol, atol, bufs):
  """The forward pass of both recorded dopri5 Functions: the device-controlled solve with a tape, in the function's `_tape_state` entry
  (state buffers `bufs`).  Returns (entry, graph, descriptor, solver, [2, n, d] output)."""
  from . import ops
  from .utils import MaxNFEException
  room = func._nfe_room()
  if room <= 0:
    raise MaxNFEException
  y0c = _lib.f32c(y0.detach())
  n, d = y0c.shape
  ent = _entry(func, '_tape_state', (n, d, str(y0c.device), float(rtol), float(atol)), n, d, y0c.device, bufs)
  if ent['x0'] is not None:
    _copy_source(func, ent['x0'])
  graph = func._graph(y0c)
  desc = func._descriptor(ent['y'], x0_override=ent['x0'], graph=graph)      # (refreshes the CSR-ordered weights in place)

  def build():
    sol = ops.Dopri5Solver(desc, rtol, atol, y0c.device)
    state_bytes = max(n * desc.struct.ld * 4, 1)
    sol.set_tape(int(max(8, min(64, _TAPE_BUDGET_BYTES // (6 * state_bytes)))))
    return sol
  sol = _solver_for(ent, func._descriptor_signature(desc), build)
  out = torch.empty((2, n, d), dtype=torch.float32, device=y0c.device)
  out[0].copy_(y0c)
  _run_recorded_dopri5(func, sol, desc, y0c, t0, t1, out[1], room)
  sol.tape_generation += 1
  return ent, graph, desc, sol, out


def _check_tape(sol, gen, what, hint):
  """Backward of a recorded solve: the solver's tape must still hold the record of the forward pass stamped `gen`."""
  if sol is None or sol.handle is None or sol.tape_generation != gen:
    raise _lib.GnpdeError('%s: the tape of this forward pass was overwritten by a later solve of the same function '
                          '(backward must run before the next training forward; %s)' % (what, hint))


def _check_split_operands(func, split_sig, what):
  """Backward of a recorded solve on the BLEND split kernel: the derived operands must still be the ones its forward pass ran with."""
  if split_sig is not None and func.multihead_att_layer.split_operands()[0] != split_sig:
    raise _lib.GnpdeError('%s: the derived split-kernel projection of this forward pass was re-derived from updated parameters by a '
                          'later evaluation (backward must run before the next use of the function)' % what)


def _param_grads(by_param, params, need):
  """The gradient of every entry of `params` whose flag in `need` is set (None otherwise), cloned out of the sweep's gradient vector."""
  gparams = []
  for p, wanted in zip(params, need):
    g = by_param.get(id(p)) if wanted else None
    gparams.append(None if g is None else g.clone(memory_format=torch.contiguous_format))
  return tuple(gparams)


class _RecordedDopri5(torch.autograd.Function):
  """Forward: the device-controlled dopri5 solve (one hipGraph per trial step) that leaves the stage inputs of every ACCEPTED step
  on a tape.  Backward: what autograd does through torchdiffeq's accepted steps (step sizes constants: misc.py _optimal_step_size
  is decorated with torch.no_grad), as one native reverse sweep -- one fused row-kernel launch per evaluation, no PyTorch op and no
  host synchronisation inside (oracle/tape_reverse.py states the algebra; tests/test_tape_gpu.py)."""

  @staticmethod
  def forward(ctx, y0, edge_values, alpha_train, beta_train, func, t0, t1, rtol, atol):
    ent, graph, desc, sol, out = _recorded_dopri5_forward(func, y0, t0, t1, rtol, atol, ('y',))
    gt = graph.transposed_positions()[0]
    w_t = _weights_t(func, graph)
    ctx.func, ctx.sol, ctx.gen, ctx.gt, ctx.e = func, sol, sol.tape_generation, gt, graph.e
    ctx.x0 = ent['x0']
    ctx.x0_version = None if ent['x0'] is None else ent['x0']._version
    ctx.heads = edge_values.shape[1] if edge_values.dim() == 2 else 0
    ctx.save_for_backward(w_t, alpha_train, beta_train)
    func._last_train_solve = 'native recorded-tape dopri5'
    _tape_claim(func, '_tape_live_dopri5', ctx)
    return out

  @staticmethod
  def backward(ctx, grad_out):
    w_t, alpha_train, beta_train = ctx.saved_tensors
    sol, gt, E = ctx.sol, ctx.gt, ctx.e
    ctx.gnpde_consumed = True
    _check_tape(sol, ctx.gen, 'recorded dopri5', 'opt["gnpde_host_dopri5_training"] = True keeps a tape per forward')
    need = ctx.needs_input_grad
    with torch.no_grad():
      g1 = grad_out[1].contiguous()
      gy0, r_t, sum_g, dot = sol.tape_backward(gt, w_t, g1)
      a = torch.sigmoid(alpha_train.detach().reshape(()))
      dy0 = gy0 + grad_out[0] if need[0] else None
      dw = None
      if need[1] and E > 0:
        dw_e = torch.empty(E, dtype=torch.float32, device=g1.device)
        dw_e[gt.perm_long] = a * r_t[:E]
        dw = (dw_e / ctx.heads).unsqueeze(1).expand(E, ctx.heads).contiguous() if ctx.heads else dw_e
      dalpha = (dot.reshape(()) * (1 - a)).reshape(alpha_train.shape) if need[2] else None
      dbeta = None
      if need[3] and ctx.x0 is not None:
        if ctx.x0._version != ctx.x0_version:
          raise _lib.GnpdeError('recorded dopri5: the source term of this forward pass was overwritten before its backward')
        dbeta = (sum_g * ctx.x0).sum().reshape(beta_train.shape)
    return dy0, dw, dalpha, dbeta, None, None, None, None, None


class _RecordedDopri5NL(torch.autograd.Function):
  """GRAND-nl / GAT.  Forward: the recorded device-controlled dopri5 solve of _RecordedDopri5 (stage inputs of the accepted steps only).
  Backward: the walk of csrc/tape_reverse.h -- per recorded evaluation the VJP stage of the native adjoint solve at the recorded stage
  input (projection, attention, row kernel, normaliser backward, d q / d k, projection term, parameter-gradient pass), its epilogue
  forming the next cotangent -- as a plain sequence of launches, no PyTorch op and no host synchronisation inside.  The parameters are
  inputs (as in _RecordedFixedGrid), so their gradients come back through autograd; the backward counts no evaluation, as the
  reference's does not."""

  @staticmethod
  def forward(ctx, y0, func, t0, t1, rtol, atol, *params):
    ent, graph, desc, sol, out = _recorded_dopri5_forward(func, y0, t0, t1, rtol, atol, ('y', 'a'))
    ctx.func, ctx.ent, ctx.sol, ctx.gen, ctx.desc, ctx.graph, ctx.params = func, ent, sol, sol.tape_generation, desc, graph, params
    ctx.x0_version = None if ent['x0'] is None else ent['x0']._version
    lay = getattr(func, 'multihead_att_layer', None)
    ctx.split_sig = lay.split_operands()[0] if getattr(lay, 'split_kernel', False) else None      # (the derived operands this solve ran with)
    func._last_train_solve = 'native recorded-tape dopri5 (VJP stage per recorded evaluation)'
    _tape_claim(func, '_tape_live_dopri5', ctx)
    return out

  @staticmethod
  def backward(ctx, grad_out):
    func, ent, sol, graph, desc = ctx.func, ctx.ent, ctx.sol, ctx.graph, ctx.desc
    ctx.gnpde_consumed = True
    _check_tape(sol, ctx.gen, 'recorded dopri5', 'opt["gnpde_host_dopri5_training"] = True keeps a tape per forward')
    if ent['x0'] is not None and ent['x0']._version != ctx.x0_version:
      raise _lib.GnpdeError('recorded dopri5: the source term of this forward pass was overwritten before its backward')
    need = ctx.needs_input_grad
    with torch.no_grad():
      n, d = grad_out.shape[1], grad_out.shape[2]
      dev = grad_out.device
      _check_split_operands(func, ctx.split_sig, 'recorded dopri5')
      _vjp_sweep(func, ent, 'sweep', (ent['sig'],), desc, graph, 'dopri5_tape', (), dev, forward_values=True)
      ent['sweep'].set_dopri5_tape(sol, graph.csr_positions())      # (the accepted steps differ from one iteration to the next)
      ab = ent['a']
      ab.copy_(grad_out[1])
      ent['sweep'].run(ent['y'], ab, ent['grads'], use_graph=False)      # (y is not read: the state comes from the tape)
      dy0 = ab + grad_out[0] if need[0] else None
      gparams = _param_grads(_grad_vector_by_param(func, ent['grads'], d, ent['extra']), ctx.params, need[6:])
    return (dy0, None, None, None, None, None) + gparams


def _solve_dopri5_recorded(func, y0, t, rtol, atol):
  t0_, t1_ = end_points(t)
  nfe0 = func.nfe
  try:
    if func.__class__.__name__ != 'LaplacianODEFunc':
      params = tuple(p for p in func.parameters() if p.requires_grad)
      return _RecordedDopri5NL.apply(y0, func, t0_, t1_, float(rtol), float(atol), *params)
    return _RecordedDopri5.apply(y0, func._edge_values(), func.alpha_train, func.beta_train, func, t0_, t1_, float(rtol),
                                 float(atol))
  except _TapeTooLong as exc:
    func.nfe = nfe0
    func._last_train_solve = 'differentiable host loop (%s)' % exc
    return _solve_dopri5(func, y0, t, rtol, atol)


# --------------------------------------------------------------------------------------------------
# recorded fixed-grid solve: training WITHOUT the adjoint method through euler / midpoint / rk4 -- `python run_GNN.py --function
# transformer --block constant --method rk4` (reference run_GNN.py:336 `--adjoint` is store_true, base_classes.py:44-47 then picks
# torchdiffeq.odeint and loss.backward() runs through its Python loop, run_GNN.py:62-96)
# --------------------------------------------------------------------------------------------------
def _transformer_stage_native(func):
  """GRAND-nl per-evaluation attention the native VJP stage of csrc/adjoint.hip covers: scaled-dot scores, and (round 6) cosine_sim /
  pearson -- the scaled dot product of unit (mean-centred) head vectors, d_k in {4, 8, 16} -- and exp_kernel, with any normaliser.
  Scaled-dot scores take any d_k with attention_dim % 4 == 0 (16-byte q||k rows for the stage kernels) and <= 256 (d q / d k by the
  generic head-SpMM); the other scores keep d_k % 4 == 0 with attention_dim / 4 a power of two.  The BLEND split kernel (beltrami +
  exp_kernel) is ONE exp kernel over the derived projection of SpGraphTransAttentionLayer._split_qk_weights: the exp-kernel rule
  applies to its width kernel_att_dim = 2 attention_dim and its heads of 2 d_k (gnpde_split_kernel_grads maps the gradients of the
  derived operands back to the layer's parameters, _grad_vector_by_param)."""
  lay, opt = func.multihead_att_layer, func.opt
  if opt['mix_features']:
    return False
  if getattr(lay, 'split_kernel', False):
    A, dk = lay.kernel_att_dim, 2 * lay.d_k
  else:
    A, dk = lay.attention_dim, lay.d_k
  a4 = A // 4
  if opt['attention_type'] == 'scaled_dot':
    return A % lay.h == 0 and A % 4 == 0 and A <= 256
  if not (dk % 4 == 0 and A % 4 == 0 and a4 <= 64 and (a4 & (a4 - 1)) == 0):
    return False
  if opt['attention_type'] == 'exp_kernel':       # (exp_node_bwd_kernel walks the 2A <= 512 columns of a q||k row)
    return A <= 256 and lay.h <= 8
  return opt['attention_type'] in ('cosine_sim', 'pearson') and lay.d_k in (4, 8, 16)


def _gat_stage_native(func):
  """The GAT function (reference src/function_GAT_attention.py) on the native VJP stage: 2..8 heads, attention_dim a multiple of 4."""
  lay, opt = func.multihead_att_layer, func.opt
  return (not opt['mix_features']) and 2 <= lay.h <= 8 and lay.attention_dim % 4 == 0 and lay.attention_dim <= 256


def _stage_projection_t(func, ex, dev, forward_values=False):
  """[d, m] projection weights of the per-evaluation attention, transposed for P = d(q||k) W, in a buffer with a persistent address.
  forward_values (the reverse sweep of a recorded solve): the BLEND split kernel's derived projection is taken as the forward pass left
  it, not re-derived from parameters an optimiser may have stepped since."""
  lay = func.multihead_att_layer
  if func.__class__.__name__ == 'ODEFuncAtt':
    src = lay.W.detach()                    # [d, A] as the reference stores it
  elif forward_values and getattr(lay, 'split_kernel', False):
    src = lay.split_operands()[1].t()
  else:
    wqk, _ = lay.qk_weights()
    src = wqk.t()
  if ex.get('proj_wt') is None or ex['proj_wt'].shape != tuple(src.shape):
    ex['proj_wt'] = torch.empty(tuple(src.shape), dtype=torch.float32, device=dev)
  ex['proj_wt'].copy_(src)                 # refreshed in place: the captured graph keeps the pointer
  return ex['proj_wt']


def _nl_stage(func):
  """Whether the VJP stage recomputes the attention at every evaluation (GRAND-nl, GAT) instead of reading constant weights (GRAND-l)."""
  return func.__class__.__name__ in ('ODEFuncTransformerAtt', 'ODEFuncAtt')


def _vjp_sweep(func, ent, name, sig, desc, graph, method, dts, dev, forward_values=False):
  """The VJP-stage sweep (ops.AdjointSolver) of the entry -- ent['solver'] of the fixed-grid adjoint, ent['sweep'] of a recorded solve --
  over the transposed graph, with its operand refreshed in a buffer of ent['extra'] whose address persists (captured graphs keep the
  pointer): the transposed projection of GRAND-nl / GAT (_stage_projection_t), or the Laplacian weights in the transposed graph's entry
  order.  A miss of the caller's signature `sig` rebuilds the sweep and the gradient vector ent['grads'].
  Returns (the sweep, whether it was just built)."""
  from . import ops
  gt, t_from_csr = graph.transposed_positions()
  nl = _nl_stage(func)
  ex = ent['extra']
  proj_wt = w_t = None
  if nl:
    proj_wt = _stage_projection_t(func, ex, dev, forward_values=forward_values)
  else:
    if ex.get('w_t') is None or ex['w_t'].numel() != max(graph.e, 1):
      ex['w_t'] = torch.empty(max(graph.e, 1), dtype=torch.float32, device=dev)
    w_t = _weights_t(func, graph, out=ex['w_t'])
  built = []

  def build():
    sweep = ops.AdjointSolver(desc, gt, t_from_csr if nl else None, proj_wt, w_t, method, dts, dev)
    ent['grads'] = torch.zeros(sweep.n_grad, dtype=torch.float32, device=dev)
    built.append(True)
    return sweep
  return _solver_for(ent, sig + (id(gt),), build, name), bool(built)


def _split_kernel_grads(func, g, d, ex):
  """{id(parameter): gradient} of the BLEND split kernel's twelve parameters from the gradients of the derived operands
  (gnpde_split_kernel_grads: one launch into a persistent buffer, no host synchronisation)."""
  from . import ops
  lay, opt = func.multihead_att_layer, func.opt
  A, h, dk = lay.attention_dim, lay.h, lay.d_k
  f0, p0 = int(opt['feat_hidden_dim']), int(opt['pos_enc_hidden_dim'])
  _, wcat, bcat, scal = lay.split_operands()
  L = _lib.lib()
  nf = int(L.gnpde_split_kernel_grad_floats(h, dk, d))
  out = ex.get('split_grads')
  if out is None or out.numel() != nf or out.device != g.device:
    out = ex['split_grads'] = torch.zeros(nf, dtype=torch.float32, device=g.device)
  _lib.require_hip(g, wcat, bcat, scal, out)
  _lib.check(L.gnpde_split_kernel_grads(_lib.ptr(g), _lib.ptr(wcat), _lib.ptr(bcat), _lib.ptr(scal[0:1]), _lib.ptr(scal[1:2]), _lib.ptr(scal[2:3]),
                                        _lib.ptr(scal[3:4]), h, dk, d, f0, p0, _lib.ptr(out), _lib.stream_of(g)))
  by_param, pos = {}, 0
  for lin, w in ((lay.Qx, d - p0), (lay.Kx, d - p0), (lay.Qp, p0), (lay.Kp, p0)):
    by_param[id(lin.weight)] = out[pos:pos + A * w].view(A, w)
    by_param[id(lin.bias)] = out[pos + A * w:pos + A * w + A]
    pos += A * (w + 1)
  for i, p in enumerate((lay.lengthscale_x, lay.lengthscale_p, lay.output_var_x, lay.output_var_p)):
    by_param[id(p)] = out[pos + i].reshape(p.shape)
  return by_param


def _grad_vector_by_param(func, g, d, ex=None):
  """{id(parameter): its slice of the native gradient vector} (gnpde_adjoint_run: d[Wq;Wk], d[bq;bk], d alpha_train, d beta_train).
  BLEND split kernel: the vector holds the gradients of the DERIVED operands (Wcat [4A, d], bcat [4A], output_var, lengthscale = 1);
  the twelve parameters get theirs through gnpde_split_kernel_grads into a buffer kept in `ex`."""
  by_param = {}
  tail = 0
  if func.__class__.__name__ == 'ODEFuncTransformerAtt':
    lay = func.multihead_att_layer
    A = lay.kernel_att_dim
    tail = 2 * A * d + 2 * A
    if getattr(lay, 'split_kernel', False):
      by_param = _split_kernel_grads(func, g, d, ex if ex is not None else func.__dict__.setdefault('_split_grad_state', {}))
      tail += 2
    else:
      gram = g[:2 * A * d].view(2 * A, d)
      gb = g[2 * A * d:2 * A * d + 2 * A]
      by_param = {id(lay.Q.weight): gram[:A], id(lay.K.weight): gram[A:], id(lay.Q.bias): gb[:A], id(lay.K.bias): gb[A:]}
      if func.opt['attention_type'] == 'exp_kernel':      # two more slots: d output_var, d lengthscale
        by_param[id(lay.output_var)] = g[tail].reshape(lay.output_var.shape)
        by_param[id(lay.lengthscale)] = g[tail + 1].reshape(lay.lengthscale.shape)
        tail += 2
  elif func.__class__.__name__ == 'ODEFuncAtt':      # d W^T [A, d], then d a in the first 2 d_k of the A slots behind it
    lay = func.multihead_att_layer
    A = lay.attention_dim
    by_param = {id(lay.W): g[:A * d].view(A, d).t(), id(lay.a): g[A * d:A * d + 2 * lay.d_k].reshape(lay.a.shape)}
    tail = A * d + A
  by_param[id(func.alpha_train)] = g[tail].reshape(func.alpha_train.shape)
  if func.opt['add_source']:
    by_param[id(func.beta_train)] = g[tail + 1].reshape(func.beta_train.shape)
  return by_param


class _RecordedFixedGrid(torch.autograd.Function):
  """Forward: the native fixed-grid solver with a tape (no extra pass: the stage epilogues write their outputs into the tape's slots).
  Backward: the reverse sweep through the recorded evaluations -- per evaluation the VJP stage of the native adjoint solve (projection,
  attention, row kernel with the edge products, normaliser backward, d q / d k, aggregation on the transposed graph whose epilogue forms
  the next cotangent, parameter-gradient pass), all steps in one hipGraph, no PyTorch op and no host synchronisation inside."""

  @staticmethod
  def forward(ctx, y0, edge_values, func, method, dts, *params):
    from . import ops
    n_evals = len(dts) * _EVALS_PER_STEP[method]
    func._charge_fixed_nfe(n_evals)
    y0c = _lib.f32c(y0.detach())
    n, d = y0c.shape
    view = func._locality_view(y0c) if hasattr(func, '_locality_view') else None
    ent = _entry(func, '_fixed_tape_state', (method, tuple(dts), n, d, str(y0c.device), id(view)), n, d, y0c.device, ('y', 'a'), view=view)
    _rows_in(view, y0c, ent['y'])
    if ent['x0'] is not None:
      _copy_source(func, ent['x0'], view)
    graph = func._graph(y0c) if view is None else view.graph
    desc = func._descriptor(ent['y'], x0_override=ent['x0'], graph=graph)      # (refreshes the CSR-ordered weights in place)

    def build():
      sol = ops.FixedStepSolver(desc, method, dts, y0c.device)
      sol.set_tape(True)
      return sol
    sol = _solver_for(ent, func._descriptor_signature(desc), build)
    sol.run(ent['y'])
    func.nfe += n_evals
    sol.tape_generation += 1
    out = torch.empty((2, n, d), dtype=torch.float32, device=y0c.device)
    out[0].copy_(y0c)
    _rows_out(view, ent['y'], out[1])
    ctx.func, ctx.ent, ctx.gen, ctx.desc, ctx.graph, ctx.view = func, ent, sol.tape_generation, desc, graph, view
    lay = getattr(func, 'multihead_att_layer', None)
    ctx.split_sig = lay.split_operands()[0] if getattr(lay, 'split_kernel', False) else None      # (the derived operands this solve ran with)
    ctx.method, ctx.dts, ctx.params = method, dts, params
    ctx.heads = 0 if edge_values is None else (edge_values.shape[1] if edge_values.dim() == 2 else 0)
    ctx.has_edge_values = edge_values is not None
    func._last_train_solve = 'native recorded fixed-grid %s' % method
    _tape_claim(func, '_tape_live_fixed', ctx)
    return out

  @staticmethod
  def backward(ctx, grad_out):
    func, ent, graph, view, desc = ctx.func, ctx.ent, ctx.graph, ctx.view, ctx.desc
    ctx.gnpde_consumed = True
    sol = ent['solver']
    _check_tape(sol, ctx.gen, 'recorded fixed-grid solve', 'opt["gnpde_host_fixed_training"] = True keeps a graph per forward')
    need = ctx.needs_input_grad
    nl = _nl_stage(func)
    with torch.no_grad():
      n, d = grad_out.shape[1], grad_out.shape[2]
      dev = grad_out.device
      ex = ent['extra']
      _check_split_operands(func, ctx.split_sig, 'recorded fixed-grid solve')
      want_dw = (not nl) and ctx.has_edge_values and need[1] and graph.e > 0
      if not nl and (ex.get('r_acc') is None or ex['r_acc'].numel() != max(graph.e, 1)):
        ex['r_acc'] = torch.zeros(max(graph.e, 1), dtype=torch.float32, device=dev)
      sweep, built = _vjp_sweep(func, ent, 'sweep', (ent['sig'], bool(want_dw), id(sol)), desc, graph, ctx.method, ctx.dts, dev, forward_values=True)
      if built:
        sweep.set_tape(sol.tape, ex['r_acc'] if want_dw else None, graph.csr_positions() if nl else None)
      ab = ent['a']
      g1 = grad_out[1]
      _rows_in(view, g1 if view is None else g1.contiguous(), ab)
      sweep.run(ent['y'], ab, ent['grads'])      # (y is not read in the taped mode: the state comes from the tape)
      dy0 = None
      if need[0]:
        dy0 = _rows_out(view, ab, torch.empty((n, d), dtype=torch.float32, device=dev))
        dy0 += grad_out[0]
      dw = None
      if want_dw:
        a = func.alpha_train.detach().reshape(())
        if not func.opt['no_alpha_sigmoid']:
          a = torch.sigmoid(a)
        E = graph.e
        dw_e = torch.empty(E, dtype=torch.float32, device=dev)
        order = (graph.transposed_positions()[0] if sweep.swapped else graph).perm_long      # (the products lie in the order of the graph the row kernel ran on)
        dw_e[order] = a * ex['r_acc'][:E]
        dw = (dw_e / ctx.heads).unsqueeze(1).expand(E, ctx.heads).contiguous() if ctx.heads else dw_e
      gparams = _param_grads(_grad_vector_by_param(func, ent['grads'], d, ex), ctx.params, need[5:])
    return (dy0, dw, None, None, None) + gparams


_FIXED_TAPE_BUDGET_BYTES = 96 << 30     # a recorded fixed-grid solve that would need more than this (or more than 70 % of the free device memory) runs the host loop


def _fixed_tape_estimate(func, y0, n_evals):
  """Bytes of the record of a fixed-grid solve: n_evals + 1 stage inputs and, for GRAND-nl with scaled-dot scores, q||k and the weights
  of every evaluation (csrc/solver.hip gnpde_solver_tape_bytes; an upper estimate without building the descriptor)."""
  n, d = y0.shape
  ld = (d + 3) // 4 * 4
  total = (n_evals + 1) * n * ld * 4
  lay = getattr(func, 'multihead_att_layer', None)
  if func.__class__.__name__ == 'ODEFuncTransformerAtt' and lay is not None and func.edge_index is not None:
    total += n_evals * (n * 2 * lay.kernel_att_dim * 4 + int(func.edge_index.shape[1]) * 4)
  return total


def _solve_fixed_recorded(func, y0, t, method, step_size):
  dts = step_sizes(t, step_size)
  need = _fixed_tape_estimate(func, y0, len(dts) * _EVALS_PER_STEP[method])
  try:
    free = torch.cuda.mem_get_info(y0.device)[0]
  except Exception:   # noqa: BLE001
    free = _FIXED_TAPE_BUDGET_BYTES
  # (a tape of this method, grid and shape that already exists is not allocated again: the key of _RecordedFixedGrid.forward)
  cached = any(key[:4] == (method, tuple(dts), y0.shape[0], y0.shape[1]) for key in func.__dict__.get('_fixed_tape_state', ()))
  if not cached and need > min(_FIXED_TAPE_BUDGET_BYTES, 0.7 * free):
    func._last_train_solve = 'differentiable host loop (the record of %d evaluations would take %.1f GB)' % (len(dts) * _EVALS_PER_STEP[method], need / 1e9)
    return _solve_fixed_host(func, y0, t, method, step_size)
  params = tuple(p for p in func.parameters() if p.requires_grad)
  edge_values = None
  if func.__class__.__name__ == 'LaplacianODEFunc':
    ev = func._edge_values()
    edge_values = ev if ev.requires_grad else None
  return _RecordedFixedGrid.apply(y0, edge_values, func, method, dts, *params)


class _TupleFunc(object):
  """A function of a tuple state seen as a function of the flattened concatenation (torchdiffeq misc.py _TupleFunc):
  the regularised training state (x, r_1, ..., r_k) of reference src/block_constant.py:40-43."""

  def __init__(self, func, shapes):
    self.func, self.shapes = func, shapes

  def __call__(self, t, flat):
    out = self.func(t, tuple(_unflatten(flat, self.shapes)))
    return _flatten(out)

  def parameters(self):
    return self.func.parameters() if isinstance(self.func, torch.nn.Module) else iter(())


def _solve_tuple(solver, func, y0, t, kw):
  shapes = [p.shape for p in y0]
  if kw.get('method') in (None, 'dopri5', 'adaptive_heun'):     # torchdiffeq's default norm of a tuple state
    kw = dict(kw, options=dict(kw.get('options') or {}))
    kw['options'].setdefault('norm', _mixed_norm(shapes))
  flat = solver(_TupleFunc(func, shapes), _flatten(y0), t, **kw)          # [len(t), total]
  outs, pos = [], 0
  for sh in shapes:
    cnt = int(torch.Size(sh).numel())
    outs.append(flat[:, pos:pos + cnt].reshape((flat.shape[0],) + tuple(sh)))
    pos += cnt
  return tuple(outs)


def odeint(func, y0, t, *, rtol=1e-7, atol=1e-9, method=None, options=None, use_graph=True, **adjoint_kwargs):
  """Drop-in for torchdiffeq.odeint on this path.  Unknown options (e.g. `max_iters`, which the
  reference passes and torchdiffeq ignores with a warning) are ignored."""
  if isinstance(y0, tuple):
    return _solve_tuple(odeint, func, y0, t, dict(rtol=rtol, atol=atol, method=method, options=options, use_graph=use_graph))
  options = dict(options or {})
  method = 'dopri5' if method is None else method
  gather_dtype_requested(func)      # (a bad value raises whatever path the solve takes)
  _note_gather(func, 'fp32')        # only the native fixed-step solve below runs anything else
  route, reason = routes.forward(func, y0, t, method, options)
  if len(t) > 2:
    _note_output_solve(func, route, reason)
  if reason is routes.TAPE_BUSY:
    func._last_train_solve = 'differentiable host loop (%s)' % reason
  step_size = options.get('step_size')
  if route == 'native_fixed':
    return _solve_native(func, y0, t, method, step_size, use_graph=use_graph)
  if route == 'device_controller':
    return _solve_dopri5_device(func, y0, t, rtol, atol, trials_per_sync=options.get('trials_per_sync'), pair=method)
  if route == 'recorded_fixed':
    return _solve_fixed_recorded(func, y0, t, method, step_size)
  if route == 'recorded_dopri5':
    return _solve_dopri5_recorded(func, y0, t, rtol, atol)
  if route == 'host_fixed':
    return _solve_fixed_host(func, y0, t, method, step_size)
  if route == 'host_loop':
    return _solve_dopri5(func, y0, t, rtol, atol, tableau=method, norm=options.get('norm'))
  if route == 'host_stages':
    return _solve_dopri5_native(func, y0, t, rtol, atol)
  from . import distributed as D      # 'sharded': one process per GPU, rows partitioned over the ranks
  if method in routes.FIXED:
    return D.solve_sharded(func, y0, t, method, step_size, use_graph=use_graph)
  return D.solve_sharded(func, y0, t, method, None, rtol=rtol, atol=atol)


# --------------------------------------------------------------------------------------------------
# adjoint sensitivity (torchdiffeq 0.2.1 adjoint.py, as selected by opt['adjoint'], reference
# src/base_classes.py:44-47, src/block_constant.py:45-55)
# --------------------------------------------------------------------------------------------------
def _flatten(parts):
  return torch.cat([p.reshape(-1) for p in parts])


def _unflatten(v, shapes):
  out, pos = [], 0
  for sh in shapes:
    cnt = int(torch.Size(sh).numel())
    out.append(v[pos:pos + cnt].view(sh))
    pos += cnt
  return out


def _adjoint_fixed_grid(func, params, y, a, gparams, span, method, step_size):
  """euler / rk4 (3/8 rule) on the augmented system over the reversed-time grid s = -t (torchdiffeq's grid: the
  short step lands next to the earlier time), written on the separate components (y, a, g_theta) with fused
  axpy updates instead of one flat vector: per stage one evaluation F = f(u_y) and one vector-Jacobian product
  (V_y, V_theta) = u_a^T df/d(y, theta); in s the derivatives are  y' = -F,  a' = +V_y,  g' = +V_theta.
  Same stage formulas as rk_common.rk4_alt_step_func; agrees with the flat-vector path to rounding (the products
  dt * k / 3 are formed as k * (dt / 3))."""
  grid = time_grid(span, step_size)
  dts = (grid[1:] - grid[:-1]).tolist()
  y, a = y.clone(), a.clone()
  gparams = [g.clone() for g in gparams]

  def stage(uy, ua, s_now):
    with torch.enable_grad():
      yy = uy.detach().requires_grad_(True)
      F = func(-s_now, yy)
      grads = torch.autograd.grad(F, (yy,) + tuple(params), ua, allow_unused=True)
    V = grads[0] if grads[0] is not None else torch.zeros_like(uy)
    return F.detach(), V, grads[1:]

  def comb(base, terms, inplace=False):
    """base + sum_j c_j v_j: one fused pass on the device (gnpde_lincomb), chained axpys elsewhere."""
    if base.is_cuda and base.dtype == torch.float32 and base.is_contiguous() and all(
        v.is_contiguous() and v.dtype == torch.float32 for v, _ in terms):
      from . import ops
      return ops.lincomb(base, terms, out=base if inplace else None)
    out = base if inplace else None
    for v, c in terms:
      out = torch.add(base, v, alpha=c) if out is None else out.add_(v, alpha=c)
    return out

  def acc_params(vps, coef):
    for g, v in zip(gparams, vps):
      if v is not None:
        g.add_(v, alpha=coef)

  for step, dt in enumerate(dts):
    s0, s1 = grid[step], grid[step + 1]
    if method == 'euler':
      F1, V1, P1 = stage(y, a, s0)
      y = comb(y, [(F1, -dt)], inplace=True)
      a = comb(a, [(V1, dt)], inplace=True)
      acc_params(P1, dt)
      continue
    third, eighth = dt / 3.0, dt * 0.125
    F1, V1, P1 = stage(y, a, s0)
    F2, V2, P2 = stage(comb(y, [(F1, -third)]), comb(a, [(V1, third)]), s0 + third)
    F3, V3, P3 = stage(comb(y, [(F2, -dt), (F1, third)]), comb(a, [(V2, dt), (V1, -third)]), s0 + 2 * third)
    F4, V4, P4 = stage(comb(y, [(F1, -dt), (F2, dt), (F3, -dt)]), comb(a, [(V1, dt), (V2, -dt), (V3, dt)]), s1)
    y = comb(y, [(F1, -eighth), (F2, -3 * eighth), (F3, -3 * eighth), (F4, -eighth)], inplace=True)
    a = comb(a, [(V1, eighth), (V2, 3 * eighth), (V3, 3 * eighth), (V4, eighth)], inplace=True)
    for P, c in ((P1, eighth), (P2, 3 * eighth), (P3, 3 * eighth), (P4, eighth)):
      acc_params(P, c)
  return a, gparams


def _adjoint_native(func, params, y, a, span, method, step_size):
  """(a at the earlier time, [gradient contribution per entry of `params`]) of one backward interval, by the native solver."""
  grid = time_grid(span.detach().to('cpu'), step_size)
  dts = (grid[1:] - grid[:-1]).tolist()
  n_evals = len(dts) * (4 if method == 'rk4' else 1)
  func._charge_fixed_nfe(n_evals)
  view = func._locality_view(y, forward_solve=False) if hasattr(func, '_locality_view') else None
  key = (method, tuple(dts), tuple(y.shape), str(y.device), id(view))
  ent = _entry(func, '_adjoint_state', key, y.shape[0], y.shape[1], y.device, ('y', 'a'), view=view)
  yb, ab = ent['y'], ent['a']
  _rows_in(view, y.detach(), yb)
  _rows_in(view, a.detach(), ab)
  if ent['x0'] is not None:
    _copy_source(func, ent['x0'], view)
  graph = func._graph(y) if view is None else view.graph
  desc = func._descriptor(yb, x0_override=ent['x0'], graph=graph)
  sol = _vjp_sweep(func, ent, 'solver', (func._descriptor_signature(desc),), desc, graph, method, dts, y.device)[0]
  sol.run(yb, ab, ent['grads'])
  func.nfe += n_evals
  a_out = _rows_out(view, ab, torch.empty_like(a, memory_format=torch.contiguous_format))
  by_param = _grad_vector_by_param(func, ent['grads'], y.shape[1], ent['extra'])
  return a_out, [by_param.get(id(p)) for p in params]


def _adjoint_adaptive_native(func, params, y, a, gparams, span, method, rtol, atol, device_controller=False):
  """One backward interval of torchdiffeq's adjoint with an ADAPTIVE adjoint method, for f(u) = alpha' (A u - u) + beta x0: the augmented
  system (vjp_t, y, a, g_theta) in reversed time s = -t is

      y' = -f(y),   a' = alpha' (A^T a - a),   g_alpha' = (1 - alpha') <a, f(y) - beta x0>,   g_beta' = <a, x0>,   everything else 0,

  integrated by the embedded pair with torchdiffeq 0.2.1's controller (mixed norm = the largest component rms, the scalars being
  components of their own) exactly as `_solve_dopri5` does on the flat vector -- but by _solve_pair_host on the components: a
  y-component of sign -1 on the graph, an a-component of sign +1 on the transposed graph, the scalar pair (two dot products per
  stage), no autograd graph; per trial step two error-norm launches and one host read.  The initial step always runs there; the rest
  of the interval runs on the device controller where the route rule says so (`device_controller`: routes.adjoint names the two).  Buffers
  and the device solver: slot _adjoint_adaptive.
  Returns (a at the earlier time, new accumulated gradients of alpha_train / beta_train as a dict by parameter id)."""
  import types
  from . import ops
  stages = len(_TABLEAUS[method]['alpha'])
  dev = y.device
  n, d = y.shape
  graph = func._graph(y)
  gt = graph.transposed_positions()[0]
  ynames, anames = _component_bufs('y', stages), _component_bufs('a', stages)
  ent = _host_pair_entry(func, '_adjoint_adaptive', (n, d, str(dev), method), n, d, dev, ynames + anames)
  ex = ent['extra']
  Y, A_, X0 = ent['y'], ent['a'], ent['x0']
  Y.copy_(y.detach())
  A_.copy_(a.detach())
  has_src = X0 is not None
  if has_src:
    _copy_source(func, X0)
  desc_f = func._descriptor(Y, x0_override=X0, graph=graph)
  w_t = _weights_t(func, graph)
  alpha_d = ops._scalar_dev(func.alpha_train, Y)
  desc_b = ops.RhsDescriptor(_lib.RHS_LAPLACIAN, gt, d, Y.stride(0), alpha_d, None, None, True, w_csr=w_t, padded_rows=_lib.is_padded(Y))
  one_minus_a = 1 - torch.sigmoid(func.alpha_train.detach().reshape(()))
  beta = func.beta_train.detach().reshape(()) if has_src else None
  ids = [id(p) for p in params]
  ia = ids.index(id(func.alpha_train)) if id(func.alpha_train) in ids else None
  ib = ids.index(id(func.beta_train)) if (has_src and id(func.beta_train) in ids) else None
  g = torch.zeros(2, dtype=torch.float32, device=dev)          # (g_alpha, g_beta) accumulated so far: they scale the tolerance of their components
  if ia is not None:
    g[0] = gparams[ia].reshape(())
  if ib is not None:
    g[1] = gparams[ib].reshape(())
  rt, at = float(rtol), float(atol)
  scratch = (ex['ratio_dev'], ex['err_ws'])
  # (the descriptor of f reads y-independent operands only: alpha, beta, x0, the weights -- its `ld` is every buffer's)
  cy = _StageComponent(desc_f, -1, [ent[nm] for nm in ynames], rt, at, scratch)       # y' = -f(y)
  ca = _StageComponent(desc_b, 1, [ent[nm] for nm in anames], rt, at, scratch)        # a' = alpha' (A^T a - a)

  def dot(u, v):
    return (u * v).sum()

  def scal_stage(j, src):
    """(g_alpha', g_beta') at the stage inputs src = (uy, ua), after K_j of y"""
    dx0 = dot(src[1], X0) if has_src else torch.zeros((), device=dev)
    dF = dot(src[1], cy.K[j])
    ka = one_minus_a * (dF - beta * dx0) if has_src else one_minus_a * dF
    return torch.stack([ka, dx0])

  def scal_ratio(v, g0, g1):
    tol = at + rt * torch.max(g0.abs(), g1.abs())
    r = (v / tol).abs()
    if ia is None:
      r = r * torch.tensor([0.0, 1.0], device=dev)
    if ib is None:
      r = r * torch.tensor([1.0, 0.0], device=dev)
    return r.max().reshape(1)

  sc = types.SimpleNamespace(g=g, g1=None, K=[None] * (stages + 1), stage=scal_stage, ratio=scal_ratio)
  T0, T1 = float(span[0]), float(span[-1])
  if device_controller and Y.stride(0) % 4 == 0:      # (route 'adjoint_device'; the 16-byte rows are this runner's own allocation)
    # the initial step on the host, the rest of the interval with the controller on the device (csrc/adjoint_adaptive.hip: one
    # hipGraph replay per trial step of the embedded pair; the host reads a record once per batch)
    from .utils import MaxNFEException
    dt = _solve_pair_host(method, [cy, ca], T0, T1, func._check_nfe, scalars=sc, initial_step_only=True)[0]
    if ex.get('w_t') is None or ex['w_t'].numel() != max(graph.e, 1):
      ex['w_t'] = torch.empty(max(graph.e, 1), dtype=torch.float32, device=dev)
    if graph.e > 0:
      ex['w_t'][:graph.e].copy_(w_t)          # persistent address: the captured trial steps keep the pointer
    sol = _solver_for(ent, (func._descriptor_signature(desc_f), id(gt), rt, at),
                      lambda: ops.AdjointAdaptiveSolver(desc_f, gt, ex['w_t'], method, rt, at, dev))
    room = func._nfe_room()
    if room <= 0:
      raise MaxNFEException
    finished = sol.run(Y, A_, g, T0, T1, dt, trials_per_sync=default_trials_per_sync(Y.numel()), max_evals=room)
    spent = sol.stats()['evals']
    func._adjoint_adaptive_stats = sol.stats()
    func._settle_adaptive_nfe(room, finished, spent)
    new = {ia: g[0].reshape(gparams[ia].shape)}
    if ib is not None:
      new[ib] = g[1].reshape(gparams[ib].shape)
    return A_[:, :d].clone(memory_format=torch.contiguous_format), new
  end = {'a': None, 'g': g}

  def interp(x, h, c_mid):
    """torchdiffeq's quartic interpolation at the end time (only a and the scalars are returned)"""
    def quartic(v0, v1, k0, k1, mid):
      ca_ = 2 * h * (k1 - k0) - 8 * (v1 + v0) + 16 * mid
      cb = h * (5 * k0 - 3 * k1) + 18 * v0 + 14 * v1 - 32 * mid
      cc = h * (k1 - 4 * k0) - 11 * v0 - 5 * v1 + 16 * mid
      cd = h * k0
      return v0 + x * cd + x ** 2 * cc + x ** 3 * cb + x ** 4 * ca_
    a_mid = ca.axpys(c_mid, torch.empty_like(ca.y))
    end['a'] = quartic(ca.y, ca.y1, ca.K[0], ca.K[stages], a_mid)[:, :d].contiguous()
    g_mid = sc.g + sum(sc.K[j] * c_mid[j] for j in range(stages + 1) if c_mid[j] != 0.0)
    end['g'] = quartic(sc.g, sc.g1, sc.K[0], sc.K[stages], g_mid)
  _solve_pair_host(method, [cy, ca], T0, T1, func._check_nfe, scalars=sc, interp=interp)
  new = {}
  if ia is not None:
    new[ia] = end['g'][0].reshape(gparams[ia].shape)
  if ib is not None:
    new[ib] = end['g'][1].reshape(gparams[ib].shape)
  return end['a'], new


class _AdjointSolve(torch.autograd.Function):
  """Forward: the plain solve WITHOUT a tape -- on this package's functions that is the native hipGraph solver, so
  the training forward runs at inference speed and stores two states, not the trajectory.  Backward: the augmented
  system (vjp_t, y, a, g_theta) with  dy/dt = f,  da/dt = -a^T df/dy,  dg/dt = -a^T df/dtheta  is integrated from
  t[i] back to t[i-1] with the ADJOINT method / step size / tolerances; like torchdiffeq, the time reversal is the
  substitution s = -t (so a fixed grid puts its short step next to t[i-1]), the tuple is integrated as one flat
  vector (mixed linf-rms norm for adaptive methods), y is reset to the stored forward value and the incoming
  gradient is added at every output time.  f and its vector-Jacobian products run through the native kernels."""

  @staticmethod
  def forward(ctx, func, y0, t, fwd, adj, *params):
    ctx.func, ctx.adj = func, adj
    with _fp32_gather():      # the forward of an adjoint solve is part of training: it keeps the fp32 gather operand
      ans = odeint(func, y0.detach(), t, **fwd)
    ctx.save_for_backward(t, ans, *params)
    return ans

  @staticmethod
  def backward(ctx, grad_out):
    func, adj = ctx.func, ctx.adj
    t, ans, *params = ctx.saved_tensors
    params = tuple(params)
    with torch.no_grad():
      state = [torch.zeros((), dtype=ans.dtype, device=ans.device), ans[-1], grad_out[-1].contiguous()]
      state.extend(torch.zeros_like(p) for p in params)
      shapes = [s_.shape for s_ in state]

      def reversed_flat_dynamics(s, flat):
        """-(vjp_t, f, vjp_y, vjp_params) at time t = -s, vjp = grad(f, ., -a)  (adjoint.py augmented_dynamics
        under misc.py _ReverseFunc and _TupleFunc)."""
        parts = _unflatten(flat, shapes)
        with torch.enable_grad():
          # fresh allocations, not views into the flat vector: a view starts one float after the vjp_t slot, which
          # would push every kernel onto its unaligned (scalar-load) variant
          y = parts[1].detach().clone().requires_grad_(True)
          f_eval = func(-s, y)
          grads = torch.autograd.grad(f_eval, (y,) + params, -parts[2], allow_unused=True)
        outs = [torch.zeros_like(parts[0]), f_eval.detach()]
        outs.append(torch.zeros_like(y) if grads[0] is None else grads[0])
        for p, g in zip(params, grads[1:]):
          outs.append(torch.zeros_like(p) if g is None else g)
        return -_flatten(outs)

      options = dict(adj['options'])
      if adj['method'] in routes.ADAPTIVE and 'norm' not in options:
        options['norm'] = _mixed_norm(shapes)
      # (every interval starts from a slice of `ans`: one route for all of them)
      route = routes.adjoint(func, ans[-1], adj['method'], adj['options'], params)[0]
      for i in range(len(t) - 1, 0, -1):
        span = -t[i - 1:i + 1].flip(0)
        if route == 'adjoint_native':
          # the whole interval as one native object (one hipGraph; no PyTorch op between the stages)
          state[2], contrib = _adjoint_native(func, params, state[1], state[2], span, adj['method'], options['step_size'])
          state = state[:3] + [gp if c is None else gp + c.reshape(gp.shape) for gp, c in zip(state[3:], contrib)]
        elif route == 'adjoint_stagewise':
          state[2], gp = _adjoint_fixed_grid(func, params, state[1], state[2], state[3:], span, adj['method'],
                                             options['step_size'])
          state = state[:3] + list(gp)
        elif route in ('adjoint_device', 'adjoint_host_pair'):
          # adaptive adjoint method on the Laplacian function: native stages on the components (no autograd graph, no flat vector)
          state[2], new = _adjoint_adaptive_native(func, params, state[1], state[2], state[3:], span, adj['method'], adj['rtol'], adj['atol'],
                                                   device_controller=route == 'adjoint_device')
          for idx, val in new.items():
            state[3 + idx] = val
        else:
          flat = odeint(reversed_flat_dynamics, _flatten(state), span, rtol=adj['rtol'], atol=adj['atol'],
                        method=adj['method'], options=options)[1]
          state = [p.clone() for p in _unflatten(flat, shapes)]
        state[1] = ans[i - 1]
        state[2] = state[2] + grad_out[i - 1]
    return (None, state[2], None, None, None) + tuple(state[3:])


def odeint_adjoint(func, y0, t, *, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint_rtol=None, adjoint_atol=None,
                   adjoint_method=None, adjoint_options=None, adjoint_params=None, use_graph=True):
  """Drop-in for torchdiffeq.odeint_adjoint: same values as `odeint`; gradients with respect to y0 and the
  function's parameters come from solving the adjoint ODE backwards (see _AdjointSolve), not from a tape."""
  if isinstance(y0, tuple):
    if adjoint_params is None:
      adjoint_params = tuple(func.parameters()) if isinstance(func, torch.nn.Module) else ()
    return _solve_tuple(odeint_adjoint, func, y0, t,
                        dict(rtol=rtol, atol=atol, method=method, options=options, adjoint_rtol=adjoint_rtol,
                             adjoint_atol=adjoint_atol, adjoint_method=adjoint_method, adjoint_options=adjoint_options,
                             adjoint_params=tuple(adjoint_params), use_graph=use_graph))
  options = dict(options or {})
  fwd = dict(rtol=rtol, atol=atol, method=method, options=options, use_graph=use_graph)
  if adjoint_params is None:
    adjoint_params = tuple(func.parameters()) if isinstance(func, torch.nn.Module) else ()
  params = tuple(p for p in adjoint_params if p.requires_grad)
  if not torch.is_grad_enabled() or not (y0.requires_grad or params):
    return odeint(func, y0, t, **fwd)
  adj = dict(rtol=rtol if adjoint_rtol is None else adjoint_rtol, atol=atol if adjoint_atol is None else adjoint_atol,
             method=(method or 'dopri5') if adjoint_method is None else adjoint_method,
             options={k: v for k, v in options.items() if k != 'norm'} if adjoint_options is None else dict(adjoint_options))
  return _AdjointSolve.apply(func, y0, t, fwd, adj, *params)
