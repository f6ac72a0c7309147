"""The table behind tests/test_solve_routes_cpu.py: duck-typed stubs for state and function, the rows (what is asked of `odeint`, of the
early-stopping integrators and of `_AdjointSolve.backward`), and `observe`, which runs a row through the real entry point with every
runner replaced by a recorder.  No device.

The expected outcomes are tests/golden/solve_routes.json, recorded by running this file (`python tests/solve_routes_cases.py`) on the
commit BEFORE the route rule existed: the table pins what the ladders did, unintended-looking cases included."""
import importlib
import inspect
import itertools
import json
import os
import sys
import types
import weakref

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
import gnpde_amd  # noqa: E402,F401

O = importlib.import_module('gnpde_amd.odeint')
ES = importlib.import_module('gnpde_amd.early_stop_solver')
D = importlib.import_module('gnpde_amd.distributed')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'solve_routes.json')

# runner -> the arguments that select a variant of it
RUNNERS = {
  '_solve_native': ('method', 'use_graph', 'evaluator'),
  '_solve_fixed_host': ('method', 'on_step'),
  '_solve_fixed_recorded': ('method',),
  '_solve_dopri5': ('tableau', 'norm', 'stop_after', 'on_accept'),
  '_solve_dopri5_native': ('stop_after', 'on_accept'),
  '_solve_dopri5_device': ('pair', 'evaluator', 'stop_after', 'trials_per_sync'),
  '_solve_dopri5_recorded': (),
  'solve_sharded': ('method', 'step_size', 'use_graph', 'rtol'),
  '_adjoint_native': ('method',),
  '_adjoint_fixed_grid': ('method',),
  '_adjoint_adaptive_native': ('method',),
  'odeint': ('method', 'norm'),       # the flat augmented system of a backward interval
}
# runner -> the route name of the rule (the adaptive adjoint's two names share a runner: those rows say which)
ROUTE_OF = {'_solve_native': 'native_fixed', 'solve_sharded': 'sharded', '_solve_fixed_recorded': 'recorded_fixed',
            '_solve_fixed_host': 'host_fixed', '_solve_dopri5_device': 'device_controller', '_solve_dopri5_native': 'host_stages',
            '_solve_dopri5_recorded': 'recorded_dopri5', '_solve_dopri5': 'host_loop', '_adjoint_native': 'adjoint_native',
            '_adjoint_fixed_grid': 'adjoint_stagewise', 'odeint': 'adjoint_flat'}


class _DeviceState(torch.Tensor):
  """A host tensor that says it lives on a device: all the rule asks of a state is is_cuda, dim(), dtype, shape and requires_grad."""
  is_cuda = True


def state(device=True, width=4, dtype=torch.float32, grad=False, lead=()):
  y = torch.zeros(tuple(lead) + (3, width), dtype=dtype)
  if device:
    y = y.as_subclass(_DeviceState)
  return y.requires_grad_(grad)


def caller_norm(v):
  return v.abs().max()


class _Func(object):
  """What the route rule and the ladders ask of one of the package's function objects."""

  def __init__(self, opt, differentiated, native_rhs, layer):
    self.opt = dict(add_source=False, mix_features=False, attention_type='scaled_dot')
    self.opt.update(opt)
    self.differentiated, self.native_rhs = differentiated, native_rhs
    self.multihead_att_layer = types.SimpleNamespace(**dict(dict(h=2, d_k=4, attention_dim=8, kernel_att_dim=8, split_kernel=False), **layer))
    self.alpha_train, self.beta_train = torch.nn.Parameter(torch.zeros(())), torch.nn.Parameter(torch.zeros(()))
    self.weight = torch.nn.Parameter(torch.zeros(2))
    self.edge_index = None
    self.nfe = 0

  def _descriptor(self, *a, **k):
    raise AssertionError('no native solve on the host')

  def _needs_grad(self, y):
    return self.differentiated and torch.is_grad_enabled()

  def _has_native_rhs(self, y):
    return self.native_rhs

  def parameters(self):
    return iter((self.alpha_train, self.beta_train, self.weight))

  def __call__(self, t, y):
    raise AssertionError('no evaluation: every runner is a recorder')


def function(kind='LaplacianODEFunc', opt=(), differentiated=False, native_rhs=True, layer=()):
  if kind is None:
    return lambda t, y: -y
  return type(kind, (_Func,), {})(dict(opt), differentiated, native_rhs, dict(layer))


class _Node(object):
  """Stands for the autograd node of an earlier recorded forward pass."""

  def __init__(self, consumed):
    self.gnpde_consumed = consumed


class _Evaluator(object):
  def reset(self):
    pass

  def read(self):
    return {'best_hits': [0, 0, 0], 'trace': None}


# --------------------------------------------------------------------------------------------------
# the rows: (id, spec); spec keys -- entry ('odeint' | 'rk4' | 'dopri5' | 'backward'), kind, opt, differentiated, native_rhs, layer,
# device, width, times, tdtype, method, options, env, shard (the process group is up), tape (None | 'live' | 'consumed' | 'dead'),
# use_graph; early: solver (keywords of the solver), max_test_steps; backward: adjoint_options, params, route
# --------------------------------------------------------------------------------------------------
T2, T3 = (0.0, 1.0), (0.0, 0.5, 1.0)
STEP = {'step_size': 0.25}


def _forward_product():
  rows = []
  for method, diff, device, times, tdtype, option in itertools.product(
      ('euler', 'midpoint', 'rk4', 'dopri5', 'adaptive_heun'), (False, True), (True, False), (T2, T3), ('float32', 'float64'),
      (None, 'host_controller', 'eager_stages', 'norm')):
    options = dict(STEP) if method in ('euler', 'midpoint', 'rk4') else {}
    if option is not None:
      options[option] = caller_norm if option == 'norm' else True
    rid = 'odeint-%s-%s-%s-%dt-%s-%s' % (method, 'grad' if diff else 'nograd', 'dev' if device else 'host', len(times), tdtype, option)
    rows.append((rid, dict(entry='odeint', method=method, differentiated=diff, device=device, times=times, tdtype=tdtype, options=options)))
  return rows


def _row(rid, entry='odeint', **spec):
  return rid, dict(spec, entry=entry)


def _forward_special():
  fx, nl, gat = dict(STEP), 'ODEFuncTransformerAtt', 'ODEFuncAtt'
  rows = [
    _row('unknown-method', method='bosh3'),
    _row('unknown-method-foreign', method='bosh3', kind=None),
    _row('default-method', method=None),
    _row('rk4-no-step-size', method='rk4'),
    _row('rk4-no-step-size-foreign-3t', method='rk4', kind=None, times=T3),
    _row('rk4-no-graph', method='rk4', options=fx, use_graph=False),
    _row('dopri5-trials-per-sync', method='dopri5', options={'trials_per_sync': 3}),
    _row('dopri5-trials-per-sync-3t', method='dopri5', options={'trials_per_sync': 3}, times=T3),
    _row('dopri5-norm-and-eager', method='dopri5', options={'norm': caller_norm, 'eager_stages': True}),
    _row('heun-eager-3t', method='adaptive_heun', options={'eager_stages': True}, times=T3),
    _row('dopri5-grad-mode-off', method='dopri5', differentiated=True, no_grad=True),
    _row('rk4-grad-mode-off', method='rk4', options=fx, differentiated=True, no_grad=True),
  ]
  for method, options in (('rk4', fx), ('dopri5', {}), ('adaptive_heun', {})):
    for times in (T2, T3):
      rows.append(_row('%s-foreign-%dt' % (method, len(times)), method=method, options=options, kind=None, times=times))
      rows.append(_row('%s-no-native-rhs-%dt' % (method, len(times)), method=method, options=options, kind=gat, native_rhs=False,
                       opt={'mix_features': True}, times=times))
      rows.append(_row('%s-host-outputs-%dt' % (method, len(times)), method=method, options=options, opt={'gnpde_host_outputs': True}, times=times))
      rows.append(_row('%s-shard-%dt' % (method, len(times)), method=method, options=options, opt={'gnpde_shard': True}, shard=True, times=times))
    rows.append(_row('%s-shard-grad' % method, method=method, options=options, opt={'gnpde_shard': True}, shard=True, differentiated=True))
    rows.append(_row('%s-shard-host-state' % method, method=method, options=options, opt={'gnpde_shard': True}, shard=True, device=False))
    rows.append(_row('%s-shard-no-group' % method, method=method, options=options, opt={'gnpde_shard': True}))
    rows.append(_row('%s-shard-foreign' % method, method=method, options=options, kind=None, shard=True))
    rows.append(_row('%s-env-host-outputs-3t' % method, method=method, options=options, env={'GNPDE_HOST_OUTPUTS': '1'}, times=T3))
    rows.append(_row('%s-times-repeat' % method, method=method, options=options, times=(0.0, 1.0, 1.0)))
    rows.append(_row('%s-times-back' % method, method=method, options=options, times=(0.0, 1.0, 0.5)))
    rows.append(_row('%s-wide-nograd' % method, method=method, options=options, width=257))
  rows.append(_row('midpoint-shard', method='midpoint', options=fx, opt={'gnpde_shard': True}, shard=True))
  rows.append(_row('midpoint-shard-3t', method='midpoint', options=fx, opt={'gnpde_shard': True}, shard=True, times=T3))
  # differentiated solves: the recorded routes and everything that refuses them
  for method, options, host_switch in (('rk4', fx, 'fixed'), ('euler', fx, 'fixed'), ('midpoint', fx, 'fixed'), ('dopri5', {}, 'dopri5')):
    g = dict(method=method, options=options, differentiated=True)
    for kind in ('LaplacianODEFunc', nl, gat, 'ODEFuncBeltramiAtt'):
      rows.append(_row('%s-grad-%s' % (method, kind), kind=kind, **g))
      rows.append(_row('%s-grad-%s-no-alpha-sigmoid' % (method, kind), kind=kind, opt={'no_alpha_sigmoid': True}, **g))
      rows.append(_row('%s-grad-%s-shard-option' % (method, kind), kind=kind, opt={'gnpde_shard': True}, **g))
    for kind in (nl, gat):
      rows.append(_row('%s-grad-%s-mix-features' % (method, kind), kind=kind, opt={'mix_features': True}, **g))
    rows.append(_row('%s-grad-nl-attention-260' % method, kind=nl, layer={'attention_dim': 260, 'kernel_att_dim': 260, 'h': 4, 'd_k': 65}, **g))
    rows.append(_row('%s-grad-gat-one-head' % method, kind=gat, layer={'h': 1}, **g))
    for width in (256, 257):
      rows.append(_row('%s-grad-width-%d' % (method, width), width=width, **g))
    for switch in ('gnpde_host_%s_training' % host_switch, 'gnpde_composite_backward',
                   'gnpde_host_%s_training' % ('dopri5' if host_switch == 'fixed' else 'fixed')):
      rows.append(_row('%s-grad-%s' % (method, switch), opt={switch: True}, **g))
    for name in ('GNPDE_HOST_DOPRI5_TRAINING', 'GNPDE_HOST_FIXED_TRAINING'):
      rows.append(_row('%s-grad-env-%s' % (method, name), env={name: '1'}, **g))
    for tape in ('live', 'consumed', 'dead'):
      rows.append(_row('%s-grad-tape-%s' % (method, tape), tape=tape, **g))
    rows.append(_row('%s-grad-tape-live-of-the-other-solver' % method, tape='live', tape_slot='other', **g))
  rows.append(_row('heun-grad-dev', method='adaptive_heun', differentiated=True, tape='live'))
  return rows


def _early_rows():
  rows = []
  for solver, kw in (('rk4', {'step_size': 0.25}), ('dopri5', {}), ('dopri5', {'eager_stages': True}), ('dopri5', {'host_controller': True}),
                     ('dopri5', {'trials_per_sync': 2})):
    tag = solver + ''.join('-' + k for k in kw if k != 'step_size')
    for device, times, tdtype in itertools.product((True, False), (T2, T3), ('float32', 'float64')):
      rows.append(_row('early-%s-%s-%dt-%s' % (tag, 'dev' if device else 'host', len(times), tdtype), entry=solver, solver=kw, device=device,
                       times=times, tdtype=tdtype))
    rows.append(_row('early-%s-foreign' % tag, entry=solver, solver=kw, kind=None))
    rows.append(_row('early-%s-grad' % tag, entry=solver, solver=kw, differentiated=True))
    rows.append(_row('early-%s-no-native-rhs' % tag, entry=solver, solver=kw, kind='ODEFuncAtt', native_rhs=False))
    rows.append(_row('early-%s-shard' % tag, entry=solver, solver=kw, opt={'gnpde_shard': True}, shard=True))
  for steps in (0, 1):
    for kw in ({}, {'eager_stages': True}):
      rows.append(_row('early-dopri5%s-max-test-steps-%d' % ('-eager' if kw else '', steps), entry='dopri5', solver=kw, max_test_steps=steps))
    rows.append(_row('early-dopri5-max-test-steps-%d-host' % steps, entry='dopri5', solver={}, max_test_steps=steps, device=False))
  return rows


def _backward_rows():
  rows = []
  nl, gat = 'ODEFuncTransformerAtt', 'ODEFuncAtt'
  for method in ('euler', 'rk4', 'midpoint', 'dopri5', 'adaptive_heun', 'bosh3'):
    ao = dict(STEP) if method in ('euler', 'rk4', 'midpoint') else {}
    b = dict(entry='backward', method=method, adjoint_options=ao)
    adaptive = method in ('dopri5', 'adaptive_heun')
    dev = dict(route='adjoint_device') if adaptive else {}
    pair = dict(route='adjoint_host_pair') if adaptive else {}
    rows.append(_row('adjoint-%s' % method, **dict(b, **dev)))
    rows.append(_row('adjoint-%s-3t' % method, times=T3, **dict(b, **dev)))
    rows.append(_row('adjoint-%s-host-state' % method, device=False, **b))
    rows.append(_row('adjoint-%s-float64-state' % method, sdtype='float64', **b))
    rows.append(_row('adjoint-%s-foreign' % method, kind=None, **b))
    rows.append(_row('adjoint-%s-width-256' % method, width=256, **dict(b, **dev)))
    rows.append(_row('adjoint-%s-width-257' % method, width=257, **dict(b, **pair)))
    for kind in (nl, gat, 'ODEFuncBeltramiAtt'):
      rows.append(_row('adjoint-%s-%s' % (method, kind), kind=kind, **b))
    rows.append(_row('adjoint-%s-gat-mix-features' % method, kind=gat, opt={'mix_features': True}, **b))
    rows.append(_row('adjoint-%s-nl-attention-260' % method, kind=nl, layer={'attention_dim': 260, 'kernel_att_dim': 260, 'h': 4, 'd_k': 65}, **b))
    for switch in ('gnpde_composite_backward', 'gnpde_host_adjoint'):
      rows.append(_row('adjoint-%s-%s' % (method, switch), opt={switch: True}, **b))
    rows.append(_row('adjoint-%s-no-alpha-sigmoid' % method, opt={'no_alpha_sigmoid': True}, **b))
    rows.append(_row('adjoint-%s-gnpde_host_controller_adjoint' % method, opt={'gnpde_host_controller_adjoint': True}, **dict(b, **pair)))
    rows.append(_row('adjoint-%s-host-flat' % method, **dict(b, adjoint_options=dict(ao, host_flat=True))))
    rows.append(_row('adjoint-%s-norm' % method, **dict(b, adjoint_options=dict(ao, norm=caller_norm))))
    rows.append(_row('adjoint-%s-without-alpha' % method, params=('weight',), **dict(b, **pair)))
    rows.append(_row('adjoint-%s-source' % method, opt={'add_source': True}, **dict(b, **dev)))
    rows.append(_row('adjoint-%s-source-without-beta' % method, opt={'add_source': True}, params=('alpha_train', 'weight'), **dict(b, **pair)))
    rows.append(_row('adjoint-%s-alpha-alone' % method, params=('alpha_train',), **dict(b, **dev)))
  for method in ('euler', 'rk4'):
    rows.append(_row('adjoint-%s-no-step-size' % method, entry='backward', method=method, adjoint_options={}))
  rows.append(_row('adjoint-midpoint-no-step-size', entry='backward', method='midpoint', adjoint_options={}))
  return rows


ROWS = _forward_product() + _forward_special() + _early_rows() + _backward_rows()


# --------------------------------------------------------------------------------------------------
# running a row
# --------------------------------------------------------------------------------------------------
def _shown(name, value):
  if name == 'norm':
    return None if value is None else ('caller' if value is caller_norm else 'mixed')
  if name in ('evaluator', 'on_step', 'on_accept'):
    return value is not None
  return value


class Setup(object):
  """A row's objects, and its environment for the time of a `with`."""

  def __init__(self, spec, monkeypatch):
    s = self.spec = spec
    self.mp = monkeypatch
    self.func = function(s.get('kind', 'LaplacianODEFunc'), s.get('opt', ()), s.get('differentiated', False), s.get('native_rhs', True),
                         s.get('layer', ()))
    self.t = torch.tensor(s.get('times', T2), dtype=getattr(torch, s.get('tdtype', 'float32')))
    self.y0 = state(s.get('device', True), s.get('width', 4), getattr(torch, s.get('sdtype', 'float32')))
    self.keep = None
    if s.get('tape') is not None:
      slot = {'rk4': '_tape_live_fixed', 'euler': '_tape_live_fixed', 'midpoint': '_tape_live_fixed'}.get(s['method'], '_tape_live_dopri5')
      if s.get('tape_slot') == 'other':
        slot = '_tape_live_dopri5' if slot == '_tape_live_fixed' else '_tape_live_fixed'
      ctx = _Node(s['tape'] == 'consumed')
      self.func.__dict__[slot] = weakref.ref(ctx)
      self.keep = None if s['tape'] == 'dead' else ctx

  def __enter__(self):
    for name, value in self.spec.get('env', {}).items():
      self.mp.setenv(name, value)
    # (an initialised process group, as far as the ladders ask: distributed.shard_requested without torch.distributed)
    up = bool(self.spec.get('shard'))
    self.mp.setattr(D, 'shard_requested', lambda f: up and bool(f.opt.get('gnpde_shard')))
    self.grad = torch.no_grad() if self.spec.get('no_grad') else torch.enable_grad()
    self.grad.__enter__()
    return self

  def __exit__(self, *exc):
    self.grad.__exit__(*exc)
    return False


def _install(mp, log, live_tape):
  """Every runner of the odeint module (and the names early_stop_solver imported) becomes a recorder that returns a token."""
  def recorder(name, orig, result):
    sig = inspect.signature(orig)

    def rec(*a, **k):
      bound = sig.bind(*a, **k)
      bound.apply_defaults()
      log.append([name, {arg: _shown(arg, bound.arguments[arg]) for arg in RUNNERS[name]}])
      return result(bound.arguments)
    return rec

  def token(name):
    return lambda args: 'result of ' + name
  results = {
    '_solve_dopri5_device': lambda args: 'result of _solve_dopri5_device' if args['evaluator'] is None else ('result of _solve_dopri5_device', [0.0]),
    '_adjoint_native': lambda args: (args['a'], [None] * len(args['params'])),
    '_adjoint_fixed_grid': lambda args: (args['a'], list(args['gparams'])),
    '_adjoint_adaptive_native': lambda args: (args['a'], {}),
  }
  for name in RUNNERS:
    if name == 'odeint' or (live_tape and name in ('_solve_fixed_recorded', '_solve_dopri5_recorded')):
      continue        # (a live tape is noticed inside the recorded runners on the commit this table was recorded on: they run)
    module = D if name == 'solve_sharded' else O
    rec = recorder(name, getattr(module, name), results.get(name, token(name)))
    mp.setattr(module, name, rec)
    if hasattr(ES, name):
      mp.setattr(ES, name, rec)


def observe(spec, monkeypatch):
  """The outcome of a row: the runner calls with their selecting arguments and the reports on the function, or the exception."""
  log = []
  with Setup(spec, monkeypatch) as S:
    _install(monkeypatch, log, spec.get('tape') == 'live' and spec.get('tape_slot') != 'other')
    func, entry = S.func, spec['entry']
    try:
      if entry == 'odeint':
        out = O.odeint(func, S.y0, S.t, method=spec['method'], options=spec.get('options'), use_graph=spec.get('use_graph', True),
                       rtol=1e-3, atol=1e-4)
        assert out == 'result of ' + log[-1][0]
      elif entry in ('rk4', 'dopri5'):
        opt = {'dataset': 'Cora', 'max_test_steps': spec.get('max_test_steps', 100)}
        kw = dict(func=func, y0=S.y0, opt=opt, rtol=1e-3, atol=1e-4, **spec['solver'])
        solver = ES.EarlyStopRK4(**kw) if entry == 'rk4' else ES.EarlyStopDopri5(**kw)
        solver.evaluator = _Evaluator()
        out = solver.integrate(S.t)[1]
        assert out == 'result of ' + log[-1][0]
      else:
        _backward(S, spec, monkeypatch, log)
    except Exception as exc:   # noqa: BLE001
      return {'raises': type(exc).__name__, 'message': str(exc), 'calls': log}
    reports = {name: getattr(func, name, None) for name in ('_last_train_solve', '_last_output_solve', 'gather_dtype_used', 'nfe')}
    return {'calls': log, 'reports': reports}


def backward_inputs(S, spec):
  func = S.func
  names = spec.get('params', ('alpha_train', 'beta_train', 'weight'))
  params = tuple(getattr(func, n) for n in names) if hasattr(func, 'opt') else ()
  ans = state(spec.get('device', True), spec.get('width', 4), getattr(torch, spec.get('sdtype', 'float32')), lead=(len(S.t),))
  adj = dict(rtol=1e-3, atol=1e-4, method=spec['method'], options=dict(spec['adjoint_options']))
  return params, ans, adj


def _backward(S, spec, monkeypatch, log):
  params, ans, adj = backward_inputs(S, spec)

  def flat(func, y0, t, **kw):
    log.append(['odeint', {'method': kw['method'], 'norm': _shown('norm', kw['options'].get('norm'))}])
    return torch.stack([y0, y0])
  monkeypatch.setattr(O, 'odeint', flat)
  ctx = types.SimpleNamespace(func=S.func, adj=adj, saved_tensors=(S.t, ans) + params)
  grads = O._AdjointSolve.backward(ctx, torch.zeros_like(ans))
  assert len(grads) == 5 + len(params) and len(log) == len(S.t) - 1


def ask_rule(R, spec, monkeypatch):
  """What the rule, queried on its own, says of a row: (route, reason), or the exception."""
  with Setup(spec, monkeypatch) as S:
    try:
      if spec['entry'] == 'odeint':
        return R.forward(S.func, S.y0, S.t, 'dopri5' if spec['method'] is None else spec['method'], dict(spec.get('options') or {}))
      if spec['entry'] == 'backward':
        params, ans, adj = backward_inputs(S, spec)
        return R.adjoint(S.func, ans[-1], adj['method'], adj['options'], params)
      kw = spec['solver']
      return R.early(S.func, S.y0, S.t, spec['entry'], bool(kw.get('eager_stages') or kw.get('host_controller')), spec.get('max_test_steps', 100))
    except Exception as exc:   # noqa: BLE001
      return {'raises': type(exc).__name__, 'message': str(exc)}


if __name__ == '__main__':
  import pytest
  recorded = {}
  for rid, spec in ROWS:
    mp = pytest.MonkeyPatch()
    try:
      recorded[rid] = observe(spec, mp)
    finally:
      mp.undo()
  assert len(recorded) == len(ROWS), 'row ids repeat'
  with open(GOLDEN, 'w') as fh:
    json.dump(recorded, fh, indent=0, sort_keys=True)
    fh.write('\n')
  print('%d rows -> %s' % (len(recorded), GOLDEN))
