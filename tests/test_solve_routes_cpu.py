"""Which runner takes which solve: the whole of `odeint`'s ladder, of the early-stopping integrators' and of the adjoint's backward
intervals, row by row (solve_routes_cases.ROWS) against the outcomes recorded before the route rule existed
(tests/golden/solve_routes.json).  Stubs for state and function, recorders for runners: no device."""
import importlib
import json

import pytest

import solve_routes_cases as C

with open(C.GOLDEN) as fh:
  RECORDED = json.load(fh)
# the reasons the ladders write into `_last_output_solve` as 'host loop (<reason>)' (a foreign callable gets no report: it is no object of ours)
OUTPUT_REASONS = ('state is not a float32 [n, d] tensor on a HIP device', 'differentiated solve',
                  'no native right-hand side for this configuration', 'gnpde_host_outputs',
                  'gnpde_shard: the row-partitioned solver has two output times', 'output times are not strictly increasing',
                  'times are not float32', 'host_controller', 'eager_stages', 'a norm of the caller')


def test_the_table_is_the_recorded_one():
  assert len(C.ROWS) == len(dict(C.ROWS)) and sorted(dict(C.ROWS)) == sorted(RECORDED)


@pytest.mark.parametrize('rid,spec', C.ROWS, ids=[rid for rid, _ in C.ROWS])
def test_row_takes_the_recorded_runner(rid, spec, monkeypatch):
  """The runner calls with the arguments that select a variant (pair, tableau, norm, evaluator, stop_after, use_graph, ...) and the
  reports left on the function (`_last_train_solve`, `_last_output_solve`, `gather_dtype_used`, `nfe`), or the exception's type and
  message, and the calls made before it."""
  assert json.loads(json.dumps(C.observe(spec, monkeypatch))) == RECORDED[rid]


def test_examples_of_the_table():
  def runner(rid):
    return RECORDED[rid]['calls'][0]
  row = RECORDED['odeint-rk4-nograd-dev-3t-float64-None']
  assert runner('odeint-rk4-nograd-dev-3t-float64-None')[0] == '_solve_native' and row['reports']['_last_output_solve'] == 'native fixed grid'
  row = RECORDED['odeint-dopri5-nograd-dev-3t-float64-None']
  assert runner('odeint-dopri5-nograd-dev-3t-float64-None')[0] == '_solve_dopri5'
  assert row['reports']['_last_output_solve'] == 'host loop (times are not float32)'
  name, args = runner('odeint-adaptive_heun-grad-dev-2t-float32-None')
  assert name == '_solve_dopri5' and args['tableau'] == 'adaptive_heun'
  # gnpde_shard with more than two output times: a fixed grid quietly takes the host loop, an adaptive method raises
  assert runner('rk4-shard-3t')[0] == '_solve_fixed_host' and RECORDED['dopri5-shard-3t']['raises'] == 'GnpdeError'


def test_every_runner_and_every_reported_reason_has_a_row():
  hit = {call[0] for row in RECORDED.values() for call in row['calls']}
  assert hit == set(C.RUNNERS)
  reports = {row['reports']['_last_output_solve'] for row in RECORDED.values() if 'reports' in row}
  for reason in OUTPUT_REASONS:
    assert 'host loop (%s)' % reason in reports, reason
  assert reports == {None, 'native fixed grid', 'native device controller'} | {'host loop (%s)' % r for r in OUTPUT_REASONS}
  trains = {row['reports']['_last_train_solve'] for row in RECORDED.values() if 'reports' in row}
  assert trains == {None, 'differentiable host loop (the record of an earlier forward pass still awaits its backward)'}


def test_the_rule_on_its_own_names_the_recorded_route():
  """routes.forward / early / adjoint, asked without any entry point around them, name the route whose runner the row took (or raise what
  the row raised) -- and between them the rows draw every route and every reason the rule can give."""
  R = importlib.import_module('gnpde_amd.routes')
  assert set(C.ROUTE_OF.values()) | {'adjoint_device', 'adjoint_host_pair'} == set(R.ROUTES)
  routes, reasons = set(), set()
  for rid, spec in C.ROWS:
    with pytest.MonkeyPatch.context() as mp:
      want, got = RECORDED[rid], C.ask_rule(R, spec, mp)
    if 'raises' in want and not want['calls']:
      assert got == {'raises': want['raises'], 'message': want['message']}, rid
      continue
    runner = want['calls'][0][0]
    assert all(call[0] == runner for call in want['calls']), rid
    assert got[0] == spec.get('route', C.ROUTE_OF.get(runner)), (rid, got)
    assert (got[1] is None) == (got[0] in ('native_fixed', 'sharded', 'recorded_fixed', 'device_controller', 'recorded_dopri5',
                                           'adjoint_native', 'adjoint_device')), (rid, got)
    if spec['entry'] == 'odeint' and len(spec.get('times', C.T2)) > 2 and spec.get('kind', '') is not None:
      report = want['reports']['_last_output_solve']
      assert report == ('host loop (%s)' % got[1] if got[1] else report), (rid, got)
    routes.add(got[0])
    reasons.add(got[1])
  assert routes == set(R.ROUTES)
  assert reasons == set(R.REASONS) | {None}, (reasons ^ (set(R.REASONS) | {None}))
