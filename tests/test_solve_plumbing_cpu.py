"""The host plumbing every native solve path shares (odeint._entry, _solver_for, _copy_source; ODEFunc's bulk NFE accounting), on stub
function and solver objects: no kernel runs, the state buffers are CPU tensors."""
import importlib

import pytest
import torch

import gnpde_amd as G
from gnpde_amd import _lib
from gnpde_amd.base_classes import ODEFunc
from gnpde_amd.utils import MaxNFEException

O = importlib.import_module('gnpde_amd.odeint')
CPU = torch.device('cpu')


class StubFunc(object):
  """What the helpers read of a function object: opt, nfe, x0 and its own __dict__ for the slots."""
  _nfe_room = ODEFunc._nfe_room
  _charge_fixed_nfe = ODEFunc._charge_fixed_nfe
  _settle_adaptive_nfe = ODEFunc._settle_adaptive_nfe

  def __init__(self, add_source=False, max_nfe=10, nfe=0):
    self.opt = {'add_source': add_source, 'max_nfe': max_nfe}
    self.nfe = nfe
    self.x0 = None


class StubSolver(object):
  def __init__(self):
    self.closed = 0

  def close(self):
    self.closed += 1


def _filled(func, slot, key):
  ent = O._entry(func, slot, key, 5, 8, CPU, ('y', 'a'))
  ent['solver'], ent['sweep'] = StubSolver(), StubSolver()
  return ent


def test_entry_miss_closes_the_slot_and_its_siblings():
  f = StubFunc()
  old = _filled(f, '_solver_state', 'k0')
  sib = _filled(f, '_dopri5_device', 'k1')
  other = _filled(f, '_tape_state', 'k2')
  ent = O._entry(f, '_solver_state', 'k3', 5, 8, CPU, ('y',), siblings=('_dopri5_device',))
  assert [old['solver'].closed, old['sweep'].closed, sib['solver'].closed, sib['sweep'].closed] == [1, 1, 1, 1]
  assert f.__dict__['_solver_state'] == {'k3': ent} and f.__dict__['_dopri5_device'] == {}
  assert other['solver'].closed == 0 and f.__dict__['_tape_state'] == {'k2': other}      # no sibling: left alone
  assert ent['solver'] is None and ent['sweep'] is None and ent['sig'] is None and ent['sweep_sig'] is None
  assert 'a' not in ent and tuple(ent['y'].shape) == (5, 8)


def test_entry_hit_returns_the_entry_and_closes_nothing():
  f = StubFunc()
  ent = _filled(f, '_fixed_tape_state', 'k')
  sib = _filled(f, '_adjoint_state', 'k')
  again = O._entry(f, '_fixed_tape_state', 'k', 5, 8, CPU, ('y', 'a'), siblings=('_adjoint_state',))
  assert again is ent
  assert ent['solver'].closed == ent['sweep'].closed == sib['solver'].closed == sib['sweep'].closed == 0
  assert f.__dict__['_adjoint_state'] == {'k': sib}


@pytest.mark.parametrize('add_source', [False, True])
def test_entry_buffers(add_source):
  f = StubFunc(add_source=add_source)
  view = object()
  ent = O._entry(f, '_adjoint_state', 'k', 7, 6, CPU, ('y', 'a'), view=view)
  for name in ('y', 'a') + (('x0',) if add_source else ()):
    assert tuple(ent[name].shape) == (7, 6) and ent[name].stride(0) == 8 and _lib.is_padded(ent[name]), name
  assert (ent['x0'] is not None) == add_source
  assert ent['view'] is view and ent['extra'] == {}
  assert not _lib.is_padded(O._entry(StubFunc(), '_adjoint_state', 'k', 7, 8, CPU)['y'])


def test_solver_for_keeps_the_solver_of_the_same_signature():
  ent = _filled(StubFunc(), '_fixed_tape_state', 'k')
  built = []

  def build():
    built.append(StubSolver())
    return built[-1]
  first = O._solver_for(ent, ('sig', 1), build)
  ent['sweep'] = sweep = StubSolver()
  assert O._solver_for(ent, ('sig', 1), build) is first and len(built) == 1
  assert first.closed == 0 and sweep.closed == 0 and ent['sweep'] is sweep
  second = O._solver_for(ent, ('sig', 2), build)
  assert second is built[1] is ent['solver'] and ent['sig'] == ('sig', 2)
  assert first.closed == 1 and sweep.closed == 1 and ent['sweep'] is None and second.closed == 0


@pytest.mark.parametrize('slot,bufs', [('_dopri5_host', O._component_bufs('y', 6) + ('out',)),
                                       ('_adjoint_adaptive', O._component_bufs('y', 1) + O._component_bufs('a', 1))])
def test_host_pair_slots(slot, bufs):
  """The two host-controlled embedded-pair solves keep their buffers, the scratch of the norm reductions and (the adjoint) the
  device solver and its transposed weights in an _entry like every other path."""
  f = StubFunc(add_source=True)
  ent = O._host_pair_entry(f, slot, 'k0', 5, 6, CPU, bufs)
  assert len(set(bufs)) == len(bufs) and all(tuple(ent[nm].shape) == (5, 6) and _lib.is_padded(ent[nm]) for nm in bufs + ('x0',))
  assert ent['extra']['ratio_dev'].tolist() == [0.0] and ent['extra']['err_ws'].numel() == 4096
  ent['extra']['w_t'] = torch.ones(3)
  solver = O._solver_for(ent, ('sig', 1), StubSolver)
  held = [ent[nm] for nm in bufs + ('x0',)] + [ent['extra'][nm] for nm in ('ratio_dev', 'err_ws', 'w_t')]
  again = O._host_pair_entry(f, slot, 'k0', 5, 6, CPU, bufs)                  # a hit: the same buffers, extras and solver
  assert again is ent and all(a is b for a, b in zip(held, [ent[nm] for nm in bufs + ('x0',)] + list(ent['extra'].values())))
  assert O._solver_for(ent, ('sig', 1), StubSolver) is solver and solver.closed == 0
  other = _filled(f, '_adjoint_state', 'k')
  new = O._host_pair_entry(f, slot, 'k1', 5, 6, CPU, bufs)                    # a miss: closes the old solver, and only that slot's
  assert solver.closed == 1 and other['solver'].closed == 0 and f.__dict__[slot] == {'k1': new}
  assert new['solver'] is None and 'w_t' not in new['extra'] and new['y'] is not ent['y']
  assert new['extra']['ratio_dev'] is not ent['extra']['ratio_dev']


def test_fixed_nfe_charge():
  f = StubFunc(max_nfe=10, nfe=3)
  f._charge_fixed_nfe(8)                 # evaluations 4 .. 11 find nfe = 3 .. 10: none of them raises
  assert f.nfe == 3                      # (the caller adds the 8 once the solve has run)
  with pytest.raises(MaxNFEException):
    f._charge_fixed_nfe(9)               # the ninth finds nfe = 11
  assert f.nfe == 11
  f = StubFunc(max_nfe=10, nfe=12)
  with pytest.raises(MaxNFEException):
    f._charge_fixed_nfe(1)
  assert f.nfe == 12


def test_adaptive_nfe_settle():
  f = StubFunc(max_nfe=10, nfe=3)
  room = f._nfe_room()
  assert room == 8
  with pytest.raises(MaxNFEException):
    f._settle_adaptive_nfe(room, False, 6)           # gave up before the end point
  assert f.nfe == 9
  f.nfe = 3
  with pytest.raises(MaxNFEException):
    f._settle_adaptive_nfe(room, True, 13)           # the batch in flight ran past the allowance
  assert f.nfe == 11
  f.nfe = 3
  f._settle_adaptive_nfe(room, True, 8)
  assert f.nfe == 11


def test_source_copy():
  f = StubFunc(add_source=True)
  ent = O._entry(f, '_tape_state', 'k', 4, 6, CPU)
  with pytest.raises(G.GnpdeError, match='add_source is set but x0 was never assigned'):
    O._copy_source(f, ent['x0'])
  f.x0 = torch.arange(24.0).reshape(4, 6).requires_grad_(True)
  O._copy_source(f, ent['x0'])
  assert torch.equal(ent['x0'], f.x0.detach()) and not ent['x0'].requires_grad

  class View(object):
    order = torch.tensor([2, 0, 3, 1])

    def enter(self, x, out):
      return out.copy_(x.index_select(0, self.order))
  O._copy_source(f, ent['x0'], View())
  assert torch.equal(ent['x0'], f.x0.detach()[View.order])
