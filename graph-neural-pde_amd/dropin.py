"""Run the reference's own scripts (`run_GNN.py`, `GNN.py`, `GNN_early.py`, `model_configurations.py`) on the MI355X classes
without editing them.

The reference looks its functions and blocks up by MODULE name (`from function_transformer_attention import
ODEFuncTransformerAtt`, src/model_configurations.py:1-9; `from base_classes import BaseGNN`, src/GNN.py:4; `from
early_stop_solver import EarlyStopInt`, src/GNN_early.py:10).  `install()` answers those imports with the modules of this
package, whatever the order of `sys.path`:

    python -m gnpde_amd.dropin [--native-gnn] [--native-knn] [--native-gdc] [--native-gdc-push] [--native-posdist] [--native-edge-sampling] /path/to/graph-neural-pde/src/run_GNN.py --dataset Cora --function transformer ...

or, from Python, `import gnpde_amd.dropin; gnpde_amd.dropin.install()` before the first import of a reference module.

* the function / block / early-stopping modules are this package's modules under the reference's names (`MODULES`);
* `base_classes` is MERGED, lazily, at its first import: everything the reference's own file defines (`BaseGNN`, the
  regulariser registry `REGULARIZATION_FNS`, ...) with `ODEFunc`, `ODEblock` and `RegularizedODEfunc` replaced by this
  package's -- the reference file is searched on `sys.path` at that moment, so the path may be set up after `install()`;
* `GNN` (optional, `native_gnn=True` / `--native-gnn`): the model of `gnpde_amd/GNN.py`, whose encoder and `relu -> m2`
  decoder are single native launches at test time; without it the reference's own `GNN.py` runs over the classes above;
* `graph_rewiring` (optional, `native_knn=True` / `--native-knn`): merged like `base_classes` -- the reference's own module with
  `KNN` replaced by the native search of `gnpde_amd/graph_rewiring.py`.  `apply_KNN` looks `KNN` up when it is called, so
  `run_GNN.py --rewire_KNN` then runs the native kernel; with no reference file on the path the module is this package's alone.
  `native_gdc=True` / `--native-gdc` merges the same module with `apply_gdc` and `GDCWrapper` replaced (graph diffusion rewiring,
  `--rewiring gdc` and `--pos_enc_type GDC`): `data.py`'s `from graph_rewiring import apply_gdc` then gets the native one.  Both
  flags together replace all three names.  `native_gdc_push=True` / `--native-gdc-push` is `--native-gdc` plus the option
  `gnpde_gdc_approx = 'push'` for every `apply_gdc` call whose opt does not set it: `run_GNN.py --rewiring gdc --gdc_sparsification
  threshold` without `--exact` then runs the approximate forward push, as the reference does.  `native_posdist=True` / `--native-posdist` likewise replaces `apply_pos_dist_rewire`
  (positional-distance rewiring, `--rewiring pos_enc_knn`) and the helpers it calls (`apply_beltrami`, `hyperbolize`,
  `apply_feat_KNN`, `apply_dist_KNN`, `apply_dist_threshold`); the flags combine.
  `native_edge_sampling=True` / `--native-edge-sampling` replaces `add_edges`, `add_outgoing_attention_edges`, `edge_sampling` and
  `apply_edge_sampling` in the same merged module and serves a module `GNN_KNN` whose class `GNN_KNN` is this package's `GNN_FA`
  (GNN_KNN with the fully-adjacent layer), so `run_GNN.py --fa_layer` runs the native layer.
"""
import importlib
import importlib.abc
import importlib.util
import os
import sys
import types

# reference module name (src/<name>.py) -> module of this package that provides its classes
MODULES = {
  'function_laplacian_diffusion': 'gnpde_amd.function_laplacian_diffusion',      # LaplacianODEFunc
  'function_transformer_attention': 'gnpde_amd.function_transformer_attention',  # ODEFuncTransformerAtt, SpGraphTransAttentionLayer
  'function_GAT_attention': 'gnpde_amd.function_GAT_attention',                  # ODEFuncAtt, SpGraphAttentionLayer
  'block_constant': 'gnpde_amd.block_constant',                                  # ConstantODEblock
  'block_transformer_attention': 'gnpde_amd.block_transformer_attention',        # AttODEblock
  'block_mixed': 'gnpde_amd.block_mixed',                                        # MixedODEblock
  'block_transformer_hard_attention': 'gnpde_amd.block_transformer_hard_attention',   # HardAttODEblock
  'block_transformer_rewiring': 'gnpde_amd.block_transformer_rewiring',          # RewireAttODEblock
  'early_stop_solver': 'gnpde_amd.early_stop_solver',                            # EarlyStopInt, EarlyStopRK4, EarlyStopDopri5, SOLVERS
}
NATIVE_GNN = {'GNN': 'gnpde_amd.GNN'}                                            # GNN, BaseGNN (optional)
MERGED = 'base_classes'
OVERRIDES = ('ODEFunc', 'ODEblock', 'RegularizedODEfunc')                        # what base_classes takes from this package
# merged modules: reference module name -> (module of this package, names taken from it, standalone).  The rest of the module
# is the reference's own file where one is on sys.path; `standalone`: without such a file the module is this package's own, and
# with one the reference's functions see the replaced names too (they look their siblings up when called: apply_KNN -> KNN).
MERGES = {MERGED: ('gnpde_amd.base_classes', OVERRIDES, False)}
NATIVE_KNN = {'graph_rewiring': ('gnpde_amd.graph_rewiring', ('KNN',), True)}    # optional: the native neighbour search
NATIVE_GDC = {'graph_rewiring': ('gnpde_amd.graph_rewiring', ('apply_gdc', 'GDCWrapper'), True)}   # optional: native graph diffusion rewiring
# optional: native positional-distance rewiring (--rewiring pos_enc_knn) with the helpers it calls
NATIVE_POSDIST = {'graph_rewiring': ('gnpde_amd.graph_rewiring', ('apply_pos_dist_rewire', 'apply_beltrami', 'hyperbolize', 'apply_feat_KNN',
                                                                   'apply_dist_KNN', 'apply_dist_threshold'), True)}
# optional: native edge-sampling rewiring (the fully-adjacent layer) and the model class that runs it, served as GNN_KNN.GNN_KNN
NATIVE_EDGE_SAMPLING = {'graph_rewiring': ('gnpde_amd.graph_rewiring', ('add_edges', 'add_outgoing_attention_edges', 'edge_sampling',
                                                                         'apply_edge_sampling'), True)}
FA_MODULE = 'GNN_KNN'


def _fa_module():
  """Module `GNN_KNN` of the drop-in: the name GNN_KNN bound to GNN_FA."""
  from gnpde_amd.GNN_FA import GNN_FA
  m = types.ModuleType(FA_MODULE)
  m.GNN_KNN = m.GNN_FA = GNN_FA
  m.__gnpde_reference__ = None
  return m


def _reference_file(name):
  """First `<name>.py` on sys.path that is not part of this package."""
  here = os.path.dirname(os.path.abspath(__file__))
  for p in sys.path:
    cand = os.path.abspath(os.path.join(p or '.', name + '.py'))
    if os.path.isfile(cand) and os.path.dirname(cand) != here:
      return cand
  return None


class _MergedModules(importlib.abc.MetaPathFinder, importlib.abc.Loader):
  """`import <name>` for the names of `table`: the reference's module with the listed names replaced by this package's (see
  the module docstring); without a reference file on the path, this package's module alone."""

  def __init__(self):
    self.table = dict(MERGES)

  def find_spec(self, fullname, path=None, target=None):
    if fullname not in self.table:
      return None
    return importlib.util.spec_from_loader(fullname, self)

  def create_module(self, spec):
    return None

  def exec_module(self, module):
    name = module.__name__
    target, overrides, standalone = self.table[name]
    ours = importlib.import_module(target)
    ref_path = _reference_file(name)
    if ref_path is not None:
      spec = importlib.util.spec_from_file_location('_reference_' + name, ref_path)
      ref = importlib.util.module_from_spec(spec)
      sys.modules[spec.name] = ref
      spec.loader.exec_module(ref)
      for attr in dir(ref):
        if not attr.startswith('__'):
          setattr(module, attr, getattr(ref, attr))
      module.__file__ = ref_path
      if standalone:
        for attr in overrides:
          setattr(ref, attr, getattr(ours, attr))
    elif standalone:
      for attr in dir(ours):
        if not attr.startswith('__'):
          setattr(module, attr, getattr(ours, attr))
    for attr in overrides:
      setattr(module, attr, getattr(ours, attr))
    module.__gnpde_reference__ = ref_path


_finder = _MergedModules()


def installed():
  return _finder in sys.meta_path


def install(native_gnn=False, native_knn=False, native_gdc=False, native_posdist=False, native_edge_sampling=False, native_gdc_push=False):
  """Answer the reference's module names with this package (idempotent).  Returns the list of names now served."""
  merges = dict(MERGES)
  native_gdc = native_gdc or native_gdc_push
  for on, extra in ((native_knn, NATIVE_KNN), (native_gdc, NATIVE_GDC), (native_posdist, NATIVE_POSDIST),
                    (native_edge_sampling, NATIVE_EDGE_SAMPLING)):
    if on:
      for name, (target, names, standalone) in extra.items():
        before = merges.get(name, (target, (), standalone))[1]
        merges[name] = (target, before + names, standalone)
  extra_names = [FA_MODULE] if native_edge_sampling else []
  already = {name: sys.modules[name] for name in list(MODULES) + list(merges) + extra_names if name in sys.modules}
  table = dict(MODULES)
  if native_gnn:
    table.update(NATIVE_GNN)
  foreign = [n for n, m in already.items()
             if not getattr(m, '__name__', '').startswith('gnpde_amd') and not hasattr(m, '__gnpde_reference__')]
  if foreign:
    raise ImportError('gnpde_amd.dropin.install(): %s already imported from elsewhere; install the drop-in before the '
                      'first import of a reference module' % ', '.join(sorted(foreign)))
  for name, target in table.items():
    sys.modules[name] = importlib.import_module(target)
  if native_edge_sampling:
    sys.modules[FA_MODULE] = _fa_module()
  _finder.table = merges
  if native_gdc_push:
    importlib.import_module('gnpde_amd.graph_rewiring').GDC_APPROX_DEFAULT = 'push'
  if _finder not in sys.meta_path:
    sys.meta_path.insert(0, _finder)
  return sorted(list(table) + extra_names) + [MERGED] + sorted(n for n in merges if n != MERGED)


def uninstall():
  """Undo install() (tests)."""
  if _finder in sys.meta_path:
    sys.meta_path.remove(_finder)
  _finder.table = dict(MERGES)
  if 'gnpde_amd.graph_rewiring' in sys.modules:
    sys.modules['gnpde_amd.graph_rewiring'].GDC_APPROX_DEFAULT = None
  merged = sorted(set(MERGES) | set(NATIVE_KNN) | set(NATIVE_GDC) | set(NATIVE_POSDIST))
  for name in list(MODULES) + list(NATIVE_GNN) + [FA_MODULE] + merged + ['_reference_' + m for m in merged]:
    m = sys.modules.get(name)
    if isinstance(m, types.ModuleType) and (getattr(m, '__name__', '').startswith('gnpde_amd') or
                                            hasattr(m, '__gnpde_reference__') or name.startswith('_reference_')):
      del sys.modules[name]


def main(argv=None):
  """python -m gnpde_amd.dropin [--native-gnn] [--native-knn] [--native-gdc] [--native-gdc-push] [--native-posdist] [--native-edge-sampling] SCRIPT [ARGS...]: install(), then run SCRIPT as __main__ (its directory goes
  to the front of sys.path, as `python SCRIPT` would put it)."""
  import runpy
  argv = list(sys.argv[1:] if argv is None else argv)
  native = False
  native_knn = False
  native_gdc = False
  native_gdc_push = False
  native_posdist = False
  native_edge_sampling = False
  while argv and argv[0].startswith('--'):
    flag = argv.pop(0)
    if flag == '--native-gnn':
      native = True
    elif flag == '--native-knn':
      native_knn = True
    elif flag == '--native-gdc':
      native_gdc = True
    elif flag == '--native-gdc-push':
      native_gdc_push = True
    elif flag == '--native-posdist':
      native_posdist = True
    elif flag == '--native-edge-sampling':
      native_edge_sampling = True
    else:
      raise SystemExit('gnpde_amd.dropin: unknown option %s\nusage: python -m gnpde_amd.dropin [--native-gnn] [--native-knn] [--native-gdc] [--native-gdc-push] [--native-posdist] [--native-edge-sampling] SCRIPT [ARGS...]' % flag)
  if not argv:
    raise SystemExit('usage: python -m gnpde_amd.dropin [--native-gnn] [--native-knn] [--native-gdc] [--native-gdc-push] [--native-posdist] [--native-edge-sampling] SCRIPT [ARGS...]')
  script = os.path.abspath(argv[0])
  if not os.path.isfile(script):
    raise SystemExit('gnpde_amd.dropin: no such script: %s' % argv[0])
  sys.path.insert(0, os.path.dirname(script))
  install(native_gnn=native, native_knn=native_knn, native_gdc=native_gdc, native_posdist=native_posdist,
          native_edge_sampling=native_edge_sampling, native_gdc_push=native_gdc_push)
  sys.argv = [script] + argv[1:]
  runpy.run_path(script, run_name='__main__')


if __name__ == '__main__':
  main()
