"""Population rollouts without a GPU: the four ddd_population_* entry points in the header,
the ctypes table and the library's exports, the refusals of ddd_population_create and of
the integrate entry points that come before any device work, and the ``launch`` keyword of
run_integrate_population."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from ddd1d_amd import _lib, evaluation, training

ERR_INVALID_ARGUMENT = -1
NAMES = ('ddd_population_create', 'ddd_population_destroy',
         'ddd_population_integrate_adaptive_f64', 'ddd_population_integrate_fixed')


def test_names_in_header_ctypes_table_and_exports():
  with open(os.path.join(ROOT, 'include', 'ddd1d.h')) as f:
    header = f.read()
  declared = set(re.findall(r'DDD_API\s+[\w\s\*]+?\b(ddd_\w+)\s*\(', header))
  lib = _lib.load_library()
  for name in NAMES:
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
  assert 'typedef struct ddd_population ddd_population;' in header
  assert lib.ddd_abi_version() == 1
  assert _lib.MAX_REPLICAS == int(re.search(r'#define DDD_MAX_REPLICAS (\d+)', header).group(1))


def _create(models, replicas, out):
  lib = _lib.load_library()
  status = lib.ddd_population_create(models, replicas, out)
  return status, lib.ddd_last_error()


def test_create_refuses_bad_arguments_before_device_work():
  handles = (ctypes.c_void_p * 2)(0x1000, 0x2000)   # (fake: never dereferenced below)
  out = ctypes.c_void_p(0x3000)
  status, text = _create(None, 2, ctypes.byref(out))
  assert status == ERR_INVALID_ARGUMENT and b'models' in text
  assert out.value is None   # cleared before anything else
  status, text = _create(handles, 2, None)
  assert status == ERR_INVALID_ARGUMENT and b'out' in text
  for replicas in (0, -1, _lib.MAX_REPLICAS + 1):
    status, text = _create(handles, replicas, ctypes.byref(out))
    assert status == ERR_INVALID_ARGUMENT and b'replicas' in text, replicas
  null_entry = (ctypes.c_void_p * 2)(None, None)
  status, text = _create(null_entry, 2, ctypes.byref(out))
  assert status == ERR_INVALID_ARGUMENT and b'models[0]' in text
  assert _lib.load_library().ddd_population_destroy(None) == 0


def test_integrate_entry_points_refuse_a_null_population():
  lib = _lib.load_library()
  times = np.array([0.0, 0.1])
  status = lib.ddd_population_integrate_adaptive_f64(
      None, times.ctypes.data_as(_lib._D), 2, 1e-3, 1e-6, 0.01, 0, 0x1000, 0x1000, 0x1000,
      0x1000, 1, None)
  assert status == ERR_INVALID_ARGUMENT and b'population' in lib.ddd_last_error()
  status = lib.ddd_population_integrate_fixed(None, _lib.SCHEMES['midpoint'], 0.0, 1e-3, 2, 1,
                                              0x1000, 0x1000, 1, None)
  assert status == ERR_INVALID_ARGUMENT and b'population' in lib.ddd_last_error()


def test_launch_keyword():
  parameters = inspect.signature(evaluation.run_integrate_population).parameters
  assert parameters['launch'].default == 'streams'
  assert evaluation.LAUNCHES == ('streams', 'population', 'auto')
  # refused before any device work: neither a device nor a model is needed to get here
  with pytest.raises(ValueError, match='launch'):
    evaluation.run_integrate_population([], None, np.zeros((1, 8)), np.array([0.0, 0.1]),
                                        launch='one_launch')
  assert inspect.signature(training.training_population).parameters[
      'rollout_launch'].default == 'streams'
