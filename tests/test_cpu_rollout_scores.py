"""Rollout scores without a GPU: evaluation.max_error_thresholds against np.quantile, the
header / ctypes agreement and every refusal of ddd_rollout_reference / ddd_rollout_scores
(all before device work: the device pointers below are fake), and the host side of the
selection (select_replica's survival keys, rollout_metrics, training_population's
signature)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT
from ddd1d_amd import _lib, evaluation, training

ERR_INVALID_ARGUMENT = -1
QUANTILES = (0.5, 0.8, 0.9, 0.95)


# ---------------------------------------------------------------------------
# max_error_thresholds
# ---------------------------------------------------------------------------
def _values(size, seed):
  rs = np.random.RandomState(seed)
  return rs.standard_normal(size) * rs.lognormal(0.0, 2.0, size)


@pytest.mark.parametrize('size', [5, 17, 4097])
def test_thresholds_equal_numpy_quantile(size):
  y = _values(size, size)
  got = evaluation.max_error_thresholds(torch.from_numpy(y), QUANTILES)
  assert got.dtype == np.float64 and got.shape == (len(QUANTILES),)
  for value, q in zip(got, QUANTILES):
    assert value == float(np.quantile(np.abs(y), 1 - q)), (size, q)
  # a [sample, time, x] array is scored as a whole, and NumPy input is taken too
  cube = _values(2 * 3 * 40, 7).reshape(2, 3, 40)
  got = evaluation.max_error_thresholds(cube, QUANTILES)
  for value, q in zip(got, QUANTILES):
    assert value == float(np.quantile(np.abs(cube), 1 - q))


def test_thresholds_with_ties_and_float32():
  ties = np.round(_values(257, 3) * 2.0) / 2.0   # many equal magnitudes, zeros included
  assert len(np.unique(np.abs(ties))) < ties.size // 2
  got = evaluation.max_error_thresholds(torch.from_numpy(ties), QUANTILES)
  for value, q in zip(got, QUANTILES):
    assert value == float(np.quantile(np.abs(ties), 1 - q))
  single = _values(1001, 4).astype(np.float32)
  got = evaluation.max_error_thresholds(torch.from_numpy(single), QUANTILES)
  for value, q in zip(got, QUANTILES):
    assert value == float(np.quantile(np.abs(single), 1 - q)), q


def test_thresholds_refuse_nan():
  y = _values(64, 5)
  y[17] = np.nan
  with pytest.raises(ValueError, match='NaN'):
    evaluation.max_error_thresholds(torch.from_numpy(y), (0.8,))


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def test_header_signatures_and_struct_layout():
  with open(os.path.join(ROOT, 'include', 'ddd1d.h')) as f:
    header = f.read()
  declared = set(re.findall(r'DDD_API\s+[\w\s\*]+?\b(ddd_\w+)\s*\(', header))
  lib = _lib.load_library()
  for name in ('ddd_rollout_reference', 'ddd_rollout_scores_workspace_bytes',
               'ddd_rollout_scores'):
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
  for name, value in (('QUANTILES', 8), ('STOP_TIMES', 16), ('POINTS', 1024), ('FACTOR', 128)):
    assert '#define DDD_ROLLOUT_MAX_{} {}'.format(name, value) in header
    assert getattr(_lib, 'ROLLOUT_MAX_' + name) == value
  # five int32 (padded to 24), two pointers
  ref = _lib.DDDRolloutReferenceArgs
  assert ctypes.sizeof(ref) == 40
  assert [getattr(ref, n).offset for n, _ in ref._fields_] == [0, 4, 8, 12, 16, 24, 32]
  # eight int32, eleven pointers, one size_t
  scores = _lib.DDDRolloutScoresArgs
  assert ctypes.sizeof(scores) == 32 + 12 * 8
  assert ([getattr(scores, n).offset for n, _ in scores._fields_] ==
          [4 * i for i in range(8)] + [32 + 8 * i for i in range(12)])


def _reference_args(**fields):
  args = _lib.DDDRolloutReferenceArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDRolloutReferenceArgs)
  args.num_samples, args.num_times, args.num_points_exact, args.num_points = 3, 2, 64, 8
  args.y_exact = args.exact_low = 0x1000
  for name, value in fields.items():
    setattr(args, name, value)
  return args


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(y_exact=None), b'NULL'),
    (dict(exact_low=None), b'NULL'),
    (dict(num_samples=0), b'num_samples'),
    (dict(num_times=0), b'num_times'),
    (dict(num_points=0), b'num_points'),
    (dict(num_points=1025, num_points_exact=1025), b'num_points'),
    (dict(num_points_exact=60), b'multiple'),
    (dict(num_points_exact=4), b'multiple'),
    (dict(num_points_exact=8 * 129), b'129'),
])
def test_reference_refusals(fields, text):
  lib = _lib.load_library()
  assert lib.ddd_rollout_reference(ctypes.byref(_reference_args(**fields)),
                                   None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()
  assert lib.ddd_rollout_reference(None, None) == ERR_INVALID_ARGUMENT


class _ScoreArgs(object):
  """ddd_rollout_scores_args with real host arrays and fake device pointers."""

  def __init__(self, time_values=(0.0, 0.5, 1.0), quantiles=3, stops=4, **fields):
    self.host = [np.asarray(time_values, np.float64), np.full(max(quantiles, 1), 0.5),
                 np.full(max(quantiles, 1), 0.8), np.arange(1.0, max(stops, 1) + 1.0)]
    args = _lib.DDDRolloutScoresArgs()
    args.struct_size = ctypes.sizeof(_lib.DDDRolloutScoresArgs)
    args.replicas, args.num_times, args.num_samples, args.num_points = 2, len(time_values), 5, 8
    args.num_quantiles, args.num_stop_times, args.dtype = quantiles, stops, _lib.ROLLOUT_F64
    for name, array in zip(('times', 'max_error', 'frac_good', 'stop_times'), self.host):
      setattr(args, name, array.ctypes.data)
    for name in ('y_model', 'exact_low', 'mae', 'survival', 'workspace'):
      setattr(args, name, 0x1000)
    args.workspace_bytes = 1 << 40
    for name, value in fields.items():
      setattr(args, name, value)
    self.args = args


@pytest.mark.parametrize('kwargs,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(struct_size=ctypes.sizeof(_lib.DDDRolloutReferenceArgs)), b'struct_size'),
    (dict(y_model=None), b'NULL'),
    (dict(exact_low=None), b'NULL'),
    (dict(mae=None), b'NULL'),
    (dict(survival=None), b'NULL'),
    (dict(times=None), b'NULL'),
    (dict(max_error=None), b'NULL'),
    (dict(frac_good=None), b'NULL'),
    (dict(stop_times=None), b'NULL'),
    (dict(replicas=0), b'replicas'),
    (dict(replicas=_lib.MAX_REPLICAS + 1), b'replicas'),
    (dict(num_samples=0), b'num_samples'),
    (dict(num_points=0), b'num_points'),
    (dict(num_points=1025), b'num_points'),
    (dict(quantiles=9), b'num_quantiles'),
    (dict(quantiles=0), b'num_quantiles'),
    (dict(stops=17), b'num_stop_times'),
    (dict(stops=0), b'num_stop_times'),
    (dict(time_values=(0.0, 0.5, 0.5)), b'strictly increasing'),
    (dict(time_values=(0.0, 1.0, 0.5)), b'strictly increasing'),
    (dict(time_values=(0.0, np.nan, 1.0)), b'strictly increasing'),
    (dict(time_values=(0.0, 1.0, np.inf)), b'finite'),
    (dict(dtype=2), b'dtype'),
    (dict(workspace=None), b'ddd_rollout_scores_workspace_bytes'),
    (dict(workspace_bytes=8), b'ddd_rollout_scores_workspace_bytes'),
])
def test_scores_refusals(kwargs, text):
  lib = _lib.load_library()
  held = _ScoreArgs(**kwargs)
  assert lib.ddd_rollout_scores(ctypes.byref(held.args), None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()
  assert lib.ddd_rollout_scores(None, None) == ERR_INVALID_ARGUMENT


def test_workspace_bytes():
  lib = _lib.load_library()
  size = lib.ddd_rollout_scores_workspace_bytes
  # the row sums, the flags padded to eight bytes, the times
  assert size(2, 3, 5, 3) == 2 * 3 * 5 * 8 + 96 + 3 * 8
  assert size(1, 1, 1, 1) == 8 + 8 + 8
  assert size(_lib.MAX_REPLICAS, 3, 5, 8) > 0
  for bad in ((0, 3, 5, 3), (_lib.MAX_REPLICAS + 1, 3, 5, 3), (2, 0, 5, 3), (2, 3, 0, 3),
              (2, 3, 5, 0), (2, 3, 5, 9)):
    assert size(*bad) == 0, bad
  assert b'num_quantiles' in lib.ddd_last_error()
  # exactly that many bytes are enough for the checks: one fewer is refused
  held = _ScoreArgs(workspace_bytes=size(2, 3, 5, 3) - 1)
  assert lib.ddd_rollout_scores(ctypes.byref(held.args), None) == ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------
def _rows(key, values):
  return [[{'step': 0, key: 0.0}, {'step': 2, key: value}] for value in values]


def test_select_replica_survival_keys_pick_the_largest():
  assert training.select_replica(_rows('rollout_survival/0.8', [1.0, 3.5, 2.0]),
                                 'rollout_survival/0.8') == (1, 3.5)
  assert training.select_replica(_rows('rollout_survival/0.8', [np.nan, 0.5, 0.25]),
                                 'rollout_survival/0.8') == (1, 0.5)
  assert training.select_replica(_rows('rollout_survival/0.9', [2.0, 2.0]),
                                 'rollout_survival/0.9') == (0, 2.0)
  # the rollout error is an error: the smallest wins, NaN never
  assert training.select_replica(_rows('rollout_mae/10', [np.nan, 0.3, 0.2]),
                                 'rollout_mae/10') == (2, 0.2)
  # ... and the keys from before keep their sense
  assert training.select_replica(_rows('loss', [0.3, 0.1, np.nan]), 'loss') == (1, 0.1)
  assert training.select_replica(_rows('test_frac_below_baseline/u_t', [0.3, 0.9, np.nan]),
                                 'test_frac_below_baseline/u_t') == (1, 0.9)
  assert training.select_replica(_rows('test_mae/u_t', [0.3, 0.9, 0.2]),
                                 'test_mae/u_t') == (2, 0.2)
  with pytest.raises(KeyError):
    training.select_replica(_rows('loss', [0.3]), 'rollout_survival/0.8')


def test_rollout_metrics():
  result = dict(
      mae=np.array([[[1.0, 3.0], [2.0, 6.0]], [[0.5, np.nan], [1.0, 1.0]]]),   # [R][K][S]
      survival=np.array([[[10.0, 20.0]], [[5.0, 6.0]]]),                         # [R][Q][S]
      stop_times=np.array([5, 10]), quantiles=np.array([0.8]))
  rows = training.rollout_metrics(result)
  assert len(rows) == 2
  assert rows[0] == {'rollout_mae/5': 2.0, 'rollout_mae/10': 4.0, 'rollout_survival/0.8': 15.0}
  assert np.isnan(rows[1]['rollout_mae/5']) and rows[1]['rollout_mae/10'] == 1.0
  assert rows[1]['rollout_survival/0.8'] == 5.5
  assert all(isinstance(v, float) for row in rows for v in row.values())
  # the keys a default RolloutReference gives
  default = dict(mae=np.zeros((1, 4, 1)), survival=np.zeros((1, 3, 1)),
                 stop_times=np.asarray((5, 10, 20, 40)), quantiles=np.asarray((0.8, 0.9, 0.95)))
  assert sorted(training.rollout_metrics(default)[0]) == sorted(
      ['rollout_mae/5', 'rollout_mae/10', 'rollout_mae/20', 'rollout_mae/40',
       'rollout_survival/0.8', 'rollout_survival/0.9', 'rollout_survival/0.95'])


def test_signatures():
  assert inspect.signature(training.training_population).parameters['rollout'].default is None
  params = inspect.signature(evaluation.run_integrate_population).parameters
  assert [params[n].default for n in ('warmup', 'max_step', 'scheme', 'adaptive', 'first_seed')
          ] == [0, 0.01, 'bs3', None, 0]
  assert params['streams'].default in (1, 4)
  from ddd1d_amd import model as model_lib
  for name in ('integrate_adaptive', 'integrate_fixed'):
    method = getattr(model_lib._DeviceModel, name)
    assert inspect.signature(method).parameters['out'].default is None
