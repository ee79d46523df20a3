"""Evaluation metrics without a GPU: the header / ctypes agreement and the configuration and
argument checks of ddd_eval_metrics, the host functions (calculate_metrics,
metrics_from_sums, metrics_one_linear, metrics_to_dataframe) against the committed output of
the reference's own (tests/golden/reference_metrics.npz, written by
tests/golden/make_golden_metrics.py), and the row / selection logic of training_loop and
training_population with the device calls replaced."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from helpers import ROOT, make_hparams
from test_cpu_training import _config
from ddd1d_amd import _lib, equations, model as model_lib, training

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'reference_metrics.npz')


def _args(**fields):
  """ddd_eval_metrics_args with fake (never dereferenced) device pointers: every case below
  fails on the host."""
  args = _lib.DDDEvalMetricsArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDEvalMetricsArgs)
  args.rows_evaluated = 4
  args.num_rows = 4
  args.num_time_steps = 0
  args.replicas = 2
  args.index_per_replica = 0
  args.time_step = 1e-3
  for name in ('weights', 'y', 'labels', 'baseline', 'sums', 'below', 'workspace'):
    setattr(args, name, 0x1000)
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


def test_header_export_map_and_signatures_agree():
  with open(os.path.join(ROOT, 'include', 'ddd1d.h')) as f:
    header = f.read()
  declared = set(re.findall(r'DDD_API\s+[\w\s\*]+?\b(ddd_\w+)\s*\(', header))
  for name in ('ddd_eval_metrics_workspace_bytes', 'ddd_eval_metrics'):
    assert name in declared and name in _lib.SIGNATURES
  assert declared == set(_lib.SIGNATURES)
  with open(os.path.join(ROOT, 'data-driven-discretization-1d_amd', 'csrc', 'exports.map')) as f:
    assert 'ddd_*' in f.read()   # every ddd_ symbol is exported, nothing else
  lib = _lib.load_library()
  assert hasattr(lib, 'ddd_eval_metrics') and hasattr(lib, 'ddd_eval_metrics_workspace_bytes')
  with open(os.path.join(ROOT, 'README.md')) as f:
    assert '{} `ddd_*` functions'.format(len(declared)) in f.read()
  # the struct: six int32, seven pointers, three float [H'] rows and time_step, five pointers
  # / sizes; ctypes and the C compiler pad alike (struct_size is checked by the library)
  assert _lib.DDDEvalMetricsArgs.weights.offset == 24
  heads = _lib.MAX_UNROLLED_HEADS
  assert _lib.DDDEvalMetricsArgs.time_step.offset == 24 + 7 * 8 + 3 * 4 * heads
  assert _lib.METRIC_SUMS == 7


@pytest.mark.parametrize('fields,text', [
    (dict(equation=6, num_derivatives=3), b'Godunov'),
    (dict(model_target=3), b'flux'),
    (dict(num_layers=0), b'num_layers'),
    (dict(kernel_size=9), b'kernel_size'),
    (dict(filter_size=65), b'filter_size'),
    (dict(num_points=4), b'num_points'),
    (dict(num_points=512), b'num_points'),
])
@pytest.mark.parametrize('steps', [0, 2])
def test_refusals_are_those_of_training(fields, text, steps):
  lib = _lib.load_library()
  cfg = _config(**fields)
  if steps:
    assert lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(cfg), 4, steps) == 0
  else:
    assert lib.ddd_train_workspace_bytes(ctypes.byref(cfg), 4) == 0
  want = lib.ddd_last_error()
  assert text in want and want.startswith(b'training: ')
  assert lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(cfg), 4, steps, 2) == 0
  got = lib.ddd_last_error()
  assert got.startswith(b'evaluation metrics: ')
  assert got[len(b'evaluation metrics: '):] == want[len(b'training: '):]
  assert lib.ddd_eval_metrics(ctypes.byref(cfg), ctypes.byref(_args(num_time_steps=steps)),
                              None) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == got


@pytest.mark.parametrize('steps', [0, 2])
def test_workspace_bytes(steps):
  lib = _lib.load_library()
  good = _config()
  one = lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 6, steps, 1)
  assert one > 0
  for replicas in (2, 5, _lib.MAX_REPLICAS):
    assert (lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 6, steps, replicas) ==
            replicas * one)
  # no gradient part: smaller than the forward-only parent's workspace
  parent = (lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 6, steps) if steps
            else lib.ddd_train_workspace_bytes(ctypes.byref(good), 6))
  assert one < parent
  # the workgroups stop at 512: 515 rows need no more than 512
  assert (lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 515, steps, 1) ==
          lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 512, steps, 1))
  for replicas in (0, _lib.MAX_REPLICAS + 1):
    assert lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 6, steps, replicas) == 0
    assert b'replicas' in lib.ddd_last_error()
  assert lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 0, steps, 1) == 0
  assert lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 6, -1, 1) == 0
  assert lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 6, _lib.MAX_TIME_STEPS + 1,
                                              1) == 0
  size = lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(good), 4, steps, 2)
  args = _args(num_time_steps=steps, workspace_bytes=size - 1)
  assert lib.ddd_eval_metrics(ctypes.byref(good), ctypes.byref(args), None) == -1
  assert b'ddd_eval_metrics_workspace_bytes' in lib.ddd_last_error()


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(struct_size=ctypes.sizeof(_lib.DDDTrainPopulationArgs)), b'struct_size'),
    (dict(weights=None), b'NULL'),
    (dict(y=None), b'NULL'),
    (dict(labels=None), b'NULL'),
    (dict(baseline=None), b'NULL'),
    (dict(sums=None), b'NULL'),
    (dict(below=None), b'NULL'),
    (dict(replicas=0), b'replicas'),
    (dict(replicas=_lib.MAX_REPLICAS + 1), b'replicas'),
    (dict(index_per_replica=2), b'index_per_replica'),
    (dict(index_per_replica=1), b'sample_index'),
    (dict(rows_evaluated=0), b'batch'),
    (dict(rows_evaluated=5), b'rows_evaluated'),
    (dict(num_rows=0), b'num_rows'),
    (dict(num_time_steps=-1), b'num_time_steps'),
    (dict(num_time_steps=2, time_step=float('nan')), b'time_step'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
])
def test_argument_errors(fields, text):
  lib = _lib.load_library()
  assert lib.ddd_eval_metrics(ctypes.byref(_config()), ctypes.byref(_args(**fields)),
                              None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()
  assert lib.ddd_eval_metrics(ctypes.byref(_config()), None, None) == ERR_INVALID_ARGUMENT


# ---- the host functions against the reference's own output ---------------------------------
def _golden_cases():
  with np.load(GOLDEN) as z:
    for i in range(int(z['num_cases'])):
      prefix = 'case{}_'.format(i)
      yield {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def _data_of(case):
  data = {k: case[k] for k in ('labels', 'baseline', 'predictions')}
  data.update(zip((str(k) for k in case['loss_keys']), case['loss_values']))
  return data


def test_fixture_shapes():
  cases = list(_golden_cases())
  assert [c['labels'].shape[-1] for c in cases] == [3, 4, 6]
  assert 'mae/u(t)' in [str(k) for k in cases[2]['keys']]
  assert 'mae/u(t)' not in [str(k) for k in cases[1]['keys']]


def test_calculate_metrics_reproduces_the_reference():
  for case in _golden_cases():
    equation_type = getattr(equations, str(case['equation']))
    got = training.calculate_metrics(_data_of(case), equation_type)
    keys = [str(k) for k in case['keys']]
    assert sorted(got) == keys
    assert isinstance(got['count'], int) and got['count'] == len(case['labels'])
    np.testing.assert_allclose([got[k] for k in keys], case['values'], rtol=1e-12, atol=0)
    assert training.metrics_one_linear(got) == str(case['one_line'])


def test_metrics_from_sums_equals_calculate_metrics():
  for case in _golden_cases():
    equation_type = getattr(equations, str(case['equation']))
    data = _data_of(case)
    want = training.calculate_metrics(data, equation_type)
    l, b, p = (np.asarray(data[k], np.float64) for k in ('labels', 'baseline', 'predictions'))
    over = (0, 1)
    sums = np.zeros((7, l.shape[-1]))
    sums[2] = np.abs(l - p).sum(over)
    sums[3] = np.abs(l - b).sum(over)
    sums[4] = ((l - p) ** 2).sum(over)
    sums[5] = ((l - b) ** 2).sum(over)
    sums[6] = (np.log(np.maximum(np.abs(l - p), 1e-8)) -
               np.log(np.maximum(np.abs(l - b), 1e-8))).sum(over)
    below = ((l - p) ** 2 < (l - b) ** 2).sum(over)
    losses = {k: v for k, v in data.items() if 'loss' in k}
    got = training.metrics_from_sums(sums, below, l.shape[0], l.shape[1], equation_type, losses)
    assert sorted(got) == sorted(want)
    for key in want:
      np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, err_msg=key)


def test_metrics_to_dataframe_and_loss_metrics():
  frame = training.metrics_to_dataframe([(9, {'loss': 1.0, 'mae/u_t': 0.5}, {'loss': 2.0}),
                                         (19, {'loss': 0.5, 'mae/u_t': 0.4}, {'loss': 1.0})])
  assert sorted(frame.columns) == ['step', 'test_loss', 'test_mae/u_t', 'train_loss']
  assert frame['step'].tolist() == [9, 19] and frame['test_mae/u_t'].tolist() == [0.5, 0.4]
  hp = make_hparams('burgers', conservative=False, num_points=32, num_time_steps=2)
  per_head = np.arange(10, dtype=np.float64).reshape(2, 5)
  got = training.loss_metrics(per_head, hp, equations.equation_type_from_hparams(hp))
  assert got['loss'] == float(model_lib.weighted_loss(per_head, hp))
  assert got['loss/space_derivatives'] == np.mean([0, 1, 5, 6])
  assert got['loss/time_derivative'] == np.mean([2, 7])
  assert got['loss/integrated_solution'] == np.mean([3, 4, 8, 9])


# ---- training_loop / training_population with the device calls replaced --------------------
class _FakeData(object):
  def __init__(self, examples):
    import torch
    self.inputs = torch.zeros(examples, 32)
    self.labels = torch.zeros(examples, 32, 3)
    self.baseline = torch.zeros(examples, 32, 3)

  @property
  def num_examples(self):
    return int(self.inputs.shape[0])

  def batch_indices(self):
    import torch
    while True:
      yield torch.zeros(4, dtype=torch.int32)


class _FakeModel(object):
  def save(self, checkpoint_dir):
    with open(os.path.join(checkpoint_dir, 'saved'), 'w') as f:
      f.write('x')


def _fabricated(replica, step, split):
  """Metrics of a replica that improves with its index (and with the steps)."""
  value = 1.0 / (1 + replica) / (1 + step) + (0.25 if split == 'train' else 0.0)
  return {'count': 7, 'loss': value, 'loss/space_derivatives': value,
          'loss/time_derivative': value, 'mae/u_t': value, 'mae/u_x': 2 * value,
          'frac_below_baseline/u_t': 1.0 - value}


@pytest.fixture
def patched(monkeypatch):
  import torch

  class FakeTrainer(object):
    def __init__(self, model, hparams):
      self.hparams, self.torch, self.steps = hparams, torch, 0

    def loss_and_grad(self, data, want_grad=True):
      return np.full((2, 3), 1.0 / (1 + self.steps)), None, None

    def step(self, data, index):
      self.steps += 1

    def run(self, data, num_steps, index):
      self.steps += num_steps

    def export(self):
      return _FakeModel()

  class FakePopulation(object):
    def __init__(self, models, hparams, learning_rates=None):
      self.hparams, self.torch, self.steps, self.models = hparams, torch, 0, list(models)

    def loss(self, data):
      return np.stack([np.full((2, 3), 1.0 / (1 + r) / (1 + self.steps))
                       for r in range(len(self.models))])

    def run(self, data, num_steps, index):
      self.steps += num_steps

    def export(self):
      return [_FakeModel() for _ in self.models]

  class FakeInferer(object):
    splits = []

    def __init__(self, dataset, trainer):
      self.trainer = trainer
      self.split = 'test' if len(FakeInferer.splits) % 2 == 0 else 'train'
      FakeInferer.splits.append(dataset)

    def run_async(self):
      return self.trainer.steps, None, None

    def metrics(self, steps, below):
      replicas = len(getattr(self.trainer, 'models', [None]))
      return [_fabricated(r, steps, self.split) for r in range(replicas)]

  def fake_set(hparams, snapshots, seed=0):
    hparams.error_scale = [1.0] * 6
    hparams.error_floor = [1e-3] * 3
    return _FakeData(12)

  monkeypatch.setattr(training, 'set_data_dependent_hparams', fake_set)
  monkeypatch.setattr(model_lib, 'make_dataset',
                      lambda *a, **k: _FakeData(7 if a[2] is model_lib.Dataset.VALIDATION else 5))
  monkeypatch.setattr(model_lib, 'LearnedStencilModel', lambda *a, **k: object())
  monkeypatch.setattr(training, 'Trainer', FakeTrainer)
  monkeypatch.setattr(training, 'PopulationTrainer', FakePopulation)
  monkeypatch.setattr(training, 'Inferer', FakeInferer)
  return FakeInferer


def _hp():
  return make_hparams('burgers', conservative=False, num_points=32, eval_interval=2,
                      learning_rates=[1e-3], learning_stops=[4])


@pytest.mark.parametrize('fused', [False, True])
def test_training_loop_rows(patched, tmp_path, fused):
  rows = training.training_loop(np.zeros((4, 128)), str(tmp_path / 'a'), _hp(), fused=fused)
  assert [row['step'] for row in rows] == [0, 2, 4]
  for row in rows:
    assert sorted(row) == ['loss', 'loss_per_head', 'step']   # today's keys, nothing more
  assert not patched.splits   # no Inferer without metrics
  rows = training.training_loop(np.zeros((4, 128)), str(tmp_path / 'b'), _hp(), fused=fused,
                                metrics=True)
  assert [d.num_examples for d in patched.splits[-2:]] == [7, 5]   # validation, training
  assert [row['step'] for row in rows] == [0, 2, 4]
  for k, row in enumerate(rows):
    want = training._metrics_row(row['step'], _fabricated(0, 2 * k, 'test'),
                                 _fabricated(0, 2 * k, 'train'))
    assert {key: row[key] for key in want} == want
    assert sorted(row) == sorted(set(want) | {'loss', 'loss_per_head'})
  frame = training.metrics_to_dataframe(
      [(row['step'], {k[5:]: v for k, v in row.items() if k.startswith('test_')},
        {k[6:]: v for k, v in row.items() if k.startswith('train_')}) for row in rows])
  assert frame['test_mae/u_t'].tolist() == [row['test_mae/u_t'] for row in rows]


def test_training_population_rows_and_selection(patched, tmp_path):
  dirs = [str(tmp_path / 'pop' / 'r{}'.format(r)) for r in range(3)]
  snapshots = np.zeros((4, 128))
  rows = training.training_population(snapshots, dirs, _hp(), [0, 1, 2])
  assert len(rows) == 3 and not patched.splits
  for replica_rows in rows:
    assert [row['step'] for row in replica_rows] == [0, 2, 4]
    for row in replica_rows:
      assert sorted(row) == ['loss', 'loss_per_head', 'step']
  assert not os.path.exists(str(tmp_path / 'pop' / 'best.json'))
  # select on the loss needs no metrics: replica 2 has the smallest
  rows, best = training.training_population(snapshots, dirs, _hp(), [0, 1, 2], select='loss')
  assert best == 2
  with open(str(tmp_path / 'pop' / 'best.json')) as f:
    saved = json.load(f)
  assert saved == {'replica': 2, 'key': 'loss', 'value': rows[2][-1]['loss'],
                   'checkpoint_dir': dirs[2]}
  with pytest.raises(KeyError, match='test_mae/u_t'):
    training.training_population(snapshots, dirs, _hp(), [0, 1, 2], select='test_mae/u_t')
  rows, best = training.training_population(snapshots, dirs, _hp(), [0, 1, 2], metrics=True,
                                            select='test_mae/u_t')
  assert best == 2 and len(patched.splits) == 2   # two Inferers for all replicas
  for r, replica_rows in enumerate(rows):
    for k, row in enumerate(replica_rows):
      assert row['test_mae/u_t'] == _fabricated(r, 2 * k, 'test')['mae/u_t']
      assert row['train_mae/u_x'] == _fabricated(r, 2 * k, 'train')['mae/u_x']
  with open(str(tmp_path / 'pop' / 'best.json')) as f:
    assert json.load(f)['key'] == 'test_mae/u_t'


def test_select_replica():
  rows = [[{'loss': 9.0}, {'loss': 0.3, 'test_frac_below_baseline/u_t': 0.5}],
          [{'loss': 0.1}, {'loss': float('nan'), 'test_frac_below_baseline/u_t': 0.9}],
          [{'loss': 5.0}, {'loss': 0.3, 'test_frac_below_baseline/u_t': float('nan')}]]
  assert training.select_replica(rows, 'loss') == (0, 0.3)   # last rows; NaN loses; first tie
  assert training.select_replica(rows, 'test_frac_below_baseline/u_t') == (1, 0.9)   # larger
  with pytest.raises(KeyError):
    training.select_replica(rows, 'test_mae/u_t')
