"""Replica populations without a GPU: the configuration and argument checks of
ddd_train_population_workspace_bytes / ddd_train_population_run, the workspace size, what
PopulationTrainer refuses and the learning-rate table it hands over."""
import ctypes

import pytest

from helpers import make_hparams, make_model
from test_cpu_training import _config
from ddd1d_amd import _lib, training

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2


def _args(num_steps=3, replicas=2, **fields):
  """ddd_train_population_args with fake (never dereferenced) device pointers: every case
  below fails on the host.  The learning rates [R][num_steps] are a real host array, kept
  alive on the struct."""
  args = _lib.DDDTrainPopulationArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDTrainPopulationArgs)
  args.batch = 4
  args.num_rows = 4
  args.num_time_steps = 0
  args.first_step = 0
  args.num_steps = num_steps
  args.replicas = replicas
  args.index_per_replica = 0
  args.time_step = 1e-3
  for name in ('weights', 'adam_m', 'adam_v', 'y', 'labels', 'baseline', 'sample_index',
               'head_means_log', 'workspace'):
    setattr(args, name, 0x1000)
  count = max(replicas, 1) * max(num_steps, 1)
  args.rates = (ctypes.c_double * count)(*([1e-3] * count))
  args.learning_rate = ctypes.cast(args.rates, ctypes.POINTER(ctypes.c_double))
  args.beta1, args.beta2, args.epsilon = 0.9, 0.99, 1e-8
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


def test_struct_layout():
  # ddd_train_run_args with two more int32 (replicas, index_per_replica) behind num_steps
  assert (ctypes.sizeof(_lib.DDDTrainPopulationArgs) ==
          ctypes.sizeof(_lib.DDDTrainRunArgs) + 8)
  assert _lib.DDDTrainPopulationArgs.replicas.offset == 24
  assert _lib.DDDTrainPopulationArgs.weights.offset == 32
  for name in ('learning_rate', 'error_max', 'time_step', 'workspace_bytes'):
    assert (getattr(_lib.DDDTrainPopulationArgs, name).offset ==
            getattr(_lib.DDDTrainRunArgs, name).offset + 8)
  assert _lib.MAX_REPLICAS == 64


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
def test_refusals_are_those_of_the_training_run(fields, text, steps):
  lib = _lib.load_library()
  cfg = _config(**fields)
  assert lib.ddd_train_run_workspace_bytes(ctypes.byref(cfg), 4, steps) == 0
  want = lib.ddd_last_error()
  assert text in want and want.startswith(b'training run: ')
  assert lib.ddd_train_population_workspace_bytes(ctypes.byref(cfg), 4, steps, 2) == 0
  got = lib.ddd_last_error()
  assert b'training population' in got and got.startswith(b'training population: ')
  assert got[len(b'training population: '):] == want[len(b'training run: '):]
  assert lib.ddd_train_population_run(ctypes.byref(cfg),
                                      ctypes.byref(_args(num_time_steps=steps)),
                                      None) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == got


def _bad_rates(index, value, count=6):
  rates = (ctypes.c_double * count)(*([1e-3] * count))
  rates[index] = value
  return rates


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(struct_size=ctypes.sizeof(_lib.DDDTrainRunArgs)), b'struct_size'),
    (dict(weights=None), b'NULL'),
    (dict(adam_m=None), b'NULL'),
    (dict(adam_v=None), b'NULL'),
    (dict(y=None), b'NULL'),
    (dict(labels=None), b'NULL'),
    (dict(baseline=None), b'NULL'),
    (dict(sample_index=None), b'NULL'),
    (dict(head_means_log=None), b'NULL'),
    (dict(learning_rate=ctypes.POINTER(ctypes.c_double)()), b'NULL'),
    (dict(replicas=0), b'replicas'),
    (dict(replicas=-1), b'replicas'),
    (dict(replicas=_lib.MAX_REPLICAS + 1), b'replicas'),
    (dict(index_per_replica=2), b'index_per_replica'),
    (dict(num_steps=0), b'num_steps'),
    (dict(first_step=-1), b'first_step'),
    (dict(batch=0), b'batch'),
    (dict(num_rows=0), b'num_rows'),
    # [R = 2][num_steps = 3]: entry 4 is replica 1, step 1
    (dict(rates=_bad_rates(4, float('nan'))), b'replica 1, step 1'),
    (dict(rates=_bad_rates(2, float('inf'))), b'replica 0, step 2'),
    (dict(rates=_bad_rates(3, -1e-3)), b'replica 1, step 0'),
    (dict(beta1=1.0), b'beta1'),
    (dict(beta2=float('nan')), b'beta2'),
    (dict(epsilon=0.0), b'epsilon'),
    (dict(error_max=-1.0), b'error_max'),
    (dict(num_time_steps=2, time_step=float('nan')), b'time_step'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
])
def test_argument_errors(fields, text):
  lib = _lib.load_library()
  args = _args(**fields)
  if 'rates' in fields:
    args.learning_rate = ctypes.cast(args.rates, ctypes.POINTER(ctypes.c_double))
  assert lib.ddd_train_population_run(ctypes.byref(_config()), ctypes.byref(args),
                                      None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


def test_the_largest_population_passes_the_replica_check():
  lib = _lib.load_library()
  args = _args(num_steps=1, replicas=_lib.MAX_REPLICAS, workspace_bytes=16)
  assert lib.ddd_train_population_run(ctypes.byref(_config()), ctypes.byref(args),
                                      None) == ERR_INVALID_ARGUMENT
  assert b'workspace' in lib.ddd_last_error()   # (the last check before the device work)


@pytest.mark.parametrize('steps', [0, 2])
def test_workspace_is_replicas_times_that_of_the_training_run(steps):
  lib = _lib.load_library()
  good = _config()
  for batch in (1, 6, 600):
    solo = lib.ddd_train_run_workspace_bytes(ctypes.byref(good), batch, steps)
    assert solo > 0
    for replicas in (1, 2, 5, _lib.MAX_REPLICAS):
      got = lib.ddd_train_population_workspace_bytes(ctypes.byref(good), batch, steps, replicas)
      assert got == replicas * solo
      assert got == lib.ddd_train_population_workspace_bytes(ctypes.byref(good), batch, steps,
                                                             replicas)
  for replicas in (0, _lib.MAX_REPLICAS + 1):
    assert lib.ddd_train_population_workspace_bytes(ctypes.byref(good), 6, steps, replicas) == 0
    assert b'replicas' in lib.ddd_last_error()
  bad = _config(kernel_size=9)
  assert lib.ddd_train_population_workspace_bytes(ctypes.byref(bad), 6, steps, 2) == 0
  assert b'training population: kernel_size' in lib.ddd_last_error()
  # a workspace one byte short of R solo workspaces is refused
  size = lib.ddd_train_population_workspace_bytes(ctypes.byref(good), 4, steps, 2)
  args = _args(num_time_steps=steps, workspace_bytes=size - 1)
  assert lib.ddd_train_population_run(ctypes.byref(good), ctypes.byref(args), None) == -1
  assert b'ddd_train_population_workspace_bytes' in lib.ddd_last_error()


def test_population_trainer_refuses_mixed_and_unsupported_models():
  burgers = make_model('burgers', conservative=False, num_points=32)
  hp = burgers.hparams
  with pytest.raises(ValueError, match='architecture'):
    training.PopulationTrainer(
        [burgers, make_model('burgers', conservative=False, num_points=32, filter_size=16)], hp)
  with pytest.raises(ValueError, match='architecture'):
    training.PopulationTrainer(
        [burgers, make_model('burgers', conservative=False, num_points=64)], hp)
  with pytest.raises(ValueError, match='equation'):
    training.PopulationTrainer(
        [burgers, make_model('burgers', conservative=True, num_points=32)], hp)
  with pytest.raises(ValueError, match='equation'):
    training.PopulationTrainer([burgers, make_model('kdv', conservative=False, num_points=32)],
                               hp)
  with pytest.raises(ValueError, match='models'):
    training.PopulationTrainer([], hp)
  with pytest.raises(ValueError, match='learning_rates'):
    training.PopulationTrainer([burgers, burgers], hp, learning_rates=[[1e-3, 1e-4]])
  for overrides, match in ((dict(numerical_flux=True), 'numerical_flux'),
                           (dict(model_target='flux'), 'flux'),
                           (dict(kernel_size=9), 'kernel_size'),
                           (dict(num_time_steps=_lib.MAX_TIME_STEPS + 1), 'num_time_steps')):
    with pytest.raises(NotImplementedError, match=match):
      training.PopulationTrainer([burgers, burgers], make_hparams('burgers', **overrides))


def test_learning_rate_table_follows_each_replicas_schedule():
  """learning_rates[r] replaces hparams.learning_rates on the same learning_stops, across a
  stop inside a run and across two runs.  (No device tensors: the object is put together
  by hand, as test_cpu_train_run does for Trainer.)"""
  import copy
  hp = make_hparams('burgers', conservative=False, num_points=32,
                    learning_rates=[1e-3, 1e-4], learning_stops=[3, 6])
  rows = [[1e-3, 1e-4], [5e-3, 5e-5], [2e-3, 2e-3]]
  trainer = training.PopulationTrainer.__new__(training.PopulationTrainer)
  trainer.hparams = hp
  trainer.replica_hparams = []
  for row in rows:
    replica = copy.copy(hp)
    replica.learning_rates = row
    trainer.replica_hparams.append(replica)
  trainer.step_count = 0
  # piecewise_constant: step <= 3 is the first piece
  want = [[row[0]] * 4 + [row[1]] * 2 for row in rows]
  assert trainer.learning_rate_table(6) == want
  trainer.step_count = 2
  assert trainer.learning_rate_table(4) == [row[2:] for row in want]
  # without per-replica rates every row is the schedule of hparams
  trainer.replica_hparams = [copy.copy(hp) for _ in rows]
  trainer.step_count = 0
  assert trainer.learning_rate_table(6) == [want[0]] * 3
  assert hp.learning_rates == [1e-3, 1e-4]
