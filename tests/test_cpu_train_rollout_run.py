"""Rollout fine-tuning on the device without a GPU: the configuration and argument checks of
ddd_train_rollout_run_workspace_bytes / ddd_train_rollout_run through ctypes with a NULL
stream (every call returns before any device work), the workspace size, and what
RolloutPopulationTrainer refuses."""
import ctypes

import pytest

from helpers import make_hparams, make_model
from test_cpu_training import _config
from test_cpu_train_rollout import FORCING, UNSUPPORTED
from ddd1d_amd import _lib, training

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2
WHO = b'ddd_train_rollout_run'
REPLICAS, OPT_STEPS = 2, 3


def _args(**fields):
  """ddd_train_rollout_run_args with fake (never dereferenced) device pointers and a real
  host table of learning rates: every case below fails on the host.  learning_rate: the
  [R][K] values (default 1e-3 each)."""
  args = _lib.DDDTrainRolloutRunArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDTrainRolloutRunArgs)
  args.batch = 4
  args.num_rows = 4
  args.num_steps = 6
  args.save_every = 2
  args.num_opt_steps = OPT_STEPS
  args.replicas = REPLICAS
  args.dt = 1e-3
  for name in ('weights', 'adam_m', 'adam_v', 'adam_step', 'y0', 'targets', 'step_weights',
               'sample_index', 'step_means_log', 'grad_norm_log', 'workspace'):
    setattr(args, name, 0x1000)
  args.beta1, args.beta2, args.epsilon = 0.9, 0.99, 1e-8
  args.workspace_bytes = 1 << 40
  rates = fields.pop('learning_rate', [1e-3] * (_lib.MAX_REPLICAS * OPT_STEPS))
  if rates is not None:
    table = (ctypes.c_double * len(rates))(*rates)
    args.learning_rate = ctypes.cast(table, ctypes.POINTER(ctypes.c_double))
    args._keep = table
  for name, value in fields.items():
    setattr(args, name, value)
  return args


def _call(lib, cfg, args):
  return lib.ddd_train_rollout_run(ctypes.byref(cfg), ctypes.byref(args), None)


def test_struct_layout():
  # nine int32 (+ 4 bytes of padding), nine pointers, dt, t0, two int32, seven pointers,
  # four doubles, four pointers, size_t
  assert ctypes.sizeof(_lib.DDDTrainRolloutRunArgs) == (
      40 + 9 * 8 + 8 + 8 + 8 + 7 * 8 + 4 * 8 + 4 * 8 + 8)
  assert _lib.DDDTrainRolloutRunArgs.weights.offset == 40
  assert _lib.DDDTrainRolloutRunArgs.dt.offset == 40 + 9 * 8


def test_a_good_call_reaches_the_workspace_check_last():
  """Every argument of _args() is accepted: with the workspace one byte short, that is what
  the call names (the checks come before any device work)."""
  lib = _lib.load_library()
  good = _config()
  size = lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(good), 4, 6, REPLICAS)
  assert size > 0
  assert _call(lib, good, _args(workspace_bytes=size - 1)) == ERR_INVALID_ARGUMENT
  assert b'ddd_train_rollout_run_workspace_bytes' in lib.ddd_last_error()
  assert _call(lib, good, _args(**dict(FORCING, workspace_bytes=size - 1))) == ERR_INVALID_ARGUMENT
  assert b'ddd_train_rollout_run_workspace_bytes' in lib.ddd_last_error()
  forward = _args(forward_only=1, num_opt_steps=1, sample_index=None, learning_rate=None,
                  adam_m=None, adam_v=None, adam_step=None, grad_norm_log=None,
                  workspace_bytes=size - 1)
  assert _call(lib, good, forward) == ERR_INVALID_ARGUMENT
  assert b'ddd_train_rollout_run_workspace_bytes' in lib.ddd_last_error()


def _rates_with(value, replica=1, step=2):
  rates = [1e-3] * (REPLICAS * OPT_STEPS)
  rates[replica * OPT_STEPS + step] = value
  return rates


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(replicas=0), b'replicas'),
    (dict(replicas=_lib.MAX_REPLICAS + 1), b'replicas'),
    (dict(num_opt_steps=0), b'num_opt_steps'),
    (dict(num_opt_steps=-1), b'num_opt_steps'),
    (dict(num_steps=0, save_every=1), b'num_steps'),
    (dict(num_steps=_lib.MAX_ROLLOUT_STEPS + 1, save_every=1), b'num_steps'),
    (dict(save_every=0), b'save_every'),
    (dict(save_every=-2), b'save_every'),
    (dict(save_every=4), b'save_every'),       # 6 steps
    (dict(save_every=12), b'save_every'),
    (dict(dt=0.0), b'dt'),
    (dict(dt=-1e-3), b'dt'),
    (dict(dt=float('nan')), b'dt'),
    (dict(clip_norm=-1.0), b'clip_norm'),
    (dict(clip_norm=float('inf')), b'clip_norm'),
    (dict(clip_norm=float('nan')), b'clip_norm'),
    (dict(beta1=1.0), b'beta1'),
    (dict(beta1=-0.1), b'beta1'),
    (dict(beta2=1.0), b'beta2'),
    (dict(beta2=float('nan')), b'beta2'),
    (dict(epsilon=0.0), b'epsilon'),
    (dict(epsilon=-1e-8), b'epsilon'),
    (dict(learning_rate=_rates_with(float('nan'))), b'learning_rate of replica 1, step 2'),
    (dict(learning_rate=_rates_with(float('inf'))), b'learning_rate of replica 1, step 2'),
    (dict(learning_rate=_rates_with(-1e-3, 0, 0)), b'learning_rate of replica 0, step 0'),
    (dict(learning_rate=None), b'NULL'),
    (dict(weights=None), b'NULL'),
    (dict(adam_m=None), b'NULL'),
    (dict(adam_v=None), b'NULL'),
    (dict(adam_step=None), b'NULL'),
    (dict(y0=None), b'NULL'),
    (dict(targets=None), b'NULL'),
    (dict(step_weights=None), b'NULL'),
    (dict(sample_index=None), b'NULL'),
    (dict(step_means_log=None), b'NULL'),
    (dict(grad_norm_log=None), b'NULL'),
    (dict(amplitude=0x1000), b'forcing'),      # the other four tables missing
    (dict(FORCING, amplitude=None), b'forcing'),
    (dict(FORCING, omega=None), b'forcing'),
    (dict(FORCING, phase=None), b'forcing'),
    (dict(FORCING, k_index=None), b'forcing'),
    (dict(FORCING, spatial_phase=None), b'forcing'),
    (dict(FORCING, nparams=0), b'nparams'),
    (dict(FORCING, n_k=0), b'n_k'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
    (dict(batch=0), b'batch'),
    (dict(num_rows=0), b'num_rows'),
    (dict(index_per_replica=2), b'index_per_replica'),
    (dict(forward_only=2), b'forward_only'),
    (dict(forward_only=1), b'num_opt_steps'),   # K = 3
    # forward only: the state may be NULL, the windows and the log may not
    (dict(forward_only=1, num_opt_steps=1, step_means_log=None), b'NULL'),
    (dict(forward_only=1, num_opt_steps=1, y0=None), b'NULL'),
    (dict(forward_only=1, num_opt_steps=1, sample_index=None, batch=8), b'num_rows'),
])
def test_argument_errors(fields, text):
  lib = _lib.load_library()
  assert _call(lib, _config(), _args(**fields)) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


def test_null_args_and_projection_tables():
  lib = _lib.load_library()
  assert lib.ddd_train_rollout_run(ctypes.byref(_config()), None, None) == ERR_INVALID_ARGUMENT
  cfg = _config(model_target=0, polynomial_accuracy_order=1)
  cfg.input_sizes[0] = cfg.input_sizes[1] = 4
  assert _call(lib, cfg, _args()) == ERR_INVALID_ARGUMENT
  assert b'nullspace' in lib.ddd_last_error()


@pytest.mark.parametrize('fields,text', UNSUPPORTED)
def test_unsupported_configurations_fail_with_the_messages_of_training(fields, text):
  lib = _lib.load_library()
  cfg = _config(**fields)
  assert lib.ddd_train_workspace_bytes(ctypes.byref(cfg), 4) == 0
  message = lib.ddd_last_error()
  assert text in message and message.startswith(b'training: ')
  want = WHO + message[len(b'training'):]   # train_params(..., who)
  assert lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(cfg), 4, 6, REPLICAS) == 0
  assert lib.ddd_last_error() == want
  assert _call(lib, cfg, _args()) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == want
  assert _call(lib, cfg, _args(**FORCING)) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == want
  assert _call(lib, cfg, _args(forward_only=1, num_opt_steps=1)) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == want


def test_workspace_size():
  lib = _lib.load_library()
  good = _config()
  for batch, steps in ((4, 6), (64, 32), (600, 2)):
    solo = lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), batch, steps)
    assert solo > 0
    sizes = [lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(good), batch, steps, r)
             for r in (1, 2, 3, 16, _lib.MAX_REPLICAS)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    for r, size in zip((1, 2, 3, 16, _lib.MAX_REPLICAS), sizes):
      # the slabs of R solo calls, a gradient buffer per replica and more
      assert size >= r * solo + r * 4 * _lib.vjp_num_weights(good)
      # it depends on cfg, batch, T and R only
      assert size == lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(good), batch,
                                                               steps, r)
  for replicas in (0, _lib.MAX_REPLICAS + 1, -1):
    assert lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(good), 4, 6, replicas) == 0
    assert b'replicas' in lib.ddd_last_error()
  for steps in (0, _lib.MAX_ROLLOUT_STEPS + 1):
    assert lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(good), 4, steps, 2) == 0
    assert b'num_steps' in lib.ddd_last_error()
  assert lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(good), 0, 6, 2) == 0


def test_rollout_population_trainer_refuses_before_device_work():
  burgers = make_model('burgers', conservative=False, num_points=32)
  hp = burgers.hparams
  with pytest.raises(ValueError, match='architecture'):
    training.RolloutPopulationTrainer(
        [burgers, make_model('burgers', conservative=False, num_points=32, filter_size=16)], hp)
  with pytest.raises(ValueError, match='architecture'):
    training.RolloutPopulationTrainer(
        [burgers, make_model('burgers', conservative=False, num_points=64)], hp)
  with pytest.raises(ValueError, match='equation'):
    training.RolloutPopulationTrainer(
        [burgers, make_model('burgers', conservative=True, num_points=32)], hp)
  with pytest.raises(ValueError, match='equation'):
    training.RolloutPopulationTrainer(
        [burgers, make_model('kdv', conservative=False, num_points=32)], hp)
  with pytest.raises(ValueError, match='models'):
    training.RolloutPopulationTrainer([], hp)
  for overrides, match in ((dict(numerical_flux=True), 'numerical_flux'),
                           (dict(model_target='flux'), 'flux'),
                           (dict(num_layers=0), 'num_layers')):
    with pytest.raises(NotImplementedError, match=match):
      training.RolloutPopulationTrainer([burgers, burgers],
                                        make_hparams('burgers', **overrides))


def test_stretches_between_evaluations():
  """fine_tune_on_rollouts evaluates after every eval_interval-th global step and after a
  horizon's last step: the fused stretches end exactly there."""
  assert training._rollout_stretches(6, 0, 3) == [3, 3]
  assert training._rollout_stretches(6, 6, 3) == [3, 3]
  assert training._rollout_stretches(5, 0, 3) == [3, 2]
  assert training._rollout_stretches(5, 5, 3) == [1, 3, 1]
  assert training._rollout_stretches(2, 0, 10) == [2]
  assert training._rollout_stretches(0, 0, 3) == []
