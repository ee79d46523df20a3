"""The optimiser loop on the device without a GPU: the configuration and argument checks
of ddd_train_run_workspace_bytes / ddd_train_run, the workspace size and the learning
rates Trainer.run hands over."""
import ctypes

import pytest

from helpers import make_hparams
from test_cpu_training import _config
from ddd1d_amd import _lib, training

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2


def _args(num_steps=3, **fields):
  """ddd_train_run_args with fake (never dereferenced) device pointers: every case below
  fails on the host.  The learning rates are a real host array, kept alive on the
  struct."""
  args = _lib.DDDTrainRunArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDTrainRunArgs)
  args.batch = 4
  args.num_rows = 4
  args.num_time_steps = 0
  args.first_step = 0
  args.num_steps = num_steps
  args.time_step = 1e-3
  for name in ('weights', 'adam_m', 'adam_v', 'y', 'labels', 'baseline', 'sample_index',
               'head_means_log', 'workspace'):
    setattr(args, name, 0x1000)
  args.rates = (ctypes.c_double * 8)(*([1e-3] * 8))
  args.learning_rate = ctypes.cast(args.rates, ctypes.POINTER(ctypes.c_double))
  args.beta1, args.beta2, args.epsilon = 0.9, 0.99, 1e-8
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


def _without_name(message):
  """A message of the form b'<entry point>: <text>' without its entry point."""
  name, _, text = message.partition(b': ')
  assert name in (b'training', b'training run'), message
  return text


def test_struct_layout():
  # six int32, nine pointers, the rates pointer, four doubles, two double and three float
  # head arrays + time_step, three pointers, size_t
  heads = _lib.MAX_UNROLLED_HEADS
  floats = 3 * heads + 1
  assert floats % 2 == 0
  assert (ctypes.sizeof(_lib.DDDTrainRunArgs) ==
          24 + 10 * 8 + 4 * 8 + 2 * 8 * heads + 4 * floats + 3 * 8 + 8)
  assert _lib.DDDTrainRunArgs.weights.offset == 24
  assert _lib.DDDTrainRunArgs.time_step.offset % 8 == 4


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
def test_unsupported_configurations_fail_with_the_messages_of_training(fields, text, steps):
  lib = _lib.load_library()
  cfg = _config(**fields)
  if steps:
    assert lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(cfg), 4, steps) == 0
  else:
    assert lib.ddd_train_workspace_bytes(ctypes.byref(cfg), 4) == 0
  want = lib.ddd_last_error()
  assert text in want and want.startswith(b'training: ')
  assert lib.ddd_train_run_workspace_bytes(ctypes.byref(cfg), 4, steps) == 0
  got = lib.ddd_last_error()
  assert got.startswith(b'training run: ') and _without_name(got) == _without_name(want)
  assert lib.ddd_train_run(ctypes.byref(cfg), ctypes.byref(_args(num_time_steps=steps)),
                           None) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == got


def test_too_many_time_steps_fail_with_the_message_of_training_through_time():
  lib = _lib.load_library()
  good = _config()
  steps = _lib.MAX_TIME_STEPS + 1
  assert lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 4, steps) == 0
  want = lib.ddd_last_error()
  assert b'num_time_steps' in want
  assert lib.ddd_train_run_workspace_bytes(ctypes.byref(good), 4, steps) == 0
  assert _without_name(lib.ddd_last_error()) == _without_name(want)
  assert lib.ddd_train_run(ctypes.byref(good), ctypes.byref(_args(num_time_steps=steps)),
                           None) == ERR_UNSUPPORTED
  assert _without_name(lib.ddd_last_error()) == _without_name(want)
  assert lib.ddd_train_run_workspace_bytes(ctypes.byref(good), 4, _lib.MAX_TIME_STEPS) > 0
  assert lib.ddd_train_run_workspace_bytes(ctypes.byref(good), 4, -1) == 0
  assert b'num_time_steps' in lib.ddd_last_error()


def _bad_rates(index, value):
  rates = (ctypes.c_double * 8)(*([1e-3] * 8))
  rates[index] = value
  return rates


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(weights=None), b'NULL'),
    (dict(adam_m=None), b'NULL'),
    (dict(adam_v=None), b'NULL'),
    (dict(y=None), b'NULL'),
    (dict(labels=None), b'NULL'),
    (dict(baseline=None), b'NULL'),
    (dict(sample_index=None), b'NULL'),
    (dict(head_means_log=None), b'NULL'),
    (dict(learning_rate=ctypes.POINTER(ctypes.c_double)()), b'NULL'),
    (dict(num_steps=0), b'num_steps'),
    (dict(num_steps=-2), b'num_steps'),
    (dict(first_step=-1), b'first_step'),
    (dict(batch=0), b'batch'),
    (dict(num_rows=0), b'num_rows'),
    (dict(rates=_bad_rates(1, float('nan'))), b'step 1'),
    (dict(rates=_bad_rates(2, float('inf'))), b'step 2'),
    (dict(rates=_bad_rates(0, -1e-3)), b'step 0'),
    (dict(beta1=1.0), b'beta1'),
    (dict(beta1=-0.1), b'beta1'),
    (dict(beta2=1.0), b'beta2'),
    (dict(beta2=float('nan')), b'beta2'),
    (dict(epsilon=0.0), b'epsilon'),
    (dict(epsilon=-1e-8), b'epsilon'),
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
  assert lib.ddd_train_run(ctypes.byref(_config()), ctypes.byref(args),
                           None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


def test_a_rate_behind_num_steps_is_not_read():
  lib = _lib.load_library()
  args = _args(num_steps=3, rates=_bad_rates(3, float('nan')), workspace_bytes=16)
  args.learning_rate = ctypes.cast(args.rates, ctypes.POINTER(ctypes.c_double))
  assert lib.ddd_train_run(ctypes.byref(_config()), ctypes.byref(args),
                           None) == ERR_INVALID_ARGUMENT
  assert b'workspace' in lib.ddd_last_error()   # (the next check: the rates passed)


@pytest.mark.parametrize('steps,head', [(0, 2), (2, 4)])
def test_non_finite_coefficients_are_refused_by_head(steps, head):
  lib = _lib.load_library()
  for name in ('error_floor', 'coef_abs', 'coef_rel'):
    args = _args(num_time_steps=steps)
    getattr(args, name)[head] = float('inf')
    assert lib.ddd_train_run(ctypes.byref(_config()), ctypes.byref(args),
                             None) == ERR_INVALID_ARGUMENT
    assert 'head {}'.format(head).encode() in lib.ddd_last_error()
  # a head the configuration does not have is not read
  args = _args(num_time_steps=steps, workspace_bytes=16)
  args.coef_abs[head + 1] = float('nan')
  assert lib.ddd_train_run(ctypes.byref(_config()), ctypes.byref(args),
                           None) == ERR_INVALID_ARGUMENT
  assert b'workspace' in lib.ddd_last_error()
  # the error scales are read with error_max > 0 only
  args = _args(num_time_steps=steps, workspace_bytes=16)
  args.error_scale_rel[head] = float('nan')
  assert lib.ddd_train_run(ctypes.byref(_config()), ctypes.byref(args), None) == -1
  assert b'workspace' in lib.ddd_last_error()
  args.error_max = 0.5
  args.workspace_bytes = 1 << 40   # (the workspace is checked before the heads)
  assert lib.ddd_train_run(ctypes.byref(_config()), ctypes.byref(args), None) == -1
  assert 'head {}'.format(head).encode() in lib.ddd_last_error()


def test_workspace_size():
  lib = _lib.load_library()
  good = _config()
  heads = good.num_derivatives + 1
  for batch in (1, 6, 64, 600):
    train = lib.ddd_train_workspace_bytes(ctypes.byref(good), batch)
    run = lib.ddd_train_run_workspace_bytes(ctypes.byref(good), batch, 0)
    # the slabs of training plus the device table [3][H'] of loss constants
    assert train > 0 and 3 * heads * 4 <= run - train <= 256
    assert run == lib.ddd_train_run_workspace_bytes(ctypes.byref(good), batch, 0)
    for steps in (1, 4):
      unrolled = lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), batch, steps)
      through = lib.ddd_train_run_workspace_bytes(ctypes.byref(good), batch, steps)
      assert unrolled > 0 and 3 * (heads + steps) * 4 <= through - unrolled <= 256
  # as many slabs as workgroups: nothing grows behind 512 samples
  assert (lib.ddd_train_run_workspace_bytes(ctypes.byref(good), 512, 0) ==
          lib.ddd_train_run_workspace_bytes(ctypes.byref(good), 4096, 0))
  # a workspace one byte short is refused, the exact size passes on to the device work
  args = _args(workspace_bytes=lib.ddd_train_run_workspace_bytes(ctypes.byref(good), 4, 0) - 1)
  assert lib.ddd_train_run(ctypes.byref(good), ctypes.byref(args), None) == -1
  assert b'workspace' in lib.ddd_last_error()


class _Recorder(object):
  """Stands in for _lib.train_run: keeps the arguments, returns a zero log."""

  def __init__(self):
    self.calls = []

  def __call__(self, cfg, weights, adam_m, adam_v, y, labels, baseline, sample_index,
               learning_rates, error_floor, coef_abs, coef_rel, **kwargs):
    import torch
    self.calls.append(dict(kwargs, learning_rates=list(learning_rates),
                           sample_index=sample_index))
    return torch.zeros((len(learning_rates), 2, labels.shape[-1])), None


def test_run_asks_for_the_schedule_of_its_steps(monkeypatch):
  """Trainer.run's learning rates are learning_rate(hparams, step_count + k), across a
  boundary of the schedule inside one run and across two runs, and first_step follows the
  optimiser's own step count.  (The device call is replaced: no GPU here.)"""
  import numpy as np
  import torch
  hp = make_hparams('burgers', conservative=False, num_points=32,
                    learning_rates=[1e-3, 1e-4], learning_stops=[3, 6])
  hp.error_scale = [1.0] * 6
  hp.error_floor = [1e-3] * 3
  want = [training.learning_rate(hp, k) for k in range(6)]
  assert want == [1e-3] * 4 + [1e-4] * 2   # piecewise_constant: step <= 3 is the first piece

  trainer = training.Trainer.__new__(training.Trainer)   # (no device tensors)
  trainer.torch = torch
  trainer.hparams = hp
  trainer.cfg = None
  trainer.model = None
  trainer.nullspace = trainer.bias = None
  trainer.weights = torch.nn.Parameter(torch.zeros(5))
  trainer.optimizer = torch.optim.Adam([trainer.weights], lr=1e-3, betas=(0.9, 0.99))
  trainer.step_count = 0
  recorder = _Recorder()
  monkeypatch.setattr(_lib, 'train_run', recorder)

  class Data(object):
    inputs = torch.zeros(12, 32)
    labels = torch.zeros(12, 32, 3)
    baseline = torch.zeros(12, 32, 3)

  index = np.arange(36, dtype=np.int32).reshape(6, 6) % 12
  out = trainer.run(Data, 6, index)
  assert out.shape == (6, 2, 3) and trainer.step_count == 6
  assert recorder.calls[0]['learning_rates'] == want
  assert recorder.calls[0]['first_step'] == 0
  assert recorder.calls[0]['betas'] == (0.9, 0.99)
  assert recorder.calls[0]['sample_index'].dtype == torch.int32
  assert float(trainer.optimizer.state[trainer.weights]['step']) == 6.0

  trainer.step_count = 0
  trainer.optimizer.state[trainer.weights]['step'] -= 6
  trainer.run(Data, 2, index[:2])
  trainer.run(Data, 4, index[2:])
  assert recorder.calls[1]['learning_rates'] + recorder.calls[2]['learning_rates'] == want
  assert [c['first_step'] for c in recorder.calls[1:]] == [0, 2]
  with pytest.raises(ValueError, match='num_steps'):
    trainer.run(Data, 0)
  with pytest.raises(ValueError, match='sample_index'):
    trainer.run(Data, 3, index[:2])
