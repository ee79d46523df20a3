"""Training through time without a GPU: the argument checks of
ddd_train_unrolled_workspace_bytes / ddd_train_unrolled_loss_grad, the hparams checker
and the loss weights of the integrated heads."""
import ctypes

import numpy as np
import pytest

from helpers import make_hparams
from test_cpu_training import _config
from ddd1d_amd import _lib, model as model_lib, training

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2


def _args(**fields):
  """ddd_train_unrolled_args with fake (never dereferenced) device pointers: every case
  below fails on the host."""
  args = _lib.DDDTrainUnrolledArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDTrainUnrolledArgs)
  args.batch = 4
  args.num_rows = 4
  args.num_time_steps = 2
  args.time_step = 1e-3
  args.weights = args.y = args.labels = args.baseline = args.head_means = 0x1000
  args.workspace = 0x1000
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


def test_struct_layout_and_limits():
  assert _lib.MAX_TIME_STEPS >= 8
  assert _lib.MAX_UNROLLED_HEADS == _lib.MAX_HEADS + _lib.MAX_TIME_STEPS
  # four int32, seven pointers, time_step + three head arrays, four pointers, size_t
  floats = 1 + 3 * _lib.MAX_UNROLLED_HEADS
  assert floats % 2 == 0
  assert ctypes.sizeof(_lib.DDDTrainUnrolledArgs) == 16 + 7 * 8 + 4 * floats + 4 * 8 + 8
  assert _lib.DDDTrainUnrolledArgs.time_step.offset == 16 + 7 * 8


def test_workspace_size():
  lib = _lib.load_library()
  good = _config()
  one = lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 64, 1)
  assert one > 0
  assert one == lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 64, 1)
  # the slabs of training plus, per workgroup, 2 T stage states, T cotangent rows and
  # 2 T head sums
  train = lib.ddd_train_workspace_bytes(ctypes.byref(good), 64)
  assert one > train
  four = lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 64, 4)
  assert four - one >= 64 * 3 * (3 * 32) * 4
  assert (lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 512, 2) ==
          lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 4096, 2))


@pytest.mark.parametrize('steps,status,text', [
    (0, ERR_INVALID_ARGUMENT, b'num_time_steps'),
    (-1, ERR_INVALID_ARGUMENT, b'num_time_steps'),
    (_lib.MAX_TIME_STEPS + 1, ERR_UNSUPPORTED, b'num_time_steps'),
])
def test_num_time_steps_out_of_range(steps, status, text):
  lib = _lib.load_library()
  good = _config()
  assert lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 4, steps) == 0
  assert text in lib.ddd_last_error()
  assert lib.ddd_train_unrolled_loss_grad(ctypes.byref(good),
                                          ctypes.byref(_args(num_time_steps=steps)),
                                          None) == status
  assert text in lib.ddd_last_error()
  assert lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(good), 4,
                                                _lib.MAX_TIME_STEPS) > 0


@pytest.mark.parametrize('fields,text', [
    (dict(equation=6, num_derivatives=3), b'Godunov'),
    (dict(model_target=3), b'flux'),
    (dict(num_layers=0), b'num_layers'),
    (dict(kernel_size=9), b'kernel_size'),
    (dict(filter_size=65), b'filter_size'),
    (dict(num_points=4), b'num_points'),
    (dict(num_points=512), b'num_points'),
])
def test_unsupported_configurations_fail_with_the_messages_of_training(fields, text):
  lib = _lib.load_library()
  cfg = _config(**fields)
  assert lib.ddd_train_workspace_bytes(ctypes.byref(cfg), 4) == 0
  want = lib.ddd_last_error()
  assert text in want
  assert lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(cfg), 4, 2) == 0
  assert lib.ddd_last_error() == want
  assert lib.ddd_train_unrolled_loss_grad(ctypes.byref(cfg), ctypes.byref(_args()),
                                          None) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == want


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(weights=None), b'NULL'),
    (dict(labels=None), b'NULL'),
    (dict(head_means=None), b'NULL'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
    (dict(batch=0), b'batch'),
    (dict(batch=8), b'num_rows'),
    (dict(time_step=float('nan')), b'time_step'),
])
def test_argument_errors(fields, text):
  lib = _lib.load_library()
  assert lib.ddd_train_unrolled_loss_grad(ctypes.byref(_config()),
                                          ctypes.byref(_args(**fields)),
                                          None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


def test_non_finite_coefficient_of_an_integrated_head_is_refused():
  lib = _lib.load_library()
  args = _args()
  args.coef_rel[4] = float('inf')   # heads: u_x, u_xx, u_t, y(t_1), y(t_2)
  assert lib.ddd_train_unrolled_loss_grad(ctypes.byref(_config()), ctypes.byref(args),
                                          None) == ERR_INVALID_ARGUMENT
  assert b'head 4' in lib.ddd_last_error()


def test_check_supported_through_time():
  training.check_supported_through_time(make_hparams('burgers', num_time_steps=1))
  training.check_supported_through_time(
      make_hparams('kdv', conservative=False, num_time_steps=_lib.MAX_TIME_STEPS))
  with pytest.raises(NotImplementedError, match='num_time_steps'):
    training.check_supported_through_time(make_hparams('burgers'))
  with pytest.raises(NotImplementedError, match='num_time_steps'):
    training.check_supported_through_time(
        make_hparams('burgers', num_time_steps=_lib.MAX_TIME_STEPS + 1))
  for overrides, match in [(dict(numerical_flux=True), 'numerical_flux'),
                           (dict(model_target='flux'), 'flux'),
                           (dict(num_layers=0), 'num_layers'),
                           (dict(kernel_size=9), 'kernel_size')]:
    hp = make_hparams('burgers', num_time_steps=2, **overrides)
    with pytest.raises(NotImplementedError, match=match):
      training.check_supported_through_time(hp)
    assert hp.num_time_steps == 2   # (checked on a copy)
  hp = make_hparams('burgers', model_target='time_derivative', space_derivatives_weight=1.0,
                    num_time_steps=2)
  with pytest.raises(ValueError, match='space derivatives'):
    training.check_supported_through_time(hp)
  # the single-evaluation checker keeps refusing the integrated loss
  with pytest.raises(NotImplementedError, match='num_time_steps'):
    training.check_supported(make_hparams('burgers', num_time_steps=3))


@pytest.mark.parametrize('steps', [1, 2, 5])
def test_loss_weights_of_the_integrated_heads(steps):
  hp = make_hparams('ks', conservative=False, absolute_error_weight=1.0,
                    relative_error_weight=3.0, space_derivatives_weight=0.6,
                    time_derivative_weight=1.0, integrated_solution_weight=2.0)
  table = model_lib.loss_weights(hp, 3 + 1 + steps)
  assert table.shape == (2, 4 + steps)
  np.testing.assert_allclose(table.sum(), 1.0, rtol=1e-12)
  channel = np.array([0.2] * 3 + [1.0] + [2.0 / steps] * steps)
  want = np.array([0.25, 0.75])[:, None] * (channel / channel.sum())[None, :]
  np.testing.assert_allclose(table, want, rtol=1e-12)
  # weighted_loss over a [2, channel] table of ones is the sum of the weights
  np.testing.assert_allclose(model_lib.weighted_loss(np.ones((2, 4 + steps)), hp), 1.0,
                             rtol=1e-12)
