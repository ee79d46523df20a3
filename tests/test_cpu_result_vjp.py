"""The differentiable-evaluation entry points without a GPU: ddd_vjp_workspace_bytes /
ddd_result_vjp refuse what the VJP kernel does not carry and malformed arguments before
any device work, and the Python wrappers do the same."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import make_model
from ddd1d_amd import _lib, model as model_lib

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2


def _config(**fields):
  cfg = _lib.DDDConfig()
  cfg.struct_size = ctypes.sizeof(_lib.DDDConfig)
  cfg.equation = 0
  cfg.num_points = 32
  cfg.num_derivatives = 2
  cfg.derivative_orders[0] = 1
  cfg.derivative_orders[1] = 2
  cfg.dx = 1.0 / 32
  cfg.period = 1.0
  cfg.standard_deviation = 1.0
  cfg.stencil_size = 6
  cfg.model_target = 1
  cfg.num_layers = 3
  cfg.filter_size = 32
  cfg.kernel_size = 5
  for name, value in fields.items():
    setattr(cfg, name, value)
  return cfg


def _args(**fields):
  """ddd_vjp_args with fake (never dereferenced) device pointers: every case below
  fails on the host."""
  args = _lib.DDDVjpArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDVjpArgs)
  args.batch = 4
  args.weights = args.y = args.cotangent = args.grad_y = 0x1000
  args.workspace = 0x1000
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


UNSUPPORTED = [
    (dict(equation=6, num_derivatives=3), b'Godunov'),
    (dict(model_target=3), b'flux'),
    (dict(num_layers=0), b'num_layers'),
    (dict(kernel_size=9), b'kernel_size'),
    (dict(filter_size=65), b'filter_size'),
    (dict(num_points=4), b'num_points'),
    (dict(num_points=512), b'num_points'),
]


@pytest.mark.parametrize('fields,text', UNSUPPORTED)
def test_unsupported_configurations_fail_before_device_work(fields, text):
  lib = _lib.load_library()
  cfg = _config(**fields)
  assert lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), 4) == 0
  assert text in lib.ddd_last_error() and b'ddd_result_vjp' in lib.ddd_last_error()
  assert lib.ddd_result_vjp(ctypes.byref(cfg), ctypes.byref(_args()), None) == ERR_UNSUPPORTED
  assert text in lib.ddd_last_error() and b'ddd_result_vjp' in lib.ddd_last_error()


def test_workspace_size_is_deterministic_and_matches_training():
  lib = _lib.load_library()
  cfg = _config()
  size = lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), 64)
  assert size > 0
  assert size == lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), 64)
  # the same slabs and scratch as the training kernel; at most 512 workgroups
  assert size == lib.ddd_train_workspace_bytes(ctypes.byref(cfg), 64)
  assert (lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), 512) ==
          lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), 4096))
  assert lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), 0) == 0


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(weights=None), b'NULL'),
    (dict(y=None), b'NULL'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
    (dict(grad_y=None, grad_weights=None), b'both NULL'),
    (dict(cotangent=None), b'need a cotangent'),
    (dict(cotangent=None, grad_y=None, predictions=None), b'nothing to compute'),
    (dict(batch=0), b'batch'),
])
def test_argument_errors(fields, text):
  lib = _lib.load_library()
  cfg = _config()
  assert lib.ddd_result_vjp(ctypes.byref(cfg), ctypes.byref(_args(**fields)),
                            None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


def test_projected_target_needs_nullspace_and_bias():
  lib = _lib.load_library()
  cfg = _config(model_target=0, polynomial_accuracy_order=1)
  for d in range(2):
    cfg.input_sizes[d] = 4
  assert lib.ddd_result_vjp(ctypes.byref(cfg), ctypes.byref(_args()),
                            None) == ERR_INVALID_ARGUMENT
  assert b'nullspace' in lib.ddd_last_error()


def test_args_struct_layout():
  # int32 struct_size, int32 batch, nine pointers, size_t
  assert ctypes.sizeof(_lib.DDDVjpArgs) == 8 + 9 * 8 + 8
  assert _lib.DDDVjpArgs.workspace_bytes.offset == 8 + 9 * 8


def test_python_wrappers_reject_unsupported_hparams():
  y = torch.zeros(2, 32)
  for overrides, text in [(dict(numerical_flux=True), 'Godunov'),
                          (dict(model_target='flux'), 'flux'),
                          (dict(kernel_size=9), 'kernel_size'),
                          (dict(filter_size=65), 'filter_size')]:
    model = make_model('burgers', conservative=True, num_points=32,
                       **overrides)
    for fn in (model_lib.differentiable_result, model_lib.differentiable_time_derivative,
               model_lib.differentiable_time_evolution):
      with pytest.raises(NotImplementedError, match=text):
        fn(y, model)
  model = make_model('burgers', conservative=True, num_points=4, resample_factor=8)
  with pytest.raises(NotImplementedError, match='num_points'):
    model_lib.differentiable_result(torch.zeros(2, 4), model)


def test_python_wrappers_reject_bad_tensors_before_device_work():
  model = make_model('burgers', conservative=False, num_points=32)
  size = model_lib.model_weights(model).size
  cfg = model_lib._vjp_setup(model)
  assert _lib.vjp_num_weights(cfg) == size
  # CPU, float64, non-contiguous and wrongly shaped states
  for y in (torch.zeros(2, 32), torch.zeros(2, 32, dtype=torch.float64),
            torch.zeros(32, 2).t(), torch.zeros(2, 31), torch.zeros(64)):
    with pytest.raises(ValueError, match='inputs'):
      model_lib.differentiable_result(y, model)
    with pytest.raises(ValueError, match='y'):
      _lib.result_vjp(cfg, torch.zeros(size), y)
  with pytest.raises(ValueError, match='num_time_steps'):
    model_lib.differentiable_time_evolution(torch.zeros(2, 32), model, num_time_steps=0)


def test_differentiable_functions_refuse_other_models():
  from ddd1d_amd import equations
  model = make_model('burgers', conservative=False, num_points=32)
  baseline = model_lib.BaselineModel(model.equation)
  with pytest.raises(TypeError):
    model_lib.differentiable_result(torch.zeros(2, 32), baseline)
  assert isinstance(model.equation, equations.Equation)


def test_model_weights_layout():
  model = make_model('kdv', conservative=False, num_points=32)
  flat = model_lib.model_weights(model)
  assert flat.dtype == np.float32
  offset = 0
  for w, b in zip(model.conv_kernels, model.conv_biases):
    np.testing.assert_array_equal(flat[offset:offset + w.size], w.ravel())
    offset += w.size
    np.testing.assert_array_equal(flat[offset:offset + b.size], b.ravel())
    offset += b.size
  assert offset == flat.size
