"""The tangent-linear entry points without a GPU: ddd_jvp_workspace_bytes / ddd_result_jvp
and ddd_tangent_rollout_workspace_bytes / ddd_tangent_rollout refuse exactly what the VJP
refuses, under their own names, and malformed arguments before any device work; the Python
wrappers do the same."""
import ctypes

import pytest
import torch

from helpers import make_model
from test_cpu_result_vjp import _config, UNSUPPORTED
from ddd1d_amd import _lib, evaluation, model as model_lib

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2


def _jvp_args(**fields):
  """ddd_jvp_args with fake (never dereferenced) device pointers: every case below fails on
  the host."""
  args = _lib.DDDJvpArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDJvpArgs)
  args.batch = 4
  args.tangents = 3
  args.weights = args.y = args.tangent_y = args.tangents_out = 0x1000
  args.workspace = 0x1000
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


def _rollout_args(**fields):
  args = _lib.DDDTangentRolloutArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDTangentRolloutArgs)
  args.batch = 4
  args.tangents = 3
  args.num_steps = 2
  args.dt = 1e-3
  args.weights = args.y0 = args.tangents0 = args.state_out = args.tangents_out = 0x1000
  args.workspace = 0x1000
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


ENTRY_POINTS = [
    ('ddd_jvp_workspace_bytes', 'ddd_result_jvp', _jvp_args),
    ('ddd_tangent_rollout_workspace_bytes', 'ddd_tangent_rollout', _rollout_args),
]


@pytest.mark.parametrize('ws_fn,fn,make_args', ENTRY_POINTS, ids=['jvp', 'rollout'])
def test_workspace_size_is_positive_and_repeatable(ws_fn, fn, make_args):
  lib = _lib.load_library()
  cfg = _config()
  size = getattr(lib, ws_fn)(ctypes.byref(cfg), 64, 3)
  assert size > 0
  assert size == getattr(lib, ws_fn)(ctypes.byref(cfg), 64, 3)
  # at most 512 workgroups, each with its own scratch
  assert (getattr(lib, ws_fn)(ctypes.byref(cfg), 512, 3) ==
          getattr(lib, ws_fn)(ctypes.byref(cfg), 4096, 3))
  assert getattr(lib, ws_fn)(ctypes.byref(cfg), 0, 3) == 0


def test_rollout_workspace_grows_with_the_tangents_and_the_jvp_does_not():
  lib = _lib.load_library()
  cfg = _config()
  # the rollout keeps the tangents and the midpoint's, [M][N] each, in every slab
  one = lib.ddd_tangent_rollout_workspace_bytes(ctypes.byref(cfg), 4, 1)
  three = lib.ddd_tangent_rollout_workspace_bytes(ctypes.byref(cfg), 4, 3)
  assert three - one == 4 * (2 * 2 * 32) * 4
  assert (lib.ddd_jvp_workspace_bytes(ctypes.byref(cfg), 4, 1) ==
          lib.ddd_jvp_workspace_bytes(ctypes.byref(cfg), 4, 32))


@pytest.mark.parametrize('ws_fn,fn,make_args', ENTRY_POINTS, ids=['jvp', 'rollout'])
@pytest.mark.parametrize('fields,text', UNSUPPORTED)
def test_unsupported_configurations_fail_before_device_work(ws_fn, fn, make_args, fields, text):
  lib = _lib.load_library()
  cfg = _config(**fields)
  assert getattr(lib, ws_fn)(ctypes.byref(cfg), 4, 3) == 0
  assert text in lib.ddd_last_error() and fn.encode() in lib.ddd_last_error()
  assert getattr(lib, fn)(ctypes.byref(cfg), ctypes.byref(make_args()),
                          None) == ERR_UNSUPPORTED
  assert text in lib.ddd_last_error() and fn.encode() in lib.ddd_last_error()


@pytest.mark.parametrize('ws_fn,fn,make_args', ENTRY_POINTS, ids=['jvp', 'rollout'])
@pytest.mark.parametrize('tangents', [0, 33, -1])
def test_tangent_count_outside_1_to_32_is_refused(ws_fn, fn, make_args, tangents):
  lib = _lib.load_library()
  cfg = _config()
  assert _lib.MAX_TANGENTS == 32
  assert getattr(lib, ws_fn)(ctypes.byref(cfg), 4, tangents) == 0
  assert b'tangents' in lib.ddd_last_error()
  assert getattr(lib, fn)(ctypes.byref(cfg), ctypes.byref(make_args(tangents=tangents)),
                          None) == ERR_INVALID_ARGUMENT
  assert b'tangents' in lib.ddd_last_error()
  assert getattr(lib, ws_fn)(ctypes.byref(cfg), 4, 32) > 0


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(weights=None), b'NULL'),
    (dict(y=None), b'NULL'),
    (dict(tangents_out=None), b'NULL'),
    (dict(tangent_y=None, tangent_weights=None), b'both NULL'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
    (dict(batch=0), b'batch'),
])
def test_jvp_argument_errors(fields, text):
  lib = _lib.load_library()
  cfg = _config()
  assert lib.ddd_result_jvp(ctypes.byref(cfg), ctypes.byref(_jvp_args(**fields)),
                            None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(num_steps=0), b'num_steps'),
    (dict(num_steps=-3), b'num_steps'),
    (dict(dt=float('nan')), b'dt'),
    (dict(weights=None), b'NULL'),
    (dict(y0=None), b'NULL'),
    (dict(tangents0=None), b'NULL'),
    (dict(state_out=None), b'NULL'),
    (dict(tangents_out=None), b'NULL'),
    (dict(workspace_bytes=16), b'workspace'),
    (dict(workspace=None), b'workspace'),
    (dict(batch=0), b'batch'),
])
def test_rollout_argument_errors(fields, text):
  lib = _lib.load_library()
  cfg = _config()
  assert lib.ddd_tangent_rollout(ctypes.byref(cfg), ctypes.byref(_rollout_args(**fields)),
                                 None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


@pytest.mark.parametrize('fn,make_args', [('ddd_result_jvp', _jvp_args),
                                          ('ddd_tangent_rollout', _rollout_args)])
def test_projected_target_needs_nullspace_and_bias(fn, make_args):
  lib = _lib.load_library()
  cfg = _config(model_target=0, polynomial_accuracy_order=1)
  for d in range(2):
    cfg.input_sizes[d] = 4
  assert getattr(lib, fn)(ctypes.byref(cfg), ctypes.byref(make_args()),
                          None) == ERR_INVALID_ARGUMENT
  assert b'nullspace' in lib.ddd_last_error()


def test_args_struct_layouts():
  # four int32, eight pointers, two pointer-sized / four int32, a double, seven pointers, two
  assert ctypes.sizeof(_lib.DDDJvpArgs) == 16 + 8 * 8 + 16
  assert _lib.DDDJvpArgs.weights.offset == 16
  assert _lib.DDDJvpArgs.workspace_bytes.offset == 16 + 9 * 8
  assert ctypes.sizeof(_lib.DDDTangentRolloutArgs) == 16 + 8 + 7 * 8 + 16
  assert _lib.DDDTangentRolloutArgs.dt.offset == 16
  assert _lib.DDDTangentRolloutArgs.workspace_bytes.offset == 24 + 8 * 8


def test_python_wrappers_reject_unsupported_hparams():
  y, t = torch.zeros(2, 32), torch.zeros(2, 3, 32)
  for overrides, text in [(dict(numerical_flux=True), 'Godunov'),
                          (dict(model_target='flux'), 'flux'),
                          (dict(kernel_size=9), 'kernel_size'),
                          (dict(filter_size=65), 'filter_size')]:
    model = make_model('burgers', conservative=True, num_points=32, **overrides)
    with pytest.raises(NotImplementedError, match=text):
      model_lib.tangent_result(y, t, model)
    with pytest.raises(NotImplementedError, match=text):
      model_lib.tangent_time_evolution(y, t, model, 2)
  model = make_model('burgers', conservative=True, num_points=4, resample_factor=8)
  with pytest.raises(NotImplementedError, match='num_points'):
    model_lib.tangent_result(torch.zeros(2, 4), torch.zeros(2, 3, 4), model)


def test_python_wrappers_reject_bad_tensors_before_device_work():
  model = make_model('burgers', conservative=False, num_points=32)
  size = model_lib.model_weights(model).size
  cfg = model_lib._vjp_setup(model)
  t = torch.zeros(2, 3, 32)
  # CPU, float64, non-contiguous and wrongly shaped states
  for y in (torch.zeros(2, 32), torch.zeros(2, 32, dtype=torch.float64),
            torch.zeros(32, 2).t(), torch.zeros(2, 31), torch.zeros(64)):
    with pytest.raises(ValueError, match='inputs'):
      model_lib.tangent_result(y, t, model)
    with pytest.raises(ValueError, match='inputs'):
      model_lib.tangent_time_evolution(y, t, model, 2)
    with pytest.raises(ValueError, match='y'):
      _lib.result_jvp(cfg, torch.zeros(size), y, t)
    with pytest.raises(ValueError, match='y0'):
      _lib.tangent_rollout(cfg, torch.zeros(size), y, t, 2, 1e-3)
  with pytest.raises(ValueError, match='num_time_steps'):
    model_lib.tangent_time_evolution(torch.zeros(2, 32), t, model, 0)
  # the checks of _lib.result_jvp / tangent_rollout that need no device
  y = torch.zeros(2, 32)
  with pytest.raises(ValueError, match='both None'):
    _lib.result_jvp(cfg, torch.zeros(size), y)
  with pytest.raises(ValueError, match='tangents = 33'):
    _lib.result_jvp(cfg, torch.zeros(size), y, torch.zeros(2, 33, 32))
  with pytest.raises(ValueError, match='tangents = 0'):
    _lib.tangent_rollout(cfg, torch.zeros(size), y, torch.zeros(2, 0, 32), 2, 1e-3)
  with pytest.raises(ValueError, match='num_steps'):
    _lib.tangent_rollout(cfg, torch.zeros(size), y, t, 0, 1e-3)
  with pytest.raises(ValueError, match='tangent_y'):
    _lib.result_jvp(cfg, torch.zeros(size), y, torch.zeros(2, 32))


def test_tangent_functions_refuse_other_models():
  model = make_model('burgers', conservative=False, num_points=32)
  baseline = model_lib.BaselineModel(model.equation)
  with pytest.raises(TypeError):
    model_lib.tangent_result(torch.zeros(2, 32), torch.zeros(2, 3, 32), baseline)


def test_lyapunov_initial_tangents_are_seeded_and_orthonormal():
  a = evaluation.lyapunov_initial_tangents(2, 3, 32, seed=5)
  b = evaluation.lyapunov_initial_tangents(2, 3, 32, seed=5)
  c = evaluation.lyapunov_initial_tangents(2, 3, 32, seed=6)
  assert a.shape == (2, 3, 32) and a.dtype.name == 'float32'
  assert (a == b).all() and not (a == c).all()
  gram = torch.as_tensor(a).double() @ torch.as_tensor(a).double().transpose(1, 2)
  assert (gram - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-6
