"""Training on rollout error without a GPU: the argument checks of
ddd_train_rollout_workspace_bytes / ddd_train_rollout_loss_grad through ctypes with a NULL
stream, and make_rollout_windows on synthetic exact data."""
import ctypes

import numpy as np
import pytest

from helpers import make_hparams
from test_cpu_training import _config
from ddd1d_amd import _lib, duckarray, equations, model as model_lib, training

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2
WHO = b'ddd_train_rollout_loss_grad'


def _args(**fields):
  """ddd_train_rollout_args with fake (never dereferenced) device pointers: every case
  below fails on the host."""
  args = _lib.DDDTrainRolloutArgs()
  args.struct_size = ctypes.sizeof(_lib.DDDTrainRolloutArgs)
  args.batch = 4
  args.num_rows = 4
  args.num_steps = 6
  args.save_every = 2
  args.dt = 1e-3
  args.weights = args.y0 = args.targets = args.step_weights = args.step_means = 0x1000
  args.workspace = 0x1000
  args.workspace_bytes = 1 << 40
  for name, value in fields.items():
    setattr(args, name, value)
  return args


FORCING = dict(nparams=3, n_k=2, amplitude=0x1000, omega=0x1000, phase=0x1000, k_index=0x1000,
               spatial_phase=0x1000)


def test_struct_layout_and_limits():
  assert _lib.MAX_ROLLOUT_STEPS == 256
  # five int32 (+ 4 bytes of padding), seven pointers, dt, t0, two int32, nine pointers, size_t
  assert ctypes.sizeof(_lib.DDDTrainRolloutArgs) == 24 + 7 * 8 + 8 + 8 + 8 + 9 * 8 + 8
  assert _lib.DDDTrainRolloutArgs.dt.offset == 24 + 7 * 8


def test_workspace_size():
  lib = _lib.load_library()
  good = _config()
  sizes = [lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), 64, steps)
           for steps in (1, 2, 8, 9, 64, _lib.MAX_ROLLOUT_STEPS)]
  assert sizes[0] > 0
  assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
  # per workgroup 2 T stage states and up to T cotangent rows of N floats
  assert sizes[3] - sizes[2] >= 64 * 3 * 32 * 4
  assert sizes[0] > lib.ddd_train_workspace_bytes(ctypes.byref(good), 64)
  assert sizes[2] == lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), 64, 8)
  # no more slabs than workgroups
  assert (lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), 512, 16) ==
          lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), 4096, 16))
  # the stage states of the longest horizon on the largest grid: 512 KiB per workgroup
  big = _config(num_points=256, dx=1.0 / 256)
  assert lib.ddd_train_rollout_workspace_bytes(
      ctypes.byref(big), 1, _lib.MAX_ROLLOUT_STEPS) >= 2 * 256 * 256 * 4


@pytest.mark.parametrize('steps', [0, -1, _lib.MAX_ROLLOUT_STEPS + 1])
def test_num_steps_out_of_range(steps):
  lib = _lib.load_library()
  good = _config()
  assert lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), 4, steps) == 0
  assert b'num_steps' in lib.ddd_last_error()
  assert lib.ddd_train_rollout_loss_grad(
      ctypes.byref(good), ctypes.byref(_args(num_steps=steps, save_every=1)),
      None) == ERR_INVALID_ARGUMENT
  assert b'num_steps' in lib.ddd_last_error()
  assert lib.ddd_train_rollout_workspace_bytes(ctypes.byref(good), 4,
                                               _lib.MAX_ROLLOUT_STEPS) > 0


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
def test_unsupported_configurations_fail_with_the_messages_of_training(fields, text):
  lib = _lib.load_library()
  cfg = _config(**fields)
  assert lib.ddd_train_workspace_bytes(ctypes.byref(cfg), 4) == 0
  message = lib.ddd_last_error()
  assert text in message and message.startswith(b'training: ')
  want = WHO + message[len(b'training'):]   # train_params(..., who)
  assert lib.ddd_train_rollout_workspace_bytes(ctypes.byref(cfg), 4, 6) == 0
  assert lib.ddd_last_error() == want
  assert lib.ddd_train_rollout_loss_grad(ctypes.byref(cfg), ctypes.byref(_args()),
                                         None) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == want
  # ... with the forcing tables given too
  assert lib.ddd_train_rollout_loss_grad(ctypes.byref(cfg), ctypes.byref(_args(**FORCING)),
                                         None) == ERR_UNSUPPORTED
  assert lib.ddd_last_error() == want


@pytest.mark.parametrize('fields,text', [
    (dict(struct_size=8), b'struct_size'),
    (dict(save_every=0), b'save_every'),
    (dict(save_every=-2), b'save_every'),
    (dict(save_every=4), b'save_every'),       # 6 steps
    (dict(save_every=12), b'save_every'),
    (dict(dt=0.0), b'dt'),
    (dict(dt=-1e-3), b'dt'),
    (dict(dt=float('nan')), b'dt'),
    (dict(y0=None), b'NULL'),
    (dict(targets=None), b'NULL'),
    (dict(step_weights=None), b'NULL'),
    (dict(step_means=None), b'NULL'),
    (dict(weights=None), b'NULL'),
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
    (dict(batch=8), b'num_rows'),
    (dict(num_rows=0), b'num_rows'),
])
def test_argument_errors(fields, text):
  lib = _lib.load_library()
  assert lib.ddd_train_rollout_loss_grad(ctypes.byref(_config()),
                                         ctypes.byref(_args(**fields)),
                                         None) == ERR_INVALID_ARGUMENT
  assert text in lib.ddd_last_error(), lib.ddd_last_error()


def test_null_args_and_projection_tables():
  lib = _lib.load_library()
  assert lib.ddd_train_rollout_loss_grad(ctypes.byref(_config()), None,
                                         None) == ERR_INVALID_ARGUMENT
  # model_target 'coefficients' with an accuracy order projects: nullspace / bias needed
  cfg = _config(model_target=0, polynomial_accuracy_order=1)
  cfg.input_sizes[0] = cfg.input_sizes[1] = 4
  assert lib.ddd_train_rollout_loss_grad(ctypes.byref(cfg), ctypes.byref(_args()),
                                         None) == ERR_INVALID_ARGUMENT
  assert b'nullspace' in lib.ddd_last_error()


# ---- make_rollout_windows ---------------------------------------------------------------
@pytest.mark.parametrize('conservative,method', [(True, 'mean'), (False, 'subsample')])
@pytest.mark.parametrize('num_steps,save_every,stride', [(4, 2, 1), (6, 1, 2), (3, 3, 1)])
def test_windows_of_synthetic_exact_data(conservative, method, num_steps, save_every, stride):
  hp = make_hparams('burgers', conservative=conservative, num_points=16, resample_factor=4)
  _, coarse = equations.from_hparams(hp)
  assert coarse.grid.resample_method == method
  samples, num_times = 3, 9
  spacing = coarse.time_step * save_every * 0.5
  times = 0.25 + spacing * np.arange(num_times)
  fine_points = 16 * 4
  x = np.arange(fine_points) / 1000.0
  y_exact = (100.0 * np.arange(samples)[:, None, None] +
             np.arange(num_times)[None, :, None] + x[None, None, :])
  w = training.make_rollout_windows(y_exact, times, hp, num_steps, save_every, stride=stride,
                                    first_seed=5, device='cpu')
  saved = num_steps // save_every
  starts = list(range(0, num_times - saved, stride))
  assert w.num_windows == samples * len(starts) and w.num_saved == saved
  assert w.num_steps == num_steps and w.save_every == save_every
  assert tuple(w.y0.shape) == (w.num_windows, 16)
  assert tuple(w.targets.shape) == (w.num_windows, saved, 16)
  assert w.t0.dtype.is_floating_point and w.t0.element_size() == 8
  np.testing.assert_allclose(w.dt, spacing / save_every, rtol=1e-12)
  low = duckarray.RESAMPLE_FUNCS[method](y_exact, 4, axis=-1)
  for i in range(w.num_windows):
    s, k = divmod(i, len(starts))
    start = starts[k]
    assert (w.sample[i], w.start[i]) == (s, start)
    np.testing.assert_array_equal(w.y0[i].numpy(), low[s, start].astype(np.float32))
    for j in range(saved):
      np.testing.assert_array_equal(w.targets[i, j].numpy(),
                                    low[s, start + 1 + j].astype(np.float32))
    assert w.t0[i].item() == times[start]
  # the forcing rows are those of each window's sample, seeded first_seed + sample
  eqs = [equations.from_hparams(hp, random_seed=5 + s)[1] for s in range(samples)]
  tables = model_lib.forcing_kernel_tables(model_lib.forcing_from_equations(eqs), coarse.grid)
  for name in ('amplitude', 'omega', 'phase', 'k_index'):
    np.testing.assert_array_equal(w.forcing[name].numpy(), tables[name][w.sample])
  np.testing.assert_array_equal(w.forcing['spatial_phase'].numpy(), tables['spatial_phase'])


def test_windows_of_an_unforced_equation_carry_no_forcing():
  hp = make_hparams('kdv', conservative=False, num_points=16, resample_factor=2)
  _, coarse = equations.from_hparams(hp)
  times = coarse.time_step * np.arange(4)
  w = training.make_rollout_windows(np.zeros((2, 4, 32)), times, hp, 2, 1, device='cpu')
  assert w.forcing is None and w.num_windows == 2 * 2


def test_window_errors():
  hp = make_hparams('burgers', conservative=True, num_points=16, resample_factor=4)
  _, coarse = equations.from_hparams(hp)
  step = coarse.time_step
  y = np.zeros((2, 5, 64))
  good = step * np.arange(5)
  training.make_rollout_windows(y, good, hp, 4, 1, device='cpu')
  with pytest.raises(ValueError, match='uniform'):
    training.make_rollout_windows(y, good * np.array([1, 1, 1, 1, 1.01]), hp, 2, 1,
                                  device='cpu')
  with pytest.raises(ValueError, match='uniform'):
    training.make_rollout_windows(y, good[::-1].copy(), hp, 2, 1, device='cpu')
  with pytest.raises(ValueError, match='time_step'):
    training.make_rollout_windows(y, 2.5 * good, hp, 4, 2, device='cpu')
  training.make_rollout_windows(y, 2.5 * good, hp, 3, 3, device='cpu')
  with pytest.raises(ValueError, match='no window fits'):
    training.make_rollout_windows(y, good, hp, 5, 1, device='cpu')
  with pytest.raises(ValueError, match='save_every'):
    training.make_rollout_windows(y, good, hp, 3, 2, device='cpu')
  with pytest.raises(ValueError, match='reference grid'):
    training.make_rollout_windows(y[..., :32], good, hp, 2, 1, device='cpu')
  with pytest.raises(ValueError, match='expected y_exact'):
    training.make_rollout_windows(y, good[:4], hp, 2, 1, device='cpu')


def test_rollout_trainer_checks_hparams_before_device_work():
  for overrides, match in [(dict(numerical_flux=True), 'numerical_flux'),
                           (dict(model_target='flux'), 'flux'),
                           (dict(num_layers=0), 'num_layers')]:
    hp = make_hparams('burgers', **overrides)
    with pytest.raises(NotImplementedError, match=match):
      training.RolloutTrainer(None, hp)
