"""Rollouts of a replica population in one launch (replicas on grid.y) on the GPU.

Every comparison is assert_array_equal: a sample's result does not depend on the ensemble
around it and the population kernels are the solo kernels' code behind moved pointers, so
replica r of a population launch must reproduce models[r]'s solo run bit for bit, NaN rows
included."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import make_hparams, make_model, random_phase_ic
from ddd1d_amd import _lib, evaluation, model as model_lib

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2
BURGERS_TIMES = np.linspace(0.0, 0.2, 5)


def _models(equation, conservative, num_points, replicas, **overrides):
  return [make_model(equation, conservative, num_points=num_points, resample_factor=4,
                     init_seed=seed, **overrides) for seed in range(replicas)]


def _create(models):
  """(status, handle, message) of ddd_population_create on the models' handles."""
  lib = _lib.load_library()
  handles = (ctypes.c_void_p * len(models))(*[m._handle.value for m in models])
  handle = ctypes.c_void_p()
  status = lib.ddd_population_create(handles, len(models), ctypes.byref(handle))
  return status, handle, lib.ddd_last_error().decode()


def _adaptive(models, y0, times, max_step=0.01, max_attempts=0):
  """ddd_population_integrate_adaptive_f64 through ctypes: (y, nfev, status) on the host."""
  lib = _lib.load_library()
  status, handle, message = _create(models)
  assert status == 0, message
  y0 = torch.from_numpy(np.ascontiguousarray(y0, dtype=np.float64)).cuda()
  times = np.ascontiguousarray(times, dtype=np.float64)
  shape = (len(models), times.size) + tuple(y0.shape)
  y = torch.full(shape, 7.0, dtype=torch.float64, device='cuda')   # (every row is written)
  nfev = torch.zeros((len(models), y0.shape[0]), dtype=torch.int32, device='cuda')
  flags = torch.zeros_like(nfev)
  try:
    _lib.check(lib.ddd_population_integrate_adaptive_f64(
        handle, times.ctypes.data_as(_lib._D), times.size, 1e-3, 1e-6, float(max_step),
        int(max_attempts), y0.data_ptr(), y.data_ptr(), nfev.data_ptr(), flags.data_ptr(),
        y0.shape[0], _lib.current_stream()))
    torch.cuda.synchronize()
  finally:
    assert lib.ddd_population_destroy(handle) == 0
  return y.cpu().numpy(), nfev.cpu().numpy(), flags.cpu().numpy()


def _solo(model, y0, times, **kwargs):
  y, nfev, status = model.integrate_adaptive(np.asarray(y0, dtype=np.float64), times, **kwargs)
  return y.cpu().numpy(), nfev.cpu().numpy(), status.cpu().numpy()


def _assert_replicas_equal_solo(got, models, y0, times, **kwargs):
  y, nfev, status = got
  for r, model in enumerate(models):
    want_y, want_nfev, want_status = _solo(model, y0, times, **kwargs)
    np.testing.assert_array_equal(y[r], want_y, err_msg='replica {}'.format(r))
    np.testing.assert_array_equal(nfev[r], want_nfev, err_msg='replica {}'.format(r))
    np.testing.assert_array_equal(status[r], want_status, err_msg='replica {}'.format(r))


def _host(tensors):
  return tuple(t.cpu().numpy() for t in tensors)


# ---------------------------------------------------------------------------
# 1. adaptive Burgers: conservative, forced, folded output layer
# ---------------------------------------------------------------------------
def test_adaptive_burgers_population_equals_solo_runs():
  hp = make_hparams('burgers', num_points=32, resample_factor=4)
  models = _models('burgers', True, 32, 3)
  # 5 samples, two per 64-row group: the third group of every replica is half empty
  y0 = 0.3 * random_phase_ic(models[0].equation, 5).astype(np.float64)
  got = evaluation.run_integrate_population(models, hp, y0, BURGERS_TIMES, launch='population')
  assert got[0].dtype == torch.float64 and tuple(got[0].shape) == (3, 5, 5, 32)
  assert got[1].dtype == torch.int32 and tuple(got[1].shape) == (3, 5) == tuple(got[2].shape)
  got = _host(got)
  assert models[0].kernel_name == 'mfma_f32_r64'
  _assert_replicas_equal_solo(got, models, y0, BURGERS_TIMES)   # (the forcing is set on all)
  assert (got[2] == 0).all()
  assert not np.array_equal(got[0][0], got[0][1])   # (different nets)


# ---------------------------------------------------------------------------
# 2. all six per-equation kernels, one and four samples per group
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('num_points', [64, 16])
@pytest.mark.parametrize('equation,conservative', [
    ('burgers', True), ('burgers', False), ('kdv', True), ('kdv', False),
    ('ks', True), ('ks', False)])
def test_every_per_equation_kernel(equation, conservative, num_points):
  """test_gpu_adaptive.test_reference_settings_n64's span and step ceiling: times to 0.2,
  max_step = 0.01, Burgers forced and scaled by 0.3.  3 samples: at N = 16 the one group is
  three-quarters full.  The Burgers forcing has 10 modes per sample: four samples per group
  put 4 P (sample, mode) pairs on the group's 64 lanes, so the per-equation kernels carry at
  most 16 modes at N = 16 (with the 20 of run_integrate_population's own forcing such a
  model runs on the run-time-parameterised kernels, and has no population form)."""
  models = _models(equation, conservative, num_points, 2)
  scale = 0.3 if equation == 'burgers' else 1.0
  y0 = (scale * random_phase_ic(models[0].equation, 3)).astype(np.float64)
  if equation == 'burgers':
    forcing = model_lib.batched_forcing_parameters(range(3), nparams=10)
    for model in models:
      model.set_forcing(forcing)
  got = _adaptive(models, y0, BURGERS_TIMES, max_step=0.01)
  _assert_replicas_equal_solo(got, models, y0, BURGERS_TIMES, max_step=0.01)
  assert not np.array_equal(got[0][0], got[0][1], equal_nan=True)


# ---------------------------------------------------------------------------
# 3. fixed step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('scheme', ['midpoint', 'bs3'])
@pytest.mark.parametrize('equation,num_points,replicas,samples,dt', [
    ('kdv', 64, 2, 3, 2.5e-5), ('burgers', 32, 3, 5, 1e-3)])
def test_fixed_step_population_equals_integrate_fixed(equation, num_points, replicas, samples,
                                                      dt, scheme):
  hp = make_hparams(equation, num_points=num_points, resample_factor=4)
  models = _models(equation, True, num_points, replicas)
  scale = 0.3 if equation == 'burgers' else 1.0
  y0 = (scale * random_phase_ic(models[0].equation, samples)).astype(np.float32)
  times = 2 * dt * np.arange(4)   # 6 steps, save_every = 2
  y, nfev, status = evaluation.run_integrate_population(
      models, hp, y0, times, max_step=dt, scheme=scheme, adaptive=False, launch='population')
  assert y.dtype == torch.float32 and tuple(y.shape) == (replicas, 4, samples, num_points)
  y, nfev, status = _host((y, nfev, status))
  stages = _lib.load_library().ddd_scheme_stages(_lib.SCHEMES[scheme])
  for r, model in enumerate(models):
    want = model.integrate_fixed(y0, 6, dt=dt, t0=0.0, scheme=scheme, save_every=2)
    np.testing.assert_array_equal(y[r, 1:], want.cpu().numpy(), err_msg='replica {}'.format(r))
    np.testing.assert_array_equal(y[r, 0], y0)
  assert (nfev == 6 * stages).all() and (status == 0).all()
  assert not np.array_equal(y[0], y[1])


# ---------------------------------------------------------------------------
# 4. replica isolation
# ---------------------------------------------------------------------------
def test_a_nan_replica_reaches_no_other_replica():
  """Replica 1's output layer is NaN: a replica stride applied to the wrong array would
  carry its NaNs, or replica 0's or 2's weights, into a neighbour."""
  models = _models('kdv', True, 32, 3)
  sick = models[1]
  kernels = [k.copy() for k in sick.conv_kernels]
  kernels[-1][:] = np.nan
  models[1] = model_lib.LearnedStencilModel(sick.equation, sick.hparams, kernels,
                                            sick.conv_biases, sick.nullspaces, sick.biases)
  y0 = random_phase_ic(models[0].equation, 3).astype(np.float64)
  times = np.linspace(0.0, 0.05, 3)
  got = _adaptive(models, y0, times, max_attempts=200)
  _assert_replicas_equal_solo(got, models, y0, times, max_attempts=200)
  assert np.isfinite(got[0][0]).all() and np.isfinite(got[0][2]).all()
  assert (got[2][0] == 0).all() and (got[2][2] == 0).all()
  assert np.isnan(got[0][1][1:]).all()   # (the NaN weights were the ones replica 1 ran with)


# ---------------------------------------------------------------------------
# 5. one replica
# ---------------------------------------------------------------------------
def test_one_replica_equals_the_solo_entry_point():
  models = _models('kdv', False, 64, 1)
  y0 = random_phase_ic(models[0].equation, 3).astype(np.float64)
  times = np.linspace(0.0, 0.1, 3)
  _assert_replicas_equal_solo(_adaptive(models, y0, times), models, y0, times)


# ---------------------------------------------------------------------------
# 6. the forcing is replica 0's
# ---------------------------------------------------------------------------
def test_forcing_comes_from_replica_zero():
  models = _models('burgers', True, 32, 3)
  forcing = model_lib.batched_forcing_parameters(range(5), nparams=20)
  y0 = 0.3 * random_phase_ic(models[0].equation, 5).astype(np.float64)
  for model in models:
    model.set_forcing(forcing)
  want = [_solo(model, y0, BURGERS_TIMES) for model in models]
  models[1].set_forcing(None)
  models[2].set_forcing(None)
  # (the forcing matters: without it model 1 alone computes something else)
  assert not np.array_equal(_solo(models[1], y0, BURGERS_TIMES)[0], want[1][0])
  y, nfev, status = _adaptive(models, y0, BURGERS_TIMES)
  for r in range(3):
    np.testing.assert_array_equal(y[r], want[r][0], err_msg='replica {}'.format(r))
    np.testing.assert_array_equal(nfev[r], want[r][1])
    np.testing.assert_array_equal(status[r], want[r][2])


# ---------------------------------------------------------------------------
# 7. what the population kernels do not carry
# ---------------------------------------------------------------------------
def _unsupported_models(case):
  if case == 'n48':
    return [make_model('kdv', True, num_points=48, resample_factor=2, init_seed=s)
            for s in range(2)]
  if case == 'filters16':
    return _models('kdv', True, 64, 2, filter_size=16)
  if case == 'generic':
    models = _models('kdv', True, 64, 2)
    models[1].set_kernel('generic')
    return models
  return [make_model('kdv', True, num_points=64, resample_factor=4, init_seed=0),
          make_model('kdv', True, num_points=64, resample_factor=4, init_seed=1, filter_size=16)]


@pytest.mark.parametrize('case', ['n48', 'filters16', 'generic', 'mixed_filters'])
def test_unsupported_configurations_say_why_and_auto_takes_the_streams(case):
  models = _unsupported_models(case)
  status, handle, message = _create(models)
  assert handle.value is None
  if case == 'mixed_filters':
    assert status in (ERR_UNSUPPORTED, ERR_INVALID_ARGUMENT), (status, message)
  else:
    assert status == ERR_UNSUPPORTED, (status, message)
  assert len(message) > 20, message   # (the reason)
  print(case, '->', message)
  hp = models[0].hparams
  y0 = random_phase_ic(models[0].equation, 3).astype(np.float64)
  times = np.linspace(0.0, 0.05, 3)
  with pytest.raises(NotImplementedError):
    evaluation.run_integrate_population(models, hp, y0, times, launch='population')
  streams = _host(evaluation.run_integrate_population(models, hp, y0, times, launch='streams'))
  auto = _host(evaluation.run_integrate_population(models, hp, y0, times, launch='auto'))
  for a, b in zip(auto, streams):
    np.testing.assert_array_equal(a, b)


# ---------------------------------------------------------------------------
# 8. evaluate_population
# ---------------------------------------------------------------------------
def test_evaluate_population_on_the_population_route():
  hp = make_hparams('burgers', num_points=32, resample_factor=4)
  models = _models('burgers', True, 32, 3)
  y0 = 0.3 * random_phase_ic(models[0].equation, 5).astype(np.float64)
  own = evaluation.run_integrate_batch(models[0], hp, y0, BURGERS_TIMES)['y']
  growth = (np.arange(5) / 4.0)[None, :, None]
  noise = 0.15 * growth * np.random.RandomState(0).standard_normal(own.shape[:2] + (128,))
  y_exact = np.repeat(own, 4, axis=-1) + noise
  reference = evaluation.RolloutReference(y_exact, BURGERS_TIMES, 4, quantiles=(0.8, 0.9),
                                          stop_times=(0.1, 0.2, 1.0))
  streams = evaluation.evaluate_population(models, hp, reference, keep_trajectories=True,
                                           launch='streams')
  one = evaluation.evaluate_population(models, hp, reference, keep_trajectories=True,
                                       launch='population')
  for key in ('mae', 'survival', 'num_evals', 'status'):
    np.testing.assert_array_equal(one[key], streams[key], err_msg=key)
  np.testing.assert_array_equal(one['samples']['y'], streams['samples']['y'])
  assert (one['survival'] < BURGERS_TIMES[-1]).any()
