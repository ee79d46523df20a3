"""Population handles kept across calls and filled from device weights, on the GPU:
ddd_population_create_replicated + ddd_population_load_weights (csrc/pack_device.hip),
evaluation.RolloutPopulation, PopulationTrainer.rollout_population and
training_population(rollout_every=...).

The feature has no tolerance: a replica loaded from its flat weight vector on the device
holds bit for bit the packed arrays ddd_model_create + ddd_population_create give the same
values (the arrays themselves: test_cpu_pack_device), so every rollout is compared with
assert_array_equal against the population built from host-packed models."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import make_hparams, make_model, random_phase_ic
from ddd1d_amd import _lib, equations, evaluation, model as model_lib, training

pytestmark = pytest.mark.gpu

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -2
TIMES = np.linspace(0.0, 0.1, 3)
EQUATIONS = [('burgers', True), ('burgers', False), ('kdv', True), ('kdv', False),
             ('ks', True), ('ks', False)]


def _models(equation, conservative, num_points, replicas=3, first_seed=0, **overrides):
  return [make_model(equation, conservative, num_points=num_points, resample_factor=4,
                     init_seed=first_seed + r, **overrides) for r in range(replicas)]


def _flat(model):
  return np.concatenate([np.concatenate([w.ravel(), b.ravel()])
                         for w, b in zip(model.conv_kernels, model.conv_biases)]
                        ).astype(np.float32)


def _device_weights(models):
  return torch.from_numpy(np.stack([_flat(m) for m in models])).cuda().contiguous()


def _with_weights(model, kernels, biases):
  return model_lib.LearnedStencilModel(model.equation, model.hparams, kernels, biases,
                                       model.nullspaces, model.biases)


class Handle(object):
  """A ddd_population through ctypes, destroyed after a device synchronise."""

  def __init__(self, models=None, replicated=None):
    self.lib = _lib.load_library()
    self.handle = ctypes.c_void_p()
    if models is not None:
      handles = (ctypes.c_void_p * len(models))(*[m._handle.value for m in models])
      self.status = self.lib.ddd_population_create(handles, len(models),
                                                   ctypes.byref(self.handle))
      self.replicas = len(models)
    else:
      model, self.replicas = replicated
      self.status = self.lib.ddd_population_create_replicated(model._handle, self.replicas,
                                                              ctypes.byref(self.handle))
    self.message = self.lib.ddd_last_error().decode()

  def load(self, weights, first_replica=0, count=None, n_weights=None):
    count = int(weights.shape[0]) if count is None else count
    n_weights = int(weights.shape[1]) if n_weights is None else n_weights
    return self.lib.ddd_population_load_weights(self.handle, weights.data_ptr(), n_weights,
                                                first_replica, count, _lib.current_stream())

  def adaptive(self, y0, times=TIMES, max_attempts=0):
    """(y, nfev, status) device tensors, enqueued on the current stream."""
    y0 = torch.as_tensor(np.ascontiguousarray(y0, dtype=np.float64)).cuda()
    times = np.ascontiguousarray(times, dtype=np.float64)
    y = torch.full((self.replicas, times.size) + tuple(y0.shape), 7.0, dtype=torch.float64,
                   device='cuda')
    nfev = torch.zeros((self.replicas, y0.shape[0]), dtype=torch.int32, device='cuda')
    flags = torch.zeros_like(nfev)
    _lib.check(self.lib.ddd_population_integrate_adaptive_f64(
        self.handle, times.ctypes.data_as(_lib._D), times.size, 1e-3, 1e-6, 0.01,
        int(max_attempts), y0.data_ptr(), y.data_ptr(), nfev.data_ptr(), flags.data_ptr(),
        y0.shape[0], _lib.current_stream()))
    return y, nfev, flags, y0

  def fixed(self, y0, dt, steps=6, save_every=2):
    y0 = torch.as_tensor(np.ascontiguousarray(y0, dtype=np.float32)).cuda()
    y = torch.full((self.replicas, steps // save_every) + tuple(y0.shape), 7.0,
                   dtype=torch.float32, device='cuda')
    _lib.check(self.lib.ddd_population_integrate_fixed(
        self.handle, _lib.SCHEMES['bs3'], 0.0, float(dt), steps, save_every, y0.data_ptr(),
        y.data_ptr(), y0.shape[0], _lib.current_stream()))
    return y, y0

  def close(self):
    torch.cuda.synchronize()
    assert self.lib.ddd_population_destroy(self.handle) == 0


def _host(tensors):
  return tuple(t.cpu().numpy() for t in tensors[:3])


def _adaptive_of_models(models, y0, **kwargs):
  """The rollout of the population ddd_population_create builds from host-packed models."""
  pop = Handle(models=models)
  assert pop.status == 0, pop.message
  try:
    return _host(pop.adaptive(y0, **kwargs))
  finally:
    pop.close()


def _adaptive_of_weights(model0, weights, y0, **kwargs):
  pop = Handle(replicated=(model0, int(weights.shape[0])))
  assert pop.status == 0, pop.message
  try:
    assert pop.load(weights) == 0, pop.lib.ddd_last_error()
    return _host(pop.adaptive(y0, **kwargs))
  finally:
    pop.close()


def _assert_same(got, want):
  for name, a, b in zip(('y', 'nfev', 'status'), got, want):
    np.testing.assert_array_equal(a, b, err_msg=name)


def _initial(models, equation, samples):
  scale = 0.3 if equation == 'burgers' else 1.0
  y0 = scale * random_phase_ic(models[0].equation, samples).astype(np.float64)
  if equation == 'burgers':
    models[0].set_forcing(model_lib.batched_forcing_parameters(range(samples), nparams=10))
  return y0


# ---------------------------------------------------------------------------
# 1. rollout parity: every per-equation kernel, adaptive and float32 fixed step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('equation,conservative,num_points,samples', [
    (equation, conservative, num_points, 3)
    for num_points in (64, 16) for equation, conservative in EQUATIONS] +
                         [('burgers', True, 32, 5)])
def test_loaded_population_equals_the_host_packed_one(equation, conservative, num_points,
                                                      samples):
  """N = 32 with 5 samples: two per 64-row group, the last group half empty."""
  models = _models(equation, conservative, num_points)
  y0 = _initial(models, equation, samples)
  dt = 1e-3 if equation == 'burgers' else 2.5e-5
  host = Handle(models=models)
  device = Handle(replicated=(models[0], 3))
  assert host.status == 0 and device.status == 0, (host.message, device.message)
  try:
    assert device.load(_device_weights(models)) == 0
    want, got = _host(host.adaptive(y0)), _host(device.adaptive(y0))
    want_fixed = host.fixed(y0, dt)[0].cpu().numpy()
    got_fixed = device.fixed(y0, dt)[0].cpu().numpy()
  finally:
    host.close()
    device.close()
  _assert_same(got, want)
  np.testing.assert_array_equal(got_fixed, want_fixed)
  assert not np.array_equal(got[0][0], got[0][1], equal_nan=True)   # (different nets)
  assert not np.array_equal(got_fixed[0], got_fixed[1], equal_nan=True)
  assert np.isfinite(got[0]).all() and (got[2] == 0).all()


@pytest.mark.parametrize('overrides', [dict(filter_size=20), dict(kernel_size=4),
                                       dict(filter_size=31, kernel_size=4)])
def test_nets_embedded_in_the_default_tower(overrides):
  """4 taps / 17 .. 31 filters ride the per-equation kernels zero-padded: the device packer
  packs the embedding (tap shift, zero channels)."""
  models = _models('kdv', True, 64, **overrides)
  y0 = _initial(models, 'kdv', 3)
  want = _adaptive_of_models(models, y0)
  _assert_same(_adaptive_of_weights(models[0], _device_weights(models), y0), want)
  assert not np.array_equal(want[0][0], want[0][1])


# ---------------------------------------------------------------------------
# 2. partial loads, reloads, stream order
# ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def kdv():
  """Two sets of three KdV nets, their initial condition and their host-packed rollouts."""
  first, second = _models('kdv', True, 32), _models('kdv', True, 32, first_seed=10)
  y0 = _initial(first, 'kdv', 3)
  return dict(a=first, b=second, y0=y0, want_a=_adaptive_of_models(first, y0),
              want_b=_adaptive_of_models(second, y0),
              want_mixed=_adaptive_of_models([first[0], second[1], first[2]], y0))


def test_a_partial_load_changes_its_replicas_only(kdv):
  pop = Handle(replicated=(kdv['a'][0], 3))
  try:
    assert pop.load(_device_weights(kdv['a'])) == 0
    assert pop.load(_device_weights(kdv['b'][1:2]), first_replica=1) == 0
    got = _host(pop.adaptive(kdv['y0']))
  finally:
    pop.close()
  _assert_same(got, kdv['want_mixed'])
  assert not np.array_equal(kdv['want_mixed'][0][1], kdv['want_a'][0][1])


def test_a_reload_leaves_nothing_of_what_was_there(kdv):
  """A then B is a fresh B; all-NaN vectors, then healthy weights: no NaN."""
  poison = torch.full((3, _flat(kdv['a'][0]).size), float('nan'), device='cuda')
  pop = Handle(replicated=(kdv['a'][0], 3))
  try:
    assert pop.load(_device_weights(kdv['a'])) == 0
    assert pop.load(_device_weights(kdv['b'])) == 0
    got_b = _host(pop.adaptive(kdv['y0']))
    assert pop.load(poison) == 0
    sick = _host(pop.adaptive(kdv['y0'], max_attempts=100))
    assert pop.load(_device_weights(kdv['a'])) == 0
    got_a = _host(pop.adaptive(kdv['y0']))
  finally:
    pop.close()
  _assert_same(got_b, kdv['want_b'])
  assert np.isnan(sick[0][:, 1:]).all()   # (the poison was what ran)
  _assert_same(got_a, kdv['want_a'])
  assert np.isfinite(got_a[0]).all()


def test_loads_and_rollouts_are_ordered_by_their_stream(kdv):
  """Load, roll out, load other weights, roll out again on one side stream with no host
  wait in between: each rollout is its own weights'."""
  a, b = _device_weights(kdv['a']), _device_weights(kdv['b'])
  pop = Handle(replicated=(kdv['a'][0], 3))
  stream = torch.cuda.Stream()
  stream.wait_stream(torch.cuda.current_stream())
  try:
    with torch.cuda.stream(stream):
      assert pop.load(a) == 0
      first = pop.adaptive(kdv['y0'])
      assert pop.load(b) == 0
      second = pop.adaptive(kdv['y0'])
      assert pop.load(a) == 0   # (and a load behind the last rollout does not reach it)
    stream.synchronize()
    first, second = _host(first), _host(second)
  finally:
    pop.close()
  _assert_same(first, kdv['want_a'])
  _assert_same(second, kdv['want_b'])


def test_load_weights_works_on_a_population_of_models(kdv):
  pop = Handle(models=kdv['a'])
  try:
    assert pop.load(_device_weights(kdv['b'])) == 0
    got = _host(pop.adaptive(kdv['y0']))
  finally:
    pop.close()
  _assert_same(got, kdv['want_b'])


def test_a_replicated_population_starts_as_copies_of_its_model(kdv):
  pop = Handle(replicated=(kdv['a'][0], 2))
  try:
    got = _host(pop.adaptive(kdv['y0']))
  finally:
    pop.close()
  for r in range(2):
    for part, want in zip(got, kdv['want_a']):
      np.testing.assert_array_equal(part[r], want[0])


def test_load_weights_refuses_ranges_and_sizes(kdv):
  weights = _device_weights(kdv['a'])
  pop = Handle(replicated=(kdv['a'][0], 3))
  try:
    for first, count in ((3, 1), (1, 3), (0, 4), (4, 0)):
      assert pop.load(weights, first_replica=first, count=count) == ERR_INVALID_ARGUMENT
      assert 'outside the population' in pop.lib.ddd_last_error().decode()
    for n_weights in (int(weights.shape[1]) - 1, int(weights.shape[1]) + 1):
      assert pop.load(weights, n_weights=n_weights) == ERR_INVALID_ARGUMENT
      assert 'n_weights' in pop.lib.ddd_last_error().decode()
    assert pop.load(weights, first_replica=3, count=0) == 0   # (the empty range at the end)
    got = _host(pop.adaptive(kdv['y0']))
  finally:
    pop.close()
  for part, want in zip(got, kdv['want_a']):   # (nothing was loaded: still model 0's copies)
    np.testing.assert_array_equal(part[1], want[0])


# ---------------------------------------------------------------------------
# 3. isolation and edge values
# ---------------------------------------------------------------------------
def test_a_nan_replica_reaches_no_other_replica(kdv):
  models = list(kdv['a'])
  kernels = [k.copy() for k in models[1].conv_kernels]
  kernels[-1][:] = np.nan
  models[1] = _with_weights(models[1], kernels, models[1].conv_biases)
  got = _adaptive_of_weights(models[0], _device_weights(models), kdv['y0'], max_attempts=200)
  _assert_same(got, _adaptive_of_models(models, kdv['y0'], max_attempts=200))
  for r in (0, 2):
    for part, want in zip(got, kdv['want_a']):
      np.testing.assert_array_equal(part[r], want[r])
  assert np.isnan(got[0][1][1:]).all()


@pytest.mark.parametrize('equation,conservative', [('burgers', True), ('kdv', False)])
def test_denormal_biases_and_negative_zeros_travel_as_on_the_host(equation, conservative):
  """A bias of 1e-20 is a float32 denormal after the 2^-64 relu shift; the host keeps it
  and keeps the sign of -0.0 (folded output layer: flux-form Burgers)."""
  models = _models(equation, conservative, 64)
  for r, model in enumerate(models):
    kernels = [k.copy() for k in model.conv_kernels]
    biases = [b.copy() for b in model.conv_biases]
    for b in biases:
      b[r::3] = 1e-20
      b[(r + 1) % 3::6] = -1e-20
    for k in kernels:
      k.reshape(-1)[r::7] = -0.0
    models[r] = _with_weights(model, kernels, biases)
  y0 = _initial(models, equation, 3)
  want = _adaptive_of_models(models, y0)
  _assert_same(_adaptive_of_weights(models[0], _device_weights(models), y0), want)
  assert np.isfinite(want[0]).all()


# ---------------------------------------------------------------------------
# 4. Python: RolloutPopulation, the trainer's route, rollout_every
# ---------------------------------------------------------------------------
def _burgers_reference(times=(0.0, 0.05, 0.1)):
  x = np.arange(128) / 128.0
  times = np.array(times)
  y_exact = np.stack([
      np.stack([0.3 * (1.0 - t) * np.sin(2 * np.pi * (s % 2 + 1) * x + s) for t in times])
      for s in range(4)])
  return evaluation.RolloutReference(y_exact, times, 4, quantiles=(0.8,),
                                     stop_times=(0.05, 0.1))


def _assert_results_equal(got, want):
  assert sorted(got) == sorted(want)
  for key in want:
    if key == 'samples':
      for name in want[key]:
        np.testing.assert_array_equal(got[key][name], want[key][name], err_msg=name)
    else:
      np.testing.assert_array_equal(got[key], want[key], err_msg=key)


def test_rollout_population_in_place_of_the_models():
  hp = make_hparams('burgers', num_points=32, resample_factor=4)
  models = _models('burgers', True, 32)
  reference = _burgers_reference()
  want = evaluation.evaluate_population(models, hp, reference, keep_trajectories=True,
                                        launch='population')
  population = evaluation.RolloutPopulation(models[0], 3)
  assert population.replicas == 3 and population.load_models(models) is population
  got = evaluation.evaluate_population(population, hp, reference, keep_trajectories=True)
  _assert_results_equal(got, want)
  # fixed step, and a reload of one replica from a device tensor
  times = 2e-3 * np.arange(4)
  y0 = 0.3 * random_phase_ic(models[0].equation, 5)
  other = _models('burgers', True, 32, first_seed=7)
  population.load(_device_weights(other[1:2]), first_replica=1)
  got = evaluation.run_integrate_population(population, hp, y0, times, max_step=1e-3,
                                            adaptive=False)
  want = evaluation.run_integrate_population([models[0], other[1], models[2]], hp, y0, times,
                                             max_step=1e-3, adaptive=False, launch='population')
  for a, b in zip(got, want):
    assert torch.equal(a, b)
  with pytest.raises(ValueError, match='contiguous float32 device tensor'):
    population.load(_device_weights(models).double())
  with pytest.raises(_lib.DDDError, match='outside the population'):
    population.load(_device_weights(models), first_replica=1)
  population.close()
  population.close()   # (idempotent)
  with pytest.raises(ValueError, match='closed'):
    evaluation.run_integrate_population(population, hp, y0, times, max_step=1e-3, adaptive=False)


def _training_case(seed=3):
  snapshots = np.random.RandomState(0).randn(60, 128).astype(np.float32)
  hp = make_hparams('burgers', conservative=True, num_points=32, resample_factor=4,
                    learning_stops=[4], eval_interval=2, base_batch_size=2)
  return snapshots, hp


def test_trainer_rollout_population_equals_its_export():
  snapshots, hp = _training_case()
  data = training.set_data_dependent_hparams(hp, snapshots, 3)
  data.repeat = True
  assert data.batch_size == 8
  _, coarse = equations.from_hparams(hp, random_seed=3)
  trainer = training.PopulationTrainer(
      [model_lib.LearnedStencilModel(coarse, hp, init_seed=s) for s in (3, 4, 5)], hp)
  reference = _burgers_reference()
  trainer.run(data, 2)
  first = trainer.rollout_population()
  got = evaluation.evaluate_population(first, hp, reference, keep_trajectories=True)
  _assert_results_equal(got, evaluation.evaluate_population(
      trainer.export(), hp, reference, keep_trajectories=True, launch='population'))
  trainer.run(data, 2)   # the same handle, the new weights
  again = trainer.rollout_population()
  assert again is first
  after = evaluation.evaluate_population(again, hp, reference, keep_trajectories=True)
  _assert_results_equal(after, evaluation.evaluate_population(
      trainer.export(), hp, reference, keep_trajectories=True, launch='population'))
  assert not np.array_equal(after['samples']['y'], got['samples']['y'])
  assert not np.array_equal(after['samples']['y'][0], after['samples']['y'][1])


def test_rollout_every(tmp_path):
  snapshots, hp = _training_case()
  reference = _burgers_reference()
  keys = {'rollout_mae/0.05', 'rollout_mae/0.1', 'rollout_survival/0.8'}

  def run(name, **kwargs):
    dirs = [str(tmp_path / name / 'replica{}'.format(r)) for r in range(2)]
    return training.training_population(snapshots, dirs, hp, init_seeds=[3, 4], seed=3,
                                        num_steps=4, rollout=reference, **kwargs)
  once = run('once', rollout_launch='population')
  population = run('population', rollout_every=2, rollout_launch='population')
  streams = run('streams', rollout_every=2, rollout_launch='streams')
  for r in range(2):
    assert [row['step'] for row in population[r]] == [0, 2, 4]
    for row in population[r]:
      assert keys <= set(row), row['step']
    assert not any(keys & set(row) for row in once[r][:-1])
    assert population[r][-1] == once[r][-1]
    assert population[r] == streams[r]
    # (the rollouts follow the training: other weights, other scores)
    assert any(population[r][1][key] != population[r][2][key] for key in keys)
  with pytest.raises(ValueError, match='rollout_every'):
    training.training_population(snapshots, [str(tmp_path / 'none')], hp, init_seeds=[3],
                                 seed=3, num_steps=2, rollout_every=2)


# ---------------------------------------------------------------------------
# 5. what the population kernels do not carry
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['filters16', 'n128', 'tanh'])
def test_unsupported_models_are_refused_with_the_reason(case):
  overrides = {'filters16': dict(filter_size=16), 'n128': {},
               'tanh': dict(nonlinearity='tanh')}[case]
  model = make_model('kdv', True, num_points=128 if case == 'n128' else 64, resample_factor=2,
                     **overrides)
  pop = Handle(replicated=(model, 3))
  assert pop.status == ERR_UNSUPPORTED and pop.handle.value is None, (pop.status, pop.message)
  assert 'no population kernel' in pop.message and len(pop.message) > 40, pop.message
  print(case, '->', pop.message)
  with pytest.raises(NotImplementedError, match='no population kernel'):
    evaluation.RolloutPopulation(model, 3)
