"""Batched evaluation of a learned-stencil model against exact solutions.

What ``scripts/run_evaluation.py`` (136-221) and ``analysis.py`` (39-90)
compute, without Beam / xarray / netCDF: every sample of an exact data set is
integrated by the coarse model from its resampled initial condition, then the
mean absolute error up to each stop time and the "mostly good" survival time
are reported.

The reference integrates one sample per Beam worker with SciPy RK23 through a
TF session.  Here ``run_integrate`` keeps that execution shape (one sample, one
adaptive solve, HIP right-hand side) and ``run_integrate_batch`` advances all
samples together in one launch with the same adaptive RK23 -- one
SciPy-identical step-size controller per sample on the device
(``ddd_integrate_adaptive_f64``), so every sample gets the trajectory and the
``num_evals`` of its own ``solve_ivp`` call whatever its stiffness.
``adaptive=False`` selects the fixed-step Bogacki-Shampine scheme at
``max_step`` instead (equal only while the controller is saturated, as in
notebooks/time-integration.ipynb).  With more than one rank the samples are
sharded and gathered (``distributed``), the analogue of
``beam.CombineGlobally(ConcatCombineFn('sample'))`` (run_evaluation.py:218).

Arrays are plain NumPy: ``y_model`` [sample, time, x_low], ``y_exact``
[sample, time, x_high], ``times`` [time].

``evaluate_population`` scores R models at once without the trajectories leaving
the device: a ``RolloutReference`` prepares what does not depend on the model
once (the block-averaged exact solution, the error thresholds, the initial
conditions), ``run_integrate_population`` enqueues the R rollouts side by side
into one slab -- or, with ``launch='population'``, rolls all of them out in ONE launch
whose grid carries the replicas (``ddd_population_integrate_*``) -- and
``ddd_rollout_scores`` scores them in two launches; one small host read returns
``mae`` [replica, time_max, sample] and ``survival`` [replica,
quantile, sample].  A ``RolloutPopulation`` keeps the one-launch handle across calls and
takes its replicas' weights from device tensors (``ddd_population_load_weights``), so a
trained population is rolled out without its weights leaving the device.
"""
import atexit
import ctypes
from typing import Dict, Optional, Sequence
import weakref

import numpy as np

from . import _lib
from . import distributed
from . import duckarray
from . import equations as equations_lib
from . import integrate
from . import model as model_lib


# ---------------------------------------------------------------------------
# analysis.py
# ---------------------------------------------------------------------------
def unify_x_coords(y_low: np.ndarray, y_high: np.ndarray) -> np.ndarray:
  """High-resolution data block-averaged onto the low-resolution grid
  (analysis.unify_x_coords, analysis.py:39-53)."""
  factor = y_high.shape[-1] // y_low.shape[-1]
  return duckarray.resample_mean(y_high, factor)


def is_good(model, exact, max_error: float = 0.5):
  """Pointwise accuracy within ``max_error`` (analysis.py:56-62)."""
  return np.abs(model - exact) <= max_error


def mostly_good(model, exact, max_error: float = 0.5, frac_good: float = 0.8):
  """Per time: at least ``frac_good`` of the points accurate (analysis.py:65-72)."""
  return is_good(model, exact, max_error=max_error).mean(axis=-1) >= frac_good


def calculate_survival(good: np.ndarray, times: np.ndarray) -> np.ndarray:
  """"Lifetime" of a boolean [..., time] array: the first time it is False,
  the last time if it never is (analysis.py:75-79)."""
  good = np.asarray(good).astype(bool)
  times = np.asarray(times)
  first_bad = np.argmin(good, axis=-1)
  return np.where(good.all(axis=-1), times.max(), times[first_bad])


def mostly_good_survival(y_models: Dict[str, np.ndarray], y_exact: np.ndarray,
                         times: np.ndarray, quantile: float = 0.8
                         ) -> Dict[str, np.ndarray]:
  """Survival time per sample of every model variable (analysis.py:82-90).

  The error threshold is the (1 - quantile) quantile of |y_exact| at full
  resolution; the comparison happens on the low-resolution grid.
  """
  max_error = float(np.quantile(np.abs(y_exact), 1 - quantile))
  out = {}
  for name, y_model in y_models.items():
    exact_low = unify_x_coords(y_model, y_exact)
    good = mostly_good(y_model, exact_low, max_error=max_error, frac_good=quantile)
    out[name] = calculate_survival(good, times)
  return out


def mean_absolute_error(y_models: Dict[str, np.ndarray], y_exact: np.ndarray,
                        times: np.ndarray, stop_times: Sequence[float]
                        ) -> Dict[str, np.ndarray]:
  """MAE over x and over times <= each stop time, per sample; NaNs propagate
  (run_evaluation.py:196-204).  Returns name -> [time_max, sample]."""
  times = np.asarray(times)
  out = {}
  for name, y_model in y_models.items():
    exact_low = unify_x_coords(y_model, y_exact)
    rows = []
    for time_max in stop_times:
      keep = times <= time_max
      rows.append(np.abs(y_model[:, keep] - exact_low[:, keep]).mean(axis=(1, 2)))
    out[name] = np.stack(rows)
  return out


# ---------------------------------------------------------------------------
# run_evaluation.py
# ---------------------------------------------------------------------------
def load_initial_conditions(y_exact: np.ndarray, resample_factor: int,
                            num_samples: Optional[int] = None) -> np.ndarray:
  """t = 0 of the exact data block-averaged to the model grid
  (run_evaluation.py:136-150)."""
  initial_conditions = duckarray.resample_mean(y_exact[:, 0, :], resample_factor)
  if np.isnan(initial_conditions).any():
    raise ValueError('initial conditions cannot have NaNs')
  if num_samples is not None and y_exact.shape[0] != num_samples:
    raise ValueError('invalid number of samples in exact dataset')
  return initial_conditions


def run_integrate(seed_and_initial_condition, model: model_lib.LearnedStencilModel,
                  hparams, times: np.ndarray, warmup: float = 0,
                  integrate_method: str = 'RK23'):
  """One sample, SciPy adaptive stepping, HIP right-hand side
  (run_evaluation.py:152-174)."""
  random_seed, y0 = seed_and_initial_condition
  _, equation_coarse = equations_lib.from_hparams(hparams, random_seed=random_seed)
  differentiator = integrate.SavedModelDifferentiator(None, equation_coarse,
                                                      hparams, model=model)
  solution, num_evals = integrate.odeint(y0, differentiator, warmup + times,
                                         method=integrate_method)
  return dict(y=solution, time=warmup + times,
              x=equation_coarse.grid.solution_x, num_evals=num_evals,
              sample=random_seed)


def run_integrate_batch(model: model_lib.LearnedStencilModel, hparams,
                        initial_conditions: np.ndarray, times: np.ndarray,
                        warmup: float = 0, max_step: float = 0.01,
                        scheme: str = 'bs3', first_seed: int = 0,
                        adaptive: Optional[bool] = None):
  """All samples of this rank together: adaptive RK23 with one controller per
  sample (``adaptive=True``; the default for scheme='bs3'), or the fixed step
  ``max_step`` with ``scheme``.

  Sample i uses random_seed = first_seed + i for its forcing, like the
  reference's per-seed equations.  With torch.distributed initialised the
  samples are split across ranks and the trajectories gathered on every rank.
  Returns dict(y [sample, time, x], time, x, num_evals, sample).
  """
  times = np.asarray(times, dtype=np.float64)
  total = initial_conditions.shape[0]
  rank, _, world = distributed.world_info()
  lo, hi = distributed.shard_bounds(total, rank, world)
  seeds = range(first_seed + lo, first_seed + hi)
  forcing = None
  if model.equation.has_time_dependent_forcing and hi > lo:
    eqs = [equations_lib.from_hparams(hparams, random_seed=s)[1] for s in seeds]
    forcing = model_lib.forcing_from_equations(eqs)
  if adaptive is None:   # RK23's own tableau: the reference's integrator, on the device
    adaptive = scheme == 'bs3'
  if hi > lo:
    ds = integrate.integrate_batch(model, initial_conditions[lo:hi], warmup + times,
                                   dt=max_step, scheme=scheme, forcing=forcing,
                                   adaptive=adaptive)
    y_local = _data(ds, 'y')
    evals_local = np.broadcast_to(np.asarray(_coord(ds, 'num_evals'), dtype=np.int64),
                                  (hi - lo,)).copy()
  else:
    dtype = np.float64 if adaptive else np.float32
    y_local = np.zeros((0, len(times), initial_conditions.shape[1]), dtype)
    evals_local = np.zeros(0, np.int64)
  y = y_local
  num_evals = evals_local
  if world > 1:
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
      raise RuntimeError('WORLD_SIZE > 1 but torch.distributed is not initialised')
    device = 'cuda' if dist.get_backend() == 'nccl' else 'cpu'
    y = distributed.gather_states(torch.from_numpy(np.ascontiguousarray(y_local)).to(device),
                                  total).cpu().numpy()
    num_evals = distributed.gather_states(
        torch.from_numpy(evals_local).to(device), total).cpu().numpy()
  return dict(y=y, time=warmup + times, x=model.equation.grid.solution_x,
              num_evals=num_evals, sample=first_seed + np.arange(total))


def evaluate(model: model_lib.LearnedStencilModel, hparams, y_exact: np.ndarray,
             times: np.ndarray, stop_times: Sequence[float] = (5, 10, 20, 40),
             quantiles: Sequence[float] = (0.8, 0.9, 0.95), warmup: float = 0,
             batched: bool = True, **kwargs):
  """Integrate every sample and score it (run_evaluation.py:181-216).

  ``y_exact`` [sample, time, x_high] holds the exact solution at ``times``.
  Returns dict(samples=..., mae [time_max, sample], survival [quantile, sample]).
  """
  y0 = load_initial_conditions(y_exact, hparams.resample_factor)
  if batched:
    samples = run_integrate_batch(model, hparams, y0, times, warmup=warmup, **kwargs)
  else:
    rows = [run_integrate((seed, y0[seed]), model, hparams, times, warmup=warmup, **kwargs)
            for seed in range(y0.shape[0])]
    samples = dict(y=np.stack([r['y'] for r in rows]), time=rows[0]['time'],
                   x=rows[0]['x'], num_evals=np.array([r['num_evals'] for r in rows]),
                   sample=np.array([r['sample'] for r in rows]))
  models = {'y_model': samples['y']}
  mae = mean_absolute_error(models, y_exact, samples['time'], stop_times)['y_model']
  survival = np.stack([
      mostly_good_survival(models, y_exact, samples['time'], q)['y_model']
      for q in quantiles])
  return dict(samples=samples, mae=mae, stop_times=np.asarray(stop_times),
              survival=survival, quantiles=np.asarray(quantiles))


# ---------------------------------------------------------------------------
# populations of models, scored on the device
# ---------------------------------------------------------------------------
def max_error_thresholds(y_exact, quantiles: Sequence[float]) -> np.ndarray:
  """``np.quantile(np.abs(y_exact), 1 - quantile)`` for every quantile from ONE sort
  (mostly_good_survival sorts the full-resolution data once per quantile and model).

  ``y_exact`` is a torch tensor, on the device or not, or anything
  ``torch.as_tensor`` takes.  Per quantile the two order statistics around
  ``(n - 1) (1 - quantile)`` are read and interpolated on the host as NumPy's
  'linear' method does, in the data's own precision, so the values are equal to
  ``np.quantile``'s, not merely close.  NaNs raise ValueError.
  """
  import torch
  tensor = y_exact if isinstance(y_exact, torch.Tensor) else torch.as_tensor(np.asarray(y_exact))
  if not tensor.is_floating_point():
    tensor = tensor.to(torch.float64)
  ordered, _ = torch.sort(tensor.detach().abs().reshape(-1))
  n = int(ordered.numel())
  if n == 0:
    raise ValueError('y_exact is empty')
  scalar = np.dtype(str(tensor.dtype).replace('torch.', '')).type
  picks = []
  for quantile in quantiles:
    virtual = (n - 1) * scalar(1 - quantile)
    lo = min(max(int(np.floor(virtual)), 0), n - 1)
    picks.append((lo, min(lo + 1, n - 1), scalar(virtual - scalar(np.floor(virtual)))))
  index = torch.tensor([i for lo, hi, _ in picks for i in (lo, hi)] + [n - 1],
                       dtype=torch.int64, device=ordered.device)
  values = ordered[index].cpu().numpy()   # (the only host read; NaNs sort last)
  if np.isnan(values[-1]):
    raise ValueError('y_exact cannot have NaNs')
  out = []
  for i, (_, _, t) in enumerate(picks):
    a, b = values[2 * i], values[2 * i + 1]
    diff = b - a
    out.append(float(a + diff * t if t < 0.5 else b - diff * (1 - t)))
  return np.asarray(out, dtype=np.float64)


class RolloutReference(object):
  """What scoring rollouts needs of the exact data and does not depend on the model,
  prepared once and kept on the device: ``exact_low`` [time, sample, x_low]
  (analysis.unify_x_coords, bit for bit, in the integrators' layout), ``y0`` =
  ``exact_low[0]`` (load_initial_conditions), ``max_error`` per quantile.  Reusable
  across calls and replicas."""

  def __init__(self, y_exact, times, resample_factor: int,
               quantiles: Sequence[float] = (0.8, 0.9, 0.95),
               stop_times: Sequence[float] = (5, 10, 20, 40)):
    torch = _lib.require_gpu()
    raw = _lib.as_device(y_exact)   # the one upload
    if raw.dim() != 3:
      raise ValueError('y_exact must be [sample, time, x_high]')
    self.times = np.asarray(times, dtype=np.float64)
    if self.times.shape != (int(raw.shape[1]),):
      raise ValueError('times must have one entry per time of y_exact')
    if int(raw.shape[2]) % int(resample_factor):
      raise ValueError('resample_factor must divide the size of y_exact')
    self.resample_factor = int(resample_factor)
    self.quantiles = np.asarray(quantiles, dtype=np.float64)
    self.stop_times = np.asarray(stop_times)
    # (in the precision of the data given, as evaluate's np.quantile)
    self.max_error = max_error_thresholds(raw, [float(q) for q in quantiles])
    self.y_exact = raw.to(torch.float64)
    self.exact_low = _lib.rollout_reference(self.y_exact,
                                            int(raw.shape[2]) // self.resample_factor)
    self.y0 = self.exact_low[0]

  @property
  def num_samples(self) -> int:
    return int(self.exact_low.shape[1])


def run_integrate_population(models: Sequence[model_lib.LearnedStencilModel], hparams, y0,
                             times: np.ndarray, warmup: float = 0, max_step: float = 0.01,
                             scheme: str = 'bs3', adaptive: Optional[bool] = None,
                             first_seed: int = 0, streams: int = 4,
                             launch: str = 'streams'):
  """run_integrate_batch for R models of one equation at once, everything staying on the
  device: returns ``(y [replica, time, sample, x], nfev [replica, sample], status
  [replica, sample])`` as device tensors, replica r's part being what ``models[r]``
  alone computes from ``y0`` (float64 with the adaptive integrator; float32 with the
  fixed step, where row 0 is ``y0``).

  The replicas are enqueued round-robin on ``min(R, streams)`` side streams that start
  behind the current stream and that the current stream then waits for; nothing waits on
  the host.  Single rank only: sharding stays with ``evaluate``.

  ``launch``: 'streams' is the above.  'population' rolls all replicas out in one launch
  on the current stream (``ddd_population_integrate_adaptive_f64`` /
  ``ddd_population_integrate_fixed``: replicas on the grid's second dimension, the
  forcing of every replica being ``models[0]``'s); configurations the library has no
  population kernel for raise NotImplementedError with its reason.  'auto' takes that
  route where it exists and the streams otherwise.  The tensors returned are the same
  either way, bit for bit.  Unlike the streams route the population route waits on the
  host once per call: building the per-call handle copies the replicas' packed weights
  device to device and synchronises the device (``ddd_population_create``).  With the
  fixed step it also takes a second ``[replica, time - 1, sample, x]`` buffer and one copy
  of it, because the library's rows are replica-major without row 0.  The handle and the
  models it references are released by the next population call whose launch has finished,
  by ``release_populations()``, or at interpreter exit.

  ``models`` may instead be a ``RolloutPopulation``: a handle kept across calls whose
  replicas were loaded from device tensors.  The rollout is then the one launch on the
  current stream whatever ``launch`` and ``streams`` say, with no handle built, no device
  synchronisation and no model handle per replica; the forcing is set on the population's
  model; the tensors returned are what the list of the models with those weights gives.
  """
  if launch not in LAUNCHES:
    raise ValueError('launch must be one of {}, got {!r}'.format(LAUNCHES, launch))
  torch = _lib.require_gpu()
  lib = _lib.load_library()
  if distributed.world_info()[2] > 1:
    raise RuntimeError('run_integrate_population runs on a single rank; shard with evaluate')
  population = models if isinstance(models, RolloutPopulation) else None
  if population is not None:
    population._check_open()   # pylint: disable=protected-access
    models = [population.model]
  models = list(models)
  if not models or len(set(id(m) for m in models)) != len(models):
    raise ValueError('models must be a non-empty sequence of distinct models')
  if int(streams) < 1:
    raise ValueError('streams must be at least 1')
  times = np.asarray(times, dtype=np.float64)
  if adaptive is None:
    adaptive = scheme == 'bs3'
  dtype = torch.float64 if adaptive else torch.float32
  y0 = _lib.as_device(y0, dtype)
  if y0.dim() != 2 or any(int(y0.shape[1]) != m.num_points for m in models):
    raise ValueError('y0 must be [sample, x] on the grid of every model')
  samples, points = int(y0.shape[0]), int(y0.shape[1])
  if not adaptive:
    spacing = np.diff(times)
    if len(times) < 2 or not np.allclose(spacing, spacing[0]):
      raise ValueError('times must be uniformly spaced')
    save_every = int(round(spacing[0] / max_step))
    if (save_every < 1 or
        abs(save_every * max_step - spacing[0]) > 1e-9 * max(1, spacing[0])):
      raise ValueError('output spacing {} is not a multiple of dt {}'
                       .format(spacing[0], max_step))
    num_steps = save_every * (len(times) - 1)
  if models[0].equation.has_time_dependent_forcing:
    eqs = [equations_lib.from_hparams(hparams, random_seed=s)[1]
           for s in range(first_seed, first_seed + samples)]
    forcing = model_lib.forcing_from_equations(eqs)
    for model in models:
      model.set_forcing(forcing)
  if population is None:
    for model in models:
      model._handle   # pylint: disable=pointless-statement,protected-access  (created here)
  # every buffer exists before the fork and is returned, so it outlives the join
  replicas = len(models) if population is None else population.replicas
  shape = (replicas, len(times), samples, points)
  y = torch.empty(shape, dtype=dtype, device=y0.device)
  nfev = torch.zeros((replicas, samples), dtype=torch.int32, device=y0.device)
  status = torch.zeros((replicas, samples), dtype=torch.int32, device=y0.device)
  if not adaptive:
    y[:, 0] = y0
    nfev.fill_(lib.ddd_scheme_stages(_lib.SCHEMES[scheme]) * num_steps)
  if population is not None:   # the kept handle: nothing is built, nothing waits
    _population_launch(lib, torch, population._handle, replicas, adaptive, y0, warmup + times,
                       max_step, scheme, num_steps if not adaptive else 0,
                       save_every if not adaptive else 1, y, nfev, status)
    population._launched()   # pylint: disable=protected-access
    return y, nfev, status
  if launch != 'streams':
    try:
      _population_rollout(lib, torch, models, adaptive, y0, warmup + times, max_step, scheme,
                          num_steps if not adaptive else 0, save_every if not adaptive else 1,
                          y, nfev, status)
      return y, nfev, status
    except NotImplementedError:
      if launch == 'population':
        raise
  current = torch.cuda.current_stream()
  side = [torch.cuda.Stream() for _ in range(min(len(models), int(streams)))]
  for stream in side:
    stream.wait_stream(current)
  for r, model in enumerate(models):
    with torch.cuda.stream(side[r % len(side)]):
      if adaptive:
        model.integrate_adaptive(y0, warmup + times, max_step=max_step,
                                 out=(y[r], nfev[r], status[r]))
      else:
        model.integrate_fixed(y0, num_steps, dt=max_step, t0=float((warmup + times)[0]),
                              scheme=scheme, save_every=save_every, out=y[r, 1:])
  for stream in side:
    current.wait_stream(stream)
  return y, nfev, status


LAUNCHES = ('streams', 'population', 'auto')

# population handles whose launch may still be running: (event recorded behind the launch,
# handle, the models -- models[0] is read by the launch, the others only kept alive)
_PENDING = []
# the RolloutPopulations not yet closed (closed at interpreter exit, before the library goes)
_OPEN = weakref.WeakSet()


def _reap_populations(lib, wait: bool = False):
  """Destroy the population handles whose launches have finished (``wait``: all of them,
  after waiting for their launches)."""
  for entry in list(_PENDING):
    event, handle, _ = entry
    if wait:
      event.synchronize()
    if event.query():
      lib.ddd_population_destroy(handle)
      _PENDING.remove(entry)


def release_populations():
  """Wait for the population launches still in flight and free their handles (the weight
  copies on the device) and the references to their models.  Also runs at interpreter
  exit; call it to give the memory back earlier."""
  if _PENDING and _lib._lib is not None:   # pylint: disable=protected-access
    try:
      _reap_populations(_lib._lib, wait=True)   # pylint: disable=protected-access
    except RuntimeError:   # (at exit: the device runtime may be gone before this runs)
      del _PENDING[:]


def _close_rollout_populations():
  for population in list(_OPEN):
    try:
      population.close()
    except RuntimeError:   # (at exit: the device runtime may be gone before this runs)
      pass


atexit.register(release_populations)
atexit.register(_close_rollout_populations)


def _population_rollout(lib, torch, models, adaptive, y0, times, max_step, scheme, num_steps,
                        save_every, y, nfev, status):
  """One ddd_population_integrate_* call on the current stream into ``y`` / ``nfev`` /
  ``status`` (run_integrate_population's buffers).  The handle is built from the models'
  handles for this call and destroyed once its launch has run (_reap_populations, at the
  next call); NotImplementedError where the library has no population kernel."""
  _reap_populations(lib)
  handles = (ctypes.c_void_p * len(models))(
      *[m._handle.value for m in models])   # pylint: disable=protected-access
  handle = ctypes.c_void_p()
  _lib.check_supported(lib.ddd_population_create(handles, len(models), ctypes.byref(handle)))
  try:
    _population_launch(lib, torch, handle, len(models), adaptive, y0, times, max_step, scheme,
                       num_steps, save_every, y, nfev, status)
  except Exception:
    torch.cuda.current_stream().synchronize()
    lib.ddd_population_destroy(handle)
    raise
  event = torch.cuda.Event()
  event.record()
  _PENDING.append((event, handle, list(models)))


def _population_launch(lib, torch, handle, replicas, adaptive, y0, times, max_step, scheme,
                       num_steps, save_every, y, nfev, status):
  """The ddd_population_integrate_* call of population `handle` on the current stream."""
  samples = int(y0.shape[0])
  stream = _lib.current_stream()
  if adaptive:
    times = np.ascontiguousarray(times, dtype=np.float64)
    _lib.check_supported(lib.ddd_population_integrate_adaptive_f64(
        handle, times.ctypes.data_as(_lib._D), int(times.size), 1e-3, 1e-6, float(max_step),
        0, y0.data_ptr(), y.data_ptr(), nfev.data_ptr(), status.data_ptr(), samples, stream))
  else:
    # (the library's rows are the saved states [replica, save, sample, x]; row 0 of y is y0)
    saved = torch.empty((replicas, int(y.shape[1]) - 1) + tuple(y0.shape), dtype=y.dtype,
                        device=y.device)
    _lib.check_supported(lib.ddd_population_integrate_fixed(
        handle, _lib.SCHEMES[scheme], float(times[0]), float(max_step), int(num_steps),
        int(save_every), y0.data_ptr(), saved.data_ptr(), samples, stream))
    y[:, 1:] = saved


class RolloutPopulation(object):
  """A population handle kept across calls: room for ``replicas`` sets of packed weights of
  ``model``'s architecture on the device (``ddd_population_create_replicated``), filled from
  device tensors by ``load`` (``ddd_population_load_weights``: the device packer of
  csrc/pack_device.hip, no host packing, no model handle per replica).  Pass it to
  ``run_integrate_population`` / ``evaluate_population`` in place of the models: the
  rollouts are then one launch on the current stream, and nothing is created, copied or
  waited for per call.  ``model`` plays models[0] -- launch parameters, forcing,
  projection tables -- and is kept alive here; until the first ``load`` every replica
  holds ``model``'s own weights.  NotImplementedError, with the library's reason, where
  there is no population kernel for ``model``.

  Loads and rollouts are ordered by the stream they are enqueued on: use one stream, or
  order the streams yourself."""

  def __init__(self, model: model_lib.LearnedStencilModel, replicas: int):
    _lib.require_gpu()
    lib = _lib.load_library()
    self.model = model
    self.replicas = int(replicas)
    self.n_weights = int(sum(w.size + b.size
                             for w, b in zip(model.conv_kernels, model.conv_biases)))
    self._event = None
    self._handle = None
    handle = ctypes.c_void_p()
    _lib.check_supported(lib.ddd_population_create_replicated(
        model._handle, self.replicas, ctypes.byref(handle)))   # pylint: disable=protected-access
    self._handle = handle
    _OPEN.add(self)

  def _check_open(self):
    if self._handle is None:
      raise ValueError('this RolloutPopulation is closed')

  def _launched(self):
    """Records the event close() waits for, behind what was just enqueued."""
    torch = _lib.require_gpu()
    if self._event is None:
      self._event = torch.cuda.Event()
    self._event.record()

  def load(self, weights, first_replica: int = 0):
    """Replicas first_replica .. first_replica + count - 1 take ``weights``: a contiguous
    float32 device tensor [count, n_weights] in ddd_model_create's layout (a Trainer's or
    PopulationTrainer's ``weights``).  Enqueued on the current stream; ``weights`` must stay
    unchanged until that work has run."""
    torch = _lib.require_gpu()
    self._check_open()
    if (not isinstance(weights, torch.Tensor) or weights.device.type != 'cuda' or
        weights.dtype != torch.float32 or weights.dim() != 2 or not weights.is_contiguous()):
      raise ValueError('weights must be a contiguous float32 device tensor [count, n_weights]')
    _lib.check(_lib.load_library().ddd_population_load_weights(
        self._handle, weights.data_ptr(), int(weights.shape[1]), int(first_replica),
        int(weights.shape[0]), _lib.current_stream()))
    self._launched()
    return self

  def load_models(self, models: Sequence[model_lib.LearnedStencilModel], first_replica: int = 0):
    """``load`` of the models' flat weights, stacked and uploaded."""
    torch = _lib.require_gpu()
    flat = np.stack([np.concatenate([np.concatenate([w.ravel(), b.ravel()])
                                     for w, b in zip(m.conv_kernels, m.conv_biases)])
                     for m in models]).astype(np.float32)
    weights = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
    self.load(weights, first_replica)
    # (the stream's caching allocator keeps `weights` whole until the load has run)
    return self

  def close(self):
    """Waits for the last load or rollout enqueued through this object, then frees the
    handle.  Also runs at interpreter exit (release_populations)."""
    handle, self._handle = self._handle, None
    if handle is None or _lib._lib is None:   # pylint: disable=protected-access
      return
    if self._event is not None:
      self._event.synchronize()
    _lib._lib.ddd_population_destroy(handle)   # pylint: disable=protected-access
    _OPEN.discard(self)

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass


def evaluate_population(models: Sequence[model_lib.LearnedStencilModel], hparams,
                        reference: RolloutReference, keep_trajectories: bool = False,
                        **kwargs):
  """``evaluate`` for R models at once (run_evaluation.py:181-216 per model): the
  rollouts of ``run_integrate_population`` (``kwargs``) from ``reference.y0``, scored by
  ``ddd_rollout_scores`` against ``reference``, then one host read.

  ``models`` may be a ``RolloutPopulation`` (see run_integrate_population).

  Returns dict(mae [replica, time_max, sample], survival [replica, quantile, sample],
  num_evals [replica, sample], status [replica, sample], stop_times, quantiles) and,
  with ``keep_trajectories``, samples = dict(y [replica, sample, time, x], time, x,
  sample).
  """
  torch = _lib.require_gpu()
  time = kwargs.get('warmup', 0) + reference.times
  y, nfev, status = run_integrate_population(models, hparams, reference.y0, reference.times,
                                             **kwargs)
  mae, survival = _lib.rollout_scores(y, reference.exact_low, time, reference.max_error,
                                      reference.quantiles, reference.stop_times)
  parts = (mae, survival, nfev, status)   # (int32 is exact in float64)
  host = torch.cat([part.reshape(-1).to(torch.float64) for part in parts]).cpu().numpy()
  mae, survival, nfev, status = (
      chunk.reshape(tuple(part.shape)) for chunk, part in
      zip(np.split(host, np.cumsum([part.numel() for part in parts])[:-1]), parts))
  out = dict(mae=mae, survival=survival, num_evals=nfev.astype(np.int64),
             status=status.astype(np.int32), stop_times=np.asarray(reference.stop_times),
             quantiles=np.asarray(reference.quantiles))
  if keep_trajectories:
    first = models.model if isinstance(models, RolloutPopulation) else models[0]
    out['samples'] = dict(
        y=y.permute(0, 2, 1, 3).contiguous().cpu().numpy(), time=time,
        x=first.equation.grid.solution_x,
        sample=kwargs.get('first_seed', 0) + np.arange(reference.num_samples))
  return out


def lyapunov_initial_tangents(batch: int, num_exponents: int, num_points: int, seed: int = 0):
  """The seeded draw lyapunov_exponents starts from: [batch, M, x] float32 on the host,
  the rows of each sample orthonormal (a float64 Gaussian draw, QR on the host)."""
  draw = np.random.RandomState(seed).randn(batch, num_points, num_exponents)
  q, _ = np.linalg.qr(draw)
  return np.ascontiguousarray(np.swapaxes(q, 1, 2)).astype(np.float32)


def lyapunov_exponents(model: model_lib.LearnedStencilModel, y0, num_exponents: int,
                       num_steps: int, steps_per_orthonormalisation: int,
                       warmup_steps: int = 0, seed: int = 0, weights=None, tangents=None):
  """The leading Lyapunov exponents of the learned right-hand side along the midpoint
  rollout from y0 [batch, x] (float32 device tensor), by Benettin's method: M = num_exponents
  orthonormal state tangents per sample are carried by ddd_tangent_rollout
  (model.tangent_time_evolution) for steps_per_orthonormalisation steps of
  equation.time_step, re-orthonormalised by a batched QR on the device, and log|diag R| is
  accumulated in float64.  Unforced, like the tangent rollout.

  warmup_steps: steps (in the same stretches, the rest as a shorter one) that align the
  tangents before anything is accumulated.  tangents: the initial [batch, M, x] instead of
  the seeded draw (lyapunov_initial_tangents).  num_steps must be a multiple of
  steps_per_orthonormalisation.

  Returns dict(exponents [batch, M] = log_growth.sum(0) / (num_steps * time_step),
  log_growth [stretches, batch, M] (float64 device tensors), state [batch, x],
  tangents [batch, M, x] (float32, orthonormal))."""
  torch = _lib.require_gpu()
  stretch = int(steps_per_orthonormalisation)
  if stretch < 1:
    raise ValueError('steps_per_orthonormalisation must be >= 1, got {}'.format(stretch))
  if int(num_steps) < 1 or int(num_steps) % stretch != 0:
    raise ValueError('num_steps = {} must be a positive multiple of '
                     'steps_per_orthonormalisation = {}'.format(num_steps, stretch))
  if int(warmup_steps) < 0:
    raise ValueError('warmup_steps must be >= 0, got {}'.format(warmup_steps))
  if not isinstance(y0, torch.Tensor) or y0.dim() != 2:
    raise ValueError('y0 must be a float32 device tensor [batch, x]')
  batch, n = y0.shape
  if not 1 <= int(num_exponents) <= min(_lib.MAX_TANGENTS, n):
    raise ValueError('num_exponents = {} out of range [1, {}]'.format(
        num_exponents, min(_lib.MAX_TANGENTS, n)))
  if tangents is None:
    tangents = torch.as_tensor(
        lyapunov_initial_tangents(batch, int(num_exponents), n, seed), device=y0.device)
  elif tuple(tangents.shape) != (batch, int(num_exponents), n):
    raise ValueError('tangents must have shape {}'.format((batch, int(num_exponents), n)))

  def advance(state, tangents, steps):
    state, tangents = model_lib.tangent_time_evolution(state, tangents, model, steps,
                                                       weights=weights)
    # (QR in float64: its rounding stays below the float32 rollout's)
    q, r = torch.linalg.qr(tangents.double().transpose(1, 2))
    growth = torch.log(torch.diagonal(r, dim1=1, dim2=2).abs())
    return state, q.transpose(1, 2).float().contiguous(), growth

  state = y0
  left = int(warmup_steps)
  while left > 0:
    state, tangents, _ = advance(state, tangents, min(left, stretch))
    left -= stretch
  log_growth = []
  for _ in range(int(num_steps) // stretch):
    state, tangents, growth = advance(state, tangents, stretch)
    log_growth.append(growth)
  log_growth = torch.stack(log_growth)
  exponents = log_growth.sum(0) / (int(num_steps) * model.equation.time_step)
  return dict(exponents=exponents, log_growth=log_growth, state=state, tangents=tangents)


def _data(ds, name):
  v = ds.data_vars[name]
  return np.asarray(v[1] if isinstance(v, tuple) else v)


def _coord(ds, name):
  v = ds.coords[name]
  return v[1] if isinstance(v, tuple) else v
