"""The reference's training loop (training.py) over the fused HIP loss-and-gradient
kernels (ddd_train_loss_grad, csrc/train.hip; with num_time_steps > 0
ddd_train_unrolled_loss_grad, csrc/train_unrolled.hip), without TensorFlow.

Reference: training.py:168-189 (set_data_dependent_hparams), 358-417
(determine_loss_scales), 570-636 (training_loop); model.py:664-810 for the loss.
The optimiser is torch.optim.Adam(beta2=0.99) on the piecewise-constant schedule
of learning_rates / learning_stops (training.py:191-218); the gradient comes from
the kernel, not from autograd.  Trainer.run / training_loop(fused=True) hand a whole
stretch of optimiser steps to the device in one call (ddd_train_run,
csrc/train_population.hip: the same gradient with Adam fused into its slab sum, error_max
decided on the device).  PopulationTrainer / training_population train R replicas of one
architecture -- R initial seeds, R learning-rate schedules -- in one such call
(ddd_train_population_run): the replicas are a second grid dimension of the same kernels,
and ddd_train_run is the population of one.
RolloutTrainer / fine_tune_on_rollouts train on the error of the model's own forced
rollout against exact data (ddd_train_rollout_loss_grad, csrc/train_rollout.hip), over
windows cut by make_rollout_windows.  RolloutTrainer.run / fine_tune_on_rollouts(fused=True)
hand a stretch of such steps to the device (ddd_train_rollout_run,
csrc/train_rollout_population.hip: norm, skip, clip and Adam decided there), and
RolloutPopulationTrainer / fine_tune_population_on_rollouts do so for R replicas at once;
PopulationTrainer.rollout_trainer() fine-tunes a trained population where it lies.
Inferer evaluates a trainer or a population over a whole dataset in one call
(ddd_eval_metrics, csrc/train_metrics.hip) and returns the reference's calculate_metrics
(training.py:433-491) per replica; training_loop / training_population(metrics=True) log
them for both splits as the reference's loop does.
"""
import copy
import json
import logging
import os
from typing import Dict, List, Sequence

import numpy as np

from . import _lib
from . import equations as equations_lib
from . import hparams as hparams_lib
from . import integrate
from . import model as model_lib


def check_supported(hparams):
  """Raises before any device work for what the training kernel does not carry."""
  equation_type = equations_lib.equation_type_from_hparams(hparams)
  if equation_type in equations_lib.FLUX_EQUATION_TYPES.values():
    raise NotImplementedError('training: numerical_flux (Godunov) equations are not '
                              'supported')
  if hparams.model_target not in ('coefficients', 'space_derivatives', 'time_derivative'):
    raise NotImplementedError('training: model_target {!r} is not supported'.format(
        hparams.model_target))
  if hparams.num_layers < 1:
    raise NotImplementedError('training: num_layers = 0 is not supported')
  if hparams.num_time_steps:
    raise NotImplementedError('training: num_time_steps > 0 (back-propagation through '
                              'time integration) is not supported')
  if hparams.kernel_size > 7 or hparams.filter_size > 64 or hparams.num_layers > 8:
    raise NotImplementedError('training: kernel_size <= 7, filter_size <= 64 and '
                              'num_layers <= 8 are supported')
  if hparams.model_target == 'time_derivative' and hparams.space_derivatives_weight:
    raise ValueError('space derivatives are not predicted by model {}'.format(
        hparams.model_target))


def check_supported_through_time(hparams):
  """check_supported for hparams with num_time_steps > 0 (the integrated_solution loss,
  ddd_train_unrolled_loss_grad): the same rules, and 1 <= num_time_steps <=
  DDD_MAX_TIME_STEPS."""
  steps = hparams.num_time_steps
  if not steps or steps < 1:
    raise NotImplementedError('training through time: num_time_steps = {} (>= 1 needed; '
                              'check_supported covers 0)'.format(steps))
  if steps > _lib.MAX_TIME_STEPS:
    raise NotImplementedError('training through time: num_time_steps = {} > {}'.format(
        steps, _lib.MAX_TIME_STEPS))
  single = copy.copy(hparams)
  single.num_time_steps = 0
  check_supported(single)


def _checker(hparams):
  return check_supported_through_time if hparams.num_time_steps else check_supported


def determine_loss_scales(dataset: model_lib.DeviceDataset, hparams):
  """training.py:358-417 on a dataset already made (make_dataset, repeat=False):
  (error_floor [channel], error_scale [2, channel]).  Zero predictions over the whole
  dataset then give a weighted loss of 1.0."""
  labels = dataset.labels.double().cpu().numpy()
  baseline = dataset.baseline.double().cpu().numpy()
  baseline_error = (labels - baseline) ** 2
  error_floor = np.maximum(
      np.percentile(baseline_error, 100 * hparams.error_floor_quantile, axis=(0, 1)),
      1e-12)
  predictions = np.zeros_like(labels)
  components = np.stack(model_lib.abs_and_rel_error(predictions, labels, baseline,
                                                    error_floor))
  mean_error = np.mean(components, axis=(1, 2))
  error_scale = np.where(mean_error > 0, 1.0 / np.where(mean_error > 0, mean_error, 1.0), 0)
  return error_floor, error_scale


def set_data_dependent_hparams(hparams, snapshots, seed: int = 0):
  """training.py:168-189: adds error_scale (2 * channel) and error_floor (channel)."""
  dataset = model_lib.make_dataset(snapshots, hparams, repeat=False, seed=seed)
  error_floor, error_scale = determine_loss_scales(dataset, hparams)
  hparams.error_scale = error_scale.ravel().tolist()
  hparams.error_floor = error_floor.tolist()
  return dataset


def learning_rate(hparams, step: int) -> float:
  """tf.train.piecewise_constant(step, learning_stops[:-1], learning_rates)."""
  for stop, rate in zip(hparams.learning_stops[:-1], hparams.learning_rates):
    if step <= stop:
      return float(rate)
  return float(hparams.learning_rates[len(hparams.learning_stops) - 1])


def _train_config(model: model_lib.LearnedStencilModel) -> _lib.DDDConfig:
  hp = model.hparams
  cfg = model._base_config(model.equation, model.stencil_size)
  cfg.model_target = _lib.MODEL_TARGETS[hp.model_target]
  cfg.num_layers = hp.num_layers
  cfg.filter_size = hp.filter_size
  cfg.kernel_size = hp.kernel_size
  cfg.activation = _lib.ACTIVATIONS[hp.nonlinearity]
  cfg.polynomial_accuracy_order = int(hp.polynomial_accuracy_order or 0)
  cfg.ensure_unbiased_coefficients = int(bool(hp.ensure_unbiased_coefficients))
  for i, size in enumerate(model.input_sizes):
    cfg.input_sizes[i] = size
  return cfg


class Trainer(object):
  """A flat float32 device weight vector (ddd_model_create layout), the kernel's
  loss and gradient, and Adam(beta2=0.99) on the learning-rate schedule."""

  def __init__(self, model: model_lib.LearnedStencilModel, hparams=None):
    import torch
    self.torch = torch
    self.model = model
    self.hparams = hparams or model.hparams
    _checker(self.hparams)(self.hparams)
    self.cfg = _train_config(model)
    flat = np.concatenate([np.concatenate([w.ravel(), b.ravel()])
                           for w, b in zip(model.conv_kernels, model.conv_biases)])
    self.weights = torch.nn.Parameter(
        torch.as_tensor(flat.astype(np.float32), device='cuda'))
    self.nullspace = self.bias = None
    if model.input_sizes:   # null spaces computed once (the model's)
      self.nullspace = torch.as_tensor(np.concatenate(
          [n.ravel() for n in model.nullspaces]).astype(np.float32), device='cuda')
      self.bias = torch.as_tensor(np.concatenate(
          [b.ravel() for b in model.biases]).astype(np.float32), device='cuda')
    self.optimizer = torch.optim.Adam([self.weights], lr=learning_rate(self.hparams, 0),
                                      betas=(0.9, 0.99))
    self.step_count = 0

  def coefficients(self, num_channels: int):
    """(error_floor, coef_abs, coef_rel) host vectors: error_scale, the normalised
    abs/rel weights and the channel weights folded together."""
    hp = self.hparams
    weights = model_lib.loss_weights(hp, num_channels)
    scale = np.array(hp.error_scale, np.float64).reshape(2, -1)
    coef = weights * scale
    return np.array(hp.error_floor, np.float64), coef[0], coef[1]

  def loss_and_grad(self, dataset, sample_index=None, want_grad=True,
                    want_predictions=False, batch=None):
    """(loss_per_head [2, channel] float64 host, grad or None, predictions or None);
    error_max clipping as two calls (ddd1d.h)."""
    hp = self.hparams
    heads = int(dataset.labels.shape[-1])
    floor, coef_abs, coef_rel = self.coefficients(heads)
    scale = np.array(hp.error_scale, np.float64).reshape(2, -1)
    if batch is None and sample_index is None:
      batch = dataset.num_examples
    call = dict(nullspace=self.nullspace, bias=self.bias, sample_index=sample_index,
                batch=batch, want_predictions=want_predictions)
    if hp.error_max and want_grad:
      means, _, _ = self._call(dataset, floor, coef_abs, coef_rel, want_grad=False, **call)
      clipped = means.double().cpu().numpy() * scale >= hp.error_max
      coef_abs = np.where(clipped[0], 0.0, coef_abs)
      coef_rel = np.where(clipped[1], 0.0, coef_rel)
    means, grad, preds = self._call(dataset, floor, coef_abs, coef_rel,
                                    want_grad=want_grad, **call)
    per_head = means.double().cpu().numpy() * scale
    if hp.error_max:
      per_head = np.where(per_head < hp.error_max, per_head, hp.error_max)
    return per_head, grad, preds

  def _call(self, dataset, floor, coef_abs, coef_rel, **kwargs):
    steps = self.hparams.num_time_steps
    if steps:   # the integrated heads too: the kernel through time
      return _lib.train_unrolled_loss_grad(
          self.cfg, self.weights.detach(), dataset.inputs, dataset.labels, dataset.baseline,
          floor, coef_abs, coef_rel, steps, self.model.equation.time_step, **kwargs)
    means, grad, preds = _lib.train_loss_grad(
        self.cfg, self.weights.detach(), dataset.inputs, dataset.labels, dataset.baseline,
        floor, coef_abs, coef_rel, **kwargs)
    return means, grad, preds

  def step(self, dataset, sample_index):
    """One optimiser step on the minibatch `sample_index`; returns loss_per_head."""
    for group in self.optimizer.param_groups:
      group['lr'] = learning_rate(self.hparams, self.step_count)
    per_head, grad, _ = self.loss_and_grad(dataset, sample_index)
    self.weights.grad = grad
    self.optimizer.step()
    self.step_count += 1
    return per_head

  def _adam_state(self):
    """The optimiser's state of the weights (exp_avg, exp_avg_sq, step), created as
    torch.optim.Adam creates it on its first step."""
    torch = self.torch
    state = self.optimizer.state[self.weights]
    if len(state) == 0:
      state['step'] = torch.tensor(0.0, dtype=torch.float32)
      state['exp_avg'] = torch.zeros_like(self.weights, memory_format=torch.preserve_format)
      state['exp_avg_sq'] = torch.zeros_like(self.weights,
                                             memory_format=torch.preserve_format)
    return state

  def run(self, dataset, num_steps: int, sample_index=None) -> np.ndarray:
    """num_steps optimiser steps in one ddd_train_run call: the gradient of `step`, Adam
    fused into its slab sum, error_max decided on the device; the host reads once, after
    the call.  Returns loss_per_head of every step [num_steps, 2, channel], scaled and
    clipped as `step` returns it.  Minibatches: dataset.batch_indices(), drawn up front,
    or sample_index, an int32 [num_steps, batch] tensor / array.  Shares the optimiser
    state with `step`, so the two may be interleaved."""
    torch = self.torch
    hp = self.hparams
    num_steps = int(num_steps)
    if num_steps < 1:
      raise ValueError('num_steps = {} (>= 1)'.format(num_steps))
    if sample_index is None:
      batches = dataset.batch_indices()
      rows = [next(batches) for _ in range(num_steps)]
      sample_index = torch.stack([torch.as_tensor(r, dtype=torch.int32) for r in rows])
    sample_index = torch.as_tensor(sample_index, dtype=torch.int32).to(
        self.weights.device).contiguous()
    if sample_index.dim() != 2 or int(sample_index.shape[0]) != num_steps:
      raise ValueError('sample_index must be [num_steps, batch]')
    heads = int(dataset.labels.shape[-1])
    floor, coef_abs, coef_rel = self.coefficients(heads)
    scale = np.array(hp.error_scale, np.float64).reshape(2, -1)
    rates = [learning_rate(hp, self.step_count + k) for k in range(num_steps)]
    state = self._adam_state()
    group = self.optimizer.param_groups[0]
    steps = hp.num_time_steps or 0
    log, _ = _lib.train_run(
        self.cfg, self.weights.detach(), state['exp_avg'], state['exp_avg_sq'],
        dataset.inputs, dataset.labels, dataset.baseline, sample_index, rates, floor,
        coef_abs, coef_rel, first_step=int(state['step']), betas=group['betas'],
        epsilon=group['eps'], num_time_steps=steps,
        time_step=self.model.equation.time_step if steps else 0.0,
        error_max=hp.error_max or 0.0, error_scale=scale, nullspace=self.nullspace,
        bias=self.bias)
    state['step'] += num_steps
    group['lr'] = rates[-1]
    self.step_count += num_steps
    per_head = log.double().cpu().numpy() * scale
    if hp.error_max:
      per_head = np.where(per_head < hp.error_max, per_head, hp.error_max)
    return per_head

  def export(self) -> model_lib.LearnedStencilModel:
    """The current weights as a LearnedStencilModel (same equation / hparams)."""
    flat = self.weights.detach().cpu().numpy()
    kernels, biases, offset = [], [], 0
    for w, b in zip(self.model.conv_kernels, self.model.conv_biases):
      kernels.append(flat[offset:offset + w.size].reshape(w.shape))
      offset += w.size
      biases.append(flat[offset:offset + b.size].reshape(b.shape))
      offset += b.size
    return model_lib.LearnedStencilModel(
        self.model.equation, self.hparams, kernels, biases, self.model.nullspaces,
        self.model.biases)


class RolloutWindows(object):
  """The windows make_rollout_windows cut: tensors with one row per window (on the device
  where there is one) and the clock they share."""

  def __init__(self, y0, targets, t0, forcing, dt, num_steps, save_every, sample, start):
    self.y0 = y0                  # [W, N] float32
    self.targets = targets        # [W, num_steps // save_every, N] float32
    self.t0 = t0                  # [W] float64
    self.forcing = forcing        # forcing_kernel_tables' keys, one row per window, or None
    self.dt = dt                  # the step of the midpoint rule
    self.num_steps = num_steps
    self.save_every = save_every
    self.sample = sample          # [W] host: the sample of y_exact a window is cut from
    self.start = start            # [W] host: the index into `times` of its start

  @property
  def num_windows(self) -> int:
    return int(self.y0.shape[0])

  @property
  def num_saved(self) -> int:
    return self.num_steps // self.save_every


def make_rollout_windows(y_exact, times, hparams, num_steps: int, save_every: int,
                         stride: int = 1, first_seed: int = 0, device=None) -> RolloutWindows:
  """Training windows of rollout error from exact data: y_exact [sample, time, x_fine] at
  the uniform `times` is coarse-grained with the equation's own resample method
  (Grid.resample: block means for conservative equations, subsampling otherwise, as
  evaluation.RolloutReference and load_initial_conditions do) and cut into windows
  (sample, start) every `stride` saved times: y0 = the coarse state at times[start], targets
  the num_steps // save_every saved states after it, t0 = times[start].  The model takes
  save_every midpoint steps of dt = (times[1] - times[0]) / save_every between two saved
  times.  Sample i is forced with random_seed = first_seed + i, as run_integrate_batch
  forces it.  device: 'cuda' where there is one, else 'cpu'."""
  import torch
  if device is None:
    device = 'cuda' if torch.cuda.is_available() else 'cpu'
  y_exact = np.asarray(y_exact)
  times = np.asarray(times, np.float64)
  num_steps, save_every, stride = int(num_steps), int(save_every), int(stride)
  if y_exact.ndim != 3 or times.ndim != 1 or y_exact.shape[1] != times.shape[0]:
    raise ValueError('expected y_exact [sample, time, x_fine] and times [time]')
  if save_every < 1 or num_steps < 1 or num_steps % save_every or stride < 1:
    raise ValueError('save_every = {} must be >= 1 and divide num_steps = {}; stride = {} '
                     '(>= 1)'.format(save_every, num_steps, stride))
  if times.shape[0] < 2:
    raise ValueError('no window fits: {} saved times'.format(times.shape[0]))
  steps = np.diff(times)
  if not (steps[0] > 0) or not np.allclose(steps, steps[0], rtol=1e-9, atol=0.0):
    raise ValueError('times must be uniform and increasing')
  _, coarse = equations_lib.from_hparams(hparams, random_seed=first_seed)
  dt = float(steps[0]) / save_every
  if dt > coarse.time_step * (1 + 1e-9):
    raise ValueError('dt = {:g} between model steps exceeds equation.time_step = {:g}: '
                     'raise save_every'.format(dt, coarse.time_step))
  grid = coarse.grid
  if y_exact.shape[2] != grid.reference_num_points:
    raise ValueError('y_exact has {} points, the reference grid {}'.format(
        y_exact.shape[2], grid.reference_num_points))
  num_saved = num_steps // save_every
  starts = np.arange(0, times.shape[0] - num_saved, stride)
  if starts.size == 0:
    raise ValueError('no window fits: {} saved times, {} needed'.format(times.shape[0],
                                                                        num_saved + 1))
  low = grid.resample(y_exact.astype(np.float64), axis=-1)   # [sample, time, N]
  samples = y_exact.shape[0]
  sample = np.repeat(np.arange(samples), starts.size)
  start = np.tile(starts, samples)
  y0 = low[sample, start].astype(np.float32)
  targets = low[sample[:, None], start[:, None] + 1 + np.arange(num_saved)[None, :]].astype(
      np.float32)
  forcing = None
  if coarse.has_time_dependent_forcing:
    eqs = [equations_lib.from_hparams(hparams, random_seed=first_seed + i)[1]
           for i in range(samples)]
    tables = model_lib.forcing_kernel_tables(model_lib.forcing_from_equations(eqs), grid)
    forcing = {name: torch.as_tensor(np.ascontiguousarray(tables[name][sample]), device=device)
               for name in ('amplitude', 'omega', 'phase', 'k_index')}
    forcing['spatial_phase'] = torch.as_tensor(
        np.ascontiguousarray(tables['spatial_phase']), device=device)
  return RolloutWindows(
      torch.as_tensor(np.ascontiguousarray(y0), device=device),
      torch.as_tensor(np.ascontiguousarray(targets), device=device),
      torch.as_tensor(np.ascontiguousarray(times[start]), device=device), forcing, dt,
      num_steps, save_every, sample, start)


def _rollout_step_weights(windows: RolloutWindows, step_weights, device):
  """The loss constants c_j as a float32 device tensor [num_saved]: 1 / num_saved each by
  default, else the given host or device values."""
  import torch
  saved = windows.num_saved
  if step_weights is None:
    return torch.full((saved,), 1.0 / saved, dtype=torch.float32, device=device)
  return torch.as_tensor(step_weights, dtype=torch.float32).to(device).contiguous()


def _rollout_minibatches(sample_index, num_steps: int, replicas: int, windows, device):
  """sample_index of a rollout run as a contiguous int32 device tensor [K, batch] or
  [K, R, batch]; None: every step trains on all windows."""
  import torch
  if sample_index is None:
    sample_index = torch.arange(windows.num_windows, dtype=torch.int32).repeat(num_steps, 1)
  sample_index = torch.as_tensor(sample_index, dtype=torch.int32).to(device).contiguous()
  if (sample_index.dim() not in (2, 3) or int(sample_index.shape[0]) != num_steps or
      (sample_index.dim() == 3 and int(sample_index.shape[1]) != replicas)):
    raise ValueError('sample_index must be [num_steps, batch] or [num_steps, R, batch]')
  return sample_index


class RolloutTrainer(object):
  """Training on rollout error (ddd_train_rollout_loss_grad, csrc/train_rollout.hip): the
  flat weight vector, null spaces and Adam(beta2 = 0.99) of Trainer; the loss is
  sum_j step_weights[j] step_means[j] over the saved steps of RolloutWindows, its gradient
  one launch.  clip_norm: the gradient is rescaled to that global norm where it exceeds
  it, on the device.  `run` hands a whole stretch of steps to the device
  (ddd_train_rollout_run, csrc/train_rollout_population.hip, as the population of one)."""

  def __init__(self, model: model_lib.LearnedStencilModel, hparams=None, clip_norm=None):
    hparams = hparams or model.hparams
    single = copy.copy(hparams)   # (the horizon is the windows', not num_time_steps)
    single.num_time_steps = 0
    check_supported(single)
    base = Trainer(model, hparams)
    self._base = base
    self.torch = base.torch
    self.model, self.hparams, self.cfg = model, hparams, base.cfg
    self.weights, self.optimizer = base.weights, base.optimizer
    self.nullspace, self.bias = base.nullspace, base.bias
    self.clip_norm = None if clip_norm is None else float(clip_norm)
    self.step_count = 0
    self.skipped_steps = 0
    self._workspace = None

  def loss_and_grad(self, windows: RolloutWindows, sample_index=None, step_weights=None,
                    want_grad=True, want_trajectory=False):
    """(step_means [num_saved] device, grad or None, trajectory or None) on the windows
    `sample_index` (int32 device tensor; None: all).  step_weights: [num_saved] host or
    device values c_j, 1 / num_saved each by default."""
    torch = self.torch
    step_weights = _rollout_step_weights(windows, step_weights, self.weights.device)
    batch = windows.num_windows if sample_index is None else int(sample_index.shape[0])
    need = _lib.load_library().ddd_train_rollout_workspace_bytes(
        self.cfg, batch, windows.num_steps)
    if self._workspace is None or self._workspace.numel() < need:
      self._workspace = torch.empty(max(need, 1), dtype=torch.uint8,
                                    device=self.weights.device)
    return _lib.train_rollout_loss_grad(
        self.cfg, self.weights.detach(), windows.y0, windows.targets, step_weights,
        windows.num_steps, windows.save_every, windows.dt, t0=windows.t0,
        forcing=windows.forcing, nullspace=self.nullspace, bias=self.bias,
        sample_index=sample_index, want_grad=want_grad, want_trajectory=want_trajectory,
        workspace=self._workspace)

  def step(self, windows: RolloutWindows, sample_index, lr: float, step_weights=None):
    """One optimiser step at learning rate lr on the windows `sample_index`; returns
    step_means.  A gradient that is not finite everywhere leaves the weights and Adam's
    state as they are and is counted in skipped_steps."""
    torch = self.torch
    means, grad, _ = self.loss_and_grad(windows, sample_index, step_weights)
    norm = torch.linalg.vector_norm(grad)
    if not bool(torch.isfinite(norm)):   # (the one host read of a step)
      self.skipped_steps += 1
      return means
    if self.clip_norm is not None:
      grad = grad * torch.clamp(self.clip_norm / (norm + 1e-12), max=1.0)
    for group in self.optimizer.param_groups:
      group['lr'] = float(lr)
    self.weights.grad = grad
    self.optimizer.step()
    self.step_count += 1
    return means

  def run(self, windows: RolloutWindows, num_steps: int, lr, sample_index,
          step_weights=None):
    """num_steps optimiser steps in one ddd_train_rollout_run call, as the population of
    one on this trainer's weights: the gradient of `step`, the norm, the skip of a step
    whose gradient is not finite, the clip and Adam on the device; the host reads once,
    after the call.  lr: one rate or one per step; sample_index: int32 [num_steps, batch]
    (None: all windows every step).  Returns step_means [num_steps, num_saved] (device).
    Shares the optimiser state with `step`, so the two may be interleaved; skipped steps
    are counted in skipped_steps and not in step_count, as `step` counts them."""
    torch = self.torch
    num_steps = int(num_steps)
    if num_steps < 1:
      raise ValueError('num_steps = {} (>= 1)'.format(num_steps))
    rates = ([float(lr)] * num_steps if np.isscalar(lr) else [float(rate) for rate in lr])
    if len(rates) != num_steps:
      raise ValueError('lr must be one rate or one per step')
    device = self.weights.device
    sample_index = _rollout_minibatches(sample_index, num_steps, 1, windows, device)
    state = self._base._adam_state()
    group = self.optimizer.param_groups[0]
    adam_step = torch.tensor([int(state['step'])], dtype=torch.int32, device=device)
    log, norms, _ = _lib.train_rollout_run(
        self.cfg, self.weights.detach()[None], state['exp_avg'][None],
        state['exp_avg_sq'][None], adam_step, windows.y0, windows.targets,
        _rollout_step_weights(windows, step_weights, device), windows.num_steps,
        windows.save_every, windows.dt, sample_index, [rates], betas=group['betas'],
        epsilon=group['eps'], clip_norm=self.clip_norm or 0.0, t0=windows.t0,
        forcing=windows.forcing, nullspace=self.nullspace, bias=self.bias)
    skipped = int((~torch.isfinite(norms)).sum())   # (the one host read of the run)
    state['step'] += num_steps - skipped
    group['lr'] = rates[-1]
    self.step_count += num_steps - skipped
    self.skipped_steps += skipped
    return log[:, 0]

  def export(self) -> model_lib.LearnedStencilModel:
    """The current weights as a LearnedStencilModel (same equation / hparams)."""
    return self._base.export()


def _rollout_stretches(opt_steps: int, step: int, eval_interval: int):
  """The lengths of the stretches between two evaluations of a horizon of opt_steps steps
  that begins at global step `step`: an evaluation follows every eval_interval-th global
  step and the horizon's last step."""
  lengths, begun = [], 0
  for k in range(opt_steps):
    if (step + k + 1) % eval_interval == 0 or k == opt_steps - 1:
      lengths.append(k + 1 - begun)
      begun = k + 1
  return lengths


def fine_tune_on_rollouts(model: model_lib.LearnedStencilModel, y_exact, times, hparams,
                          checkpoint_dir: str, horizons, save_every: int, batch: int,
                          learning_rate: float, seed: int = 0, stride: int = 1,
                          first_seed: int = 0, clip_norm=None,
                          fused: bool = False) -> List[Dict[str, float]]:
  """A curriculum of growing horizons over one RolloutTrainer: for every (opt_steps,
  num_steps) of `horizons`, opt_steps optimiser steps on seeded minibatches of `batch`
  windows of num_steps model steps (make_rollout_windows of y_exact / times).  Writes
  hparams.json + model.npz to checkpoint_dir.  Returns one row at the start of every
  horizon, at every hparams.eval_interval-th step and at the end of every horizon:
  'step' (over all horizons), 'num_steps', 'loss' and 'step_means' over ALL windows of
  that horizon (forward only, uniform step weights), and 'skipped_steps' so far.
  fused: every stretch between two evaluations is one RolloutTrainer.run call (the same
  minibatches) instead of RolloutTrainer.step calls."""
  hparams = copy.deepcopy(hparams)
  trainer = RolloutTrainer(model, hparams, clip_norm=clip_norm)
  torch = trainer.torch
  os.makedirs(checkpoint_dir, exist_ok=True)
  hparams_lib.save_hparams(hparams, checkpoint_dir)
  rs = np.random.RandomState(seed)
  rows, step = [], 0

  def evaluate(windows):
    means, _, _ = trainer.loss_and_grad(windows, want_grad=False)
    means = means.double().cpu().numpy()
    rows.append({'step': step, 'num_steps': windows.num_steps, 'loss': float(means.mean()),
                 'step_means': means.tolist(), 'skipped_steps': trainer.skipped_steps})

  for opt_steps, num_steps in horizons:
    windows = make_rollout_windows(y_exact, times, hparams, num_steps, save_every,
                                   stride=stride, first_seed=first_seed)
    count = min(int(batch), windows.num_windows)
    evaluate(windows)
    if fused:
      for length in _rollout_stretches(int(opt_steps), step, hparams.eval_interval):
        index = np.stack([rs.choice(windows.num_windows, size=count, replace=False)
                          .astype(np.int32) for _ in range(length)])
        trainer.run(windows, length, learning_rate, index)
        step += length
        evaluate(windows)
      continue
    for k in range(int(opt_steps)):
      index = torch.as_tensor(rs.choice(windows.num_windows, size=count, replace=False)
                              .astype(np.int32), device=trainer.weights.device)
      trainer.step(windows, index, learning_rate)
      step += 1
      if step % hparams.eval_interval == 0 or k == int(opt_steps) - 1:
        evaluate(windows)
  trainer.export().save(checkpoint_dir)
  return rows


def _checked_population(models, hparams, checker) -> list:
  """What PopulationTrainer and RolloutPopulationTrainer refuse before any device work: a
  replica count outside 1 .. DDD_MAX_REPLICAS, hparams that `checker` raises for, and
  replicas that differ in their equation, architecture or grid.  Returns list(models)."""
  models = list(models)
  if not 1 <= len(models) <= _lib.MAX_REPLICAS:
    raise ValueError('{} models (1 .. {})'.format(len(models), _lib.MAX_REPLICAS))
  checker(hparams)
  configs = [bytes(_train_config(model)) for model in models]
  for r, model in enumerate(models):
    if type(model.equation) is not type(models[0].equation):
      raise ValueError('replica {} solves {}, replica 0 {}: one equation per '
                       'population'.format(r, type(model.equation).__name__,
                                           type(models[0].equation).__name__))
    if (configs[r] != configs[0] or [w.shape for w in model.conv_kernels] !=
        [w.shape for w in models[0].conv_kernels]):
      raise ValueError('replica {} differs from replica 0 in its architecture or grid: '
                       'one architecture per population'.format(r))
  return models


class PopulationTrainer(object):
  """R replicas of one architecture on one equation, trained together
  (ddd_train_population_run, csrc/train_population.hip): `weights` is one [R, n_weights]
  device tensor, Adam's state (`adam_m`, `adam_v`, beta2 = 0.99 as Trainer) [R, n_weights],
  one step count for all.  learning_rates[r], when given, replaces hparams.learning_rates
  for replica r on the same learning_stops.  Replica r of `run` is bit for bit
  Trainer.run on models[r] with that schedule."""

  BETAS = (0.9, 0.99)
  EPSILON = 1e-8   # torch.optim.Adam's default, Trainer's

  def __init__(self, models: Sequence[model_lib.LearnedStencilModel], hparams,
               learning_rates=None):
    models = _checked_population(models, hparams, _checker(hparams))
    if learning_rates is not None:
      learning_rates = [[float(rate) for rate in row] for row in learning_rates]
      if len(learning_rates) != len(models):
        raise ValueError('learning_rates must have one row per replica')
      if any(len(row) != len(hparams.learning_rates) for row in learning_rates):
        raise ValueError('every row of learning_rates must have len(hparams.learning_rates) '
                         '= {} entries'.format(len(hparams.learning_rates)))
    import torch
    self.torch = torch
    self.models = models
    self.hparams = hparams
    self.replica_hparams = []
    for r in range(len(models)):
      hp = copy.copy(hparams)
      if learning_rates is not None:
        hp.learning_rates = learning_rates[r]
      self.replica_hparams.append(hp)
    # one Trainer per replica for what needs no population call (the forward-only loss,
    # export), each on its row of `weights`
    self.trainers = [Trainer(model, hparams) for model in models]
    self.cfg = self.trainers[0].cfg
    self.nullspace, self.bias = self.trainers[0].nullspace, self.trainers[0].bias
    self.weights = torch.stack([t.weights.detach() for t in self.trainers]).contiguous()
    for r, trainer in enumerate(self.trainers):
      trainer.weights = self.weights[r]
      trainer.optimizer = None   # (the state is this object's)
    self.adam_m = torch.zeros_like(self.weights)
    self.adam_v = torch.zeros_like(self.weights)
    self.step_count = 0
    self._rollout_population = None   # rollout_population()'s handle, built on first use

  @property
  def replicas(self) -> int:
    return len(self.models)

  def learning_rate_table(self, num_steps: int) -> List[List[float]]:
    """[R][num_steps]: replica r's learning rate at steps step_count .. + num_steps - 1."""
    return [[learning_rate(hp, self.step_count + k) for k in range(num_steps)]
            for hp in self.replica_hparams]

  def run(self, dataset, num_steps: int, sample_index=None) -> np.ndarray:
    """num_steps optimiser steps of every replica in one call.  Returns loss_per_head
    [num_steps, R, 2, channel], scaled and clipped as Trainer.run returns it.
    Minibatches: dataset.batch_indices(), drawn up front and shared, or sample_index,
    int32 [num_steps, batch] (shared) or [num_steps, R, batch]."""
    torch = self.torch
    hp = self.hparams
    num_steps = int(num_steps)
    if num_steps < 1:
      raise ValueError('num_steps = {} (>= 1)'.format(num_steps))
    if sample_index is None:
      batches = dataset.batch_indices()
      rows = [next(batches) for _ in range(num_steps)]
      sample_index = torch.stack([torch.as_tensor(r, dtype=torch.int32) for r in rows])
    sample_index = torch.as_tensor(sample_index, dtype=torch.int32).to(
        self.weights.device).contiguous()
    if (sample_index.dim() not in (2, 3) or int(sample_index.shape[0]) != num_steps or
        (sample_index.dim() == 3 and int(sample_index.shape[1]) != self.replicas)):
      raise ValueError('sample_index must be [num_steps, batch] or [num_steps, R, batch]')
    heads = int(dataset.labels.shape[-1])
    floor, coef_abs, coef_rel = self.trainers[0].coefficients(heads)
    scale = np.array(hp.error_scale, np.float64).reshape(2, -1)
    steps = hp.num_time_steps or 0
    log, _ = _lib.train_population_run(
        self.cfg, self.weights, self.adam_m, self.adam_v, dataset.inputs, dataset.labels,
        dataset.baseline, sample_index, self.learning_rate_table(num_steps), floor, coef_abs,
        coef_rel, first_step=self.step_count, betas=self.BETAS, epsilon=self.EPSILON,
        num_time_steps=steps,
        time_step=self.models[0].equation.time_step if steps else 0.0,
        error_max=hp.error_max or 0.0, error_scale=scale, nullspace=self.nullspace,
        bias=self.bias)
    self.step_count += num_steps
    per_head = log.double().cpu().numpy() * scale
    if hp.error_max:
      per_head = np.where(per_head < hp.error_max, per_head, hp.error_max)
    return per_head

  def loss(self, dataset) -> np.ndarray:
    """loss_per_head [R, 2, channel] over the whole dataset, forward only: one
    ddd_eval_metrics call and one host read for all replicas.  Its two loss rows are bit
    for bit the head_means of a forward-only ddd_train_loss_grad /
    ddd_train_unrolled_loss_grad call per replica."""
    sums, _, _ = Inferer(dataset, self).run_async()
    return _scaled_loss_per_head(sums, self.hparams)

  def export(self) -> List[model_lib.LearnedStencilModel]:
    """The current weights as R LearnedStencilModels."""
    return [trainer.export() for trainer in self.trainers]

  def rollout_population(self):
    """The current weights as an evaluation.RolloutPopulation, without leaving the device:
    the handle is built once, around models[0], and `weights` is packed into it again on
    every call (ddd_population_load_weights, enqueued on the current stream).  What
    evaluate_population makes of it is what it makes of export(), bit for bit.
    NotImplementedError where the library has no population kernel for the models."""
    from . import evaluation   # (evaluation does not import training)
    if self._rollout_population is None:
      self._rollout_population = evaluation.RolloutPopulation(self.models[0], self.replicas)
    return self._rollout_population.load(self.weights)

  def rollout_trainer(self, clip_norm=None) -> 'RolloutPopulationTrainer':
    """A RolloutPopulationTrainer on this population's `weights` tensor (the same storage:
    what it trains, rollout_population() and export() see) with a fresh Adam state, so that
    training_population -> rollout fine-tuning -> rollout scoring never leaves the device."""
    return RolloutPopulationTrainer(self.models, self.hparams, clip_norm=clip_norm,
                                    population=self)


class RolloutPopulationTrainer(object):
  """R replicas of one architecture fine-tuned together on rollout error
  (ddd_train_rollout_run, csrc/train_rollout_population.hip): `weights`, `adam_m`, `adam_v`
  [R, n_weights] and `adam_steps` int32 [R] (the updates each replica has applied) on the
  device, Adam(beta2 = 0.99) and clip_norm as RolloutTrainer.  A step whose gradient is not
  finite is skipped for that replica alone and counted in skipped_steps [R].  Replica r of
  `run` is bit for bit the population of one on models[r].  population: the
  PopulationTrainer whose weights to train in place (PopulationTrainer.rollout_trainer)."""

  BETAS = PopulationTrainer.BETAS
  EPSILON = PopulationTrainer.EPSILON

  def __init__(self, models: Sequence[model_lib.LearnedStencilModel], hparams,
               clip_norm=None, population: PopulationTrainer = None):
    single = copy.copy(hparams)   # (the horizon is the windows', not num_time_steps)
    single.num_time_steps = 0
    models = _checked_population(models, single, check_supported)
    if population is None:
      population = PopulationTrainer(models, hparams)
    torch = population.torch
    self.torch = torch
    self.population = population
    self.models, self.hparams, self.cfg = models, hparams, population.cfg
    self.nullspace, self.bias = population.nullspace, population.bias
    self.weights = population.weights
    self.adam_m = torch.zeros_like(self.weights)
    self.adam_v = torch.zeros_like(self.weights)
    self.adam_steps = torch.zeros(len(models), dtype=torch.int32, device=self.weights.device)
    self.clip_norm = None if clip_norm is None else float(clip_norm)
    self.skipped_steps = np.zeros(len(models), np.int64)
    self._workspace = None

  @property
  def replicas(self) -> int:
    return len(self.models)

  def _call(self, windows, sample_index, rates, step_weights, forward_only):
    torch = self.torch
    device = self.weights.device
    batch = windows.num_windows if sample_index is None else int(sample_index.shape[-1])
    need = _lib.load_library().ddd_train_rollout_run_workspace_bytes(
        self.cfg, batch, windows.num_steps, self.replicas)
    if self._workspace is None or self._workspace.numel() < need:
      self._workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=device)
    return _lib.train_rollout_run(
        self.cfg, self.weights, self.adam_m, self.adam_v, self.adam_steps, windows.y0,
        windows.targets, _rollout_step_weights(windows, step_weights, device),
        windows.num_steps, windows.save_every, windows.dt, sample_index, rates,
        betas=self.BETAS, epsilon=self.EPSILON, clip_norm=self.clip_norm or 0.0,
        t0=windows.t0, forcing=windows.forcing, nullspace=self.nullspace, bias=self.bias,
        forward_only=forward_only, workspace=self._workspace)

  def run(self, windows: RolloutWindows, num_steps: int, learning_rates, sample_index=None,
          step_weights=None):
    """num_steps optimiser steps of every replica in one call.  learning_rates: one rate,
    one per replica [R] or one per replica and step [R][num_steps]; sample_index: int32
    [num_steps, batch] (shared) or [num_steps, R, batch] (None: all windows every step).
    Returns, after one host read, (step_means [num_steps, R, num_saved], grad_norms
    [num_steps, R]) as float32 host arrays; a norm that is not finite marks a skipped step
    and is counted in skipped_steps."""
    torch = self.torch
    num_steps, R = int(num_steps), self.replicas
    if num_steps < 1:
      raise ValueError('num_steps = {} (>= 1)'.format(num_steps))
    rates = np.asarray(learning_rates, np.float64)
    if rates.ndim == 1 and rates.shape[0] == R:
      rates = rates[:, None]
    if rates.ndim not in (0, 2) or (rates.ndim == 2 and (
        rates.shape[0] != R or rates.shape[1] not in (1, num_steps))):
      raise ValueError('learning_rates must be one rate, [R] or [R][num_steps]')
    rates = np.broadcast_to(rates, (R, num_steps)).tolist()
    sample_index = _rollout_minibatches(sample_index, num_steps, R, windows,
                                        self.weights.device)
    log, norms, _ = self._call(windows, sample_index, rates, step_weights, False)
    both = torch.cat([log, norms[..., None]], dim=-1).cpu().numpy()   # (the one host read)
    means, norms = both[..., :-1], both[..., -1]
    self.skipped_steps += (~np.isfinite(norms)).sum(axis=0)
    return means, norms

  def loss(self, windows: RolloutWindows, step_weights=None) -> np.ndarray:
    """step_means [R, num_saved] float64 over ALL windows, forward only: one call and one
    host read for all replicas; row r is bit for bit the step_means of a forward-only
    ddd_train_rollout_loss_grad call on replica r."""
    log, _, _ = self._call(windows, None, None, step_weights, True)
    return log[0].double().cpu().numpy()

  def export(self) -> List[model_lib.LearnedStencilModel]:
    """The current weights as R LearnedStencilModels."""
    return self.population.export()


def fine_tune_population_on_rollouts(models: Sequence[model_lib.LearnedStencilModel], y_exact,
                                     times, hparams, checkpoint_dirs: Sequence[str], horizons,
                                     save_every: int, batch: int, learning_rates,
                                     seed: int = 0, stride: int = 1, first_seed: int = 0,
                                     clip_norm=None) -> List[List[Dict[str, float]]]:
  """fine_tune_on_rollouts(..., seed=seed, fused=True) for R replicas at once: the same
  curriculum, windows and minibatch order (shared by the replicas), replica r at
  learning_rates[r]; every stretch between two evaluations is one
  RolloutPopulationTrainer.run, every evaluation one forward-only call for all replicas.
  Writes hparams.json + model.npz to checkpoint_dirs[r]; returns one list of rows per
  replica, with fine_tune_on_rollouts' keys."""
  models = list(models)
  learning_rates = [float(rate) for rate in learning_rates]
  if len(checkpoint_dirs) != len(models) or len(learning_rates) != len(models):
    raise ValueError('one checkpoint directory and one learning rate per model')
  hparams = copy.deepcopy(hparams)
  trainer = RolloutPopulationTrainer(models, hparams, clip_norm=clip_norm)
  for checkpoint_dir in checkpoint_dirs:
    os.makedirs(checkpoint_dir, exist_ok=True)
    hparams_lib.save_hparams(hparams, checkpoint_dir)
  rs = np.random.RandomState(seed)
  rows, step = [[] for _ in models], 0

  def evaluate(windows):
    for r, means in enumerate(trainer.loss(windows)):
      rows[r].append({'step': step, 'num_steps': windows.num_steps,
                      'loss': float(means.mean()), 'step_means': means.tolist(),
                      'skipped_steps': int(trainer.skipped_steps[r])})

  for opt_steps, num_steps in horizons:
    windows = make_rollout_windows(y_exact, times, hparams, num_steps, save_every,
                                   stride=stride, first_seed=first_seed)
    count = min(int(batch), windows.num_windows)
    evaluate(windows)
    for length in _rollout_stretches(int(opt_steps), step, hparams.eval_interval):
      index = np.stack([rs.choice(windows.num_windows, size=count, replace=False)
                        .astype(np.int32) for _ in range(length)])
      trainer.run(windows, length, learning_rates, index)
      step += length
      evaluate(windows)
  for model, checkpoint_dir in zip(trainer.export(), checkpoint_dirs):
    model.save(checkpoint_dir)
  return rows


def _scaled_loss_per_head(sums, hparams) -> np.ndarray:
  """[R, 2, channel] float64: the two loss rows of ddd_eval_metrics' sums (one host read),
  scaled by error_scale and clipped at error_max as Trainer.loss_and_grad returns them."""
  scale = np.array(hparams.error_scale, np.float64).reshape(2, -1)
  per_head = sums[:, :2].double().cpu().numpy() * scale
  if hparams.error_max:
    per_head = np.where(per_head < hparams.error_max, per_head, hparams.error_max)
  return per_head


METRIC_NAMES = ('mae', 'rms_error', 'mean_abs_relative_error', 'frac_below_baseline')


def _target_metrics(mae, rms_error, geometric, below, equation_type) -> Dict[str, float]:
  """The per-target keys of calculate_metrics from per-channel vectors: one entry per
  space derivative and 'u_t', then 'u(t)' = the mean over the integrated heads."""
  per_channel = dict(zip(METRIC_NAMES, (mae, rms_error, geometric, below)))
  targets = list(equation_type.DERIVATIVE_NAMES) + ['u_t']
  if len(mae) < len(targets):
    raise ValueError('{} channels, {} targets'.format(len(mae), len(targets)))
  metrics = {}
  for i, target in enumerate(targets):
    for name in METRIC_NAMES:
      metrics['{}/{}'.format(name, target)] = per_channel[name][i]
  if len(mae) > len(targets):
    for name in METRIC_NAMES:
      metrics[name + '/u(t)'] = per_channel[name][len(targets):].mean()
  return metrics


def calculate_metrics(data: Dict[str, np.ndarray], equation_type) -> Dict[str, float]:
  """training.py:433-491 on host arrays: data holds 'labels', 'baseline' and
  'predictions' [examples, x, channel] and scalar 'loss...' entries.  Per target the MAE
  and RMS error relative to the baseline's, the geometric-mean relative error and the
  fraction of points whose squared error is below the baseline's; 'count' examples; the
  loss entries as floats."""
  labels = np.asarray(data['labels'])
  baseline = np.asarray(data['baseline'])
  predictions = np.asarray(data['predictions'])
  labels = model_lib.align_labels(labels, baseline)
  err, base = labels - predictions, labels - baseline
  over = (0, 1)
  mae = np.mean(np.abs(err), axis=over) / np.mean(np.abs(base), axis=over)
  rms_error = np.sqrt(np.mean(err ** 2, axis=over) / np.mean(base ** 2, axis=over))
  ratio = np.maximum(np.abs(err), 1e-8) / np.maximum(np.abs(base), 1e-8)
  geometric = np.exp(np.mean(np.log(ratio), axis=over))
  below = np.mean(err ** 2 < base ** 2, axis=over)
  metrics = {'count': len(labels)}
  metrics.update({k: float(v) for k, v in data.items() if 'loss' in k})
  metrics.update(_target_metrics(mae, rms_error, geometric, below, equation_type))
  return metrics


def metrics_from_sums(sums, below, count: int, num_points: int, equation_type,
                      losses: Dict[str, float] = None) -> Dict[str, float]:
  """calculate_metrics from the sums of ddd_eval_metrics for one replica: sums
  [7, channel] (rows 2 .. 6: sum |l - p|, sum |l - b|, sum (l - p)^2, sum (l - b)^2,
  sum log max(|l - p|, 1e-8) - log max(|l - b|, 1e-8); rows 0, 1 are not read), below
  [channel] points under the baseline, over `count` examples of num_points points.  The
  divisions, the root and the exponential are taken here, in float64.  losses: the
  'loss...' entries to carry."""
  sums = np.asarray(sums, np.float64)
  total = float(count) * float(num_points)
  mae = sums[2] / sums[3]
  rms_error = np.sqrt(sums[4] / sums[5])
  geometric = np.exp(sums[6] / total)
  fraction = np.asarray(below, np.float64) / total
  metrics = {'count': int(count)}
  metrics.update({k: float(v) for k, v in (losses or {}).items()})
  metrics.update(_target_metrics(mae, rms_error, geometric, fraction, equation_type))
  return metrics


def metrics_one_linear(metrics: Dict[str, float]) -> str:
  """training.py:494-507: one line of the loss and, per target in key order, the MAE,
  the geometric-mean relative error and the fraction below the baseline."""
  def matching(like):
    return '/'.join('{}={:1.4f}'.format(k.split('/')[-1], v)
                    for k, v in sorted(metrics.items()) if like in k)
  return 'loss: {:1.7f}, abs_error: {}, rel_error: {}, below_baseline: {}'.format(
      metrics['loss'], matching('mae'), matching('mean_abs_relative_error'),
      matching('frac_below_baseline'))


def metrics_to_dataframe(logged_metrics):
  """training.py:537-547: [(step, test_metrics, train_metrics)] -> one DataFrame row per
  evaluation, keys prefixed 'test_' / 'train_', plus 'step'."""
  import pandas as pd
  return pd.DataFrame([_metrics_row(*logged) for logged in logged_metrics])


def _metrics_row(step, test_metrics, train_metrics) -> Dict[str, float]:
  row = {'test_' + k: v for k, v in test_metrics.items()}
  row.update({'train_' + k: v for k, v in train_metrics.items()})
  row['step'] = step
  return row


def loss_metrics(per_head: np.ndarray, hparams, equation_type) -> Dict[str, float]:
  """training.py:279-297 from loss_per_head [2, channel]: 'loss' (weighted_loss) and the
  means of its space-derivative, time-derivative and integrated-solution entries."""
  space, time, integrated = model_lib.result_unstack(per_head, equation_type)
  losses = {'loss': float(model_lib.weighted_loss(per_head, hparams)),
            'loss/space_derivatives': float(np.mean(space)),
            'loss/time_derivative': float(np.mean(time))}
  if integrated is not None:
    losses['loss/integrated_solution'] = float(np.mean(integrated))
  return losses


class Inferer(object):
  """training.py:253-314 for a Trainer or a PopulationTrainer: the evaluation metrics of
  every replica over the whole `dataset` (a DeviceDataset) in one ddd_eval_metrics call.

  'loss' and 'loss/*' are computed from the means over the whole dataset.  The reference
  averages the per-batch means with equal weight (tf.metrics.mean over batches); the two
  agree when the batches are equal in size, and differ by the weight of a shorter last
  batch otherwise."""

  def __init__(self, dataset, trainer):
    self.dataset = dataset
    self.trainer = trainer
    self.population = isinstance(trainer, PopulationTrainer)
    self.hparams = trainer.hparams
    self.equation_type = equations_lib.equation_type_from_hparams(self.hparams)

  def run_async(self, want_predictions: bool = False):
    """Enqueues the call; returns the device tensors (sums [R, 7, channel], below
    [R, channel], predictions [R, examples, x, channel] or None) without waiting, so that
    several stretches and evaluations can be enqueued before one read."""
    trainer, dataset, hp = self.trainer, self.dataset, self.hparams
    first = trainer.trainers[0] if self.population else trainer
    weights = trainer.weights if self.population else trainer.weights.detach()[None]
    heads = int(dataset.labels.shape[-1])
    floor, coef_abs, coef_rel = first.coefficients(heads)
    steps = hp.num_time_steps or 0
    model = trainer.models[0] if self.population else trainer.model
    return _lib.eval_metrics(
        first.cfg, weights, dataset.inputs, dataset.labels, dataset.baseline, floor, coef_abs,
        coef_rel, num_time_steps=steps,
        time_step=model.equation.time_step if steps else 0.0, nullspace=first.nullspace,
        bias=first.bias, want_predictions=want_predictions)

  def metrics(self, sums, below) -> List[Dict[str, float]]:
    """The metrics dicts of run_async's tensors: one host read, then float64."""
    per_head = _scaled_loss_per_head(sums, self.hparams)
    sums = sums.double().cpu().numpy()
    below = below.cpu().numpy()
    return [metrics_from_sums(
        sums[r], below[r], self.dataset.num_examples, int(self.dataset.inputs.shape[1]),
        self.equation_type, loss_metrics(per_head[r], self.hparams, self.equation_type))
            for r in range(sums.shape[0])]

  def run(self) -> List[Dict[str, float]]:
    """One metrics dict per replica, with the keys of calculate_metrics."""
    sums, below, _ = self.run_async()
    return self.metrics(sums, below)


def select_replica(rows, key: str):
  """(replica, value) of the best replica at the last evaluation: the smallest last-row
  value of `key` ('loss' or a metric key such as 'test_mae/u_t'), the largest for a
  'frac_below_baseline' or a 'survival' key (rollout_metrics); NaN never wins; ties go to
  the lowest index."""
  values = []
  for replica_rows in rows:
    if key not in replica_rows[-1]:
      raise KeyError('select = {!r}: the rows have {}'.format(key, sorted(replica_rows[-1])))
    values.append(float(replica_rows[-1][key]))
  sign = -1.0 if 'frac_below_baseline' in key or 'survival' in key else 1.0
  ranked = [sign * v if np.isfinite(v) else np.inf for v in values]
  best = int(np.argmin(ranked))
  return best, values[best]


def rollout_metrics(result) -> List[Dict[str, float]]:
  """One dict per replica from evaluation.evaluate_population's result: the means over the
  samples, 'rollout_mae/<stop time>' (smaller is better) and 'rollout_survival/<quantile>'
  (larger is better; select_replica knows).  A NaN sample makes its mean NaN."""
  mae, survival = np.asarray(result['mae']), np.asarray(result['survival'])
  rows = []
  for r in range(mae.shape[0]):
    row = {'rollout_mae/{:g}'.format(float(stop)): float(np.mean(mae[r, k]))
           for k, stop in enumerate(result['stop_times'])}
    row.update({'rollout_survival/{:g}'.format(float(q)): float(np.mean(survival[r, i]))
                for i, q in enumerate(result['quantiles'])})
    rows.append(row)
  return rows


def training_population(snapshots: np.ndarray, checkpoint_dirs: Sequence[str], hparams,
                        init_seeds: Sequence[int], learning_rates=None, seed: int = 0,
                        num_steps: int = None, metrics: bool = False, select: str = None,
                        rollout=None, rollout_launch: str = 'streams',
                        rollout_every: int = None):
  """training_loop(..., seed=seed, fused=True) for R replicas at once: the same dataset,
  train / validation split and minibatch order; replica r starts from
  LearnedStencilModel(coarse, hparams, init_seed=init_seeds[r]) and follows
  learning_rates[r] (default: hparams.learning_rates); every stretch between two
  evaluations is one PopulationTrainer.run.  Writes hparams.json + model.npz to
  checkpoint_dirs[r]; returns one list of metric rows per replica.

  metrics: every evaluation also runs an Inferer over the validation and the training
  split (one call each for all replicas) and adds their 'test_*' / 'train_*' entries
  (metrics_to_dataframe's keys) to the rows; the test metrics of every replica are logged
  with metrics_one_linear.  select: 'loss' or, with metrics, any key of the rows such as
  'test_mae/u_t': returns (rows, best) with best the index of the best replica at the last
  evaluation (select_replica), and writes best.json {'replica', 'key', 'value',
  'checkpoint_dir'} next to the checkpoint directories.

  rollout: an evaluation.RolloutReference; the exported models are then rolled out once
  after the last stretch (evaluation.evaluate_population) and the keys of rollout_metrics
  are added to every replica's last row, where select can name them.  rollout_launch is
  evaluate_population's ``launch`` ('streams', 'population' or 'auto').

  rollout_every = k (with a rollout): the evaluations at steps that are multiples of k
  (step 0 included) also roll the replicas out as they are then and add the same keys to
  that row; the last row gets those of the final weights as before, with the same values as
  under rollout_every=None.  Under rollout_launch 'population' or 'auto' these rollouts go
  through PopulationTrainer.rollout_population(): the weights are packed on the device into
  one handle kept for the whole run, with no export and no model handle per replica;
  under 'streams', or where 'auto' finds no population kernel, by export() and the streams."""
  if rollout_every is not None:
    if rollout is None:
      raise ValueError('rollout_every needs a rollout (an evaluation.RolloutReference)')
    if int(rollout_every) != rollout_every or rollout_every < 1:
      raise ValueError('rollout_every = {!r} (a positive number of steps)'.format(rollout_every))
  if len(checkpoint_dirs) != len(init_seeds):
    raise ValueError('one checkpoint directory per init seed')
  hparams = copy.deepcopy(hparams)
  _checker(hparams)(hparams)
  train_data = set_data_dependent_hparams(hparams, snapshots, seed)
  train_data.repeat = True
  valid_data = model_lib.make_dataset(snapshots, hparams, model_lib.Dataset.VALIDATION,
                                      repeat=False, evaluation=True, seed=seed)
  for checkpoint_dir in checkpoint_dirs:
    os.makedirs(checkpoint_dir, exist_ok=True)
    hparams_lib.save_hparams(hparams, checkpoint_dir)
  _, coarse = equations_lib.from_hparams(hparams, random_seed=seed)
  trainer = PopulationTrainer(
      [model_lib.LearnedStencilModel(coarse, hparams, init_seed=int(s)) for s in init_seeds],
      hparams, learning_rates)
  steps = hparams.learning_stops[-1] if num_steps is None else int(num_steps)
  weights = model_lib.loss_weights(hparams, int(train_data.labels.shape[-1]))
  rows = [[] for _ in init_seeds]

  inferers = None
  if metrics:   # the reference's two Inferers: each split without rolls or noise
    train_eval = model_lib.make_dataset(snapshots, hparams, model_lib.Dataset.TRAINING,
                                        repeat=False, evaluation=True, seed=seed)
    inferers = (Inferer(valid_data if valid_data.num_examples else train_eval, trainer),
                Inferer(train_eval, trainer))

  rolled_out_at = [None]   # the step whose weights the last rows' rollout keys are of

  def roll_out(step):
    """The rollout keys of the current weights into every replica's last row."""
    from . import evaluation   # (evaluation does not import training)
    scores = None
    if rollout_launch != 'streams':
      try:
        scores = evaluation.evaluate_population(trainer.rollout_population(), hparams, rollout)
      except NotImplementedError:
        if rollout_launch == 'population':
          raise
    if scores is None:
      scores = evaluation.evaluate_population(trainer.export(), hparams, rollout,
                                              launch='streams')
    for replica_rows, row in zip(rows, rollout_metrics(scores)):
      replica_rows[-1].update(row)
    rolled_out_at[0] = step

  def evaluate(step):
    data = valid_data if valid_data.num_examples else train_data
    logged = None
    if metrics:   # both splits enqueued, then read
      pending = [inferer.run_async() for inferer in inferers]
      logged = [inferer.metrics(sums, below)
                for inferer, (sums, below, _) in zip(inferers, pending)]
    for r, (replica_rows, per_head) in enumerate(zip(rows, trainer.loss(data))):
      row = {'step': step, 'loss': float(np.sum(weights * per_head)),
             'loss_per_head': per_head.tolist()}
      if metrics:
        row.update(_metrics_row(step, logged[0][r], logged[1][r]))
        logging.info('replica %d: %s', r, metrics_one_linear(logged[0][r]))
      replica_rows.append(row)
    if rollout_every is not None and step % rollout_every == 0:
      roll_out(step)

  evaluate(0)
  batches = train_data.batch_indices()
  torch = trainer.torch
  step = 0
  while step < steps:   # up to the next evaluation, or the end
    stop = min(steps, (step // hparams.eval_interval + 1) * hparams.eval_interval)
    index = torch.stack([next(batches) for _ in range(stop - step)])
    trainer.run(train_data, stop - step, index)
    step = stop
    if step % hparams.eval_interval == 0:
      evaluate(step)
  exported = trainer.export()
  for model, checkpoint_dir in zip(exported, checkpoint_dirs):
    model.save(checkpoint_dir)
  if rollout_every is not None:
    if rolled_out_at[0] != steps:   # (the last evaluation was not one of them, or came earlier)
      roll_out(steps)
  elif rollout is not None:
    from . import evaluation   # (evaluation does not import training)
    scores = rollout_metrics(evaluation.evaluate_population(exported, hparams, rollout,
                                                            launch=rollout_launch))
    for replica_rows, row in zip(rows, scores):
      replica_rows[-1].update(row)
  if select is None:
    return rows
  best, value = select_replica(rows, select)
  parent = os.path.dirname(os.path.abspath(checkpoint_dirs[best]))
  with open(os.path.join(parent, 'best.json'), 'w') as f:
    json.dump({'replica': best, 'key': select, 'value': value,
               'checkpoint_dir': checkpoint_dirs[best]}, f)
  return rows, best


def training_loop(snapshots: np.ndarray, checkpoint_dir: str, hparams,
                  seed: int = 0, num_steps: int = None,
                  fused: bool = False, metrics: bool = False) -> List[Dict[str, float]]:
  """training.py:570-636: trains on fine snapshots [examples, x], writes hparams.json +
  model.npz (LearnedStencilModel.save) to checkpoint_dir and returns one metrics row
  per eval_interval steps: the validation loss and loss per head.  num_steps defaults
  to learning_stops[-1].  fused: every stretch between two evaluations is one
  Trainer.run call (the same minibatch order) instead of eval_interval Trainer.step
  calls.  metrics: every evaluation also runs an Inferer over the validation and the
  training split, as the reference's loop does, adds their 'test_*' / 'train_*' entries
  (metrics_to_dataframe's keys) to the row and logs metrics_one_linear of the test
  metrics."""
  hparams = copy.deepcopy(hparams)
  _checker(hparams)(hparams)
  train_data = set_data_dependent_hparams(hparams, snapshots, seed)
  train_data.repeat = True
  valid_data = model_lib.make_dataset(snapshots, hparams, model_lib.Dataset.VALIDATION,
                                      repeat=False, evaluation=True, seed=seed)
  os.makedirs(checkpoint_dir, exist_ok=True)
  hparams_lib.save_hparams(hparams, checkpoint_dir)
  _, coarse = equations_lib.from_hparams(hparams, random_seed=seed)
  trainer = Trainer(model_lib.LearnedStencilModel(coarse, hparams, init_seed=seed), hparams)
  steps = hparams.learning_stops[-1] if num_steps is None else int(num_steps)
  weights = model_lib.loss_weights(hparams, int(train_data.labels.shape[-1]))
  rows = []

  inferers = None
  if metrics:   # the reference's two Inferers: each split without rolls or noise
    train_eval = model_lib.make_dataset(snapshots, hparams, model_lib.Dataset.TRAINING,
                                        repeat=False, evaluation=True, seed=seed)
    inferers = (Inferer(valid_data if valid_data.num_examples else train_eval, trainer),
                Inferer(train_eval, trainer))

  def evaluate(step):
    data = valid_data if valid_data.num_examples else train_data
    per_head, _, _ = trainer.loss_and_grad(data, want_grad=False)
    row = {'step': step, 'loss': float(np.sum(weights * per_head)),
           'loss_per_head': per_head.tolist()}
    if metrics:   # both splits enqueued, then read
      pending = [inferer.run_async() for inferer in inferers]
      test, train = [inferer.metrics(sums, below)[0]
                     for inferer, (sums, below, _) in zip(inferers, pending)]
      row.update(_metrics_row(step, test, train))
      logging.info(metrics_one_linear(test))
    rows.append(row)

  evaluate(0)
  batches = train_data.batch_indices()
  if fused:
    torch = trainer.torch
    step = 0
    while step < steps:   # up to the next evaluation, or the end
      stop = min(steps, (step // hparams.eval_interval + 1) * hparams.eval_interval)
      index = torch.stack([next(batches) for _ in range(stop - step)])
      trainer.run(train_data, stop - step, index)
      step = stop
      if step % hparams.eval_interval == 0:
        evaluate(step)
  else:
    for step in range(steps):
      trainer.step(train_data, next(batches))
      if (step + 1) % hparams.eval_interval == 0:
        evaluate(step + 1)
  trainer.export().save(checkpoint_dir)
  return rows


def create_training_snapshots(equation, seeds: Sequence[int], times) -> np.ndarray:
  """Fine-grid training data without Beam: integrate_exact_batch over one equation per
  seed (the same type and grid as `equation`), every saved time of every sample as
  one snapshot: [len(seeds) * len(times), x] float32."""
  params = equation.params()
  eqs = [type(equation)(**dict(params, random_seed=int(seed))) for seed in seeds]
  result = integrate.integrate_exact_batch(eqs, np.asarray(times, np.float64))
  y = np.asarray(result['y'])
  return y.reshape(-1, y.shape[-1]).astype(np.float32)
