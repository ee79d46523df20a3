"""ctypes binding of csrc/libddd1d.so (C ABI: include/ddd1d.h).

PyTorch is used only as the device-memory / stream provider: tensors are
allocated with torch, their ``data_ptr()`` and torch's current HIP stream are
handed to the library as plain pointers.  There is NO CPU fallback: if the
shared library or a GPU is missing, calls raise.
"""
import ctypes
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBRARY_PATH = os.path.join(_HERE, 'csrc', 'libddd1d.so')
PROBE_LIBRARY_PATH = os.path.join(_HERE, 'csrc', 'libddd1d_probe.so')

MAX_DERIVATIVES = 4

# enums (include/ddd1d.h)
ACTIVATIONS = {'relu': 0, 'relu6': 1, 'tanh': 2, 'softplus': 3, 'elu': 4}
MODEL_TARGETS = {'coefficients': 0, 'space_derivatives': 1,
                 'time_derivative': 2, 'flux': 3}
SCHEMES = {'euler': 0, 'midpoint': 1, 'bs3': 2, 'rk23': 2, 'rk4': 3}
KERNELS = {'auto': 0, 'generic': 1, 'mfma': 2, 'mfma64': 3, 'mfma256': 4,
           'mfma64w32': 5, 'mfma64w16': 6}
LAUNCH_MODES = {'persistent': 0, 'per_substep': 1, 'per_step': 2}


class DDDConfig(ctypes.Structure):
  """struct ddd_config."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('equation', ctypes.c_int32),
      ('num_points', ctypes.c_int32),
      ('num_derivatives', ctypes.c_int32),
      ('derivative_orders', ctypes.c_int32 * MAX_DERIVATIVES),
      ('dx', ctypes.c_double),
      ('period', ctypes.c_double),
      ('eta', ctypes.c_double),
      ('standard_deviation', ctypes.c_double),
      ('stencil_size', ctypes.c_int32),
      ('model_target', ctypes.c_int32),
      ('num_layers', ctypes.c_int32),
      ('filter_size', ctypes.c_int32),
      ('kernel_size', ctypes.c_int32),
      ('activation', ctypes.c_int32),
      ('polynomial_accuracy_order', ctypes.c_int32),
      ('ensure_unbiased_coefficients', ctypes.c_int32),
      ('input_sizes', ctypes.c_int32 * MAX_DERIVATIVES),
      ('weno_reconstruction', ctypes.c_int32),
      ('reserved', ctypes.c_int32 * 3),
  ]


MAX_HEADS = MAX_DERIVATIVES + 1


class DDDTrainArgs(ctypes.Structure):
  """struct ddd_train_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('reserved0', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('labels', ctypes.c_void_p),
      ('baseline', ctypes.c_void_p),
      ('error_floor', ctypes.c_float * MAX_HEADS),
      ('coef_abs', ctypes.c_float * MAX_HEADS),
      ('coef_rel', ctypes.c_float * MAX_HEADS),
      ('head_means', ctypes.c_void_p),
      ('grad', ctypes.c_void_p),
      ('predictions', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


MAX_TIME_STEPS = 8   # DDD_MAX_TIME_STEPS
MAX_UNROLLED_HEADS = MAX_HEADS + MAX_TIME_STEPS


class DDDTrainUnrolledArgs(ctypes.Structure):
  """struct ddd_train_unrolled_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('num_time_steps', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('labels', ctypes.c_void_p),
      ('baseline', ctypes.c_void_p),
      ('time_step', ctypes.c_float),
      ('error_floor', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_abs', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_rel', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('head_means', ctypes.c_void_p),
      ('grad', ctypes.c_void_p),
      ('predictions', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


MAX_ROLLOUT_STEPS = 256   # DDD_MAX_ROLLOUT_STEPS


class DDDTrainRolloutArgs(ctypes.Structure):
  """struct ddd_train_rollout_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('num_steps', ctypes.c_int32),
      ('save_every', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y0', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('targets', ctypes.c_void_p),
      ('step_weights', ctypes.c_void_p),
      ('dt', ctypes.c_double),
      ('t0', ctypes.c_void_p),
      ('nparams', ctypes.c_int32),
      ('n_k', ctypes.c_int32),
      ('amplitude', ctypes.c_void_p),
      ('omega', ctypes.c_void_p),
      ('phase', ctypes.c_void_p),
      ('k_index', ctypes.c_void_p),
      ('spatial_phase', ctypes.c_void_p),
      ('step_means', ctypes.c_void_p),
      ('grad', ctypes.c_void_p),
      ('trajectory', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


class DDDTrainRunArgs(ctypes.Structure):
  """struct ddd_train_run_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('num_time_steps', ctypes.c_int32),
      ('first_step', ctypes.c_int32),
      ('num_steps', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('adam_m', ctypes.c_void_p),
      ('adam_v', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('labels', ctypes.c_void_p),
      ('baseline', ctypes.c_void_p),
      ('learning_rate', ctypes.POINTER(ctypes.c_double)),
      ('beta1', ctypes.c_double),
      ('beta2', ctypes.c_double),
      ('epsilon', ctypes.c_double),
      ('error_max', ctypes.c_double),
      ('error_scale_abs', ctypes.c_double * MAX_UNROLLED_HEADS),
      ('error_scale_rel', ctypes.c_double * MAX_UNROLLED_HEADS),
      ('error_floor', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_abs', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_rel', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('time_step', ctypes.c_float),
      ('head_means_log', ctypes.c_void_p),
      ('last_grad', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


MAX_REPLICAS = 64   # DDD_MAX_REPLICAS


class DDDTrainPopulationArgs(ctypes.Structure):
  """struct ddd_train_population_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('num_time_steps', ctypes.c_int32),
      ('first_step', ctypes.c_int32),
      ('num_steps', ctypes.c_int32),
      ('replicas', ctypes.c_int32),
      ('index_per_replica', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('adam_m', ctypes.c_void_p),
      ('adam_v', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('labels', ctypes.c_void_p),
      ('baseline', ctypes.c_void_p),
      ('learning_rate', ctypes.POINTER(ctypes.c_double)),
      ('beta1', ctypes.c_double),
      ('beta2', ctypes.c_double),
      ('epsilon', ctypes.c_double),
      ('error_max', ctypes.c_double),
      ('error_scale_abs', ctypes.c_double * MAX_UNROLLED_HEADS),
      ('error_scale_rel', ctypes.c_double * MAX_UNROLLED_HEADS),
      ('error_floor', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_abs', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_rel', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('time_step', ctypes.c_float),
      ('head_means_log', ctypes.c_void_p),
      ('last_grad', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


class DDDTrainRolloutRunArgs(ctypes.Structure):
  """struct ddd_train_rollout_run_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('num_steps', ctypes.c_int32),
      ('save_every', ctypes.c_int32),
      ('num_opt_steps', ctypes.c_int32),
      ('replicas', ctypes.c_int32),
      ('index_per_replica', ctypes.c_int32),
      ('forward_only', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('adam_m', ctypes.c_void_p),
      ('adam_v', ctypes.c_void_p),
      ('adam_step', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y0', ctypes.c_void_p),
      ('targets', ctypes.c_void_p),
      ('step_weights', ctypes.c_void_p),
      ('dt', ctypes.c_double),
      ('t0', ctypes.c_void_p),
      ('nparams', ctypes.c_int32),
      ('n_k', ctypes.c_int32),
      ('amplitude', ctypes.c_void_p),
      ('omega', ctypes.c_void_p),
      ('phase', ctypes.c_void_p),
      ('k_index', ctypes.c_void_p),
      ('spatial_phase', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('learning_rate', ctypes.POINTER(ctypes.c_double)),
      ('beta1', ctypes.c_double),
      ('beta2', ctypes.c_double),
      ('epsilon', ctypes.c_double),
      ('clip_norm', ctypes.c_double),
      ('step_means_log', ctypes.c_void_p),
      ('grad_norm_log', ctypes.c_void_p),
      ('last_grad', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


class DDDEvalMetricsArgs(ctypes.Structure):
  """struct ddd_eval_metrics_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('rows_evaluated', ctypes.c_int32),
      ('num_rows', ctypes.c_int32),
      ('num_time_steps', ctypes.c_int32),
      ('replicas', ctypes.c_int32),
      ('index_per_replica', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('sample_index', ctypes.c_void_p),
      ('labels', ctypes.c_void_p),
      ('baseline', ctypes.c_void_p),
      ('error_floor', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_abs', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('coef_rel', ctypes.c_float * MAX_UNROLLED_HEADS),
      ('time_step', ctypes.c_float),
      ('sums', ctypes.c_void_p),
      ('below', ctypes.c_void_p),
      ('predictions', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


METRIC_SUMS = 7   # float rows of ddd_eval_metrics' `sums`


class DDDRolloutReferenceArgs(ctypes.Structure):
  """struct ddd_rollout_reference_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('num_samples', ctypes.c_int32),
      ('num_times', ctypes.c_int32),
      ('num_points_exact', ctypes.c_int32),
      ('num_points', ctypes.c_int32),
      ('y_exact', ctypes.c_void_p),
      ('exact_low', ctypes.c_void_p),
  ]


class DDDRolloutScoresArgs(ctypes.Structure):
  """struct ddd_rollout_scores_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('replicas', ctypes.c_int32),
      ('num_times', ctypes.c_int32),
      ('num_samples', ctypes.c_int32),
      ('num_points', ctypes.c_int32),
      ('num_quantiles', ctypes.c_int32),
      ('num_stop_times', ctypes.c_int32),
      ('dtype', ctypes.c_int32),
      ('y_model', ctypes.c_void_p),
      ('exact_low', ctypes.c_void_p),
      ('times', ctypes.c_void_p),
      ('max_error', ctypes.c_void_p),
      ('frac_good', ctypes.c_void_p),
      ('stop_times', ctypes.c_void_p),
      ('mae', ctypes.c_void_p),
      ('survival', ctypes.c_void_p),
      ('row_abs_sum', ctypes.c_void_p),
      ('good', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


ROLLOUT_MAX_QUANTILES = 8    # DDD_ROLLOUT_MAX_QUANTILES
ROLLOUT_MAX_STOP_TIMES = 16  # DDD_ROLLOUT_MAX_STOP_TIMES
ROLLOUT_MAX_POINTS = 1024    # DDD_ROLLOUT_MAX_POINTS
ROLLOUT_MAX_FACTOR = 128     # DDD_ROLLOUT_MAX_FACTOR
ROLLOUT_F64, ROLLOUT_F32 = 0, 1


class DDDVjpArgs(ctypes.Structure):
  """struct ddd_vjp_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('cotangent', ctypes.c_void_p),
      ('predictions', ctypes.c_void_p),
      ('grad_y', ctypes.c_void_p),
      ('grad_weights', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


MAX_TANGENTS = 32   # DDD_MAX_TANGENTS


class DDDJvpArgs(ctypes.Structure):
  """struct ddd_jvp_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('tangents', ctypes.c_int32),
      ('reserved', ctypes.c_int32),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y', ctypes.c_void_p),
      ('tangent_y', ctypes.c_void_p),
      ('tangent_weights', ctypes.c_void_p),
      ('predictions', ctypes.c_void_p),
      ('tangents_out', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


class DDDTangentRolloutArgs(ctypes.Structure):
  """struct ddd_tangent_rollout_args."""
  _fields_ = [
      ('struct_size', ctypes.c_int32),
      ('batch', ctypes.c_int32),
      ('tangents', ctypes.c_int32),
      ('num_steps', ctypes.c_int32),
      ('dt', ctypes.c_double),
      ('weights', ctypes.c_void_p),
      ('nullspace', ctypes.c_void_p),
      ('bias', ctypes.c_void_p),
      ('y0', ctypes.c_void_p),
      ('tangents0', ctypes.c_void_p),
      ('state_out', ctypes.c_void_p),
      ('tangents_out', ctypes.c_void_p),
      ('workspace', ctypes.c_void_p),
      ('workspace_bytes', ctypes.c_size_t),
  ]


class DDDError(RuntimeError):
  """A libddd1d call returned a non-zero status."""


ERR_UNSUPPORTED = -2   # DDD_ERR_UNSUPPORTED


_lib = None

_F = ctypes.POINTER(ctypes.c_float)
_D = ctypes.POINTER(ctypes.c_double)
_I = ctypes.POINTER(ctypes.c_int32)
_V = ctypes.c_void_p

# name -> (restype, argtypes); every symbol include/ddd1d.h declares.
SIGNATURES = {
    'ddd_model_create': (ctypes.c_int, [ctypes.POINTER(DDDConfig), _F,
                                        ctypes.c_size_t, _F, ctypes.c_size_t,
                                        _F, ctypes.c_size_t,
                                        ctypes.POINTER(_V)]),
    'ddd_baseline_create': (ctypes.c_int, [ctypes.POINTER(DDDConfig), _F,
                                           ctypes.c_size_t,
                                           ctypes.POINTER(_V)]),
    'ddd_spectral_create': (ctypes.c_int, [ctypes.POINTER(DDDConfig), _D,
                                           ctypes.c_size_t,
                                           ctypes.POINTER(_V)]),
    'ddd_model_destroy': (ctypes.c_int, [_V]),
    'ddd_set_forcing': (ctypes.c_int, [_V, ctypes.c_int, ctypes.c_int, _F, _F,
                                       _F, _I, _F, ctypes.c_int]),
    'ddd_clear_forcing': (ctypes.c_int, [_V]),
    'ddd_time_derivative': (ctypes.c_int, [_V, ctypes.c_double, _V, _V,
                                           ctypes.c_int, _V]),
    'ddd_rk_substep': (ctypes.c_int, [_V, ctypes.c_double, _V, _V,
                                      ctypes.c_float, _V, _V, ctypes.c_float,
                                      _V, ctypes.c_int, _V]),
    'ddd_stream_fork': (ctypes.c_int, [_V, _V]),
    'ddd_stream_join': (ctypes.c_int, [_V, _V]),
    'ddd_set_region_mode': (ctypes.c_int, [_V, ctypes.c_int]),
    'ddd_region_stats': (ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_int64)]),
    'ddd_integrate_fixed': (ctypes.c_int, [_V, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_double, ctypes.c_double,
                                           ctypes.c_int, ctypes.c_int, _V, _V,
                                           ctypes.c_int, _V]),
    'ddd_integrate_fixed_f64': (ctypes.c_int, [_V, ctypes.c_int,
                                               ctypes.c_double,
                                               ctypes.c_double, ctypes.c_int,
                                               ctypes.c_int, _V, _V,
                                               ctypes.c_int, _V]),
    'ddd_integrate_adaptive_f64': (ctypes.c_int, [_V, _D, ctypes.c_int,
                                                  ctypes.c_double,
                                                  ctypes.c_double,
                                                  ctypes.c_double,
                                                  ctypes.c_longlong, _V, _V,
                                                  _V, _V, ctypes.c_int, _V]),
    'ddd_circulant_apply_f64': (ctypes.c_int, [_V, _V, _V, ctypes.c_int,
                                               ctypes.c_int, _V]),
    'ddd_time_derivative_f64': (ctypes.c_int, [_V, ctypes.c_double, _V, _V,
                                               ctypes.c_int, _V]),
    'ddd_rk_substep_f64': (ctypes.c_int, [_V, ctypes.c_double, _V, _V,
                                          ctypes.c_double, _V, _V,
                                          ctypes.c_double, _V, ctypes.c_int,
                                          _V]),
    'ddd_space_derivatives': (ctypes.c_int, [_V, _V, _V, ctypes.c_int, _V]),
    'ddd_coefficients': (ctypes.c_int, [_V, _V, _V, ctypes.c_int, _V]),
    'ddd_conv1d_periodic': (ctypes.c_int, [_V, _V, _V, _V, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, _V]),
    'ddd_pad_periodic': (ctypes.c_int, [_V, _V, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, _V]),
    'ddd_extract_patches': (ctypes.c_int, [_V, _V, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, _V]),
    'ddd_apply_coefficients': (ctypes.c_int, [_V, _V, _V, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int,
                                              ctypes.c_int, _V]),
    'ddd_apply_space_derivatives': (ctypes.c_int, [ctypes.c_int, _V, _V, _V,
                                                   ctypes.c_int, ctypes.c_int,
                                                   ctypes.c_int, ctypes.c_double,
                                                   ctypes.c_double, _V]),
    'ddd_polynomial_accuracy_apply': (ctypes.c_int, [_V, _V, _V, _V,
                                                     ctypes.c_int64,
                                                     ctypes.c_int,
                                                     ctypes.c_int, _V]),
    'ddd_train_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig),
                                                     ctypes.c_int]),
    'ddd_train_loss_grad': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                           ctypes.POINTER(DDDTrainArgs), _V]),
    'ddd_train_unrolled_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig),
                                                              ctypes.c_int, ctypes.c_int]),
    'ddd_train_unrolled_loss_grad': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                                    ctypes.POINTER(DDDTrainUnrolledArgs),
                                                    _V]),
    'ddd_train_rollout_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig),
                                                             ctypes.c_int, ctypes.c_int]),
    'ddd_train_rollout_loss_grad': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                                   ctypes.POINTER(DDDTrainRolloutArgs),
                                                   _V]),
    'ddd_train_run_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig),
                                                         ctypes.c_int, ctypes.c_int]),
    'ddd_train_run': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                     ctypes.POINTER(DDDTrainRunArgs), _V]),
    'ddd_train_population_workspace_bytes': (ctypes.c_size_t,
                                             [ctypes.POINTER(DDDConfig), ctypes.c_int,
                                              ctypes.c_int, ctypes.c_int]),
    'ddd_train_population_run': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                                ctypes.POINTER(DDDTrainPopulationArgs), _V]),
    'ddd_train_rollout_run_workspace_bytes': (ctypes.c_size_t,
                                              [ctypes.POINTER(DDDConfig), ctypes.c_int,
                                               ctypes.c_int, ctypes.c_int]),
    'ddd_train_rollout_run': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                             ctypes.POINTER(DDDTrainRolloutRunArgs), _V]),
    'ddd_eval_metrics_workspace_bytes': (ctypes.c_size_t,
                                         [ctypes.POINTER(DDDConfig), ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int]),
    'ddd_eval_metrics': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                        ctypes.POINTER(DDDEvalMetricsArgs), _V]),
    'ddd_rollout_reference': (ctypes.c_int, [ctypes.POINTER(DDDRolloutReferenceArgs), _V]),
    'ddd_rollout_scores_workspace_bytes': (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int,
                                                              ctypes.c_int, ctypes.c_int]),
    'ddd_rollout_scores': (ctypes.c_int, [ctypes.POINTER(DDDRolloutScoresArgs), _V]),
    'ddd_population_create': (ctypes.c_int, [ctypes.POINTER(_V), ctypes.c_int,
                                             ctypes.POINTER(_V)]),
    'ddd_population_create_replicated': (ctypes.c_int, [_V, ctypes.c_int, ctypes.POINTER(_V)]),
    'ddd_population_load_weights': (ctypes.c_int, [_V, _V, ctypes.c_size_t, ctypes.c_int,
                                                   ctypes.c_int, _V]),
    'ddd_population_destroy': (ctypes.c_int, [_V]),
    'ddd_population_integrate_adaptive_f64': (ctypes.c_int, [_V, _D, ctypes.c_int,
                                                             ctypes.c_double, ctypes.c_double,
                                                             ctypes.c_double, ctypes.c_longlong,
                                                             _V, _V, _V, _V, ctypes.c_int, _V]),
    'ddd_population_integrate_fixed': (ctypes.c_int, [_V, ctypes.c_int, ctypes.c_double,
                                                      ctypes.c_double, ctypes.c_int,
                                                      ctypes.c_int, _V, _V, ctypes.c_int, _V]),
    'ddd_vjp_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig),
                                                   ctypes.c_int]),
    'ddd_result_vjp': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                      ctypes.POINTER(DDDVjpArgs), _V]),
    'ddd_jvp_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig), ctypes.c_int,
                                                   ctypes.c_int]),
    'ddd_result_jvp': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                      ctypes.POINTER(DDDJvpArgs), _V]),
    'ddd_tangent_rollout_workspace_bytes': (ctypes.c_size_t, [ctypes.POINTER(DDDConfig),
                                                               ctypes.c_int, ctypes.c_int]),
    'ddd_tangent_rollout': (ctypes.c_int, [ctypes.POINTER(DDDConfig),
                                           ctypes.POINTER(DDDTangentRolloutArgs), _V]),
    'ddd_set_kernel': (ctypes.c_int, [_V, ctypes.c_int]),
    'ddd_kernel_name': (ctypes.c_char_p, [_V]),
    'ddd_fma_per_point': (ctypes.c_int64, [_V]),
    'ddd_scheme_stages': (ctypes.c_int, [ctypes.c_int]),
    'ddd_selftest_mfma_layout': (ctypes.c_int, []),
    'ddd_abi_version': (ctypes.c_int, []),
    'ddd_last_error': (ctypes.c_char_p, []),
}


def load_library(path: Optional[str] = None):
  """dlopen libddd1d.so and attach prototypes.  Raises if it is missing."""
  global _lib
  if _lib is not None and path is None:
    return _lib
  path = path or LIBRARY_PATH
  # PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, soname
  # libamdhip64.so.7).  Import torch FIRST so that libddd1d.so binds to that
  # already-loaded runtime: torch owns the device context, allocations and
  # streams this library is handed.  Loading libddd1d.so first would pull in
  # /opt/rocm's copy as a second, separate runtime in the same process.
  import torch  # noqa: F401  pylint: disable=unused-import
  if not os.path.exists(path):
    raise ImportError(
        'HIP library {} not found: build it with '
        '`python -c "import __graft_entry__ as g; g.build()"` (needs hipcc). '
        'There is no CPU fallback for the product path.'.format(path))
  lib = ctypes.CDLL(path)
  for name, (restype, argtypes) in SIGNATURES.items():
    fn = getattr(lib, name)   # AttributeError if a declared symbol is missing
    fn.restype = restype
    fn.argtypes = argtypes
  if lib.ddd_abi_version() != 1:
    raise ImportError('libddd1d ABI version mismatch')
  if ctypes.sizeof(DDDConfig) <= 0:
    raise ImportError('bad DDDConfig')
  _lib = lib
  return lib


def check(status: int):
  if status != 0:
    message = _lib.ddd_last_error().decode('utf-8', 'replace')
    raise DDDError('libddd1d error {}: {}'.format(status, message))


def check_supported(status: int):
  """check(), with DDD_ERR_UNSUPPORTED raised as NotImplementedError (the library's
  message): for entry points whose callers may choose another route."""
  if status == ERR_UNSUPPORTED:
    raise NotImplementedError(_lib.ddd_last_error().decode('utf-8', 'replace'))
  check(status)


def _torch():
  import torch
  return torch


def require_gpu():
  torch = _torch()
  if not torch.cuda.is_available():
    raise RuntimeError('no HIP device visible: the ddd1d_amd product path needs '
                       'an AMD GPU (MI355X / gfx950); there is no CPU fallback')
  return torch


def current_stream() -> int:
  return _torch().cuda.current_stream().cuda_stream


def as_device(array, dtype=None):
  """NumPy array or torch tensor -> contiguous CUDA tensor (no copy if ok)."""
  torch = require_gpu()
  if isinstance(array, torch.Tensor):
    tensor = array
  else:
    tensor = torch.from_numpy(np.ascontiguousarray(array))
  if dtype is not None and tensor.dtype != dtype:
    tensor = tensor.to(dtype)
  if tensor.device.type != 'cuda':
    tensor = tensor.cuda()
  return tensor.contiguous()


def host_f32(array) -> np.ndarray:
  return np.ascontiguousarray(np.asarray(array, dtype=np.float32))


def fptr(array: np.ndarray):
  return array.ctypes.data_as(_F)


# ---------------------------------------------------------------------------
# standalone operators
# ---------------------------------------------------------------------------
def conv1d_periodic(inputs, filters, bias=None, center=False, activation=None):
  """layers.nn_conv1d_periodic on the GPU; see layers.py."""
  lib = load_library()
  torch = require_gpu()
  x = as_device(inputs, torch.float32)
  w = as_device(filters, torch.float32)
  if x.dim() != 3 or w.dim() != 3 or w.shape[1] != x.shape[2]:
    raise ValueError('expected inputs [batch, x, cin] and filters [k, cin, cout]')
  b = None if bias is None else as_device(bias, torch.float32)
  out = torch.empty((x.shape[0], x.shape[1], w.shape[2]), dtype=torch.float32,
                    device=x.device)
  act = -1 if activation is None else ACTIVATIONS[activation]
  check(lib.ddd_conv1d_periodic(
      x.data_ptr(), w.data_ptr(), None if b is None else b.data_ptr(),
      out.data_ptr(), x.shape[0], x.shape[1], x.shape[2], w.shape[2],
      w.shape[0], int(bool(center)), act, current_stream()))
  return out


def pad_periodic(inputs, padding: int, center: bool = False):
  lib = load_library()
  torch = require_gpu()
  x = as_device(inputs, torch.float32)
  if x.dim() != 3:
    raise ValueError('inputs must be 3D for periodic padding')
  out = torch.empty((x.shape[0], x.shape[1] + padding, x.shape[2]),
                    dtype=torch.float32, device=x.device)
  check(lib.ddd_pad_periodic(x.data_ptr(), out.data_ptr(), x.shape[0],
                             x.shape[1], x.shape[2], int(padding),
                             int(bool(center)), current_stream()))
  return out


def polynomial_accuracy_apply(inputs, nullspace, bias):
  lib = load_library()
  torch = require_gpu()
  x = as_device(inputs, torch.float32)
  ns = as_device(nullspace, torch.float32)
  b = as_device(bias, torch.float32)
  input_size, g = ns.shape
  if x.shape[-1] != input_size:
    raise ValueError('inputs last dimension must equal input_size')
  rows = x.numel() // input_size
  out = torch.empty(x.shape[:-1] + (g,), dtype=torch.float32, device=x.device)
  check(lib.ddd_polynomial_accuracy_apply(
      x.data_ptr(), ns.data_ptr(), b.data_ptr(), out.data_ptr(), rows,
      input_size, g, current_stream()))
  return out


def extract_patches(inputs, size: int):
  """model.extract_patches on the GPU: [batch, x] -> [batch, x, size]."""
  lib = load_library()
  torch = require_gpu()
  x = as_device(inputs, torch.float32)
  if x.dim() != 2:
    raise ValueError('inputs must be [batch, x]')
  out = torch.empty(tuple(x.shape) + (int(size),), dtype=torch.float32, device=x.device)
  check(lib.ddd_extract_patches(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1],
                                int(size), current_stream()))
  return out


def apply_coefficients(coefficients, inputs):
  """model.apply_coefficients on the GPU: einsum('bxdi,bxi->bxd') with patches."""
  lib = load_library()
  torch = require_gpu()
  c = as_device(coefficients, torch.float32)
  x = as_device(inputs, torch.float32)
  if c.dim() != 4 or x.dim() != 2 or tuple(c.shape[:2]) != tuple(x.shape):
    raise ValueError('expected coefficients [batch, x, derivative, stencil] and inputs [batch, x]')
  out = torch.empty(tuple(c.shape[:3]), dtype=torch.float32, device=x.device)
  check(lib.ddd_apply_coefficients(c.data_ptr(), x.data_ptr(), out.data_ptr(), x.shape[0],
                                   x.shape[1], c.shape[2], c.shape[3], current_stream()))
  return out


def apply_space_derivatives(equation_id: int, derivatives, inputs, eta: float, dx: float):
  lib = load_library()
  torch = require_gpu()
  d = as_device(derivatives, torch.float32)
  x = as_device(inputs, torch.float32)
  if d.dim() != 3 or x.dim() != 2 or tuple(d.shape[:2]) != tuple(x.shape):
    raise ValueError('expected derivatives [batch, x, derivative] and inputs [batch, x]')
  out = torch.empty_like(x)
  check(lib.ddd_apply_space_derivatives(int(equation_id), d.data_ptr(), x.data_ptr(),
                                        out.data_ptr(), x.shape[0], x.shape[1], d.shape[2],
                                        float(eta), float(dx), current_stream()))
  return out


def circulant_apply(kernel, inputs):
  """out[..., x] = sum_j kernel[(x - j) mod n] inputs[..., j] in float64 on the
  device (ddd_circulant_apply_f64): duckarray.smoothing_filter as a kernel."""
  lib = load_library()
  torch = require_gpu()
  k = as_device(kernel, torch.float64)
  x = as_device(inputs, torch.float64)
  if k.dim() != 1 or x.shape[-1] != k.shape[0]:
    raise ValueError('kernel [n] and inputs [..., n] expected')
  out = torch.empty_like(x)
  rows = x.numel() // k.shape[0]
  check(lib.ddd_circulant_apply_f64(k.data_ptr(), x.data_ptr(), out.data_ptr(), rows,
                                    k.shape[0], current_stream()))
  return out


def _train_call(entry, workspace_bytes, args, steps, cfg, weights, y, labels, baseline,
                error_floor, coef_abs, coef_rel, nullspace, bias, sample_index, batch,
                want_grad, want_predictions, workspace):
  """The body of train_loss_grad (steps None) / train_unrolled_loss_grad: shape checks,
  workspace, outputs and `args` (a DDDTrainArgs or DDDTrainUnrolledArgs with its own
  fields already set) filled, then `entry`.  workspace_bytes(batch) is the entry point's
  workspace size."""
  torch = require_gpu()
  extra_heads = 0 if steps is None else steps
  heads_text = 'num_derivatives + 1' + ('' if steps is None else ' + num_time_steps')
  shape_text = '[S, N, H]' if steps is None else "[S, N, H']"
  if batch is None:
    batch = int(sample_index.shape[0]) if sample_index is not None else int(y.shape[0])
  heads = int(labels.shape[-1])
  if heads != cfg.num_derivatives + 1 + extra_heads:
    raise ValueError('labels must have {} = {} channels, got {}'.format(
        heads_text, cfg.num_derivatives + 1 + extra_heads, heads))
  if (y.dim() != 2 or tuple(labels.shape) != tuple(y.shape) + (heads,) or
      tuple(baseline.shape) != tuple(labels.shape) or y.shape[1] != cfg.num_points):
    raise ValueError('expected y [S, N], labels / baseline {}'.format(shape_text))
  if sample_index is not None and (sample_index.dim() != 1 or
                                   int(sample_index.shape[0]) != batch):
    raise ValueError('sample_index must have `batch` entries')
  ws_bytes = workspace_bytes(int(batch))
  if ws_bytes == 0:
    check(-1)
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
  head_means = torch.empty((2, heads), dtype=torch.float32, device=y.device)
  grad = torch.empty_like(weights) if want_grad else None
  preds = (torch.empty((batch, y.shape[1], heads), dtype=torch.float32, device=y.device)
           if want_predictions else None)
  args.struct_size = ctypes.sizeof(args)
  args.batch = int(batch)
  args.num_rows = int(y.shape[0])
  for name, tensor in (('weights', weights), ('y', y), ('labels', labels),
                       ('baseline', baseline)):
    if tensor.dtype != torch.float32 or not tensor.is_contiguous() or not tensor.is_cuda:
      raise ValueError('{} must be a contiguous float32 device tensor'.format(name))
    setattr(args, name, tensor.data_ptr())
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  if sample_index is not None:
    if sample_index.dtype != torch.int32 or not sample_index.is_cuda:
      raise ValueError('sample_index must be an int32 device tensor')
    args.sample_index = sample_index.data_ptr()
  for h in range(heads):
    args.error_floor[h] = float(error_floor[h])
    args.coef_abs[h] = float(coef_abs[h])
    args.coef_rel[h] = float(coef_rel[h])
  args.head_means = head_means.data_ptr()
  args.grad = None if grad is None else grad.data_ptr()
  args.predictions = None if preds is None else preds.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(entry(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return head_means, grad, preds


def train_loss_grad(cfg, weights, y, labels, baseline, error_floor, coef_abs, coef_rel,
                    nullspace=None, bias=None, sample_index=None, batch=None,
                    want_grad=True, want_predictions=False, workspace=None):
  """ddd_train_loss_grad: (head_means [2, H], grad or None, predictions or None).

  weights / y [S, N] / labels, baseline [S, N, H] / nullspace / bias are float32
  device tensors; sample_index an int32 device tensor [batch] or None (rows
  0..batch-1); error_floor / coef_abs / coef_rel are H host floats.  `workspace`: a
  uint8 device tensor of at least ddd_train_workspace_bytes bytes, reused across
  calls when given."""
  lib = load_library()
  return _train_call(
      lib.ddd_train_loss_grad, lambda b: lib.ddd_train_workspace_bytes(ctypes.byref(cfg), b),
      DDDTrainArgs(), None, cfg, weights, y, labels, baseline, error_floor, coef_abs, coef_rel,
      nullspace, bias, sample_index, batch, want_grad, want_predictions, workspace)


def train_unrolled_loss_grad(cfg, weights, y, labels, baseline, error_floor, coef_abs,
                             coef_rel, num_time_steps, time_step, nullspace=None, bias=None,
                             sample_index=None, batch=None, want_grad=True,
                             want_predictions=False, workspace=None):
  """ddd_train_unrolled_loss_grad: (head_means [2, H'], grad or None, predictions or
  None) with H' = num_derivatives + 1 + num_time_steps heads; the other arguments as
  train_loss_grad, labels / baseline [S, N, H'], error_floor / coef_* H' host floats."""
  lib = load_library()
  steps = int(num_time_steps)
  args = DDDTrainUnrolledArgs()
  args.num_time_steps = steps
  args.time_step = float(time_step)
  return _train_call(
      lib.ddd_train_unrolled_loss_grad,
      lambda b: lib.ddd_train_unrolled_workspace_bytes(ctypes.byref(cfg), b, steps),
      args, steps, cfg, weights, y, labels, baseline, error_floor, coef_abs, coef_rel,
      nullspace, bias, sample_index, batch, want_grad, want_predictions, workspace)


def train_rollout_loss_grad(cfg, weights, y0, targets, step_weights, num_steps, save_every,
                            dt, t0=None, forcing=None, nullspace=None, bias=None,
                            sample_index=None, batch=None, want_grad=True,
                            want_trajectory=False, workspace=None):
  """ddd_train_rollout_loss_grad: (step_means [T / save_every], grad or None, trajectory
  [batch, T / save_every, N] or None).

  weights / y0 [S, N] / targets [S, T / save_every, N] / step_weights [T / save_every] /
  nullspace / bias are float32 device tensors, t0 a float64 device tensor [S] or None (0),
  sample_index an int32 device tensor [batch] or None (rows 0..batch-1).  forcing: None
  (unforced) or a dict of device tensors with one row per row of y0 -- amplitude, omega,
  phase float32 [S, P], k_index int32 [S, P], spatial_phase float32 [n_k, N]
  (model.forcing_kernel_tables' keys).  `workspace`: a uint8 device tensor of at least
  ddd_train_rollout_workspace_bytes bytes, reused across calls when given."""
  lib = load_library()
  torch = require_gpu()
  steps, every = int(num_steps), int(save_every)
  if every < 1 or steps < 1 or steps % every:
    raise ValueError('save_every = {} must be >= 1 and divide num_steps = {}'.format(
        every, steps))
  saved = steps // every
  if batch is None:
    batch = int(sample_index.shape[0]) if sample_index is not None else int(y0.shape[0])
  if y0.dim() != 2 or y0.shape[1] != cfg.num_points:
    raise ValueError('expected y0 [S, N]')
  rows, n = int(y0.shape[0]), int(y0.shape[1])
  _check_f32_device('weights', weights, (vjp_num_weights(cfg),))
  _check_f32_device('y0', y0, (rows, n))
  _check_f32_device('targets', targets, (rows, saved, n))
  _check_f32_device('step_weights', step_weights, (saved,))
  for name, tensor in (('nullspace', nullspace), ('bias', bias)):
    if tensor is not None:
      _check_f32_device(name, tensor, tuple(tensor.shape))
  if t0 is not None:
    _check_device('t0', t0, torch.float64, (rows,))
  if sample_index is not None:
    _check_device('sample_index', sample_index, torch.int32, (int(batch),))
  args = DDDTrainRolloutArgs()
  if forcing is not None:
    nparams = int(forcing['amplitude'].shape[1])
    n_k = int(forcing['spatial_phase'].shape[0])
    for name in ('amplitude', 'omega', 'phase'):
      _check_f32_device(name, forcing[name], (rows, nparams))
    _check_device('k_index', forcing['k_index'], torch.int32, (rows, nparams))
    _check_f32_device('spatial_phase', forcing['spatial_phase'], (n_k, n))
    args.nparams, args.n_k = nparams, n_k
    for name in ('amplitude', 'omega', 'phase', 'k_index', 'spatial_phase'):
      setattr(args, name, forcing[name].data_ptr())
  ws_bytes = lib.ddd_train_rollout_workspace_bytes(ctypes.byref(cfg), int(batch), steps)
  if ws_bytes == 0:
    check(-1)
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y0.device)
  step_means = torch.empty((saved,), dtype=torch.float32, device=y0.device)
  grad = torch.empty_like(weights) if want_grad else None
  trajectory = (torch.empty((int(batch), saved, n), dtype=torch.float32, device=y0.device)
                if want_trajectory else None)
  args.struct_size = ctypes.sizeof(args)
  args.batch = int(batch)
  args.num_rows = rows
  args.num_steps = steps
  args.save_every = every
  args.weights = weights.data_ptr()
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  args.y0 = y0.data_ptr()
  args.sample_index = None if sample_index is None else sample_index.data_ptr()
  args.targets = targets.data_ptr()
  args.step_weights = step_weights.data_ptr()
  args.dt = float(dt)
  args.t0 = None if t0 is None else t0.data_ptr()
  args.step_means = step_means.data_ptr()
  args.grad = None if grad is None else grad.data_ptr()
  args.trajectory = None if trajectory is None else trajectory.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_train_rollout_loss_grad(ctypes.byref(cfg), ctypes.byref(args),
                                        current_stream()))
  return step_means, grad, trajectory


def _check_training_data(cfg, steps, y, labels, baseline, nullspace, bias):
  """What train_run, train_population_run and eval_metrics check of their dataset alike:
  labels / baseline [S, N, H'] against cfg, y [S, N] and `steps` time steps, and every
  tensor contiguous float32 on the device.  Returns H'."""
  heads = int(labels.shape[-1])
  if heads != cfg.num_derivatives + 1 + steps:
    raise ValueError('labels must have num_derivatives + 1 + num_time_steps = {} channels, '
                     'got {}'.format(cfg.num_derivatives + 1 + steps, heads))
  if (y.dim() != 2 or tuple(labels.shape) != tuple(y.shape) + (heads,) or
      tuple(baseline.shape) != tuple(labels.shape) or y.shape[1] != cfg.num_points):
    raise ValueError("expected y [S, N], labels / baseline [S, N, H']")
  for name, tensor in (('y', y), ('labels', labels), ('baseline', baseline),
                       ('nullspace', nullspace), ('bias', bias)):
    if tensor is not None:
      _check_f32_device(name, tensor, tuple(tensor.shape))
  return heads


def _train_run_call(entry, args, workspace_bytes, replicas, rates, cfg, weights, adam_m, adam_v,
                    y, labels, baseline, sample_index, error_floor, coef_abs, coef_rel,
                    first_step, betas, epsilon, num_time_steps, time_step, error_max,
                    error_scale, nullspace, bias, want_last_grad, workspace):
  """The body of train_run (replicas None: flat weights / adam_m / adam_v, sample_index
  [num_steps, batch]) / train_population_run (replicas R): shape checks, workspace,
  outputs and `args` (a DDDTrainRunArgs, or a DDDTrainPopulationArgs with its own fields
  already set) filled, then `entry`.  rates: R rows (one for train_run) of num_steps host
  floats; workspace_bytes(batch) is the entry point's workspace size.  Returns
  (head_means_log [num_steps, R, 2, H'], last_grad [R, n_weights] or None)."""
  torch = require_gpu()
  solo = replicas is None
  rows = 1 if solo else replicas
  steps = int(num_time_steps)
  if float(error_max or 0.0) > 0 and error_scale is None:
    raise ValueError("error_max > 0 needs error_scale [2, H']")
  num_steps = len(rates[0]) if rates else 0
  heads = _check_training_data(cfg, steps, y, labels, baseline, nullspace, bias)
  if (not isinstance(sample_index, torch.Tensor) or sample_index.dtype != torch.int32 or
      not sample_index.is_cuda or not sample_index.is_contiguous() or
      sample_index.dim() not in ((2,) if solo else (2, 3)) or
      int(sample_index.shape[0]) != num_steps or
      (sample_index.dim() == 3 and int(sample_index.shape[1]) != rows)):
    raise ValueError('sample_index must be a contiguous int32 device tensor '
                     '[num_steps, batch]' + ('' if solo else ' or [num_steps, R, batch]'))
  batch = int(sample_index.shape[-1])
  ws_bytes = workspace_bytes(batch)
  if ws_bytes == 0:
    check(-1)
  n_weights = vjp_num_weights(cfg)
  for name, tensor in (('weights', weights), ('adam_m', adam_m), ('adam_v', adam_v)):
    if solo:
      _check_f32_device(name, tensor, (n_weights,))
      continue
    given = int(tensor.shape[0]) if isinstance(tensor, torch.Tensor) and tensor.dim() == 2 else 0
    if given < rows:
      raise ValueError('{} must be [R, n_weights] with R = {} rows'.format(name, rows))
    _check_f32_device(name, tensor, (given, n_weights))
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
  log = torch.empty((num_steps, rows, 2, heads), dtype=torch.float32, device=y.device)
  last_grad = (torch.empty((rows, n_weights), dtype=torch.float32, device=y.device)
               if want_last_grad else None)
  args.struct_size = ctypes.sizeof(args)
  args.batch = batch
  args.num_rows = int(y.shape[0])
  args.num_time_steps = steps
  args.first_step = int(first_step)
  args.num_steps = num_steps
  for name, tensor in (('weights', weights), ('adam_m', adam_m), ('adam_v', adam_v),
                       ('y', y), ('labels', labels), ('baseline', baseline),
                       ('sample_index', sample_index), ('head_means_log', log)):
    setattr(args, name, tensor.data_ptr())
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  flat = [rate for row in rates for rate in row]
  rate_array = (ctypes.c_double * max(len(flat), 1))(*flat)
  args.learning_rate = ctypes.cast(rate_array, ctypes.POINTER(ctypes.c_double))
  args.beta1, args.beta2 = float(betas[0]), float(betas[1])
  args.epsilon = float(epsilon)
  args.error_max = float(error_max or 0.0)
  for h in range(heads):
    args.error_floor[h] = float(error_floor[h])
    args.coef_abs[h] = float(coef_abs[h])
    args.coef_rel[h] = float(coef_rel[h])
    if error_scale is not None:
      args.error_scale_abs[h] = float(error_scale[0][h])
      args.error_scale_rel[h] = float(error_scale[1][h])
  args.time_step = float(time_step)
  args.last_grad = None if last_grad is None else last_grad.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(entry(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return log, last_grad


def train_run(cfg, weights, adam_m, adam_v, y, labels, baseline, sample_index,
              learning_rates, error_floor, coef_abs, coef_rel, first_step=0,
              betas=(0.9, 0.999), epsilon=1e-8, num_time_steps=0, time_step=0.0,
              error_max=0.0, error_scale=None, nullspace=None, bias=None,
              want_last_grad=False, workspace=None):
  """ddd_train_run: len(learning_rates) optimiser steps enqueued on the current stream;
  returns (head_means_log [num_steps, 2, H'] device tensor, last_grad or None) without
  waiting for the device.

  weights / adam_m / adam_v (flat, ddd_model_create layout) are updated in place;
  sample_index is an int32 device tensor [num_steps, batch]; learning_rates host floats,
  one per step (step k is optimiser step first_step + k + 1); error_floor / coef_abs /
  coef_rel H' host floats; error_scale [2, H'] host floats (needed with error_max > 0).
  The other arguments as train_loss_grad / train_unrolled_loss_grad."""
  lib = load_library()
  steps = int(num_time_steps)
  rates = [[float(rate) for rate in learning_rates]]
  log, last_grad = _train_run_call(
      lib.ddd_train_run, DDDTrainRunArgs(),
      lambda b: lib.ddd_train_run_workspace_bytes(ctypes.byref(cfg), b, steps), None, rates,
      cfg, weights, adam_m, adam_v, y, labels, baseline, sample_index, error_floor, coef_abs,
      coef_rel, first_step, betas, epsilon, steps, time_step, error_max, error_scale,
      nullspace, bias, want_last_grad, workspace)
  return log[:, 0], None if last_grad is None else last_grad[0]


def train_population_run(cfg, weights, adam_m, adam_v, y, labels, baseline, sample_index,
                         learning_rates, error_floor, coef_abs, coef_rel, first_step=0,
                         betas=(0.9, 0.999), epsilon=1e-8, num_time_steps=0, time_step=0.0,
                         error_max=0.0, error_scale=None, nullspace=None, bias=None,
                         want_last_grad=False, workspace=None):
  """ddd_train_population_run: train_run on R replicas in one call; returns
  (head_means_log [num_steps, R, 2, H'] device tensor, last_grad [R, n_weights] or None)
  without waiting for the device.

  weights / adam_m / adam_v are [R, n_weights] (rows in the ddd_model_create layout; a
  tensor with more rows is taken as its first R), updated in place; learning_rates host
  floats [R][num_steps]; sample_index an int32 device tensor [num_steps, batch] (one
  minibatch order for all replicas) or [num_steps, R, batch].  The other arguments, shared
  by the replicas, as train_run."""
  lib = load_library()
  steps = int(num_time_steps)
  rates = [[float(rate) for rate in row] for row in learning_rates]
  replicas = len(rates)
  if any(len(row) != len(rates[0]) for row in rates):
    raise ValueError('learning_rates must be [R][num_steps]')
  args = DDDTrainPopulationArgs()
  args.replicas = replicas
  args.index_per_replica = (
      1 if isinstance(sample_index, _torch().Tensor) and sample_index.dim() == 3 else 0)
  return _train_run_call(
      lib.ddd_train_population_run, args,
      lambda b: lib.ddd_train_population_workspace_bytes(ctypes.byref(cfg), b, steps, replicas),
      replicas, rates, cfg, weights, adam_m, adam_v, y, labels, baseline, sample_index,
      error_floor, coef_abs, coef_rel, first_step, betas, epsilon, steps, time_step, error_max,
      error_scale, nullspace, bias, want_last_grad, workspace)


def train_rollout_run(cfg, weights, adam_m, adam_v, adam_step, y0, targets, step_weights,
                      num_steps, save_every, dt, sample_index, learning_rates,
                      betas=(0.9, 0.999), epsilon=1e-8, clip_norm=0.0, t0=None, forcing=None,
                      nullspace=None, bias=None, forward_only=False, want_last_grad=False,
                      workspace=None):
  """ddd_train_rollout_run: K optimiser steps on rollout error for R replicas, enqueued on
  the current stream; returns (step_means_log [K, R, T / save_every], grad_norm_log [K, R],
  last_grad [R, n_weights] or None) as device tensors, without waiting for the device.

  weights / adam_m / adam_v are [R, n_weights] float32 (rows in the ddd_model_create layout;
  a tensor with more rows is taken as its first R) and adam_step int32 [R], all updated in
  place; learning_rates host floats [R][K]; sample_index an int32 device tensor [K, batch]
  (one minibatch order for all replicas) or [K, R, batch].  A step whose gradient norm is not
  finite is skipped for that replica: its row of grad_norm_log is not finite then.  The
  windows (y0, targets, step_weights, dt, t0, forcing) as train_rollout_loss_grad.

  forward_only: one loss pass per replica over the rows `sample_index` ([1, batch] or
  [1, R, batch]; None: all rows); adam_m / adam_v / adam_step / learning_rates may be None
  (R is then weights' rows) and grad_norm_log is returned as None."""
  lib = load_library()
  torch = require_gpu()
  steps, every = int(num_steps), int(save_every)
  if every < 1 or steps < 1 or steps % every:
    raise ValueError('save_every = {} must be >= 1 and divide num_steps = {}'.format(
        every, steps))
  saved = steps // every
  if forward_only:
    replicas, opt_steps = int(weights.shape[0]), 1
    rates = None
  else:
    rates = [[float(rate) for rate in row] for row in learning_rates]
    replicas = len(rates)
    if not rates or any(len(row) != len(rates[0]) for row in rates):
      raise ValueError('learning_rates must be [R][K]')
    opt_steps = len(rates[0])
  if y0.dim() != 2 or y0.shape[1] != cfg.num_points:
    raise ValueError('expected y0 [S, N]')
  rows, n = int(y0.shape[0]), int(y0.shape[1])
  if sample_index is None:
    if not forward_only:
      raise ValueError('sample_index is required')
    batch = rows
  else:
    if (not isinstance(sample_index, torch.Tensor) or sample_index.dtype != torch.int32 or
        not sample_index.is_cuda or not sample_index.is_contiguous() or
        sample_index.dim() not in (2, 3) or int(sample_index.shape[0]) != opt_steps or
        (sample_index.dim() == 3 and int(sample_index.shape[1]) != replicas)):
      raise ValueError('sample_index must be a contiguous int32 device tensor [K, batch] or '
                       '[K, R, batch]')
    batch = int(sample_index.shape[-1])
  n_weights = vjp_num_weights(cfg)
  state = [('weights', weights)]
  if not forward_only:
    state += [('adam_m', adam_m), ('adam_v', adam_v)]
    _check_device('adam_step', adam_step, torch.int32, (replicas,))
  for name, tensor in state:
    given = int(tensor.shape[0]) if isinstance(tensor, torch.Tensor) and tensor.dim() == 2 else 0
    if given < replicas:
      raise ValueError('{} must be [R, n_weights] with R = {} rows'.format(name, replicas))
    _check_f32_device(name, tensor, (given, n_weights))
  _check_f32_device('y0', y0, (rows, n))
  _check_f32_device('targets', targets, (rows, saved, n))
  _check_f32_device('step_weights', step_weights, (saved,))
  for name, tensor in (('nullspace', nullspace), ('bias', bias)):
    if tensor is not None:
      _check_f32_device(name, tensor, tuple(tensor.shape))
  if t0 is not None:
    _check_device('t0', t0, torch.float64, (rows,))
  args = DDDTrainRolloutRunArgs()
  if forcing is not None:
    nparams = int(forcing['amplitude'].shape[1])
    n_k = int(forcing['spatial_phase'].shape[0])
    for name in ('amplitude', 'omega', 'phase'):
      _check_f32_device(name, forcing[name], (rows, nparams))
    _check_device('k_index', forcing['k_index'], torch.int32, (rows, nparams))
    _check_f32_device('spatial_phase', forcing['spatial_phase'], (n_k, n))
    args.nparams, args.n_k = nparams, n_k
    for name in ('amplitude', 'omega', 'phase', 'k_index', 'spatial_phase'):
      setattr(args, name, forcing[name].data_ptr())
  ws_bytes = lib.ddd_train_rollout_run_workspace_bytes(ctypes.byref(cfg), batch, steps, replicas)
  if ws_bytes == 0:
    check(-1)
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y0.device)
  log = torch.empty((opt_steps, replicas, saved), dtype=torch.float32, device=y0.device)
  norms = (None if forward_only else
           torch.empty((opt_steps, replicas), dtype=torch.float32, device=y0.device))
  last_grad = (torch.empty((replicas, n_weights), dtype=torch.float32, device=y0.device)
               if want_last_grad and not forward_only else None)
  args.struct_size = ctypes.sizeof(args)
  args.batch = batch
  args.num_rows = rows
  args.num_steps = steps
  args.save_every = every
  args.num_opt_steps = opt_steps
  args.replicas = replicas
  args.index_per_replica = 1 if sample_index is not None and sample_index.dim() == 3 else 0
  args.forward_only = 1 if forward_only else 0
  for name, tensor in (('weights', weights), ('adam_m', adam_m), ('adam_v', adam_v),
                       ('adam_step', adam_step), ('nullspace', nullspace), ('bias', bias),
                       ('y0', y0), ('targets', targets), ('step_weights', step_weights),
                       ('t0', t0), ('sample_index', sample_index), ('step_means_log', log),
                       ('grad_norm_log', norms), ('last_grad', last_grad)):
    setattr(args, name, None if tensor is None else tensor.data_ptr())
  args.dt = float(dt)
  if rates is not None:
    flat = [rate for row in rates for rate in row]
    rate_array = (ctypes.c_double * len(flat))(*flat)
    args.learning_rate = ctypes.cast(rate_array, ctypes.POINTER(ctypes.c_double))
  args.beta1, args.beta2 = float(betas[0]), float(betas[1])
  args.epsilon = float(epsilon)
  args.clip_norm = float(clip_norm or 0.0)
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_train_rollout_run(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return log, norms, last_grad


def eval_metrics(cfg, weights, y, labels, baseline, error_floor, coef_abs, coef_rel,
                 num_time_steps=0, time_step=0.0, nullspace=None, bias=None,
                 sample_index=None, rows_evaluated=None, want_predictions=False,
                 workspace=None):
  """ddd_eval_metrics: the sums of the evaluation metrics of R replicas in one call (two
  launches); returns (sums [R, 7, H'] float32, below [R, H'] int32, predictions
  [R, B, N, H'] or None), device tensors, without waiting for the device.

  weights is [R, n_weights] (a tensor with more rows is taken as all of them: R =
  weights.shape[0]); sample_index None (rows 0 .. B-1, B = rows_evaluated or S), an int32
  device tensor [B] (shared) or [R, B]; the other arguments as train_population_run.
  sums rows 0, 1 are the head_means of the forward-only loss call, rows 2 .. 6 and below the
  sums calculate_metrics needs (training.metrics_from_sums)."""
  lib = load_library()
  torch = require_gpu()
  steps = int(num_time_steps)
  heads = _check_training_data(cfg, steps, y, labels, baseline, nullspace, bias)
  n_weights = vjp_num_weights(cfg)
  if not isinstance(weights, torch.Tensor) or weights.dim() != 2:
    raise ValueError('weights must be [R, n_weights]')
  replicas = int(weights.shape[0])
  _check_f32_device('weights', weights, (replicas, n_weights))
  if sample_index is not None:
    if (not isinstance(sample_index, torch.Tensor) or sample_index.dtype != torch.int32 or
        not sample_index.is_cuda or not sample_index.is_contiguous() or
        sample_index.dim() not in (1, 2) or
        (sample_index.dim() == 2 and int(sample_index.shape[0]) != replicas)):
      raise ValueError('sample_index must be a contiguous int32 device tensor [B] or [R, B]')
    if rows_evaluated is not None and int(rows_evaluated) != int(sample_index.shape[-1]):
      raise ValueError('sample_index must have `rows_evaluated` entries per row')
    rows_evaluated = int(sample_index.shape[-1])
  elif rows_evaluated is None:
    rows_evaluated = int(y.shape[0])
  rows_evaluated = int(rows_evaluated)
  ws_bytes = lib.ddd_eval_metrics_workspace_bytes(ctypes.byref(cfg), rows_evaluated, steps,
                                                  replicas)
  if ws_bytes == 0:
    check(-1)
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
  sums = torch.empty((replicas, METRIC_SUMS, heads), dtype=torch.float32, device=y.device)
  below = torch.empty((replicas, heads), dtype=torch.int32, device=y.device)
  preds = (torch.empty((replicas, rows_evaluated, int(y.shape[1]), heads), dtype=torch.float32,
                       device=y.device) if want_predictions else None)
  args = DDDEvalMetricsArgs()
  args.struct_size = ctypes.sizeof(DDDEvalMetricsArgs)
  args.rows_evaluated = rows_evaluated
  args.num_rows = int(y.shape[0])
  args.num_time_steps = steps
  args.replicas = replicas
  args.index_per_replica = 1 if sample_index is not None and sample_index.dim() == 2 else 0
  for name, tensor in (('weights', weights), ('y', y), ('labels', labels),
                       ('baseline', baseline), ('sums', sums), ('below', below)):
    setattr(args, name, tensor.data_ptr())
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  args.sample_index = None if sample_index is None else sample_index.data_ptr()
  for h in range(heads):
    args.error_floor[h] = float(error_floor[h])
    args.coef_abs[h] = float(coef_abs[h])
    args.coef_rel[h] = float(coef_rel[h])
  args.time_step = float(time_step)
  args.predictions = None if preds is None else preds.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_eval_metrics(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return sums, below, preds


def _check_device(name, tensor, dtype, shape):
  torch = _torch()
  if (not isinstance(tensor, torch.Tensor) or tensor.dtype != dtype or not tensor.is_cuda or
      not tensor.is_contiguous()):
    raise ValueError('{} must be a contiguous {} device tensor'.format(name, dtype))
  if shape is not None and tuple(tensor.shape) != tuple(shape):
    raise ValueError('{} has shape {}, expected {}'.format(name, tuple(tensor.shape),
                                                           tuple(shape)))


def rollout_reference(y_exact, num_points: int):
  """ddd_rollout_reference: y_exact [S, T, X] float64 on the device -> exact_low [T, S, N]
  float64, the block means of duckarray.resample_mean bit for bit, in the layout of the
  integrators' trajectories.  One launch on the current stream; nothing waits."""
  lib = load_library()
  torch = require_gpu()
  _check_device('y_exact', y_exact, torch.float64, None)
  if y_exact.dim() != 3:
    raise ValueError('y_exact must be [sample, time, x]')
  samples, num_times, fine = (int(v) for v in y_exact.shape)
  exact_low = torch.empty((num_times, samples, int(num_points)), dtype=torch.float64,
                          device=y_exact.device)
  args = DDDRolloutReferenceArgs()
  args.struct_size = ctypes.sizeof(DDDRolloutReferenceArgs)
  args.num_samples = samples
  args.num_times = num_times
  args.num_points_exact = fine
  args.num_points = int(num_points)
  args.y_exact = y_exact.data_ptr()
  args.exact_low = exact_low.data_ptr()
  check(lib.ddd_rollout_reference(ctypes.byref(args), current_stream()))
  return exact_low


def rollout_scores(y_model, exact_low, times, max_error, frac_good, stop_times,
                   want_rows=False, workspace=None):
  """ddd_rollout_scores: y_model [R, T, S, N] (float64 or float32) against exact_low
  [T, S, N]; returns device tensors (mae [R, K, S], survival [R, Q, S]) and, with
  want_rows, also (row_abs_sum [R, T, S], good [R, Q, T, S] uint8), without waiting for the
  device.  times, max_error, frac_good and stop_times are host sequences."""
  lib = load_library()
  torch = require_gpu()
  if not isinstance(y_model, torch.Tensor) or y_model.dim() != 4:
    raise ValueError('y_model must be a device tensor [replica, time, sample, x]')
  if y_model.dtype not in (torch.float64, torch.float32):
    raise ValueError('y_model must be float64 or float32')
  _check_device('y_model', y_model, y_model.dtype, None)
  replicas, num_times, samples, points = (int(v) for v in y_model.shape)
  _check_device('exact_low', exact_low, torch.float64, (num_times, samples, points))
  times = np.ascontiguousarray(times, dtype=np.float64)
  max_error = np.ascontiguousarray(max_error, dtype=np.float64)
  frac_good = np.ascontiguousarray(frac_good, dtype=np.float64)
  stop_times = np.ascontiguousarray(stop_times, dtype=np.float64)
  if times.shape != (num_times,):
    raise ValueError('times must have one entry per row of y_model')
  if max_error.ndim != 1 or max_error.shape != frac_good.shape or stop_times.ndim != 1:
    raise ValueError('max_error and frac_good [Q], stop_times [K]')
  nq, nk = int(max_error.size), int(stop_times.size)
  device = y_model.device
  ws_bytes = lib.ddd_rollout_scores_workspace_bytes(replicas, num_times, samples, nq)
  if ws_bytes == 0:
    check(-1)
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
  mae = torch.empty((replicas, nk, samples), dtype=torch.float64, device=device)
  survival = torch.empty((replicas, nq, samples), dtype=torch.float64, device=device)
  rows = good = None
  if want_rows:
    rows = torch.empty((replicas, num_times, samples), dtype=torch.float64, device=device)
    good = torch.empty((replicas, nq, num_times, samples), dtype=torch.uint8, device=device)
  args = DDDRolloutScoresArgs()
  args.struct_size = ctypes.sizeof(DDDRolloutScoresArgs)
  args.replicas = replicas
  args.num_times = num_times
  args.num_samples = samples
  args.num_points = points
  args.num_quantiles = nq
  args.num_stop_times = nk
  args.dtype = ROLLOUT_F32 if y_model.dtype == torch.float32 else ROLLOUT_F64
  args.y_model = y_model.data_ptr()
  args.exact_low = exact_low.data_ptr()
  args.times = times.ctypes.data
  args.max_error = max_error.ctypes.data
  args.frac_good = frac_good.ctypes.data
  args.stop_times = stop_times.ctypes.data
  args.mae = mae.data_ptr()
  args.survival = survival.data_ptr()
  args.row_abs_sum = None if rows is None else rows.data_ptr()
  args.good = None if good is None else good.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_rollout_scores(ctypes.byref(args), current_stream()))
  if want_rows:
    return mae, survival, rows, good
  return mae, survival


def _check_f32_device(name, tensor, shape):
  torch = _torch()
  if (not isinstance(tensor, torch.Tensor) or tensor.dtype != torch.float32 or
      not tensor.is_cuda or not tensor.is_contiguous()):
    raise ValueError('{} must be a contiguous float32 device tensor'.format(name))
  if tuple(tensor.shape) != tuple(shape):
    raise ValueError('{} has shape {}, expected {}'.format(name, tuple(tensor.shape),
                                                           tuple(shape)))


def vjp_num_weights(cfg) -> int:
  """Floats of the conv weight vector of `cfg` (ddd_model_create layout)."""
  c_out = 1
  if cfg.model_target == MODEL_TARGETS['coefficients']:
    if cfg.polynomial_accuracy_order > 0:
      c_out = sum(cfg.input_sizes[d] for d in range(cfg.num_derivatives))
    else:
      c_out = cfg.num_derivatives * cfg.stencil_size
  elif cfg.model_target == MODEL_TARGETS['space_derivatives']:
    c_out = cfg.num_derivatives
  total = 0
  for l in range(cfg.num_layers):
    cin = 1 if l == 0 else cfg.filter_size
    cout = c_out if l == cfg.num_layers - 1 else cfg.filter_size
    total += cfg.kernel_size * cin * cout + cout
  return total


def result_vjp(cfg, weights, y, cotangent=None, nullspace=None, bias=None,
               want_predictions=None, want_grad_y=True, want_grad_weights=True,
               workspace=None):
  """ddd_result_vjp: (predictions or None, grad_y or None, grad_weights or None) on the
  current stream.

  weights (flat, ddd_model_create layout) / y [batch, N] / cotangent [batch, N, H] /
  nullspace / bias are float32 device tensors.  Without a cotangent only the
  predictions [batch, N, H] are computed; with one, grad_y [batch, N] and grad_weights
  (the layout of `weights`) as asked, and the predictions when want_predictions is true
  (default: only without a cotangent).  `workspace`: a uint8 device tensor of at least
  ddd_vjp_workspace_bytes bytes, reused across calls when given.  Shapes, dtypes and
  devices are checked before any device work."""
  lib = load_library()
  torch = _torch()
  if not isinstance(y, torch.Tensor) or y.dim() != 2:
    raise ValueError('y must be a [batch, N] tensor')
  batch, heads = int(y.shape[0]), cfg.num_derivatives + 1
  ws_bytes = lib.ddd_vjp_workspace_bytes(ctypes.byref(cfg), batch)   # the config checks
  if ws_bytes == 0:
    check(-1)
  _check_f32_device('y', y, (batch, cfg.num_points))
  _check_f32_device('weights', weights, (vjp_num_weights(cfg),))
  if cotangent is not None:
    _check_f32_device('cotangent', cotangent, (batch, cfg.num_points, heads))
  for name, tensor in (('nullspace', nullspace), ('bias', bias)):
    if tensor is not None:
      _check_f32_device(name, tensor, tuple(tensor.shape))
  if want_predictions is None:
    want_predictions = cotangent is None
  if cotangent is None:
    want_grad_y = want_grad_weights = False
  require_gpu()
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
  preds = (torch.empty((batch, cfg.num_points, heads), dtype=torch.float32, device=y.device)
           if want_predictions else None)
  grad_y = torch.empty_like(y) if want_grad_y else None
  grad_w = torch.empty_like(weights) if want_grad_weights else None
  args = DDDVjpArgs()
  args.struct_size = ctypes.sizeof(DDDVjpArgs)
  args.batch = batch
  args.weights = weights.data_ptr()
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  args.y = y.data_ptr()
  args.cotangent = None if cotangent is None else cotangent.data_ptr()
  args.predictions = None if preds is None else preds.data_ptr()
  args.grad_y = None if grad_y is None else grad_y.data_ptr()
  args.grad_weights = None if grad_w is None else grad_w.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_result_vjp(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return preds, grad_y, grad_w


def _check_tangent_count(tangents):
  if not 1 <= int(tangents) <= MAX_TANGENTS:
    raise ValueError('tangents = {} out of range [1, {}]'.format(tangents, MAX_TANGENTS))


def result_jvp(cfg, weights, y, tangent_y=None, tangent_weights=None, nullspace=None,
               bias=None, want_predictions=True, workspace=None):
  """ddd_result_jvp: (predictions [batch, N, H] or None, tangents [batch, M, N, H]) on the
  current stream: the Jacobian of one evaluation applied to M directions per sample.

  tangent_y [batch, M, N] (directions of the state) and / or tangent_weights
  [M, n_weights] (directions of the weights, shared by the batch); with both, the sum of
  the two contributions.  Everything else as result_vjp, and like there shapes, dtypes and
  devices are checked before any device work."""
  lib = load_library()
  torch = _torch()
  if not isinstance(y, torch.Tensor) or y.dim() != 2:
    raise ValueError('y must be a [batch, N] tensor')
  if tangent_y is None and tangent_weights is None:
    raise ValueError('tangent_y and tangent_weights are both None')
  lead = tangent_y if tangent_y is not None else tangent_weights
  if not isinstance(lead, torch.Tensor) or lead.dim() != (3 if tangent_y is not None else 2):
    raise ValueError('tangent_y must be a [batch, M, N] tensor, tangent_weights a '
                     '[M, n_weights] tensor')
  tangents = int(lead.shape[1] if tangent_y is not None else lead.shape[0])
  _check_tangent_count(tangents)
  batch, heads = int(y.shape[0]), cfg.num_derivatives + 1
  ws_bytes = lib.ddd_jvp_workspace_bytes(ctypes.byref(cfg), batch, tangents)
  if ws_bytes == 0:
    check(-1)
  _check_f32_device('y', y, (batch, cfg.num_points))
  _check_f32_device('weights', weights, (vjp_num_weights(cfg),))
  if tangent_y is not None:
    _check_f32_device('tangent_y', tangent_y, (batch, tangents, cfg.num_points))
  if tangent_weights is not None:
    _check_f32_device('tangent_weights', tangent_weights, (tangents, vjp_num_weights(cfg)))
  for name, tensor in (('nullspace', nullspace), ('bias', bias)):
    if tensor is not None:
      _check_f32_device(name, tensor, tuple(tensor.shape))
  require_gpu()
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
  preds = (torch.empty((batch, cfg.num_points, heads), dtype=torch.float32, device=y.device)
           if want_predictions else None)
  out = torch.empty((batch, tangents, cfg.num_points, heads), dtype=torch.float32,
                    device=y.device)
  args = DDDJvpArgs()
  args.struct_size = ctypes.sizeof(DDDJvpArgs)
  args.batch = batch
  args.tangents = tangents
  args.weights = weights.data_ptr()
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  args.y = y.data_ptr()
  args.tangent_y = None if tangent_y is None else tangent_y.data_ptr()
  args.tangent_weights = None if tangent_weights is None else tangent_weights.data_ptr()
  args.predictions = None if preds is None else preds.data_ptr()
  args.tangents_out = out.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_result_jvp(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return preds, out


def tangent_rollout(cfg, weights, y0, tangents0, num_steps, dt, nullspace=None, bias=None,
                    workspace=None):
  """ddd_tangent_rollout: (state [batch, N], tangents [batch, M, N]) after num_steps
  midpoint steps of size dt of y0 [batch, N] and its state tangents tangents0
  [batch, M, N], in one launch on the current stream.  State tangents only, unforced."""
  lib = load_library()
  torch = _torch()
  if not isinstance(y0, torch.Tensor) or y0.dim() != 2:
    raise ValueError('y0 must be a [batch, N] tensor')
  if not isinstance(tangents0, torch.Tensor) or tangents0.dim() != 3:
    raise ValueError('tangents0 must be a [batch, M, N] tensor')
  tangents = int(tangents0.shape[1])
  _check_tangent_count(tangents)
  if int(num_steps) < 1:
    raise ValueError('num_steps must be >= 1, got {}'.format(num_steps))
  batch = int(y0.shape[0])
  ws_bytes = lib.ddd_tangent_rollout_workspace_bytes(ctypes.byref(cfg), batch, tangents)
  if ws_bytes == 0:
    check(-1)
  _check_f32_device('y0', y0, (batch, cfg.num_points))
  _check_f32_device('weights', weights, (vjp_num_weights(cfg),))
  _check_f32_device('tangents0', tangents0, (batch, tangents, cfg.num_points))
  for name, tensor in (('nullspace', nullspace), ('bias', bias)):
    if tensor is not None:
      _check_f32_device(name, tensor, tuple(tensor.shape))
  require_gpu()
  if workspace is None or workspace.numel() < ws_bytes:
    workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=y0.device)
  state = torch.empty_like(y0)
  out = torch.empty_like(tangents0)
  args = DDDTangentRolloutArgs()
  args.struct_size = ctypes.sizeof(DDDTangentRolloutArgs)
  args.batch = batch
  args.tangents = tangents
  args.num_steps = int(num_steps)
  args.dt = float(dt)
  args.weights = weights.data_ptr()
  args.nullspace = None if nullspace is None else nullspace.data_ptr()
  args.bias = None if bias is None else bias.data_ptr()
  args.y0 = y0.data_ptr()
  args.tangents0 = tangents0.data_ptr()
  args.state_out = state.data_ptr()
  args.tangents_out = out.data_ptr()
  args.workspace = workspace.data_ptr()
  args.workspace_bytes = workspace.numel()
  check(lib.ddd_tangent_rollout(ctypes.byref(cfg), ctypes.byref(args), current_stream()))
  return state, out


def load_probe_library():
  """dlopen libddd1d_probe.so (the -DDDD_PROBES flavour: ddd_debug_* entry points,
  phase tracing, hardware probes) INSTEAD of the product library.  Only
  profiles/tools/ and `bench.py --debug-option` do this, before any other call."""
  if not os.path.exists(PROBE_LIBRARY_PATH):
    raise ImportError(
        '{} not found: build it with `python -c "import __graft_entry__ as g; '
        'g.build_probe()"`'.format(PROBE_LIBRARY_PATH))
  return load_library(PROBE_LIBRARY_PATH)


def debug_set_option(name: str, value: int):
  """Profiling / A-B switches (capi.hip: ddd_debug_set_option); every change is
  logged to stderr by the library.  They exist in libddd1d_probe.so only: the
  product library has no such entry point (load_probe_library first)."""
  lib = load_library()
  if not hasattr(lib, 'ddd_debug_set_option'):
    raise DDDError('the product library has no debug switches: call '
                   '_lib.load_probe_library() (libddd1d_probe.so) before anything else')
  fn = lib.ddd_debug_set_option
  fn.restype = ctypes.c_int
  fn.argtypes = [ctypes.c_char_p, ctypes.c_longlong]
  check(fn(name.encode('utf-8'), int(value)))


def selftest_mfma_layout():
  lib = load_library()
  require_gpu()
  check(lib.ddd_selftest_mfma_layout())
