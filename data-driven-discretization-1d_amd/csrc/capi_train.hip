// C ABI of libddd1d.so (include/ddd1d.h), the entry points that take a ddd_config and no
// ddd_model: training, evaluation metrics, the VJP and the tangent-linear model.  Each checks its arguments, has
// train_plan.h plan the launch, copies the argument pointers into the kernel's parameter
// struct and calls the launcher of train*.h.  No kernel here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "capi_common.h"
#include "train_plan.h"

using namespace ddd::capi;
using namespace ddd::train;

static_assert(kMaxTimeSteps == DDD_MAX_TIME_STEPS, "train_unrolled.h / ddd1d.h");
static_assert(kMaxUnrolledHeads == DDD_MAX_UNROLLED_HEADS, "train_unrolled.h / ddd1d.h");
static_assert(kMaxRolloutSteps == DDD_MAX_ROLLOUT_STEPS, "train_rollout.h / ddd1d.h");
static_assert(kMaxReplicas == DDD_MAX_REPLICAS, "train_population.h / ddd1d.h");
static_assert(kMaxTangents == DDD_MAX_TANGENTS, "train.h / ddd1d.h");

namespace {

inline bool projects(const TrainParams& p) {
  return p.target == DDD_TARGET_COEFFICIENTS && p.pao > 0;
}

// What every entry point that runs the training kernels checks first of the dataset it is
// given, for any of their argument structs (equally named fields): nullspace / bias where
// the configuration of p projects, num_rows, and the `batch` rows (`name`: the argument's)
// where the sample_index is left out.
template <typename Args>
int check_dataset_args(const Args* a, const TrainParams& p, int batch, const char* name) {
  if (projects(p) && (!a->nullspace || !a->bias))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "nullspace/bias required for model_target 'coefficients' with "
                "polynomial_accuracy_order > 0");
  if (a->num_rows < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_rows = %d", a->num_rows);
  if (a->sample_index == nullptr && batch > a->num_rows)
    return fail(DDD_ERR_INVALID_ARGUMENT, "%s = %d > num_rows = %d without a sample_index",
                name, batch, a->num_rows);
  return DDD_OK;
}

// The workspace of at least ws bytes (ws_bytes_fn names the entry point's workspace
// function in the message, `prefix` the entry point where its messages carry the name),
// then it and the projection tables into p.
template <typename Args>
int take_workspace(const Args* a, TrainParams& p, size_t ws, const char* ws_bytes_fn,
                   const char* prefix = "") {
  if (a->workspace == nullptr || a->workspace_bytes < ws)
    return fail(DDD_ERR_INVALID_ARGUMENT, "%sworkspace of %zu bytes given, %s = %zu", prefix,
                a->workspace == nullptr ? (size_t)0 : a->workspace_bytes, ws_bytes_fn, ws);
  p.nullspace = projects(p) ? a->nullspace : nullptr;
  p.bias = projects(p) ? a->bias : nullptr;
  p.ws = static_cast<float*>(a->workspace);
  return DDD_OK;
}

// The learning-rate table [max(replicas, 1)][steps] (replicas = 0: one unnamed model) and
// Adam's constants
template <typename Args>
int check_adam_args(const Args* a, int replicas, int steps) {
  for (int i = 0; i < std::max(replicas, 1); ++i)
    for (int k = 0; k < steps; ++k) {
      const double rate = a->learning_rate[(size_t)i * steps + k];
      if (std::isfinite(rate) && rate >= 0.0) continue;
      if (replicas == 0)
        return fail(DDD_ERR_INVALID_ARGUMENT, "learning_rate of step %d is %g (finite, >= 0)",
                    k, rate);
      return fail(DDD_ERR_INVALID_ARGUMENT,
                  "learning_rate of replica %d, step %d is %g (finite, >= 0)", i, k, rate);
    }
  if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0))
    return fail(DDD_ERR_INVALID_ARGUMENT, "beta1 = %g, beta2 = %g outside [0, 1)", a->beta1,
                a->beta2);
  if (!(a->epsilon > 0.0) || !std::isfinite(a->epsilon))
    return fail(DDD_ERR_INVALID_ARGUMENT, "epsilon = %g (> 0)", a->epsilon);
  return DDD_OK;
}

// Last, behind the checks of an entry point's own: the workspace, the `heads` per-head loss
// constants, finite, into floor / coef_abs / coef_rel, and the dataset and workspace
// pointers into p.
template <typename Args>
int take_dataset_args(const Args* a, TrainParams& p, size_t ws, const char* ws_bytes_fn,
                      int heads, float* floor, float* coef_abs, float* coef_rel) {
  int rc = take_workspace(a, p, ws, ws_bytes_fn);
  if (rc) return rc;
  for (int h = 0; h < heads; ++h) {
    if (!std::isfinite(a->error_floor[h]) || !std::isfinite(a->coef_abs[h]) ||
        !std::isfinite(a->coef_rel[h]))
      return fail(DDD_ERR_INVALID_ARGUMENT, "non-finite error_floor / coefficient of head %d", h);
    floor[h] = a->error_floor[h];
    coef_abs[h] = a->coef_abs[h];
    coef_rel[h] = a->coef_rel[h];
  }
  p.weights = a->weights;
  p.y = a->y;
  p.rows = a->num_rows;
  p.labels = a->labels;
  p.baseline = a->baseline;
  return DDD_OK;
}

// What ddd_train_run and ddd_train_population_run check and copy alike (equally named
// fields): the arguments into r, whose configuration plan_population has filled.  The
// workspace has at least ws bytes, the coefficient table(s) table_offset bytes into it.
// replicas: 0 for ddd_train_run (learning_rate [num_steps]), otherwise R ([R][num_steps]).
template <typename Args>
int train_run_args(const Args* a, RunParams& r, size_t ws, size_t table_offset, int replicas,
                   const char* ws_bytes_fn) {
  TrainParams& p = r.q.t;
  if (!a->weights || !a->adam_m || !a->adam_v || !a->y || !a->labels || !a->baseline ||
      !a->sample_index || !a->learning_rate || !a->head_means_log)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "weights, adam_m, adam_v, y, labels, baseline, sample_index, learning_rate "
                "and head_means_log must not be NULL");
  int rc = check_dataset_args(a, p, a->batch, "batch");
  if (rc) return rc;
  if (a->num_steps < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_steps = %d (>= 1)", a->num_steps);
  if (a->first_step < 0)
    return fail(DDD_ERR_INVALID_ARGUMENT, "first_step = %d (>= 0)", a->first_step);
  rc = check_adam_args(a, replicas, a->num_steps);
  if (rc) return rc;
  if (!(a->error_max >= 0.0) || !std::isfinite(a->error_max))
    return fail(DDD_ERR_INVALID_ARGUMENT, "error_max = %g (>= 0)", a->error_max);
  if (a->num_time_steps > 0 && !std::isfinite(a->time_step))
    return fail(DDD_ERR_INVALID_ARGUMENT, "non-finite time_step");
  rc = take_dataset_args(a, p, ws, ws_bytes_fn, r.heads, r.floor, r.coef_abs, r.coef_rel);
  if (rc) return rc;
  for (int h = 0; h < r.heads; ++h) {
    if (a->error_max > 0.0 &&
        (!std::isfinite(a->error_scale_abs[h]) || !std::isfinite(a->error_scale_rel[h])))
      return fail(DDD_ERR_INVALID_ARGUMENT, "non-finite error_scale of head %d", h);
    r.q.floor[h] = r.floor[h];
    r.q.coef_abs[h] = r.coef_abs[h];
    r.q.coef_rel[h] = r.coef_rel[h];
    if (r.q.T == 0) {   // (heads = H <= kMaxHeads)
      p.floor[h] = r.floor[h];
      p.coef_abs[h] = r.coef_abs[h];
      p.coef_rel[h] = r.coef_rel[h];
    }
    r.scale_abs[h] = a->error_scale_abs[h];
    r.scale_rel[h] = a->error_scale_rel[h];
  }
  p.predictions = nullptr;
  r.q.dt = a->time_step;
  r.first_step = a->first_step;
  r.num_steps = a->num_steps;
  r.learning_rate = a->learning_rate;
  r.beta1 = a->beta1;
  r.beta2 = a->beta2;
  r.epsilon = a->epsilon;
  r.sample_index = a->sample_index;
  r.weights = a->weights;
  r.adam_m = a->adam_m;
  r.adam_v = a->adam_v;
  r.head_means_log = a->head_means_log;
  r.last_grad = a->last_grad;
  r.error_max = a->error_max;
  r.coef_table = reinterpret_cast<float*>(static_cast<char*>(a->workspace) + table_offset);
  return DDD_OK;
}

// What ddd_train_loss_grad and ddd_train_unrolled_loss_grad check and copy alike (equally
// named fields): the argument pointers into p and the `heads` per-head loss constants into
// floor / coef_abs / coef_rel.
template <typename Args>
int train_args(const Args* a, TrainParams& p, size_t ws, const char* ws_bytes_fn, int heads,
               float* floor, float* coef_abs, float* coef_rel) {
  if (!a->weights || !a->y || !a->labels || !a->baseline || !a->head_means)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "weights, y, labels, baseline and head_means must not be NULL");
  int rc = check_dataset_args(a, p, a->batch, "batch");
  if (rc) return rc;
  if constexpr (std::is_same<Args, ddd_train_unrolled_args>::value)
    if (!std::isfinite(a->time_step))
      return fail(DDD_ERR_INVALID_ARGUMENT, "non-finite time_step");
  rc = take_dataset_args(a, p, ws, ws_bytes_fn, heads, floor, coef_abs, coef_rel);
  if (rc) return rc;
  p.sample_index = a->sample_index;
  p.predictions = a->predictions;
  p.want_grad = a->grad != nullptr ? 1 : 0;
  p.grad = a->grad;
  p.head_means = a->head_means;
  return DDD_OK;
}

// What ddd_train_rollout_loss_grad and ddd_train_rollout_run check and copy alike of the
// windows (equally named fields): save_every, dt, the window tensors, the forcing tables,
// the projection tables, num_rows and the workspace of at least ws bytes, then all of them
// into q, whose configuration plan_rollout has filled.
template <typename Args>
int take_rollout_windows(const ddd_config* cfg, const Args* a, RolloutParams& q, size_t ws,
                         const char* ws_bytes_fn) {
  TrainParams& p = q.t;
  if (a->save_every < 1 || a->num_steps % a->save_every != 0)
    return fail(DDD_ERR_INVALID_ARGUMENT, "save_every = %d must be >= 1 and divide num_steps = %d",
                a->save_every, a->num_steps);
  if (!(a->dt > 0.0) || !std::isfinite(a->dt))
    return fail(DDD_ERR_INVALID_ARGUMENT, "dt = %g must be positive and finite", a->dt);
  if (!a->y0 || !a->targets || !a->step_weights)
    return fail(DDD_ERR_INVALID_ARGUMENT, "y0, targets and step_weights must not be NULL");
  const int tables = (a->amplitude != nullptr) + (a->omega != nullptr) + (a->phase != nullptr) +
                     (a->k_index != nullptr) + (a->spatial_phase != nullptr);
  if (tables != 0 && tables != 5)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "forcing: amplitude, omega, phase, k_index and spatial_phase must be given "
                "together (all NULL = unforced)");
  if (tables == 5 && (a->nparams < 1 || a->n_k < 1))
    return fail(DDD_ERR_INVALID_ARGUMENT, "forcing: nparams = %d, n_k = %d (>= 1)", a->nparams,
                a->n_k);
  int rc = check_dataset_args(a, p, a->batch, "batch");
  if (rc == DDD_OK) rc = take_workspace(a, p, ws, ws_bytes_fn);
  if (rc) return rc;
  p.y = a->y0;
  p.rows = a->num_rows;
  q.save_every = a->save_every;
  q.n_saved = a->num_steps / a->save_every;
  q.dt = (float)a->dt;
  q.dt64 = a->dt;
  q.targets = a->targets;
  q.step_weights = a->step_weights;
  q.t0 = a->t0;
  // KdV and KS: finalize_time_derivative is the identity, the tables are ignored
  q.forced = tables == 5 && is_forced_family(cfg->equation) ? 1 : 0;
  if (q.forced) {
    q.P = a->nparams;
    q.n_k = a->n_k;
    q.amplitude = a->amplitude;
    q.omega = a->omega;
    q.phase = a->phase;
    q.k_index = a->k_index;
    q.spatial_phase = a->spatial_phase;
  }
  return DDD_OK;
}

// ddd_train_population_run, and ddd_train_run (`solo`) under its own names
template <typename Args>
int train_population(const ddd_config* cfg, const Args* a, int replicas, int index_per_replica,
                     bool solo, void* stream) {
  PopulationParams pp;
  LaunchPlan lp{};
  int rc = plan_population(cfg, a->batch, a->num_time_steps, replicas, &pp.r, &lp,
                           solo ? "training run" : "training population");
  if (rc) return rc;
  if (index_per_replica != 0 && index_per_replica != 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "index_per_replica = %d (0 or 1)", index_per_replica);
  rc = train_run_args(a, pp.r, lp.ws_bytes, lp.tables, solo ? 0 : replicas,
                      solo ? "ddd_train_run_workspace_bytes"
                           : "ddd_train_population_workspace_bytes");
  if (rc) return rc;
  pp.replicas = replicas;
  pp.index_per_replica = index_per_replica;
  DDD_HIP(launch_train_population(pp, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

}  // namespace

extern "C" {

size_t ddd_train_workspace_bytes(const ddd_config* cfg, int batch) {
  TrainParams p;
  LaunchPlan lp{};
  return plan_training(cfg, batch, &p, &lp) ? 0 : lp.ws_bytes;
}

int ddd_train_loss_grad(const ddd_config* cfg, const ddd_train_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_train_args);
  TrainParams p;
  LaunchPlan lp{};
  int rc = plan_training(cfg, a->batch, &p, &lp);
  if (rc) return rc;
  rc = train_args(a, p, lp.ws_bytes, "ddd_train_workspace_bytes", p.H, p.floor, p.coef_abs,
                  p.coef_rel);
  if (rc) return rc;
  DDD_HIP(launch_loss_grad(p, lp.blocks, lp.lds_bytes, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_train_unrolled_workspace_bytes(const ddd_config* cfg, int batch, int num_time_steps) {
  UnrolledParams q;
  LaunchPlan lp{};
  return plan_unrolled(cfg, batch, num_time_steps, &q, &lp) ? 0 : lp.ws_bytes;
}

int ddd_train_unrolled_loss_grad(const ddd_config* cfg, const ddd_train_unrolled_args* a,
                                 void* stream) {
  DDD_CHECK_ARGS(a, ddd_train_unrolled_args);
  UnrolledParams q;
  LaunchPlan lp{};
  int rc = plan_unrolled(cfg, a->batch, a->num_time_steps, &q, &lp);
  if (rc) return rc;
  rc = train_args(a, q.t, lp.ws_bytes, "ddd_train_unrolled_workspace_bytes", q.HT, q.floor,
                  q.coef_abs, q.coef_rel);
  if (rc) return rc;
  q.dt = a->time_step;
  DDD_HIP(launch_unrolled_loss_grad(q, lp.blocks, lp.lds_bytes,
                                    static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_train_rollout_workspace_bytes(const ddd_config* cfg, int batch, int num_steps) {
  RolloutParams q;
  LaunchPlan lp{};
  return plan_rollout(cfg, batch, num_steps, &q, &lp) ? 0 : lp.ws_bytes;
}

int ddd_train_rollout_loss_grad(const ddd_config* cfg, const ddd_train_rollout_args* a,
                                void* stream) {
  DDD_CHECK_ARGS(a, ddd_train_rollout_args);
  RolloutParams q;
  TrainParams& p = q.t;
  LaunchPlan lp{};
  int rc = plan_rollout(cfg, a->batch, a->num_steps, &q, &lp);
  if (rc) return rc;
  if (!a->weights || !a->step_means)
    return fail(DDD_ERR_INVALID_ARGUMENT, "weights and step_means must not be NULL");
  rc = take_rollout_windows(cfg, a, q, lp.ws_bytes, "ddd_train_rollout_workspace_bytes");
  if (rc) return rc;
  p.weights = a->weights;
  p.sample_index = a->sample_index;
  p.want_grad = a->grad != nullptr ? 1 : 0;
  p.grad = a->grad;
  p.head_means = a->step_means;
  q.trajectory = a->trajectory;
  DDD_HIP(launch_rollout_loss_grad(q, lp.blocks, lp.lds_bytes,
                                   static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_train_rollout_run_workspace_bytes(const ddd_config* cfg, int batch, int num_steps,
                                             int replicas) {
  RolloutRunParams rr;
  LaunchPlan lp{};
  return plan_rollout_run(cfg, batch, num_steps, replicas, &rr, &lp) ? 0 : lp.ws_bytes;
}

int ddd_train_rollout_run(const ddd_config* cfg, const ddd_train_rollout_run_args* a,
                          void* stream) {
  DDD_CHECK_ARGS(a, ddd_train_rollout_run_args);
  RolloutRunParams rr;
  LaunchPlan lp{};
  int rc = plan_rollout_run(cfg, a->batch, a->num_steps, a->replicas, &rr, &lp);
  if (rc) return rc;
  const int R = a->replicas, K = a->num_opt_steps;
  if (a->index_per_replica != 0 && a->index_per_replica != 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "index_per_replica = %d (0 or 1)",
                a->index_per_replica);
  if (a->forward_only != 0 && a->forward_only != 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "forward_only = %d (0 or 1)", a->forward_only);
  if (K < 1 || (a->forward_only && K != 1))
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_opt_steps = %d (>= 1; 1 with forward_only)", K);
  if (!a->weights || !a->step_means_log)
    return fail(DDD_ERR_INVALID_ARGUMENT, "weights and step_means_log must not be NULL");
  if (!a->forward_only) {
    if (!a->adam_m || !a->adam_v || !a->adam_step || !a->sample_index || !a->learning_rate ||
        !a->grad_norm_log)
      return fail(DDD_ERR_INVALID_ARGUMENT,
                  "adam_m, adam_v, adam_step, sample_index, learning_rate and grad_norm_log "
                  "must not be NULL");
    rc = check_adam_args(a, R, K);
    if (rc) return rc;
    if (!(a->clip_norm >= 0.0) || !std::isfinite(a->clip_norm))
      return fail(DDD_ERR_INVALID_ARGUMENT, "clip_norm = %g (>= 0, finite)", a->clip_norm);
  }
  rc = take_rollout_windows(cfg, a, rr.q, lp.ws_bytes, "ddd_train_rollout_run_workspace_bytes");
  if (rc) return rc;
  rr.q.t.weights = a->weights;
  rr.replicas = R;
  rr.index_per_replica = a->index_per_replica;
  rr.forward_only = a->forward_only;
  rr.num_opt_steps = K;
  rr.learning_rate = a->learning_rate;
  rr.beta1 = a->beta1;
  rr.beta2 = a->beta2;
  rr.epsilon = a->epsilon;
  rr.clip_norm = a->clip_norm;
  rr.sample_index = a->sample_index;
  rr.weights = a->weights;
  rr.adam_m = a->adam_m;
  rr.adam_v = a->adam_v;
  rr.adam_step = a->adam_step;
  rr.step_means_log = a->step_means_log;
  rr.grad_norm_log = a->grad_norm_log;
  rr.last_grad = a->last_grad;
  char* base = static_cast<char*>(a->workspace);
  rr.grad_buf = reinterpret_cast<float*>(base + lp.grad_buf);
  rr.partials = reinterpret_cast<double*>(base + lp.partials);
  rr.decisions = reinterpret_cast<RolloutDecision*>(base + lp.decisions);
  DDD_HIP(launch_train_rollout_run(rr, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_train_run_workspace_bytes(const ddd_config* cfg, int batch, int num_time_steps) {
  RunParams r;
  LaunchPlan lp{};
  return plan_population(cfg, batch, num_time_steps, 1, &r, &lp, "training run") ? 0
                                                                                 : lp.ws_bytes;
}

size_t ddd_train_population_workspace_bytes(const ddd_config* cfg, int batch, int num_time_steps,
                                            int replicas) {
  RunParams r;
  LaunchPlan lp{};
  return plan_population(cfg, batch, num_time_steps, replicas, &r, &lp) ? 0 : lp.ws_bytes;
}

int ddd_train_run(const ddd_config* cfg, const ddd_train_run_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_train_run_args);
  return train_population(cfg, a, 1, 0, true, stream);   // the population of one
}

int ddd_train_population_run(const ddd_config* cfg, const ddd_train_population_args* a,
                             void* stream) {
  DDD_CHECK_ARGS(a, ddd_train_population_args);
  return train_population(cfg, a, a->replicas, a->index_per_replica, false, stream);
}

size_t ddd_eval_metrics_workspace_bytes(const ddd_config* cfg, int rows_evaluated,
                                        int num_time_steps, int replicas) {
  MetricsParams m;
  LaunchPlan lp{};
  return plan_metrics(cfg, rows_evaluated, num_time_steps, replicas, &m, &lp) ? 0 : lp.ws_bytes;
}

int ddd_eval_metrics(const ddd_config* cfg, const ddd_eval_metrics_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_eval_metrics_args);
  MetricsParams m;
  LaunchPlan lp{};
  int rc = plan_metrics(cfg, a->rows_evaluated, a->num_time_steps, a->replicas, &m, &lp);
  if (rc) return rc;
  UnrolledParams& q = m.q;
  TrainParams& p = q.t;
  if (a->index_per_replica != 0 && a->index_per_replica != 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "index_per_replica = %d (0 or 1)",
                a->index_per_replica);
  if (!a->weights || !a->y || !a->labels || !a->baseline || !a->sums || !a->below)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "weights, y, labels, baseline, sums and below must not be NULL");
  rc = check_dataset_args(a, p, a->rows_evaluated, "rows_evaluated");
  if (rc) return rc;
  if (a->sample_index == nullptr && a->index_per_replica)
    return fail(DDD_ERR_INVALID_ARGUMENT, "index_per_replica = 1 without a sample_index");
  if (a->num_time_steps > 0 && !std::isfinite(a->time_step))
    return fail(DDD_ERR_INVALID_ARGUMENT, "non-finite time_step");
  rc = take_dataset_args(a, p, lp.ws_bytes, "ddd_eval_metrics_workspace_bytes", q.HT, q.floor,
                         q.coef_abs, q.coef_rel);
  if (rc) return rc;
  p.sample_index = a->sample_index;
  p.index_stride = a->index_per_replica ? p.batch : 0;
  p.predictions = a->predictions;
  q.dt = a->time_step;
  m.sums = a->sums;
  m.below = a->below;
  DDD_HIP(launch_eval_metrics(m, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_vjp_workspace_bytes(const ddd_config* cfg, int batch) {
  TrainParams p;
  LaunchPlan lp{};
  return plan_training(cfg, batch, &p, &lp, "ddd_result_vjp") ? 0 : lp.ws_bytes;
}

int ddd_result_vjp(const ddd_config* cfg, const ddd_vjp_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_vjp_args);
  VjpParams q;
  std::memset(&q, 0, sizeof(q));
  TrainParams& p = q.t;
  LaunchPlan lp{};
  int rc = plan_training(cfg, a->batch, &p, &lp, "ddd_result_vjp");
  if (rc) return rc;
  if (!a->weights || !a->y)
    return fail(DDD_ERR_INVALID_ARGUMENT, "ddd_result_vjp: weights and y must not be NULL");
  if (projects(p) && (!a->nullspace || !a->bias))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_vjp: nullspace/bias required for model_target 'coefficients' "
                "with polynomial_accuracy_order > 0");
  const bool want_grads = a->grad_y != nullptr || a->grad_weights != nullptr;
  if (a->cotangent != nullptr && !want_grads)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_vjp: a cotangent with grad_y and grad_weights both NULL");
  if (a->cotangent == nullptr && want_grads)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_vjp: grad_y / grad_weights need a cotangent");
  if (a->cotangent == nullptr && a->predictions == nullptr)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_vjp: no cotangent and no predictions: nothing to compute");
  rc = take_workspace(a, p, lp.ws_bytes, "ddd_vjp_workspace_bytes", "ddd_result_vjp: ");
  if (rc) return rc;
  p.weights = a->weights;
  p.y = a->y;
  p.rows = a->batch;
  p.predictions = a->predictions;
  p.want_grad = a->grad_weights != nullptr ? 1 : 0;
  p.grad = a->grad_weights;
  q.cotangent = a->cotangent;
  q.grad_y = a->grad_y;
  DDD_HIP(launch_vjp(q, lp.blocks, lp.lds_bytes, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_jvp_workspace_bytes(const ddd_config* cfg, int batch, int tangents) {
  JvpParams q;
  LaunchPlan lp{};
  return plan_jvp(cfg, batch, tangents, &q, &lp) ? 0 : lp.ws_bytes;
}

int ddd_result_jvp(const ddd_config* cfg, const ddd_jvp_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_jvp_args);
  JvpParams q;
  TrainParams& p = q.t;
  LaunchPlan lp{};
  int rc = plan_jvp(cfg, a->batch, a->tangents, &q, &lp);
  if (rc) return rc;
  if (!a->weights || !a->y || !a->tangents_out)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_jvp: weights, y and tangents_out must not be NULL");
  if (projects(p) && (!a->nullspace || !a->bias))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_jvp: nullspace/bias required for model_target 'coefficients' "
                "with polynomial_accuracy_order > 0");
  if (a->tangent_y == nullptr && a->tangent_weights == nullptr)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_result_jvp: tangent_y and tangent_weights both NULL");
  rc = take_workspace(a, p, lp.ws_bytes, "ddd_jvp_workspace_bytes", "ddd_result_jvp: ");
  if (rc) return rc;
  p.weights = a->weights;
  p.y = a->y;
  p.rows = a->batch;
  p.predictions = a->predictions;
  q.tangent_y = a->tangent_y;
  q.tangent_weights = a->tangent_weights;
  q.tangents_out = a->tangents_out;
  DDD_HIP(launch_jvp(q, lp.blocks, lp.lds_bytes, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

size_t ddd_tangent_rollout_workspace_bytes(const ddd_config* cfg, int batch, int tangents) {
  TangentRolloutParams q;
  LaunchPlan lp{};
  return plan_tangent_rollout(cfg, batch, tangents, &q, &lp) ? 0 : lp.ws_bytes;
}

int ddd_tangent_rollout(const ddd_config* cfg, const ddd_tangent_rollout_args* a, void* stream) {
  DDD_CHECK_ARGS(a, ddd_tangent_rollout_args);
  TangentRolloutParams q;
  TrainParams& p = q.t;
  LaunchPlan lp{};
  int rc = plan_tangent_rollout(cfg, a->batch, a->tangents, &q, &lp);
  if (rc) return rc;
  if (a->num_steps < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "ddd_tangent_rollout: num_steps = %d (>= 1)",
                a->num_steps);
  if (!std::isfinite(a->dt))
    return fail(DDD_ERR_INVALID_ARGUMENT, "ddd_tangent_rollout: dt = %g must be finite", a->dt);
  if (!a->weights || !a->y0 || !a->tangents0 || !a->state_out || !a->tangents_out)
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_tangent_rollout: weights, y0, tangents0, state_out and tangents_out must "
                "not be NULL");
  if (projects(p) && (!a->nullspace || !a->bias))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ddd_tangent_rollout: nullspace/bias required for model_target 'coefficients' "
                "with polynomial_accuracy_order > 0");
  rc = take_workspace(a, p, lp.ws_bytes, "ddd_tangent_rollout_workspace_bytes",
                      "ddd_tangent_rollout: ");
  if (rc) return rc;
  p.weights = a->weights;
  p.y = a->y0;
  p.rows = a->batch;
  q.num_steps = a->num_steps;
  q.dt = (float)a->dt;
  q.tangents = a->tangents0;
  q.state_out = a->state_out;
  q.tangents_out = a->tangents_out;
  DDD_HIP(launch_tangent_rollout(q, lp.blocks, lp.lds_bytes, static_cast<hipStream_t>(stream)));
  return DDD_OK;
}

}  // extern "C"
