// The planner of the training, evaluation-metrics, VJP and tangent entry points (capi_train.hip):
// which configurations they admit, how a workgroup's slab of the caller's workspace is
// laid out, and whether the 32 -> 32 layers' kernels are staged in LDS.  Host only: no
// kernel and no HIP call, so tests/train_plan_harness.hip runs it without a device.  The
// kernels of train*.hip index global memory and LDS by the numbers set here; nothing outside
// this header computes a slab offset, a stride or an LDS size.  Three pieces -- configure,
// lay_out_slab, plan_lds -- and one thin composition of them per entry point.  `who` names
// the entry point in the messages of what is not supported.
#pragma once
#include <algorithm>
#include <cstring>

#include "capi_common.h"
#include "train.h"
#include "train_metrics.h"
#include "train_population.h"
#include "train_rollout.h"
#include "train_rollout_population.h"
#include "train_unrolled.h"

namespace ddd {
namespace train {

using capi::fail;

constexpr size_t kLdsLimitBytes = 160 * 1024;

inline size_t pad4(size_t floats) { return (floats + 3) & ~(size_t)3; }

// What a launch needs beside its parameter struct, and the caller's workspace in bytes
struct LaunchPlan {
  int blocks;         // workgroups (= slabs) per replica: min(batch, kMaxBlocks)
  size_t lds_bytes;   // dynamic LDS of a workgroup
  size_t z_floats;    // the hidden layers' pre-activations in a slab (padded)
  size_t ws_bytes;    // the workspace the entry point asks for: the slabs of every replica,
  size_t tables;      // then (population) the coefficient tables, from here,
  size_t grad_buf, partials, decisions;   // or (rollout run) train_rollout_population.h's tail
};

// The configuration step: the checks every entry point makes of cfg and batch, then
// everything of p that follows from them alone -- the equation, the layer tables, the
// projection's split, n_weights, batch -- and the workgroups and pre-activation floats.
inline int configure(const ddd_config* cfg, int batch, const char* who, TrainParams* tp,
                     LaunchPlan* lp) {
  int rc = capi::common_config_checks(cfg);
  if (rc) return rc;
  if (cfg->equation > DDD_EQ_KS_CONSERVATIVE)
    return fail(DDD_ERR_UNSUPPORTED,
                "%s: equation %d (numerical_flux / Godunov equations) is not supported", who,
                cfg->equation);
  if (cfg->model_target == DDD_TARGET_FLUX)
    return fail(DDD_ERR_UNSUPPORTED, "%s: model_target 'flux' is not supported", who);
  if (cfg->model_target < DDD_TARGET_COEFFICIENTS || cfg->model_target > DDD_TARGET_FLUX)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown model_target %d", cfg->model_target);
  if (cfg->num_layers < 1)
    return fail(DDD_ERR_UNSUPPORTED, "%s: num_layers = %d (a net without conv layers "
                "has no conv weights to train)", who, cfg->num_layers);
  if (cfg->num_layers > DDD_MAX_LAYERS)
    return fail(DDD_ERR_UNSUPPORTED, "%s: num_layers = %d > %d", who, cfg->num_layers,
                DDD_MAX_LAYERS);
  if (cfg->kernel_size < 1 || cfg->kernel_size > 7)
    return fail(DDD_ERR_UNSUPPORTED, "%s: kernel_size = %d out of range [1, 7]", who,
                cfg->kernel_size);
  if (cfg->filter_size < 1 || cfg->filter_size > 64)
    return fail(DDD_ERR_UNSUPPORTED, "%s: filter_size = %d out of range [1, 64]", who,
                cfg->filter_size);
  if (cfg->num_points < 8 || cfg->num_points > 256)
    return fail(DDD_ERR_UNSUPPORTED, "%s: num_points = %d out of range [8, 256]", who,
                cfg->num_points);
  if (cfg->activation < DDD_ACT_RELU || cfg->activation > DDD_ACT_ELU)
    return fail(DDD_ERR_INVALID_ARGUMENT, "unknown activation %d", cfg->activation);
  if (!(cfg->standard_deviation > 0.0))
    return fail(DDD_ERR_INVALID_ARGUMENT, "standard_deviation must be positive");
  if (cfg->polynomial_accuracy_order < 0)
    return fail(DDD_ERR_INVALID_ARGUMENT, "polynomial_accuracy_order = %d",
                cfg->polynomial_accuracy_order);
  if (batch < 1) return fail(DDD_ERR_INVALID_ARGUMENT, "batch = %d", batch);

  TrainParams& p = *tp;
  std::memset(&p, 0, sizeof(p));
  p.equation = cfg->equation;
  p.N = cfg->num_points;
  p.D = cfg->num_derivatives;
  p.G = cfg->stencil_size;
  p.H = p.D + 1;
  p.target = cfg->model_target;
  p.L = cfg->num_layers;
  p.K = cfg->kernel_size;
  p.act = cfg->activation;
  p.pao = cfg->model_target == DDD_TARGET_COEFFICIENTS ? cfg->polynomial_accuracy_order : 0;
  p.unbiased = cfg->ensure_unbiased_coefficients ? 1 : 0;
  p.conservative = capi::is_conservative(cfg->equation) ? 1 : 0;
  p.eta = (float)cfg->eta;
  p.stddev = (float)cfg->standard_deviation;
  p.inv_dx = (float)(1.0 / cfg->dx);
  if (p.unbiased && (p.target != DDD_TARGET_COEFFICIENTS || p.pao != 0))
    return fail(DDD_ERR_INVALID_ARGUMENT,
                "ensure_unbiased_coefficients needs model_target 'coefficients' with "
                "polynomial_accuracy_order = 0");
  if (p.unbiased)
    for (int d = 0; d < p.D; ++d)
      if (cfg->derivative_orders[d] == 0)
        return fail(DDD_ERR_INVALID_ARGUMENT,
                    "ensure_unbiased not yet supported for 0th order spatial derivatives");
  int c_out = 1;
  if (p.target == DDD_TARGET_COEFFICIENTS) {
    if (p.pao > 0) {
      c_out = 0;
      for (int d = 0; d < p.D; ++d) {
        if (cfg->input_sizes[d] < 1 || cfg->input_sizes[d] > p.G)
          return fail(DDD_ERR_INVALID_ARGUMENT, "input_sizes[%d] = %d out of range [1, G]", d,
                      cfg->input_sizes[d]);
        p.in_start[d] = c_out;
        p.in_size[d] = cfg->input_sizes[d];
        p.ns_off[d] = c_out * p.G;
        c_out += cfg->input_sizes[d];
      }
    } else {
      c_out = p.D * p.G;
    }
  } else if (p.target == DDD_TARGET_SPACE_DERIVATIVES) {
    c_out = p.D;
  }
  p.C_out = c_out;
  size_t off = 0, zoff = 0;
  p.cmax = 1;
  for (int l = 0; l < p.L; ++l) {
    p.cin[l] = l == 0 ? 1 : cfg->filter_size;
    p.cout[l] = l == p.L - 1 ? c_out : cfg->filter_size;
    p.cmax = std::max(p.cmax, std::max(p.cin[l], p.cout[l]));
    p.w_off[l] = (int)off;
    off += (size_t)p.K * p.cin[l] * p.cout[l] + p.cout[l];
    p.z_off[l] = (int)zoff;
    if (l < p.L - 1) zoff += (size_t)p.N * p.cout[l];
  }
  p.n_weights = (int)off;
  p.batch = batch;
  lp->blocks = std::min(batch, kMaxBlocks);
  lp->z_floats = pad4(zoff);
  return DDD_OK;
}

// The slab of one workgroup, in floats: the front part (what the kernel sums over its
// samples; padded), the pre-activations, state_rows stage states [N] at *st_off and
// cotangent_rows loss cotangents [N] at *gi_off.  st_off / gi_off null: the kernel has no
// such part.  Sets p.n_slab and p.slab_stride, and lp->ws_bytes to one replica's slabs.
inline void lay_out_slab(TrainParams& p, LaunchPlan* lp, size_t front_floats, int state_rows,
                         int cotangent_rows, int* st_off, int* gi_off) {
  p.n_slab = (int)pad4(front_floats);
  const size_t states = (size_t)p.n_slab + lp->z_floats;
  const size_t cotangents = states + (size_t)state_rows * p.N;
  if (st_off != nullptr) *st_off = (int)states;
  if (gi_off != nullptr) *gi_off = (int)cotangents;
  p.slab_stride = pad4(cotangents + (size_t)cotangent_rows * p.N);
  lp->ws_bytes = (size_t)lp->blocks * p.slab_stride * sizeof(float);
}

// The LDS of one workgroup: the rows of train.h, the staged kernels [K][32][32] of the
// 32 -> 32 layers, and extra_rows rows [N] behind them (the through-time kernels' two).
// The kernels are staged, and those layers run on MFMA, only where N is a multiple of 32
// and everything fits together; otherwise every layer runs on the VALU.
inline int plan_lds(TrainParams& p, LaunchPlan* lp, int extra_rows, const char* who) {
  const size_t extra = (size_t)extra_rows * p.N;
  int staged = 0;
  for (int l = 0; l < p.L; ++l)
    if (p.N % 32 == 0 && p.cin[l] == 32 && p.cout[l] == 32) staged += p.K * 32 * 32;
  p.mfma = staged > 0 && (lds_floats(p) + staged + extra) * sizeof(float) <= kLdsLimitBytes;
  p.wl_floats = p.mfma ? staged : 0;
  for (int l = 0, at = 0; l < p.L; ++l) {
    const bool on_mfma = p.mfma && p.cin[l] == 32 && p.cout[l] == 32;
    p.wl_off[l] = on_mfma ? at : -1;
    if (on_mfma) at += p.K * 32 * 32;
  }
  lp->lds_bytes = (lds_total_floats(p) + extra) * sizeof(float);
  if (lp->lds_bytes > kLdsLimitBytes)
    return fail(DDD_ERR_UNSUPPORTED, "%s: %zu bytes of LDS needed (> 160 KiB)", who,
                lp->lds_bytes);
  return DDD_OK;
}

inline int check_time_steps(int T, const char* who) {
  if (T < 1)
    return fail(DDD_ERR_INVALID_ARGUMENT, "num_time_steps = %d (>= 1; ddd_train_loss_grad "
                "carries the loss without integrated heads)", T);
  if (T > DDD_MAX_TIME_STEPS)
    return fail(DDD_ERR_UNSUPPORTED, "%s: num_time_steps = %d > %d", who, T, DDD_MAX_TIME_STEPS);
  return DDD_OK;
}

inline int check_replicas(int R) {
  if (R < 1 || R > DDD_MAX_REPLICAS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "replicas = %d out of range [1, %d]", R,
                DDD_MAX_REPLICAS);
  return DDD_OK;
}

// ddd_train_loss_grad, and ddd_result_vjp under its own name: the gradient and the two
// rows of head sums in front.
inline int plan_training(const ddd_config* cfg, int batch, TrainParams* p, LaunchPlan* lp,
                         const char* who = "training") {
  int rc = configure(cfg, batch, who, p, lp);
  if (rc) return rc;
  lay_out_slab(*p, lp, (size_t)p->n_weights + 2 * p->H, 0, 0, nullptr, nullptr);
  return plan_lds(*p, lp, 0, who);
}

// ddd_train_unrolled_loss_grad: the wider head part, the 2 T stage states and the T
// integrated heads' cotangents behind the pre-activations, two more LDS rows.
inline int plan_unrolled(const ddd_config* cfg, int batch, int T, UnrolledParams* q,
                         LaunchPlan* lp, const char* who = "training") {
  std::memset(q, 0, sizeof(*q));
  int rc = configure(cfg, batch, who, &q->t, lp);
  if (rc == DDD_OK) rc = check_time_steps(T, who);
  if (rc) return rc;
  q->T = T;
  q->HT = q->t.H + T;
  lay_out_slab(q->t, lp, (size_t)q->t.n_weights + 2 * q->HT, 2 * T, T, &q->st_off, &q->gi_off);
  return plan_lds(q->t, lp, 2, who);
}

// ddd_train_rollout_loss_grad (ddd_train_rollout_run passes its own name), laid out for
// save_every = 1 (the workspace function does not know it): T step sums behind the gradient,
// up to T saved-step cotangents.  The LDS plan is the unrolled kernel's.
inline int plan_rollout(const ddd_config* cfg, int batch, int T, RolloutParams* q,
                        LaunchPlan* lp, const char* who = "ddd_train_rollout_loss_grad") {
  std::memset(q, 0, sizeof(*q));
  int rc = configure(cfg, batch, who, &q->t, lp);
  if (rc) return rc;
  if (T < 1 || T > DDD_MAX_ROLLOUT_STEPS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "%s: num_steps = %d out of range [1, %d]", who, T,
                DDD_MAX_ROLLOUT_STEPS);
  q->T = T;
  lay_out_slab(q->t, lp, (size_t)q->t.n_weights + T, 2 * T, T, &q->st_off, &q->gi_off);
  return plan_lds(q->t, lp, 2, who);
}

inline int check_tangents(int M, const char* who) {
  if (M < 1 || M > DDD_MAX_TANGENTS)
    return fail(DDD_ERR_INVALID_ARGUMENT, "%s: tangents = %d out of range [1, %d]", who, M,
                DDD_MAX_TANGENTS);
  return DDD_OK;
}

// ddd_result_jvp: no sums in front; behind the pre-activations the C_out rows of the saved
// net output.  The tangents are walked one by one through rows the training plan already
// has, so the LDS plan is training's whatever M is.
inline int plan_jvp(const ddd_config* cfg, int batch, int M, JvpParams* q, LaunchPlan* lp,
                    const char* who = "ddd_result_jvp") {
  std::memset(q, 0, sizeof(*q));
  int rc = configure(cfg, batch, who, &q->t, lp);
  if (rc == DDD_OK) rc = check_tangents(M, who);
  if (rc) return rc;
  q->M = M;
  lay_out_slab(q->t, lp, 0, q->t.C_out, 0, &q->net_off, nullptr);
  return plan_lds(q->t, lp, 0, who);
}

// ddd_tangent_rollout: behind the saved net output the tangents [M][N] and the midpoint's
// [M][N]; the state lives in LDS.
inline int plan_tangent_rollout(const ddd_config* cfg, int batch, int M, TangentRolloutParams* q,
                                LaunchPlan* lp, const char* who = "ddd_tangent_rollout") {
  std::memset(q, 0, sizeof(*q));
  int rc = configure(cfg, batch, who, &q->t, lp);
  if (rc == DDD_OK) rc = check_tangents(M, who);
  if (rc) return rc;
  q->M = M;
  lay_out_slab(q->t, lp, 0, q->t.C_out + 2 * M, 0, &q->net_off, nullptr);
  q->tan_off = q->net_off + q->t.C_out * q->t.N;
  return plan_lds(q->t, lp, 0, who);
}

// ddd_train_population_run, and ddd_train_run ("training run") as the population of one:
// plan_training into r->q.t for T = 0 (r->q.T = 0), plan_unrolled otherwise; behind the R
// replicas' slabs their R coefficient tables.
inline int plan_population(const ddd_config* cfg, int batch, int T, int replicas, RunParams* r,
                           LaunchPlan* lp, const char* who = "training population") {
  std::memset(r, 0, sizeof(*r));
  int rc = T < 0    ? fail(DDD_ERR_INVALID_ARGUMENT, "num_time_steps = %d (>= 0)", T)
           : T == 0 ? plan_training(cfg, batch, &r->q.t, lp, who)
                    : plan_unrolled(cfg, batch, T, &r->q, lp, who);
  if (T == 0) r->q.HT = r->q.t.H;
  if (rc == DDD_OK) rc = check_replicas(replicas);
  if (rc) return rc;
  r->blocks = lp->blocks;
  r->lds_bytes = lp->lds_bytes;
  r->heads = r->q.HT;
  lp->tables = (size_t)replicas * lp->ws_bytes;   // (a multiple of 16 bytes)
  lp->ws_bytes = lp->tables + (size_t)replicas * kCoefTableBytes;
  return DDD_OK;
}

// ddd_eval_metrics: exactly the configurations training admits, with its workgroups and, by
// T, its LDS plan or the unrolled kernel's; the slab is this kernel's (train_metrics.h:
// sums, counts and flag; the pre-activations; the stage states; no cotangents).
inline int plan_metrics(const ddd_config* cfg, int rows_evaluated, int T, int replicas,
                        MetricsParams* m, LaunchPlan* lp) {
  const char* who = "evaluation metrics";
  std::memset(m, 0, sizeof(*m));
  UnrolledParams& q = m->q;
  if (T < 0) return fail(DDD_ERR_INVALID_ARGUMENT, "num_time_steps = %d (>= 0)", T);
  int rc = configure(cfg, rows_evaluated, who, &q.t, lp);
  if (rc == DDD_OK && T > 0) rc = check_time_steps(T, who);
  if (rc == DDD_OK) rc = check_replicas(replicas);
  if (rc) return rc;
  q.T = T;
  q.HT = q.t.H + T;
  lay_out_slab(q.t, lp, (size_t)metrics_slab_floats(q.HT), 2 * T, 0, &q.st_off, nullptr);
  lp->ws_bytes *= (size_t)replicas;
  m->replicas = replicas;
  m->blocks = lp->blocks;
  rc = plan_lds(q.t, lp, T > 0 ? 2 : 0, who);
  m->lds_bytes = lp->lds_bytes;
  return rc;
}

// ddd_train_rollout_run: behind the R replicas' slabs the gradients [R][n_weights], the
// partial sums of g^2 and the decision records [R] (train_rollout_population.h)
inline int plan_rollout_run(const ddd_config* cfg, int batch, int T, int replicas,
                            RolloutRunParams* rr, LaunchPlan* lp) {
  std::memset(rr, 0, sizeof(*rr));
  int rc = plan_rollout(cfg, batch, T, &rr->q, lp, "ddd_train_rollout_run");
  if (rc == DDD_OK) rc = check_replicas(replicas);
  if (rc) return rc;
  rr->blocks = lp->blocks;
  rr->lds_bytes = lp->lds_bytes;
  const size_t R = (size_t)replicas;
  const int n_weights = rr->q.t.n_weights;
  lp->grad_buf = R * lp->ws_bytes;
  lp->partials = lp->grad_buf + ((R * n_weights * sizeof(float) + 15) & ~(size_t)15);
  lp->ws_bytes = lp->grad_buf + rollout_run_tail_bytes(n_weights, T, replicas);
  lp->decisions = lp->ws_bytes - R * sizeof(RolloutDecision);
  return DDD_OK;
}

}  // namespace train
}  // namespace ddd
