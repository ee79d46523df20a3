// The optimiser loop on the device (ddd_train_run and ddd_train_population_run,
// include/ddd1d.h): many steps of training.py's loop -- the loss kernel of train.h (or,
// with num_time_steps > 0, of train_unrolled.h) on the step's minibatch, the fixed-order
// slab sum and Adam -- for R models of one architecture on one dataset, enqueued by one
// call that never waits for the device.  R weight vectors, R Adam states, R learning-rate
// rows and, optionally, R minibatch orders; ddd_train_run is the population of one.  The
// kernels are in train_population.hip.
//
// A step is two launches whatever R is.  The loss kernel runs on a grid (blocks, R) with
// blocks = min(batch, kMaxBlocks): workgroup (b, r) runs the body of train_body.h /
// train_unrolled_body.h (their kReplicas flag set) as workgroup b of `blocks` on replica
// r's weights, slabs, minibatch and coefficient table,
//   weights + r n_weights, ws + r blocks slab_stride, sample_index + r index_stride,
//   coef_table + r 3 heads,
// so a replica's slab partition, and with it every summation order, does not depend on R
// or on r.  slab_adam_population_kernel (grid.y the replica again) is the slab sum of
// train.hip (slab_sum_kernel: one thread per slab index, the workgroups' slabs added in
// workgroup order) whose thread, below n_weights, goes on to apply Adam to its element of
// the replica's weights in place, and behind n_weights writes the step's head means to
// the replica's row of the caller's log.  The gradient that enters the update is therefore
// the one ddd_train_loss_grad / ddd_train_unrolled_loss_grad return for the same weights
// and minibatch, bit for bit, and replica r of a call is bit for bit the call with that
// replica alone: weights, adam_m, adam_v, every log row and last_grad.  The update is the
// single-tensor path of torch.optim.Adam (no weight decay, no amsgrad), in float32 and in
// its order:
//   m += (g - m) (1 - beta1)
//   v  = beta2 v + (1 - beta2) g^2
//   denom = sqrt(v) / sqrt(1 - beta2^t) + eps
//   w -= (lr / (1 - beta1^t)) m / denom
// with lr[r] / (1 - beta1^t) (per replica, by value in the kernel arguments) and
// sqrt(1 - beta2^t) (shared: t is) formed on the host in double for step t.
//
// With error_max > 0 a step is three pieces, the decision staying on the device: the loss
// kernel forward only and slab_heads_population_kernel (the head means into the log
// rows); clip_population_kernel (one workgroup per replica, each its own table from its
// own means), which writes the loss constants [3][heads] (floor, coef_abs, coef_rel) with
// the coefficient of every clipped term (mean * error_scale >= error_max) zeroed; the
// loss kernel's twin that reads that table (TrainParams::coef_table), then
// slab_adam_population_kernel.  The logged means are the unclipped ones.  No atomics
// anywhere; plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "train_unrolled.h"

namespace ddd {
namespace train {

constexpr int kMaxReplicas = 64;   // DDD_MAX_REPLICAS

struct RunParams {
  // q.T == 0: q.t alone is the argument of the loss kernel (its floor / coef_* filled);
  // otherwise q is the through-time kernel's.  weights, ws, y / labels / baseline, rows and
  // batch are set; sample_index, index_stride, want_grad, grad, head_means and coef_table
  // are set per step by the launcher.
  UnrolledParams q;
  int blocks;
  size_t lds_bytes;
  int heads;               // H (q.T == 0) or H'
  int first_step, num_steps;
  const double* learning_rate;   // host [R][num_steps]
  double beta1, beta2, epsilon;
  const int* sample_index; // device [num_steps][batch] or [num_steps][R][batch]
  float* weights;          // [R][n_weights] in / out, = q.t.weights
  float* adam_m;           // [R][n_weights] in / out
  float* adam_v;           // [R][n_weights] in / out
  float* head_means_log;   // [num_steps][R][2][heads]
  float* last_grad;        // [R][n_weights] or null
  double error_max;        // 0: no clipping
  double scale_abs[kMaxUnrolledHeads], scale_rel[kMaxUnrolledHeads];
  float floor[kMaxUnrolledHeads], coef_abs[kMaxUnrolledHeads], coef_rel[kMaxUnrolledHeads];
  float* coef_table;       // device [R][3][heads] (the tail of the workspace)
};

// bytes per replica that the workspace holds, behind all the slabs, for coef_table
constexpr size_t kCoefTableBytes = 256;
static_assert(3 * kMaxUnrolledHeads * sizeof(float) <= kCoefTableBytes, "coefficient table");

struct PopulationParams {
  // q.t.ws R times the slabs of one replica, one behind the other
  RunParams r;
  int replicas;
  int index_per_replica;   // sample_index has a row per replica
};

// Enqueues r.num_steps optimiser steps of every replica on `stream`; no synchronisation,
// no copy to the host, no graph capture.
hipError_t launch_train_population(const PopulationParams& pp, hipStream_t stream);

}  // namespace train
}  // namespace ddd
