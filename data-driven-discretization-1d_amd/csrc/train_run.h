// The optimiser loop on the device (ddd_train_run, include/ddd1d.h): many steps of
// training.py's loop -- the loss kernel of train.h (or, with num_time_steps > 0, of
// train_unrolled.h) on the step's minibatch, the fixed-order slab sum and Adam -- enqueued
// by one call that never waits for the device.  The kernels are in train_run.hip.
//
// A step is the loss kernel and slab_adam_kernel: the slab sum of train.hip
// (slab_sum_kernel: one thread per slab index, the workgroups' slabs added in workgroup
// order) whose thread, below n_weights, goes on to apply Adam to its element of the
// weights in place, and behind n_weights writes the step's head means to row `step` of
// the caller's log.  The gradient that enters the update is therefore the one
// ddd_train_loss_grad / ddd_train_unrolled_loss_grad return for the same weights and
// minibatch, bit for bit.  The update is the single-tensor path of torch.optim.Adam (no
// weight decay, no amsgrad), in float32 and in its order:
//   m += (g - m) (1 - beta1)
//   v  = beta2 v + (1 - beta2) g^2
//   denom = sqrt(v) / sqrt(1 - beta2^t) + eps
//   w -= (lr / (1 - beta1^t)) m / denom
// with lr / (1 - beta1^t) and sqrt(1 - beta2^t) formed on the host in double for step t.
//
// With error_max > 0 a step is three pieces, the decision staying on the device: the loss
// kernel forward only and the slab sum of the head means (into the log row); clip_kernel
// (one workgroup), which writes the loss constants [3][heads] (floor, coef_abs, coef_rel)
// with the coefficient of every clipped term (mean * error_scale >= error_max) zeroed;
// the loss kernel's twin that reads that table (TrainParams::coef_table), then
// slab_adam_kernel.  The logged means are the unclipped ones.  No atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include "train_unrolled.h"

namespace ddd {
namespace train {

struct RunParams {
  // q.T == 0: q.t alone is the argument of loss_grad_kernel (its floor / coef_* filled);
  // otherwise q is unrolled_loss_grad_kernel's.  weights, ws, y / labels / baseline,
  // rows and batch are set; sample_index, want_grad, grad, head_means and coef_table are
  // set per step by the launcher.
  UnrolledParams q;
  int blocks;
  size_t lds_bytes;
  int heads;               // H (q.T == 0) or H'
  int first_step, num_steps;
  const double* learning_rate;   // host [num_steps]
  double beta1, beta2, epsilon;
  const int* sample_index; // device [num_steps][batch]
  float* weights;          // in / out, = q.t.weights
  float* adam_m;           // in / out
  float* adam_v;           // in / out
  float* head_means_log;   // [num_steps][2][heads]
  float* last_grad;        // [n_weights] or null
  double error_max;        // 0: no clipping
  double scale_abs[kMaxUnrolledHeads], scale_rel[kMaxUnrolledHeads];
  float floor[kMaxUnrolledHeads], coef_abs[kMaxUnrolledHeads], coef_rel[kMaxUnrolledHeads];
  float* coef_table;       // device [3][heads] (the tail of the workspace)
};

// bytes of the coefficient table behind the slabs in the workspace of ddd_train_run
constexpr size_t kCoefTableBytes = 256;
static_assert(3 * kMaxUnrolledHeads * sizeof(float) <= kCoefTableBytes, "coefficient table");

// Enqueues r.num_steps optimiser steps on `stream`; no synchronisation, no copy to the
// host, no graph capture.
hipError_t launch_train_run(const RunParams& r, hipStream_t stream);

}  // namespace train
}  // namespace ddd
