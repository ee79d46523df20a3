// Training on rollout error: the mean squared error of the model's own forced midpoint
// trajectory against given targets at every save_every-th of T steps, weighted per saved
// step, and its gradient with respect to the conv weights, for one minibatch of windows in
// one kernel (ddd_train_rollout_loss_grad, include/ddd1d.h).  The kernel is in
// train_rollout.hip, its body in train_rollout_body.h; each evaluation's forward and
// backward pass is train_device.h's.
//
// The sweep is train_unrolled.h's, generalised: per window a workgroup runs the 2 T
// evaluations forward, keeping all 2 T stage states y_0, y_mid_0, y_1, ... in its scratch
// slab (global memory: 2 T N floats per workgroup, 512 KiB at T = 256, N = 256; nothing is
// recomputed but each evaluation's forward pass), then walks them backwards with the
// adjoint of the midpoint rule.  What differs:
//   - the right-hand side is forward_sample's time derivative PLUS the forcing of the
//     window's row at the evaluation's time (Burgers family only; dev_params.h forcing_at's
//     arithmetic over device tables with one row per row of y0).  The forcing depends on
//     neither the state nor the weights, so the adjoint is unchanged;
//   - the loss has no D + 1 heads of one evaluation and no relative term: cotangents enter
//     at saved steps only, 2 c_j (y - target) / (batch N);
//   - the loss constants c_j are a device array and the saved-step cotangents
//     [T / save_every][N] sit next to the stage states, so nothing per step rides in the
//     kernel arguments: T goes to kMaxRolloutSteps, not train_unrolled.h's 8.
// Workgroups, slabs and the fixed-order slab sum are those of train.h: no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "train.h"
#include "train_unrolled.h"

namespace ddd {
namespace train {

constexpr int kMaxRolloutSteps = 256;   // DDD_MAX_ROLLOUT_STEPS

struct RolloutParams {
  // The configuration, weights, y (= y0) / sample_index / rows / batch, ws, want_grad /
  // grad of training; t.head_means = step_means [n_saved].  t.n_slab and t.slab_stride are
  // this kernel's (below); labels, baseline, predictions, floor / coef_* are not used.
  TrainParams t;
  int T;            // time steps
  int save_every;   // a divisor of T
  int n_saved;      // T / save_every
  float dt;         // (float) dt64: the step of the state update
  double dt64;      // the step of the forcing's clock
  int st_off;       // floats from a workgroup's slab to its stage states [2 T][N]
  int gi_off;       // ... to the loss cotangents of the saved steps [n_saved][N]
  const float* targets;       // [rows][n_saved][N]
  const float* step_weights;  // [n_saved]
  const double* t0;           // [rows] or null (0)
  int forced;       // 1: the tables below are given and the equation applies forcing
  int P, n_k;       // modes per row, rows of spatial_phase
  const float* amplitude;     // [rows][P]
  const float* omega;         // [rows][P]
  const float* phase;         // [rows][P]
  const int* k_index;         // [rows][P]
  const float* spatial_phase; // [n_k][N]
  float* trajectory;          // [batch][n_saved][N] or null
};

// The LDS plan is that of training through time (train_unrolled.h: unrolled_lds_floats):
// the forcing is evaluated by the thread that adds it and needs no row of its own.

// rollout_loss_grad_kernel on `blocks` workgroups, then the slab sum
hipError_t launch_rollout_loss_grad(const RolloutParams& q, int blocks, size_t lds_bytes,
                                    hipStream_t stream);

}  // namespace train
}  // namespace ddd
