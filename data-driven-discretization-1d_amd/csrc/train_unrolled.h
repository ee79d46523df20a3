// Training through time: the loss of model.py:704-810 over the D + 1 heads of one
// evaluation AND the T heads of the model's own midpoint trajectory (predict_time_evolution,
// model.py:643-661), and its gradient with respect to the conv weights, for one minibatch
// in one kernel (ddd_train_unrolled_loss_grad, include/ddd1d.h).  The kernel is in
// train_unrolled.hip; each evaluation's forward and backward pass is train_device.h's.
//
// Per sample a workgroup runs the 2 T evaluations of the unroll forward, keeping the 2 T
// stage states y_0, y_mid_0, y_1, ... in its scratch slab (global memory, L2-resident),
// then walks them backwards: each evaluation's forward pass is recomputed (its
// pre-activations are not kept: 2 T copies of them per workgroup would not stay in L2)
// and its vector-Jacobian product adds to the workgroup's partial weight-gradient slab
// and to the adjoint of the state.  The last evaluation of the forward sweep is the first
// of the backward sweep and runs once: 4 T - 1 forward passes and 2 T backward passes.
// Workgroups, slabs and the fixed-order slab sum are those of train.h: no atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "train.h"

namespace ddd {
namespace train {

constexpr int kMaxTimeSteps = 8;   // DDD_MAX_TIME_STEPS
constexpr int kMaxUnrolledHeads = kMaxHeads + kMaxTimeSteps;

struct UnrolledParams {
  // The configuration, weights, y / sample_index / rows / batch, ws, want_grad / grad of
  // training.  t.H = D + 1 is the row length of one evaluation's predictions in LDS;
  // labels, baseline, predictions and head_means have HT channels.  t.n_slab and
  // t.slab_stride are this kernel's (below); t.floor / t.coef_* are not used.
  TrainParams t;
  int T;           // time steps
  int HT;          // D + 1 + T heads: result_stack order, then y(t_1) .. y(t_T)
  float dt;        // the equation's time_step
  int st_off;      // floats from a workgroup's slab to its stage states [2 T][N]
  int gi_off;      // ... to the loss cotangents of the integrated heads [T][N]
  float floor[kMaxUnrolledHeads], coef_abs[kMaxUnrolledHeads], coef_rel[kMaxUnrolledHeads];
};

// the LDS plan of training plus two rows behind the staged kernels (Rows::lam, gmid):
// the adjoint of the state and the state gradient of the midpoint evaluation
__host__ __device__ inline size_t unrolled_lds_floats(const TrainParams& p) {
  return lds_total_floats(p) + 2 * (size_t)p.N;
}

// unrolled_loss_grad_kernel on `blocks` workgroups, then the slab sum
hipError_t launch_unrolled_loss_grad(const UnrolledParams& q, int blocks, size_t lds_bytes,
                                     hipStream_t stream);

}  // namespace train
}  // namespace ddd
