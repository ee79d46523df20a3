// Rollout fine-tuning on the device (ddd_train_rollout_run, include/ddd1d.h): many
// optimiser steps on the rollout loss of train_rollout.h -- the loss kernel on the step's
// minibatch of windows, the fixed-order slab sum, the global-norm clip, the skip of a step
// whose gradient is not finite, and Adam -- for R models of one architecture on one set of
// windows, enqueued by one call that never waits for the device.  The solo run is the
// population of one.  The kernels are in train_rollout_population.hip.
//
// A step is four launches whatever R is:
//   1. the loss kernel on a grid (blocks, R), blocks = min(batch, kMaxBlocks): workgroup
//      (b, r) runs rollout_loss_grad_body (train_rollout_body.h, its kReplicas flag set) as
//      workgroup b of `blocks` on replica r's weights, slabs and minibatch row,
//        weights + r n_weights, ws + r blocks slab_stride, sample_index + r index_stride,
//      so a replica's slab partition, and with it every summation order, does not depend on
//      R or on r.  An index outside [0, rows) also fills that workgroup's gradient slab with
//      NaN, as train_unrolled_body.h's replica form does;
//   2. rollout_slab_sum_population_kernel (grid.y the replica): slab_sum_kernel's sum
//      (train.hip: one thread per slab index, the workgroups' slabs added in workgroup
//      order).  Below n_weights the sum goes to the replica's row of the gradient buffer
//      (and of last_grad), behind it the step mean goes to the replica's row of the log.
//      Each workgroup also writes the sum of g^2 of its 256 indices, accumulated in float64
//      in a fixed order: butterflies within a wavefront, then the wavefronts in order;
//   3. rollout_decide_population_kernel, one workgroup per replica: the partials added in
//      index order in float64, norm = sqrt(sum), (float) norm to the log.  A norm that is
//      not finite as a float skips the step of this replica.  Otherwise
//        scale = min(1, clip_norm / (norm + 1e-12)) in double (1 without clipping),
//        t = ++adam_step[r],
//        step_size = (float)(lr / (1 - beta1^t)), bias2_sqrt = (float) sqrt(1 - beta2^t),
//      into the replica's decision record;
//   4. rollout_adam_population_kernel (grid.y the replica): returns at once for a skipped
//      replica -- weights, m and v keep their bits -- otherwise g' = g (float) scale and the
//      four statements of slab_adam_population_kernel (train_population.hip), in float32:
//        m += (g' - m) (1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
//        denom = sqrt(v) / bias2_sqrt + eps;  w -= step_size (m / denom)
//
// t lives on the device (adam_step, int32 [R], in / out): skips are decided there and are
// per replica, so the host cannot form the bias corrections by value as
// launch_train_population does.  The device's pow may differ from the host's by an ulp of
// double; every bit-for-bit statement about this entry point is between device runs.
//
// Forward only: the loss kernel without gradient and the head part of the slab sum; two
// launches.  No atomics anywhere; plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "train_population.h"
#include "train_rollout.h"

namespace ddd {
namespace train {

// What the decision kernel leaves for the Adam kernel, per replica
struct RolloutDecision {
  int skip;           // 1: the gradient's norm is not finite, nothing is updated
  float scale;        // the clip factor of the gradient
  float step_size;    // lr / (1 - beta1^t)
  float bias2_sqrt;   // sqrt(1 - beta2^t)
};

struct RolloutRunParams {
  // The loss kernel's parameters for replica 0: configuration, tables, data, t.weights,
  // t.ws (R times the slabs of one replica), save_every / n_saved / dt.  sample_index,
  // index_stride, want_grad, grad and head_means are set by the launcher.
  RolloutParams q;
  int blocks;
  size_t lds_bytes;
  int replicas;
  int index_per_replica;     // sample_index has a row per replica
  int forward_only;
  int num_opt_steps;         // K
  const double* learning_rate;   // host [R][K], or null (forward only)
  double beta1, beta2, epsilon, clip_norm;   // clip_norm 0: none
  const int* sample_index;   // device [K][batch] or [K][R][batch]; null: forward only, all rows
  float* weights;            // [R][n_weights] in / out, = q.t.weights
  float* adam_m;             // [R][n_weights] in / out
  float* adam_v;             // [R][n_weights] in / out
  int* adam_step;            // device [R] in / out: updates applied so far
  float* step_means_log;     // [K][R][n_saved]
  float* grad_norm_log;      // [K][R]: the norm before clipping
  float* last_grad;          // [R][n_weights] or null
  float* grad_buf;           // workspace: [R][n_weights]
  double* partials;          // workspace: [R][sum_blocks]
  RolloutDecision* decisions;    // workspace: [R]
};

// workgroups of the slab sum over the gradient and the step sums: one index per thread
__host__ __device__ inline int rollout_sum_blocks(int n_weights, int heads) {
  return (n_weights + heads + kThreads - 1) / kThreads;
}

// Bytes behind the R replicas' slabs: the gradient buffer, the partial sums of g^2 (laid
// out for save_every = 1: T step sums) and the decision records, each a multiple of 16
inline size_t rollout_run_tail_bytes(int n_weights, int T, int replicas) {
  const size_t R = (size_t)replicas;
  const size_t grads = (R * n_weights * sizeof(float) + 15) & ~(size_t)15;
  const size_t partials = (R * rollout_sum_blocks(n_weights, T) * sizeof(double) + 15) & ~(size_t)15;
  return grads + partials + R * sizeof(RolloutDecision);
}

static_assert(sizeof(RolloutDecision) == 16, "decision record");

// Enqueues the K optimiser steps (or the forward-only pass) of every replica on `stream`;
// no synchronisation, no copy to the host, no graph capture.
hipError_t launch_train_rollout_run(const RolloutRunParams& rr, hipStream_t stream);

}  // namespace train
}  // namespace ddd
