// Replica populations (ddd_train_population_run, include/ddd1d.h): R models of one
// architecture -- R weight vectors, R Adam states, R learning-rate rows and, optionally, R
// minibatch orders -- trained by the optimiser loop of train_run.h in one call, on one
// dataset.  The kernels are in train_population.hip.
//
// A step is still two launches whatever R is.  The loss kernel runs on a grid
// (blocks, R) with blocks = min(batch, kMaxBlocks), the solo run's: workgroup (b, r) runs
// the body of train_body.h / train_unrolled_body.h (their kReplicas flag set) as workgroup
// b of `blocks` on replica r's weights, slabs, minibatch and coefficient table,
//   weights + r n_weights, ws + r blocks slab_stride, sample_index + r index_stride,
//   coef_table + r 3 heads,
// so a replica's slab partition, and with it every summation order, is that of
// ddd_train_run given the replica's arguments.  slab_adam_population_kernel is
// slab_adam_kernel (train_run.hip) with blockIdx.y as the replica: the same sum, the same
// Adam arithmetic, sqrt(1 - beta2^t) shared (t is) and lr[r] / (1 - beta1^t) per replica,
// by value in the kernel arguments.  Replica r of a call is therefore bit for bit the
// solo call: weights, adam_m, adam_v, every log row and last_grad.
//
// With error_max > 0 the three pieces of train_run.h keep their shape: the forward-only
// pass and slab_heads_population_kernel (the head means to the log rows),
// clip_population_kernel (one workgroup per replica, each its own table from its own
// means), the kernels' twins that read the tables, then slab_adam_population_kernel.
// No atomics anywhere; plain vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>

#include "train_run.h"

namespace ddd {
namespace train {

constexpr int kMaxReplicas = 64;   // DDD_MAX_REPLICAS

struct PopulationParams {
  // r as launch_train_run takes it, with weights (= q.t.weights), adam_m, adam_v and
  // last_grad [R][n_weights]; q.t.ws R times the slabs of a solo run; coef_table R tables
  // [3][heads], one behind the other; learning_rate HOST [R][num_steps]; sample_index
  // device [num_steps][batch] or, with index_per_replica, [num_steps][R][batch];
  // head_means_log [num_steps][R][2][heads].
  RunParams r;
  int replicas;
  int index_per_replica;
};

// Enqueues r.num_steps optimiser steps of every replica on `stream`; no synchronisation,
// no copy to the host, no graph capture.
hipError_t launch_train_population(const PopulationParams& pp, hipStream_t stream);

}  // namespace train
}  // namespace ddd
