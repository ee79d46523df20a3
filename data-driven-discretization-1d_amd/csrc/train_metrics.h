// Evaluation on the device (ddd_eval_metrics, include/ddd1d.h): the sums behind the
// reference's calculate_metrics (training.py:433-491) and behind the loss, for R replicas
// over a whole dataset, in two launches whatever R is.  The kernels are in
// train_metrics.hip.
//
// metrics_kernel is forward only, on a grid (blocks, R) with blocks = min(rows evaluated,
// kMaxBlocks): workgroup (b, r) is workgroup b of replica r (weights_of, train_device.h),
// walks samples b, b + blocks, ... and per sample runs forward_sample (T = 0) or the forward
// sweep of train_unrolled_body.h (evaluations 0 .. 2 T - 1 of the midpoint rule, head
// D + 1 + step from y_new).  Per (point, head), with prediction p, label l and baseline b:
//   term 0, 1  abs_error, rel_error of head_terms (the loss)
//   term 2, 3  |l - p|, |l - b|
//   term 4, 5  (l - p)^2, (l - b)^2
//   term 6     log(max(|l - p|, 1e-8)) - log(max(|l - b|, 1e-8))
//   term 7     (l - p)^2 < (l - b)^2, the two squares formed separately; counted in int32
// Each term is summed per head over the sample's points, in point order, by one thread per
// (term, head), as the loss kernels sum their two, and added into the workgroup's own
// slab in sample order.  metrics_sum_kernel adds the slabs in workgroup order.  No atomics:
// equal inputs give equal bits, and the two loss rows are bit for bit the head_means of a
// forward-only ddd_train_loss_grad / ddd_train_unrolled_loss_grad call on the same rows.
//
// LDS: the plan of the loss kernels (carve_rows), unchanged, so exactly the configurations
// they admit fit.  The terms take the three [N][H] rows behind gp in three passes (3, 3 and
// 2 terms), y_new the row gdy.
//
// A workgroup's slab (floats): [7][H'] sums, [H'] int32 counts, one int32 flag (an index
// outside [0, rows) was met: the replica's sums are NaN, its counts -1), padded to four;
// then the hidden layers' pre-activations (forward_sample writes them) and, with T > 0,
// the stage states [2 T][N].  No gradient part.
#pragma once
#include <hip/hip_runtime.h>

#include "train_population.h"

namespace ddd {
namespace train {

constexpr int kMetricSums = 7;    // float rows of `sums`
constexpr int kMetricTerms = 8;   // ... and the indicator count

// floats of a slab's sums, counts and flag, padded
__host__ __device__ inline int metrics_slab_floats(int heads) {
  return (kMetricTerms * heads + 1 + 3) & ~3;
}

struct MetricsParams {
  // The configuration, weights [R][n_weights], y / labels / baseline / rows of training;
  // q.t.batch the rows evaluated, q.t.sample_index null, [batch] (q.t.index_stride = 0) or
  // [R][batch] (= batch); q.t.predictions [R][batch][N][H'] or null; q.T may be 0 (then
  // q.HT = q.t.H).  q.t.n_slab = metrics_slab_floats(q.HT), q.t.slab_stride and q.st_off are
  // this unit's; q.gi_off, grad, head_means and coef_table are not used.
  UnrolledParams q;
  int blocks;
  size_t lds_bytes;
  int replicas;
  float* sums;     // out [R][7][H']: rows 0, 1 means over batch N (head_means), 2 .. 6 sums
  int* below;      // out [R][H']
};

// Enqueues metrics_kernel and metrics_sum_kernel on `stream`; no synchronisation, no copy
// to the host, no graph capture.
hipError_t launch_eval_metrics(const MetricsParams& m, hipStream_t stream);

}  // namespace train
}  // namespace ddd
