// The training kernel through time (train_unrolled.h), launched by
// ddd_train_unrolled_loss_grad (capi.hip).  Per sample, with f the time-derivative head
// of one evaluation (the equation of motion, no forcing) and dt the time step:
//   forward   y_0 = the input row; for s = 0 .. T-1:
//               k1 = f(y_s), y_mid = y_s + (dt / 2) k1, k2 = f(y_mid), y_{s+1} = y_s + dt k2
//             (the evaluation at y_0 also gives the D + 1 heads of training)
//   loss      coef_abs[h] mean_abs[h] + coef_rel[h] mean_rel[h] over the D + 1 + T heads
//   backward  lam = the loss cotangent of head y(t_T); for s = T-1 .. 0:
//               g_mid = J_f(y_mid)^T (dt lam), g_s = J_f(y_s)^T ((dt / 2) g_mid)
//               (at s = 0 the cotangents of the D + 1 heads ride in the same product),
//               lam = lam + g_mid + g_s + the loss cotangent of head y(t_s) (s >= 1)
//             every product adds its weight gradient to the workgroup's slab.
// The forward pass of an evaluation, its vector-Jacobian product, the loss terms and the
// LDS plan are train_device.h's (forward_sample, evaluation_vjp, head_terms, Rows).
#include <hip/hip_runtime.h>

#include "train_device.h"
#include "train_unrolled.h"
#include "train_unrolled_body.h"

namespace ddd {
namespace train {

__global__ __launch_bounds__(kThreads) void unrolled_loss_grad_kernel(UnrolledParams q) {
  unrolled_loss_grad_body<false>(q);
}

hipError_t launch_unrolled_loss_grad(const UnrolledParams& q, int blocks, size_t lds_bytes,
                                     hipStream_t stream) {
  const TrainParams& p = q.t;
  return launch_then_sum(reinterpret_cast<const void*>(unrolled_loss_grad_kernel), &q, p, blocks,
                         lds_bytes, stream, p.want_grad ? 0 : p.n_weights,
                         p.n_weights + 2 * q.HT);
}

}  // namespace train
}  // namespace ddd
