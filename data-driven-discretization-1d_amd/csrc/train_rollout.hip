// The rollout-error training kernel (train_rollout.h), launched by
// ddd_train_rollout_loss_grad (capi.hip).  Per window, with f the time-derivative head of
// one evaluation plus the forcing of the window's row, t_s = t0 + s dt formed in float64
// and rounded to float32, and dt the step:
//   forward   y_0 = the window's start; for s = 0 .. T-1:
//               k1 = f(t_s, y_s), y_mid = y_s + (dt / 2) k1, k2 = f(t_s + dt / 2, y_mid),
//               y_{s+1} = y_s + dt k2
//   loss      sum_j c_j mean over (window, x) of (y_{(j+1) save_every} - target_j)^2
//   backward  lam = the loss cotangent of y_T; for s = T-1 .. 0:
//               g_mid = J_f(y_mid)^T (dt lam), g_s = J_f(y_s)^T ((dt / 2) g_mid),
//               lam = lam + g_mid + g_s + the loss cotangent of y_s (s >= 1, s saved)
//             every product adds its weight gradient to the workgroup's slab.
// The forcing enters neither Jacobian.  The forward pass of an evaluation, its
// vector-Jacobian product and the LDS plan are train_device.h's (forward_sample,
// evaluation_vjp, Rows).
#include <hip/hip_runtime.h>

#include "train_device.h"
#include "train_rollout.h"
#include "train_rollout_body.h"

namespace ddd {
namespace train {

__global__ __launch_bounds__(kThreads) void rollout_loss_grad_kernel(RolloutParams q) {
  rollout_loss_grad_body(q);
}

hipError_t launch_rollout_loss_grad(const RolloutParams& q, int blocks, size_t lds_bytes,
                                    hipStream_t stream) {
  const TrainParams& p = q.t;
  return launch_then_sum(reinterpret_cast<const void*>(rollout_loss_grad_kernel), &q, p, blocks,
                         lds_bytes, stream, p.want_grad ? 0 : p.n_weights,
                         p.n_weights + q.n_saved);
}

}  // namespace train
}  // namespace ddd
