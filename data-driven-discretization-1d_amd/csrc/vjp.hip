// The vector-Jacobian product of one learned-stencil model evaluation (train.h:
// VjpParams), launched by ddd_result_vjp (capi.hip).  Per sample: the forward pass, the
// caller's cotangent into the LDS row of the predictions' cotangent, and the backward
// pass down to the weights and to the state, all three train_device.h's (forward_sample,
// evaluation_vjp).  Forward only without a cotangent.
#include <hip/hip_runtime.h>

#include "train_device.h"

namespace ddd {
namespace train {

__global__ __launch_bounds__(kThreads) void vjp_kernel(VjpParams q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H;
  const Rows r = carve_rows(p, smem, false);
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  const bool want_w = p.want_grad != 0;

  // (no head sums here: only the weight gradient's part of the slab, and only when asked)
  stage_workgroup(p, slab, want_w ? p.n_weights : 0, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const size_t yoff = (size_t)s * n, poff = (size_t)s * n * H;
    for (int i = tid; i < n; i += kThreads) {
      const float v = p.y[yoff + i];
      r.u[i] = v;
      r.buf0[i] = v / p.stddev;
    }
    __syncthreads();
    float* cur = r.buf0;
    float* nxt = r.buf1;
    forward_sample(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
    if (p.predictions != nullptr)
      for (int i = tid; i < n * H; i += kThreads) p.predictions[poff + i] = r.pred[i];
    if (q.cotangent == nullptr) continue;   // (block-uniform; the next write to pred or
                                            // u is behind a barrier)
    for (int i = tid; i < n * H; i += kThreads) r.gp[i] = q.cotangent[poff + i];
    __syncthreads();
    evaluation_vjp<true>(p, r, zs, cur, nxt, slab, want_w,
                   q.grad_y != nullptr ? q.grad_y + yoff : nullptr);
  }
}

hipError_t launch_vjp(const VjpParams& q, int blocks, size_t lds_bytes, hipStream_t stream) {
  // the slab sum over the weight gradient only, and only when it is wanted
  return launch_then_sum(reinterpret_cast<const void*>(vjp_kernel), &q, q.t, blocks, lds_bytes,
                         stream, 0, q.t.want_grad ? q.t.n_weights : 0);
}

}  // namespace train
}  // namespace ddd
