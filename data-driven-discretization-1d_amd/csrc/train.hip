// Training kernels (train.h): the fused loss-and-gradient kernel (its body: train_body.h),
// launched by ddd_train_loss_grad (capi.hip), and the two pieces every kernel of train_device.h
// shares on the host side: the fixed-order sum of the workgroups' partial slabs and the
// launcher that runs a kernel and then that sum.
#include <hip/hip_runtime.h>

#include "train_body.h"
#include "train_device.h"

namespace ddd {
namespace train {

__global__ __launch_bounds__(kThreads) void loss_grad_kernel(TrainParams p) {
  loss_grad_body<false>(p);
}

// out[i] = sum over workgroups b (in order) of ws[b stride + i] for first <= i < total:
// grad below n_weights, behind it the head sums as means over `count` = batch N
__global__ __launch_bounds__(kThreads) void slab_sum_kernel(const float* ws, size_t stride,
                                                            int blocks, int first, int n_weights,
                                                            int total, float* grad,
                                                            float* head_means, float count) {
  for (int i = first + blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += ws[(size_t)b * stride + i];
    if (i < n_weights) grad[i] = acc;
    else head_means[i - n_weights] = acc / count;
  }
}

hipError_t set_dynamic_lds(const void* kernel, size_t lds_bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

hipError_t launch_then_sum(const void* kernel, const void* params, const TrainParams& p,
                           int blocks, size_t lds_bytes, hipStream_t stream, int first,
                           int total) {
  hipError_t err = set_dynamic_lds(kernel, lds_bytes);
  if (err != hipSuccess) return err;
  void* args[] = {const_cast<void*>(params)};
  err = hipLaunchKernel(kernel, dim3(blocks), dim3(kThreads), args, lds_bytes, stream);
  if (err != hipSuccess || first >= total) return err;
  const int grid = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(slab_sum_kernel, dim3(grid), dim3(kThreads), 0, stream, p.ws, p.slab_stride,
                     blocks, first, p.n_weights, total, p.grad, p.head_means,
                     (float)p.batch * (float)p.N);
  return hipGetLastError();
}

hipError_t launch_loss_grad(const TrainParams& p, int blocks, size_t lds_bytes, hipStream_t stream) {
  return launch_then_sum(reinterpret_cast<const void*>(loss_grad_kernel), &p, p, blocks, lds_bytes,
                         stream, p.want_grad ? 0 : p.n_weights, p.n_weights + 2 * p.H);
}

}  // namespace train
}  // namespace ddd
