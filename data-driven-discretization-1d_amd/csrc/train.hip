// Training kernels (train.h): the fused loss-and-gradient kernel, launched by
// ddd_train_loss_grad (capi.hip), and the two pieces every kernel of train_device.h
// shares on the host side: the fixed-order sum of the workgroups' partial slabs and the
// launcher that runs a kernel and then that sum.
#include <hip/hip_runtime.h>

#include "train_device.h"

namespace ddd {
namespace train {

// kCoefTable: the loss constants from p.coef_table (head_terms_of, train_device.h)
template <bool kCoefTable>
__device__ __forceinline__ void loss_grad_body(const TrainParams& p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, n = p.N, H = p.H;
  const Rows r = carve_rows(p, smem, false);
  float* em = r.gsd;   // the error terms, until evaluation_vjp takes the rows over
  float* er = r.gu;
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  const float inv_count = 1.0f / ((float)p.batch * (float)n);

  stage_workgroup(p, slab, p.n_slab, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const int row = p.sample_index != nullptr ? p.sample_index[s] : s;
    if (row < 0 || row >= p.rows) {
      // an index outside [0, rows): no input read, the call's head means and this sample's
      // predictions row become NaN
      const float nan = __int_as_float(0x7fc00000);
      if (tid < 2 * H) slab[p.n_weights + tid] = nan;
      if (p.predictions != nullptr)
        for (int i = tid; i < n * H; i += kThreads) p.predictions[(size_t)s * n * H + i] = nan;
      continue;   // (block-uniform)
    }
    const size_t yoff = (size_t)row * n;
    for (int i = tid; i < n; i += kThreads) {
      const float v = p.y[yoff + i];
      r.u[i] = v;
      r.buf0[i] = v / p.stddev;
    }
    __syncthreads();
    float* cur = r.buf0;
    float* nxt = r.buf1;
    forward_sample(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
    // ---- loss terms and their cotangent (abs_and_rel_error, loss_per_head, weighted_loss)
    const size_t loff = (size_t)row * n * H;
    for (int i = tid; i < n * H; i += kThreads) {
      const int h = i % H;
      const float pv = r.pred[i];
      const HeadTerms t = head_terms_of<kCoefTable>(p, p.floor, p.coef_abs, p.coef_rel, H, h, pv,
                                                    p.labels[loff + i], p.baseline[loff + i],
                                                    inv_count);
      em[i] = t.abs_error;
      er[i] = t.rel_error;
      r.gp[i] = t.cotangent;
      if (p.predictions != nullptr) p.predictions[(size_t)s * n * H + i] = pv;
    }
    __syncthreads();
    if (tid < 2 * H) {   // per-head sums over the sample's points, in point order
      const int h = tid % H;
      const float* e = tid < H ? em : er;
      float acc = 0.0f;
      for (int x = 0; x < n; ++x) acc += e[(size_t)x * H + h];
      slab[p.n_weights + tid] += acc;
    }
    if (!p.want_grad) {
      __syncthreads();
      continue;
    }
    // No barrier here: the sums above are the last readers of em / er (Rows::gsd / gu).
    // <false> forms no state gradient, so evaluation_vjp leaves those rows alone; where it
    // does write them, that is behind its two barriers after gdy and gfl.
    evaluation_vjp<false>(p, r, zs, cur, nxt, slab, true, nullptr);
  }
}

__global__ __launch_bounds__(kThreads) void loss_grad_kernel(TrainParams p) {
  loss_grad_body<false>(p);
}

__global__ __launch_bounds__(kThreads) void loss_grad_table_kernel(TrainParams p) {
  loss_grad_body<true>(p);
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

hipError_t launch_prepared_then_sum(const void* kernel, const void* params, const TrainParams& p,
                                    int blocks, size_t lds_bytes, hipStream_t stream, int first,
                                    int total) {
  void* args[] = {const_cast<void*>(params)};
  hipError_t err = hipLaunchKernel(kernel, dim3(blocks), dim3(kThreads), args, lds_bytes, stream);
  if (err != hipSuccess || first >= total) return err;
  const int grid = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(slab_sum_kernel, dim3(grid), dim3(kThreads), 0, stream, p.ws, p.slab_stride,
                     blocks, first, p.n_weights, total, p.grad, p.head_means,
                     (float)p.batch * (float)p.N);
  return hipGetLastError();
}

hipError_t launch_then_sum(const void* kernel, const void* params, const TrainParams& p,
                           int blocks, size_t lds_bytes, hipStream_t stream, int first,
                           int total) {
  hipError_t err = set_dynamic_lds(kernel, lds_bytes);
  if (err != hipSuccess) return err;
  return launch_prepared_then_sum(kernel, params, p, blocks, lds_bytes, stream, first, total);
}

hipError_t launch_loss_grad(const TrainParams& p, int blocks, size_t lds_bytes, hipStream_t stream) {
  return launch_then_sum(reinterpret_cast<const void*>(loss_grad_kernel), &p, p, blocks, lds_bytes,
                         stream, p.want_grad ? 0 : p.n_weights, p.n_weights + 2 * p.H);
}

const void* loss_grad_kernel_entry(bool coef_table) {
  return coef_table ? reinterpret_cast<const void*>(loss_grad_table_kernel)
                    : reinterpret_cast<const void*>(loss_grad_kernel);
}

}  // namespace train
}  // namespace ddd
