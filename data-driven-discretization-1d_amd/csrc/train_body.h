// The body of the fused loss-and-gradient kernel (train.h), shared by loss_grad_kernel
// (train.hip) and the replica forms of the optimiser loop (train_population.hip).  A
// workgroup is blockIdx.x of gridDim.x; whatever else a kernel's grid has is the caller's.
#pragma once
#include <hip/hip_runtime.h>

#include "train_device.h"

namespace ddd {
namespace train {

// kCoefTable: the loss constants from p.coef_table (head_terms_of, train_device.h)
// kReplicas: workgroup (blockIdx.x, blockIdx.y) is workgroup blockIdx.x of replica blockIdx.y
// (weights_of, train_device.h)
template <bool kCoefTable, bool kReplicas = false>
__device__ __forceinline__ void loss_grad_body(const TrainParams& p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, n = p.N, H = p.H;
  const Rows r = carve_rows(p, smem, false);
  float* em = r.gsd;   // the error terms, until evaluation_vjp takes the rows over
  float* er = r.gu;
  float* slab = kReplicas
                    ? p.ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * p.slab_stride
                    : p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  const float inv_count = 1.0f / ((float)p.batch * (float)n);

  stage_workgroup<kReplicas>(p, slab, p.n_slab, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const int* index =
        kReplicas ? p.sample_index + (size_t)blockIdx.y * p.index_stride : p.sample_index;
    const int row = p.sample_index != nullptr ? index[s] : s;
    if (row < 0 || row >= p.rows) {
      // an index outside [0, rows): no input read, the call's head means and this sample's
      // predictions row become NaN
      const float nan = __int_as_float(0x7fc00000);
      if (tid < 2 * H) slab[p.n_weights + tid] = nan;
      if (kReplicas)   // ... and, for the update, the replica's gradient (ddd1d.h)
        for (int i = tid; i < p.n_weights; i += kThreads) slab[i] = nan;
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
    forward_sample<kReplicas>(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
    // ---- loss terms and their cotangent (abs_and_rel_error, loss_per_head, weighted_loss)
    const size_t loff = (size_t)row * n * H;
    for (int i = tid; i < n * H; i += kThreads) {
      const int h = i % H;
      const float pv = r.pred[i];
      const HeadTerms t = head_terms_of<kCoefTable, kReplicas>(
          p, p.floor, p.coef_abs, p.coef_rel, H, h, pv, p.labels[loff + i], p.baseline[loff + i],
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
    evaluation_vjp<false, kReplicas>(p, r, zs, cur, nxt, slab, true, nullptr);
  }
}
}  // namespace train
}  // namespace ddd
