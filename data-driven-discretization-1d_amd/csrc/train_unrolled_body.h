// The body of the training kernel through time (train_unrolled.h; the scheme is written
// out at the top of train_unrolled.hip), shared by unrolled_loss_grad_kernel
// (train_unrolled.hip) and the replica forms of the optimiser loop
// (train_population.hip).  A workgroup is blockIdx.x of gridDim.x.
#pragma once
#include <hip/hip_runtime.h>

#include "train_device.h"
#include "train_unrolled.h"

namespace ddd {
namespace train {

// kCoefTable: the loss constants from q.t.coef_table (head_terms_of, train_device.h)
// kReplicas: workgroup (blockIdx.x, blockIdx.y) is workgroup blockIdx.x of replica blockIdx.y
// (weights_of, train_device.h)
template <bool kCoefTable, bool kReplicas = false>
__device__ __forceinline__ void unrolled_loss_grad_body(const UnrolledParams& q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const int T = q.T, HT = q.HT, E = 2 * T;   // E evaluations: 2 s at y_s, 2 s + 1 at y_mid_s
  const Rows r = carve_rows(p, smem, true);
  float* slab = kReplicas
                    ? p.ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * p.slab_stride
                    : p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* st = slab + q.st_off;   // [E][N] stage states
  float* gi = slab + q.gi_off;   // [T][N] loss cotangents of the integrated heads
  float* heads = slab + p.n_weights;   // [2][HT] sums of the error terms
  const float inv_count = 1.0f / ((float)p.batch * (float)n);
  const float dt = q.dt, half_dt = 0.5f * q.dt;

  stage_workgroup<kReplicas>(p, slab, p.n_slab, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const int* index =
        kReplicas ? p.sample_index + (size_t)blockIdx.y * p.index_stride : p.sample_index;
    const int row = p.sample_index != nullptr ? index[s] : s;
    const size_t poff = (size_t)s * n * HT;
    if (row < 0 || row >= p.rows) {
      // an index outside [0, rows): no input read, the call's head means and this sample's
      // predictions row become NaN
      const float nan = __int_as_float(0x7fc00000);
      if (tid < 2 * HT) heads[tid] = nan;
      if (kReplicas)   // ... and, for the update, the replica's gradient (ddd1d.h)
        for (int i = tid; i < p.n_weights; i += kThreads) slab[i] = nan;
      if (p.predictions != nullptr)
        for (int i = tid; i < n * HT; i += kThreads) p.predictions[poff + i] = nan;
      continue;   // (block-uniform)
    }
    const size_t loff = (size_t)row * n * HT;
    for (int i = tid; i < n; i += kThreads) st[i] = p.y[(size_t)row * n + i];
    __syncthreads();
    // phases 0 .. E - 2: the forward sweep over evaluations 0 .. E - 2; phases E - 1 ..
    // 2 E - 2: the backward sweep over evaluations E - 1 .. 0, each with its forward pass
    // recomputed (evaluation E - 1 runs only there)
    const int phases = p.want_grad ? 2 * E - 1 : E;
    for (int k = 0; k < phases; ++k) {
      const bool back = k >= E - 1;
      const int e = back ? 2 * E - 2 - k : k;
      const int step = e >> 1;
      const bool mid = (e & 1) != 0;
      for (int i = tid; i < n; i += kThreads) {
        const float v = st[(size_t)e * n + i];
        r.u[i] = v;
        r.buf0[i] = v / p.stddev;
      }
      __syncthreads();
      float* cur = r.buf0;
      float* nxt = r.buf1;
      forward_sample<kReplicas>(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
      if (!back && e == 0) {
        // ---- the D + 1 heads of training: error terms, their sums, the predictions
        float* em = r.gsd;
        float* er = r.gu;
        for (int i = tid; i < n * H; i += kThreads) {
          const int x = i / H, h = i - x * H;
          const size_t li = loff + (size_t)x * HT + h;
          const HeadTerms t = head_terms_of<kCoefTable, kReplicas>(
              p, q.floor, q.coef_abs, q.coef_rel, HT, h, r.pred[i], p.labels[li], p.baseline[li],
              inv_count);
          em[i] = t.abs_error;
          er[i] = t.rel_error;
          if (p.predictions != nullptr) p.predictions[poff + (size_t)x * HT + h] = r.pred[i];
        }
        __syncthreads();
        if (tid < 2 * H) {   // per-head sums over the sample's points, in point order
          const int h = tid % H;
          const float* err = tid < H ? em : er;
          float acc = 0.0f;
          for (int x = 0; x < n; ++x) acc += err[(size_t)x * H + h];
          heads[(tid < H ? 0 : HT) + h] += acc;
        }
      }
      if (!mid) {
        if (!back)
          for (int x = tid; x < n; x += kThreads)
            st[(size_t)(e + 1) * n + x] = r.u[x] + half_dt * r.pred[(size_t)x * H + D];
      } else if (!back || e == E - 1) {
        // ---- y_{step + 1} = y_step + dt k2: the next stage state and head D + 1 + step
        const int h = H + step;
        for (int x = tid; x < n; x += kThreads) {
          const float y_new = st[(size_t)(e - 1) * n + x] + dt * r.pred[(size_t)x * H + D];
          if (step + 1 < T) st[(size_t)(e + 1) * n + x] = y_new;
          const size_t li = loff + (size_t)x * HT + h;
          const HeadTerms t = head_terms_of<kCoefTable, kReplicas>(
              p, q.floor, q.coef_abs, q.coef_rel, HT, h, y_new, p.labels[li], p.baseline[li],
              inv_count);
          r.gdy[x] = t.abs_error;
          r.gfl[x] = t.rel_error;
          gi[(size_t)step * n + x] = t.cotangent;
          if (p.predictions != nullptr) p.predictions[poff + (size_t)x * HT + h] = y_new;
        }
        __syncthreads();
        if (tid < 2) {
          const float* err = tid == 0 ? r.gdy : r.gfl;
          float acc = 0.0f;
          for (int x = 0; x < n; ++x) acc += err[x];
          heads[tid * HT + h] += acc;
        }
      }
      __syncthreads();
      if (!back) continue;
      if (!p.want_grad) break;   // (block-uniform; forward and loss only)
      // ---- the cotangent of this evaluation's predictions
      for (int x = tid; x < n; x += kThreads) {
        if (e == E - 1) r.lam[x] = gi[(size_t)(T - 1) * n + x];
        const float c = mid ? dt * r.lam[x] : half_dt * r.gmid[x];
        for (int h = 0; h < H; ++h) {
          float g = h == D ? c : 0.0f;
          if (e == 0) {
            const size_t li = loff + (size_t)x * HT + h;
            g += head_terms_of<kCoefTable, kReplicas>(p, q.floor, q.coef_abs, q.coef_rel, HT, h,
                                           r.pred[(size_t)x * H + h], p.labels[li],
                                           p.baseline[li], inv_count).cotangent;
          }
          r.gp[(size_t)x * H + h] = g;
        }
      }
      __syncthreads();
      // g_mid to its own row; g_s to gdy (free once the product has read it); lam_0 is
      // not an output, so the last product skips the state gradient
      evaluation_vjp<true, kReplicas>(p, r, zs, cur, nxt, slab, true,
                     mid ? r.gmid : (e > 0 ? r.gdy : nullptr));
      if (!mid && e > 0) {
        for (int x = tid; x < n; x += kThreads)
          r.lam[x] = ((r.lam[x] + r.gmid[x]) + r.gdy[x]) + gi[(size_t)(step - 1) * n + x];
        __syncthreads();
      }
    }
  }
}
}  // namespace train
}  // namespace ddd
