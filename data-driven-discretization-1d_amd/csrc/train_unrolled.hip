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

namespace ddd {
namespace train {

// kCoefTable: the loss constants from q.t.coef_table (head_terms_of, train_device.h)
template <bool kCoefTable>
__device__ __forceinline__ void unrolled_loss_grad_body(const UnrolledParams& q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const int T = q.T, HT = q.HT, E = 2 * T;   // E evaluations: 2 s at y_s, 2 s + 1 at y_mid_s
  const Rows r = carve_rows(p, smem, true);
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* st = slab + q.st_off;   // [E][N] stage states
  float* gi = slab + q.gi_off;   // [T][N] loss cotangents of the integrated heads
  float* heads = slab + p.n_weights;   // [2][HT] sums of the error terms
  const float inv_count = 1.0f / ((float)p.batch * (float)n);
  const float dt = q.dt, half_dt = 0.5f * q.dt;

  stage_workgroup(p, slab, p.n_slab, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const int row = p.sample_index != nullptr ? p.sample_index[s] : s;
    const size_t poff = (size_t)s * n * HT;
    if (row < 0 || row >= p.rows) {
      // an index outside [0, rows): no input read, the call's head means and this sample's
      // predictions row become NaN
      const float nan = __int_as_float(0x7fc00000);
      if (tid < 2 * HT) heads[tid] = nan;
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
      forward_sample(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
      if (!back && e == 0) {
        // ---- the D + 1 heads of training: error terms, their sums, the predictions
        float* em = r.gsd;
        float* er = r.gu;
        for (int i = tid; i < n * H; i += kThreads) {
          const int x = i / H, h = i - x * H;
          const size_t li = loff + (size_t)x * HT + h;
          const HeadTerms t = head_terms_of<kCoefTable>(p, q.floor, q.coef_abs, q.coef_rel, HT, h,
                                                        r.pred[i], p.labels[li], p.baseline[li],
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
          const HeadTerms t = head_terms_of<kCoefTable>(p, q.floor, q.coef_abs, q.coef_rel, HT, h,
                                                        y_new, p.labels[li], p.baseline[li],
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
            g += head_terms_of<kCoefTable>(p, q.floor, q.coef_abs, q.coef_rel, HT, h,
                                           r.pred[(size_t)x * H + h], p.labels[li],
                                           p.baseline[li], inv_count).cotangent;
          }
          r.gp[(size_t)x * H + h] = g;
        }
      }
      __syncthreads();
      // g_mid to its own row; g_s to gdy (free once the product has read it); lam_0 is
      // not an output, so the last product skips the state gradient
      evaluation_vjp<true>(p, r, zs, cur, nxt, slab, true,
                     mid ? r.gmid : (e > 0 ? r.gdy : nullptr));
      if (!mid && e > 0) {
        for (int x = tid; x < n; x += kThreads)
          r.lam[x] = ((r.lam[x] + r.gmid[x]) + r.gdy[x]) + gi[(size_t)(step - 1) * n + x];
        __syncthreads();
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void unrolled_loss_grad_kernel(UnrolledParams q) {
  unrolled_loss_grad_body<false>(q);
}

__global__ __launch_bounds__(kThreads) void unrolled_loss_grad_table_kernel(UnrolledParams q) {
  unrolled_loss_grad_body<true>(q);
}

hipError_t launch_unrolled_loss_grad(const UnrolledParams& q, int blocks, size_t lds_bytes,
                                     hipStream_t stream) {
  const TrainParams& p = q.t;
  return launch_then_sum(reinterpret_cast<const void*>(unrolled_loss_grad_kernel), &q, p, blocks,
                         lds_bytes, stream, p.want_grad ? 0 : p.n_weights,
                         p.n_weights + 2 * q.HT);
}

const void* unrolled_loss_grad_kernel_entry(bool coef_table) {
  return coef_table ? reinterpret_cast<const void*>(unrolled_loss_grad_table_kernel)
                    : reinterpret_cast<const void*>(unrolled_loss_grad_kernel);
}

}  // namespace train
}  // namespace ddd
