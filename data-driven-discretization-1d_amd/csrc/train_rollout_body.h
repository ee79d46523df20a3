// The body of the rollout-error training kernel (train_rollout.h; the scheme is written
// out at the top of train_rollout.hip): unrolled_loss_grad_body (train_unrolled_body.h)
// with the forcing added to every time derivative, the loss at saved steps only and its
// constants read from the device.  The update expressions (u + half_dt k1, y_s + dt k2),
// the cotangent ((2 (y - target)) c) / (batch N) and the order of the slab additions are
// that body's, so that an unforced call with save_every = 1 repeats its integrated heads
// bit for bit.  A workgroup is blockIdx.x of gridDim.x.  Shared by rollout_loss_grad_kernel
// (train_rollout.hip) and the replica form of the optimiser loop
// (train_rollout_population.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "train_device.h"
#include "train_rollout.h"

namespace ddd {
namespace train {

// The forcing of row `row` at grid point pos and time t: dev_params.h's forcing_at over
// the call's device tables.  A mode whose k_index is outside [0, n_k) reads nothing and
// makes the sum NaN.
__device__ __forceinline__ float rollout_forcing(const RolloutParams& q, int row, int pos,
                                                 float t) {
  const size_t base = (size_t)row * q.P;
  float total = 0.0f;
  for (int m = 0; m < q.P; ++m) {
    const int kidx = q.k_index[base + m];
    if (kidx < 0 || kidx >= q.n_k) return __int_as_float(0x7fc00000);
    const float sp = q.spatial_phase[(size_t)kidx * q.t.N + pos];
    const float phase =
        __fadd_rn(__fadd_rn(__fmul_rn(q.omega[base + m], t), sp), q.phase[base + m]);
    total = __fadd_rn(total, __fmul_rn(q.amplitude[base + m], sinf(phase)));
  }
  return total;
}

// kReplicas: workgroup (blockIdx.x, blockIdx.y) is workgroup blockIdx.x of replica blockIdx.y
// (weights_of, train_device.h)
template <bool kReplicas = false>
__device__ __forceinline__ void rollout_loss_grad_body(const RolloutParams& q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const int T = q.T, E = 2 * T;   // E evaluations: 2 s at y_s, 2 s + 1 at y_mid_s
  const int every = q.save_every, n_saved = q.n_saved;
  const Rows r = carve_rows(p, smem, true);
  float* slab = kReplicas
                    ? p.ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * p.slab_stride
                    : p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* st = slab + q.st_off;   // [E][N] stage states
  float* gi = slab + q.gi_off;   // [n_saved][N] loss cotangents of the saved steps
  float* sums = slab + p.n_weights;   // [n_saved] sums of the squared errors
  const float inv_count = 1.0f / ((float)p.batch * (float)n);
  const float dt = q.dt, half_dt = 0.5f * q.dt;

  stage_workgroup<kReplicas>(p, slab, p.n_slab, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const int* index =
        kReplicas ? p.sample_index + (size_t)blockIdx.y * p.index_stride : p.sample_index;
    const int row = p.sample_index != nullptr ? index[s] : s;
    const size_t yoff = (size_t)s * n_saved * n;
    if (row < 0 || row >= p.rows) {
      // an index outside [0, rows): no input read, the call's step means and this sample's
      // trajectory rows become NaN
      const float nan = __int_as_float(0x7fc00000);
      if (tid < n_saved) sums[tid] = nan;
      if (kReplicas)   // ... and, for the update, the replica's gradient (ddd1d.h)
        for (int i = tid; i < p.n_weights; i += kThreads) slab[i] = nan;
      if (q.trajectory != nullptr)
        for (int i = tid; i < n_saved * n; i += kThreads) q.trajectory[yoff + i] = nan;
      continue;   // (block-uniform)
    }
    const size_t toff = (size_t)row * n_saved * n;
    const double t_start = q.t0 != nullptr ? q.t0[row] : 0.0;
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
      // the evaluation's time: float64 on the clock of the window, rounded once
      const double t64 = t_start + (double)step * q.dt64 + (mid ? 0.5 * q.dt64 : 0.0);
      const float t = (float)t64;
      if (!mid) {
        if (!back)
          for (int x = tid; x < n; x += kThreads) {
            float k1 = r.pred[(size_t)x * H + D];
            if (q.forced) k1 = k1 + rollout_forcing(q, row, x, t);
            st[(size_t)(e + 1) * n + x] = r.u[x] + half_dt * k1;
          }
      } else if (!back || e == E - 1) {
        // ---- y_{step + 1} = y_step + dt k2: the next stage state and, at a saved step,
        // its squared error, cotangent and trajectory row
        const bool saved = (step + 1) % every == 0;
        const int j = (step + 1) / every - 1;
        const float c = saved ? q.step_weights[j] : 0.0f;
        for (int x = tid; x < n; x += kThreads) {
          float k2 = r.pred[(size_t)x * H + D];
          if (q.forced) k2 = k2 + rollout_forcing(q, row, x, t);
          const float y_new = st[(size_t)(e - 1) * n + x] + dt * k2;
          if (step + 1 < T) st[(size_t)(e + 1) * n + x] = y_new;
          if (saved) {
            const float target = q.targets[toff + (size_t)j * n + x];
            const float diff = target - y_new;
            r.gdy[x] = diff * diff;
            gi[(size_t)j * n + x] = ((2.0f * (y_new - target)) * c) * inv_count;
            if (q.trajectory != nullptr) q.trajectory[yoff + (size_t)j * n + x] = y_new;
          }
        }
        if (saved) {   // (block-uniform)
          __syncthreads();
          if (tid == 0) {   // the sum over the sample's points, in point order
            float acc = 0.0f;
            for (int x = 0; x < n; ++x) acc += r.gdy[x];
            sums[j] += acc;
          }
        }
      }
      __syncthreads();
      if (!back) continue;
      if (!p.want_grad) break;   // (block-uniform; forward and loss only)
      // ---- the cotangent of this evaluation's predictions: the time derivative only
      for (int x = tid; x < n; x += kThreads) {
        if (e == E - 1) r.lam[x] = gi[(size_t)(n_saved - 1) * n + x];
        const float c = mid ? dt * r.lam[x] : half_dt * r.gmid[x];
        for (int h = 0; h < H; ++h) r.gp[(size_t)x * H + h] = h == D ? c : 0.0f;
      }
      __syncthreads();
      // g_mid to its own row; g_s to gdy (free once the product has read it); lam_0 is
      // not an output, so the last product skips the state gradient
      evaluation_vjp<true, kReplicas>(p, r, zs, cur, nxt, slab, true,
                                      mid ? r.gmid : (e > 0 ? r.gdy : nullptr));
      if (!mid && e > 0) {
        const bool saved = step % every == 0;   // y_step carries a loss term
        const int j = step / every - 1;
        for (int x = tid; x < n; x += kThreads) {
          float lam = (r.lam[x] + r.gmid[x]) + r.gdy[x];
          if (saved) lam = lam + gi[(size_t)j * n + x];
          r.lam[x] = lam;
        }
        __syncthreads();
      }
    }
  }
}
}  // namespace train
}  // namespace ddd
