// The tangent-linear kernels (train.h: JvpParams, TangentRolloutParams), launched by
// ddd_result_jvp and ddd_tangent_rollout (capi_train.hip).  Both are vjp_kernel's sample
// loop: min(batch, kMaxBlocks) workgroups, each walking over its samples with its own slab
// and LDS rows.  Per sample the primal forward pass runs once (forward_sample) and the M
// tangents are walked one by one through forward_sample_tangent (train_tangent.h).  Every
// output is per sample: no atomics, no cross-sample sum, equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include "train_tangent.h"

namespace ddd {
namespace train {

// The state of the next evaluation from u (already in r.u) into the tower's input
__device__ __forceinline__ void stage_tower_input(const TrainParams& p, const Rows& r) {
  for (int i = threadIdx.x; i < p.N; i += kThreads) r.buf0[i] = r.u[i] / p.stddev;
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void jvp_kernel(JvpParams q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, M = q.M;
  const Rows r = carve_rows(p, smem, false);
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* net = slab + q.net_off;

  stage_workgroup(p, slab, 0, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const size_t yoff = (size_t)s * n, poff = (size_t)s * n * H;
    for (int i = tid; i < n; i += kThreads) r.u[i] = p.y[yoff + i];
    __syncthreads();
    stage_tower_input(p, r);
    float* cur = r.buf0;
    float* nxt = r.buf1;
    forward_sample(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
    if (p.predictions != nullptr)
      for (int i = tid; i < n * H; i += kThreads) p.predictions[poff + i] = r.pred[i];
    save_net_output(p, cur, net);
    for (int j = 0; j < M; ++j) {
      const size_t row = (size_t)s * M + j;
      for (int i = tid; i < n; i += kThreads) {
        const float v = q.tangent_y != nullptr ? q.tangent_y[row * n + i] : 0.0f;
        r.gdy[i] = v;
        r.buf0[i] = v / p.stddev;
      }
      __syncthreads();
      forward_sample_tangent(p, r, zs, net,
                             q.tangent_weights != nullptr
                                 ? q.tangent_weights + (size_t)j * p.n_weights : nullptr,
                             r.buf0, r.buf1);
      for (int i = tid; i < n * H; i += kThreads) q.tangents_out[row * n * H + i] = r.gp[i];
      // (the next writes to gdy, buf0 and gp are behind forward_sample_tangent's last
      // barrier or the tower's first)
    }
    __syncthreads();
  }
}

// num_steps midpoint steps of the state and its M tangents (unforced):
//   k1 = f(y), dk1 = J(y) t;  y_m = y + dt/2 k1, t_m = t + dt/2 dk1;
//   k2 = f(y_m), dk2 = J(y_m) t_m;  y += dt k2, t += dt dk2.
// No adjoint follows, so nothing per step is kept: the state lives in the LDS row gsd, the
// tangents [M][N] and the midpoint's [M][N] in the workgroup's slab at tan_off.
__global__ __launch_bounds__(kThreads) void tangent_rollout_kernel(TangentRolloutParams q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D, M = q.M;
  const Rows r = carve_rows(p, smem, false);
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* net = slab + q.net_off;
  float* tan = slab + q.tan_off;            // [M][N]
  float* tan_mid = tan + (size_t)M * n;     // [M][N]
  float* y = r.gsd;                         // [N]
  const float dt = q.dt, half_dt = 0.5f * q.dt;

  stage_workgroup(p, slab, 0, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const size_t yoff = (size_t)s * n, toff = (size_t)s * M * n;
    for (int i = tid; i < n; i += kThreads) {
      const float v = p.y[yoff + i];
      y[i] = v;
      r.u[i] = v;
    }
    for (int i = tid; i < M * n; i += kThreads) tan[i] = q.tangents[toff + i];
    __syncthreads();
    for (int step = 0; step < q.num_steps; ++step) {
      for (int stage = 0; stage < 2; ++stage) {
        // r.u holds y (stage 0) or y_m (stage 1); thread i owns element i of every row [N]
        stage_tower_input(p, r);
        float* cur = r.buf0;
        float* nxt = r.buf1;
        forward_sample(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
        save_net_output(p, cur, net);
        const float* from = stage == 0 ? tan : tan_mid;
        for (int j = 0; j < M; ++j) {
          for (int i = tid; i < n; i += kThreads) {
            const float v = from[(size_t)j * n + i];
            r.gdy[i] = v;
            r.buf0[i] = v / p.stddev;
          }
          __syncthreads();
          forward_sample_tangent(p, r, zs, net, nullptr, r.buf0, r.buf1);
          for (int i = tid; i < n; i += kThreads) {
            const float dk = r.gp[(size_t)i * H + D];
            if (stage == 0) tan_mid[(size_t)j * n + i] = tan[(size_t)j * n + i] + half_dt * dk;
            else tan[(size_t)j * n + i] = tan[(size_t)j * n + i] + dt * dk;
          }
        }
        __syncthreads();
        for (int i = tid; i < n; i += kThreads) {
          const float k = r.pred[(size_t)i * H + D];
          if (stage == 0) {
            r.u[i] = y[i] + half_dt * k;
          } else {
            y[i] = y[i] + dt * k;
            r.u[i] = y[i];
          }
        }
        __syncthreads();
      }
    }
    for (int i = tid; i < n; i += kThreads) q.state_out[yoff + i] = y[i];
    for (int i = tid; i < M * n; i += kThreads) q.tangents_out[toff + i] = tan[i];
    __syncthreads();
  }
}

hipError_t launch_jvp(const JvpParams& q, int blocks, size_t lds_bytes, hipStream_t stream) {
  return launch_then_sum(reinterpret_cast<const void*>(jvp_kernel), &q, q.t, blocks, lds_bytes,
                         stream, 0, 0);
}

hipError_t launch_tangent_rollout(const TangentRolloutParams& q, int blocks, size_t lds_bytes,
                                  hipStream_t stream) {
  return launch_then_sum(reinterpret_cast<const void*>(tangent_rollout_kernel), &q, q.t, blocks,
                         lds_bytes, stream, 0, 0);
}

}  // namespace train
}  // namespace ddd
