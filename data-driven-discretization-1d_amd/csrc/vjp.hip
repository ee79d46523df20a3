// The vector-Jacobian product of one learned-stencil model evaluation (train.h:
// VjpParams), launched by ddd_result_vjp (capi.hip).  The forward pass and the tower's
// backward pass are train_device.h's; per sample this kernel adds the cotangent load,
// the backward pass through the equation of motion and the stencils, and the state
// gradient
//   grad_y[x] = (a) gfl[x] d r / d y (the explicit state terms of the equation)
//             + (b) sum_d sum_g gs[x - g + gl, d] coef[x - g + gl, d, g] (transposed
//                   stencils, gathered: coefficients target only)
//             + (c) layer 0's transposed convolution / stddev (the tower's input),
// where gs[x, d] is the cotangent of space derivative d at x.
#include <hip/hip_runtime.h>

#include "train_device.h"

namespace ddd {
namespace train {

__global__ __launch_bounds__(kThreads) void vjp_kernel(VjpParams q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  // the LDS plan of loss_grad_kernel; the two error-term rows carry no loss here
  float* u = smem;                 // [N]
  float* gdy = u + n;              // [N] cotangent of the time derivative
  float* gfl = gdy + n;            // [N] flux (forward) / cotangent of the flux (backward)
  float* pred = gfl + n;           // [N][H]
  float* gp = pred + (size_t)n * H;   // [N][H] the caller's cotangent
  float* gsd = gp + (size_t)n * H;    // [N][H] gs: cotangents of the space derivatives
  float* gu = gsd + (size_t)n * H;    // [N] state gradient, terms (a) + (b)
  float* buf0 = gu + (size_t)n * H;   // [N][cmax]
  float* buf1 = buf0 + (size_t)n * p.cmax;
  float* wl = buf1 + (size_t)n * p.cmax;   // staged 32 x 32 kernels (p.mfma)
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  const bool want_w = p.want_grad != 0;
  const bool stencils = p.target == TARGET_COEFFICIENTS;
  const bool direct_time = p.target == TARGET_TIME_DERIVATIVE;
  const bool flux_diff = !direct_time && p.conservative;
  const int gl = p.G / 2;

  if (want_w)
    for (int i = tid; i < p.n_weights; i += kThreads) slab[i] = 0.0f;
  for (int l = 0; l < p.L; ++l) {
    if (p.wl_off[l] < 0) continue;
    const float* src = p.weights + p.w_off[l];
    for (int i = tid; i < p.K * 32 * 32; i += kThreads) wl[p.wl_off[l] + i] = src[i];
  }
  __syncthreads();

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const size_t yoff = (size_t)s * n, poff = (size_t)s * n * H;
    for (int i = tid; i < n; i += kThreads) {
      const float v = p.y[yoff + i];
      u[i] = v;
      buf0[i] = v / p.stddev;
    }
    __syncthreads();
    float* cur = buf0;
    float* nxt = buf1;
    forward_sample(p, wl, zs, u, gfl, pred, cur, nxt);
    if (p.predictions != nullptr)
      for (int i = tid; i < n * H; i += kThreads) p.predictions[poff + i] = pred[i];
    if (q.cotangent == nullptr) continue;   // (block-uniform; the next write to pred or
                                            // u is behind a barrier)
    for (int i = tid; i < n * H; i += kThreads) gp[i] = q.cotangent[poff + i];
    __syncthreads();
    // ---- backward through the equation of motion and the flux difference
    for (int x = tid; x < n; x += kThreads) gdy[x] = gp[(size_t)x * H + D];
    __syncthreads();
    for (int x = tid; x < n; x += kThreads)
      gfl[x] = flux_diff ? p.inv_dx * (gdy[x] - gdy[x == 0 ? n - 1 : x - 1]) : gdy[x];
    __syncthreads();
    // ---- ... the stencils and the projection: d / d net output, into nxt; gs and the
    // state gradient's term (a)
    float* gz = nxt;
    for (int x = tid; x < n; x += kThreads) {
      if (direct_time) {
        gz[x] = gfl[x];
        gu[x] = 0.0f;
        continue;
      }
      float dv[kMaxDerivs] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int d = 0; d < D; ++d) dv[d] = pred[(size_t)x * H + d];
      gu[x] = gfl[x] * rhs_state_partial(p.equation, dv);
      for (int d = 0; d < D; ++d) {
        const float gs = gp[(size_t)x * H + d] + gfl[x] * rhs_partial(p.equation, d, u[x], dv, p.eta);
        gsd[(size_t)x * H + d] = gs;
        if (p.target == TARGET_SPACE_DERIVATIVES) {
          gz[(size_t)x * p.C_out + d] = gs;
        } else if (p.pao == 0) {
          float mean = 0.0f;
          if (p.unbiased) {
            for (int g = 0; g < p.G; ++g) mean += gs * u[wrap(x + g - gl, n)];
            mean = mean / (float)p.G;
          }
          for (int g = 0; g < p.G; ++g)
            gz[(size_t)x * p.C_out + d * p.G + g] = gs * u[wrap(x + g - gl, n)] - mean;
        } else {
          const float* __restrict__ ns = p.nullspace + p.ns_off[d];
          for (int j = 0; j < p.in_size[d]; ++j) {
            float acc = 0.0f;
            for (int g = 0; g < p.G; ++g)
              acc = fmaf(gs * u[wrap(x + g - gl, n)], ns[j * p.G + g], acc);
            gz[(size_t)x * p.C_out + p.in_start[d] + j] = acc;
          }
        }
      }
    }
    __syncthreads();
    float* gy = q.grad_y != nullptr ? q.grad_y + yoff : nullptr;
    if (gy != nullptr && stencils) {
      // term (b): point x enters the stencil of x - g + gl as tap g; the coefficients are
      // re-formed from the net output (cur, still live) exactly as forward_sample forms them
      const float* net = cur;
      for (int x = tid; x < n; x += kThreads) {
        float acc = 0.0f;
        for (int d = 0; d < D; ++d) {
          for (int g = 0; g < p.G; ++g) {
            const int xs = wrap(x - g + gl, n);
            float coeff;
            if (p.pao == 0) {
              float mean = 0.0f;
              if (p.unbiased) {
                for (int h = 0; h < p.G; ++h) mean += net[(size_t)xs * p.C_out + d * p.G + h];
                mean = mean / (float)p.G;
              }
              coeff = net[(size_t)xs * p.C_out + d * p.G + g] - mean;
            } else {
              const float* __restrict__ ns = p.nullspace + p.ns_off[d];
              const float* __restrict__ nv = net + (size_t)xs * p.C_out + p.in_start[d];
              float proj = 0.0f;
              for (int j = 0; j < p.in_size[d]; ++j) proj = fmaf(nv[j], ns[j * p.G + g], proj);
              coeff = p.bias[d * p.G + g] + proj;
            }
            acc = fmaf(gsd[(size_t)xs * H + d], coeff, acc);
          }
        }
        gu[x] += acc;
      }
      __syncthreads();
    }
    // ---- the tower, top down (the net output is no longer needed); term (c) and the
    // state gradient's store at layer 0
    tower_backward(p, wl, zs, u, gz, cur, slab, want_w, gu, gy);
    __syncthreads();
  }
}

// grad[i] = sum over workgroups b (in order) of slab_b[i], i < n_weights
__global__ __launch_bounds__(kThreads) void vjp_reduce_kernel(VjpParams q, int blocks) {
  const TrainParams& p = q.t;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < p.n_weights; i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += p.ws[(size_t)b * p.slab_stride + i];
    p.grad[i] = acc;
  }
}

hipError_t launch_vjp(const VjpParams& q, int blocks, size_t lds_bytes, hipStream_t stream) {
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(vjp_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(vjp_kernel, dim3(blocks), dim3(kThreads), lds_bytes, stream, q);
  err = hipGetLastError();
  if (err != hipSuccess || !q.t.want_grad) return err;
  const int grid = (q.t.n_weights + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(vjp_reduce_kernel, dim3(grid), dim3(kThreads), 0, stream, q, blocks);
  return hipGetLastError();
}

}  // namespace train
}  // namespace ddd
