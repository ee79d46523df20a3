// Training kernels (train.h): the fused loss-and-gradient kernel and the fixed-order
// reduction of its partial slabs, launched by ddd_train_loss_grad (capi.hip).
#include <hip/hip_runtime.h>

#include "train_device.h"

namespace ddd {
namespace train {

__global__ __launch_bounds__(kThreads) void loss_grad_kernel(TrainParams p) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  float* u = smem;                 // [N]
  float* gdy = u + n;              // [N] cotangent of the time derivative
  float* gfl = gdy + n;            // [N] flux (forward) / cotangent of the flux (backward)
  float* pred = gfl + n;           // [N][H]
  float* gp = pred + (size_t)n * H;
  float* em = gp + (size_t)n * H;
  float* er = em + (size_t)n * H;
  float* buf0 = er + (size_t)n * H;   // [N][cmax]
  float* buf1 = buf0 + (size_t)n * p.cmax;
  float* wl = buf1 + (size_t)n * p.cmax;   // staged 32 x 32 kernels (p.mfma)
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  const bool direct_time = p.target == TARGET_TIME_DERIVATIVE;
  const bool flux_diff = !direct_time && p.conservative;
  const float inv_count = 1.0f / ((float)p.batch * (float)n);
  const int gl = p.G / 2;

  for (int i = tid; i < p.n_slab; i += kThreads) slab[i] = 0.0f;
  for (int l = 0; l < p.L; ++l) {
    if (p.wl_off[l] < 0) continue;
    const float* src = p.weights + p.w_off[l];
    for (int i = tid; i < p.K * 32 * 32; i += kThreads) wl[p.wl_off[l] + i] = src[i];
  }
  __syncthreads();

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
      u[i] = v;
      buf0[i] = v / p.stddev;
    }
    __syncthreads();
    // ---- forward: the tower (model.py:420-513 / 551-615)
    float* cur = buf0;
    float* nxt = buf1;
    for (int l = 0; l < p.L; ++l) {
      const bool last = l == p.L - 1;
      if (p.wl_off[l] >= 0)
        conv_forward_mfma(p, l, wl, cur, nxt, last ? nullptr : zs + p.z_off[l],
                          last ? ACT_NONE : p.act);
      else
        conv_forward(p, l, cur, nxt, last ? nullptr : zs + p.z_off[l], last ? ACT_NONE : p.act);
      __syncthreads();
      float* t = cur; cur = nxt; nxt = t;
    }
    const float* net = cur;   // [N][C_out]
    // ---- stencils and the equation of motion
    for (int x = tid; x < n; x += kThreads) {
      float dv[kMaxDerivs] = {0.0f, 0.0f, 0.0f, 0.0f};
      float r;
      if (direct_time) {
        r = net[x];
      } else {
#pragma unroll
        for (int d = 0; d < kMaxDerivs; ++d) {
          if (d >= D) continue;
          float sd = 0.0f;
          if (p.target == TARGET_SPACE_DERIVATIVES) {
            sd = net[(size_t)x * p.C_out + d];
          } else {
            float mean = 0.0f;
            if (p.pao == 0 && p.unbiased) {
              for (int g = 0; g < p.G; ++g) mean += net[(size_t)x * p.C_out + d * p.G + g];
              mean = mean / (float)p.G;
            }
            for (int g = 0; g < p.G; ++g) {
              float coeff;
              if (p.pao == 0) {
                coeff = net[(size_t)x * p.C_out + d * p.G + g] - mean;
              } else {
                const float* __restrict__ ns = p.nullspace + p.ns_off[d];
                const float* __restrict__ nv = net + (size_t)x * p.C_out + p.in_start[d];
                float proj = 0.0f;
                for (int j = 0; j < p.in_size[d]; ++j) proj = fmaf(nv[j], ns[j * p.G + g], proj);
                coeff = p.bias[d * p.G + g] + proj;
              }
              sd = fmaf(coeff, u[wrap(x + g - gl, n)], sd);
            }
          }
          dv[d] = sd;
        }
        r = equation_rhs_or_flux(p.equation, u[x], dv, p.eta);
      }
      for (int d = 0; d < D; ++d) pred[(size_t)x * H + d] = dv[d];   // zeros: time target
      gfl[x] = r;
    }
    __syncthreads();
    for (int x = tid; x < n; x += kThreads) {
      const float r = flux_diff ? -(p.inv_dx * (gfl[x + 1 == n ? 0 : x + 1] - gfl[x])) : gfl[x];
      pred[(size_t)x * H + D] = r;
    }
    __syncthreads();
    // ---- loss terms and their cotangent (abs_and_rel_error, loss_per_head, weighted_loss)
    const size_t loff = (size_t)row * n * H;
    for (int i = tid; i < n * H; i += kThreads) {
      const int h = i % H;
      const float pv = pred[i], lv = p.labels[loff + i], bv = p.baseline[loff + i];
      const float diff = lv - pv, base = lv - bv;
      const float me = diff * diff;
      const float den = base * base + p.floor[h];
      em[i] = me;
      er[i] = me / den;
      gp[i] = ((2.0f * (pv - lv)) * (p.coef_abs[h] + p.coef_rel[h] / den)) * inv_count;
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
    // ---- backward through the equation of motion and the flux difference
    for (int x = tid; x < n; x += kThreads) gdy[x] = gp[(size_t)x * H + D];
    __syncthreads();
    for (int x = tid; x < n; x += kThreads)
      gfl[x] = flux_diff ? p.inv_dx * (gdy[x] - gdy[x == 0 ? n - 1 : x - 1]) : gdy[x];
    __syncthreads();
    // ---- ... the stencils and the projection: d loss / d net output, into nxt
    float* gz = nxt;
    for (int x = tid; x < n; x += kThreads) {
      if (direct_time) {
        gz[x] = gfl[x];
        continue;
      }
      float dv[kMaxDerivs] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int d = 0; d < D; ++d) dv[d] = pred[(size_t)x * H + d];
      for (int d = 0; d < D; ++d) {
        const float gs = gp[(size_t)x * H + d] + gfl[x] * rhs_partial(p.equation, d, u[x], dv, p.eta);
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
    // ---- the tower, top down: weight gradients, then the cotangent of the layer below
    float* act_in = cur;   // (the net output is no longer needed)
    for (int l = p.L - 1; l >= 0; --l) {
      const int cin = p.cin[l], cout = p.cout[l], left = p.K / 2;
      // the layer's input: u / stddev, or act(pre-activation of layer l - 1)
      if (l == 0) {
        for (int i = tid; i < n; i += kThreads) act_in[i] = u[i] / p.stddev;
      } else {
        const float* z = zs + p.z_off[l - 1];
        for (int i = tid; i < n * cin; i += kThreads) act_in[i] = apply_activation(z[i], p.act);
      }
      __syncthreads();
      const int kcc = p.K * cin * cout;
      float* __restrict__ gw = slab + p.w_off[l];
      if (p.wl_off[l] >= 0) conv_weight_grad_mfma(p, act_in, gz, gw);
      else
      for (int e = tid; e < kcc + cout; e += kThreads) {
        float acc = 0.0f;
        if (e < kcc) {
          const int k = e / (cin * cout), ci = (e / cout) % cin, co = e % cout;
          for (int x = 0; x < n; ++x)
            acc = fmaf(act_in[(size_t)wrap(x + k - left, n) * cin + ci], gz[(size_t)x * cout + co], acc);
        } else {
          const int co = e - kcc;
          for (int x = 0; x < n; ++x) acc += gz[(size_t)x * cout + co];
        }
        gw[e] += acc;
      }
      if (l == 0) break;
      __syncthreads();
      // d loss / d pre-activation of layer l - 1 (transposed convolution), over act_in
      const float* __restrict__ w = p.weights + p.w_off[l];
      const float* z = zs + p.z_off[l - 1];
      if (p.wl_off[l] >= 0) conv_backward_data_mfma(p, l, wl, gz, z, act_in);
      else
      for (int idx = tid; idx < n * cin; idx += kThreads) {
        const int y = idx / cin, ci = idx - y * cin;
        float acc = 0.0f;
        for (int k = 0; k < p.K; ++k) {
          const float* __restrict__ g = gz + (size_t)wrap(y - k + left, n) * cout;
          const float* __restrict__ wk = w + ((size_t)k * cin + ci) * cout;
          for (int co = 0; co < cout; ++co) acc = fmaf(g[co], wk[co], acc);
        }
        act_in[idx] = acc * activation_grad(z[idx], p.act);
      }
      __syncthreads();
      float* t = gz; gz = act_in; act_in = t;
    }
    __syncthreads();
  }
}

// grad[i] = sum over workgroups b (in order) of slab_b[i]; head_means = head sums / (batch N)
__global__ __launch_bounds__(kThreads) void reduce_kernel(TrainParams p, int blocks) {
  const int H2 = 2 * p.H;
  const int first = p.want_grad ? 0 : p.n_weights;
  const int total = p.n_weights + H2;
  for (int i = first + blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += p.ws[(size_t)b * p.slab_stride + i];
    if (i < p.n_weights) p.grad[i] = acc;
    else p.head_means[i - p.n_weights] = acc / ((float)p.batch * (float)p.N);
  }
}

hipError_t launch_loss_grad(const TrainParams& p, int blocks, size_t lds_bytes, hipStream_t stream) {
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(loss_grad_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(loss_grad_kernel, dim3(blocks), dim3(kThreads), lds_bytes, stream, p);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int total = p.n_weights + 2 * p.H;
  const int grid = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(reduce_kernel, dim3(grid), dim3(kThreads), 0, stream, p, blocks);
  return hipGetLastError();
}

}  // namespace train
}  // namespace ddd
