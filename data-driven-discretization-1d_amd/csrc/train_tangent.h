// The tangent-linear model of one learned-stencil evaluation: forward mode (J t) beside
// train_device.h's reverse mode (c^T J).  forward_sample_tangent pushes one tangent of the
// state, of the weights, or of both through the evaluation whose forward pass
// (forward_sample) has just run; jvp.hip's kernels call it once per tangent, so the primal
// pass is shared by the M tangents of a sample.  State tangents only along a rollout, and
// no forcing anywhere: the forcing term does not depend on the state or the weights.
//
// Rows used (train_device.h: Rows), all free once forward_sample has returned:
//   gdy  [N]     the state tangent tu (the caller fills it)
//   gfl  [N]     the tangent of the flux / right-hand side
//   gp   [N][H]  the tangent of the predictions (the result)
//   buf0 / buf1  the tower's tangent activations; the net output they held is saved to
//                the slab (save_net_output) before the first tangent
#pragma once
#include "train_device.h"

namespace ddd {
namespace train {

// The net output [N][C_out] from `cur` (LDS) to `net` (the slab): both activation buffers
// are then free for the tangents.  Block-wide.
__device__ __forceinline__ void save_net_output(const TrainParams& p, const float* cur,
                                                float* net) {
  for (int i = threadIdx.x; i < p.N * p.C_out; i += kThreads) net[i] = cur[i];
  __syncthreads();
}

// dz = conv(W, da) without bias, times act'(z) when z is non-null (VALU)
template <bool kReplicas = false>
__device__ inline void conv_tangent(const TrainParams& p, int l, const float* in, float* out,
                                    const float* z) {
  const int n = p.N, cin = p.cin[l], cout = p.cout[l], left = p.K / 2;
  const float* __restrict__ w = weights_of<kReplicas>(p) + p.w_off[l];
  for (int idx = threadIdx.x; idx < n * cout; idx += kThreads) {
    const int x = idx / cout, co = idx - x * cout;
    float acc = 0.0f;
    for (int k = 0; k < p.K; ++k) {
      const float* __restrict__ row = in + (size_t)wrap(x + k - left, n) * cin;
      const float* __restrict__ wk = w + (size_t)k * cin * cout + co;
      for (int ci = 0; ci < cin; ++ci) acc = fmaf(row[ci], wk[(size_t)ci * cout], acc);
    }
    out[idx] = z != nullptr ? acc * activation_grad(z[idx], p.act) : acc;
  }
}

// conv_tangent for a staged layer: in [N][32] -> out [N][32], the tile walk and operand
// layout of conv_forward_mfma
__device__ inline void conv_tangent_mfma(const TrainParams& p, int l, const float* wl,
                                         const float* in, float* out, const float* z) {
  const int n = p.N, left = p.K / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const float* __restrict__ w = wl + p.wl_off[l];
  for (int t = wave; t < n / 32; t += kThreads / 64) {
    const int x0 = 32 * t;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k = 0; k < p.K; ++k) {
      const float* __restrict__ row = in + (size_t)wrap(x0 + i + k - left, n) * 32 + half;
      const float* __restrict__ wk = w + (size_t)(k * 32 + half) * 32 + i;
      for (int c = 0; c < 32; c += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(row[c], wk[c * 32], acc, 0, 0, 0);
    }
    for (int r = 0; r < 16; ++r) {
      const int idx = (x0 + mfma_row(r, half)) * 32 + i;
      out[idx] = z != nullptr ? acc[r] * activation_grad(z[idx], p.act) : acc[r];
    }
  }
}

// One tangent through the evaluation whose forward pass has just run.  Contract with
// forward_sample and the caller: r.u and r.pred are that evaluation's, zs holds its
// pre-activations and `net` (global) its net output [N][C_out]; r.gdy holds the state
// tangent tu [N] and `in` (r.buf0 or r.buf1) tu / stddev; `out` is the other buffer.  tw,
// when non-null, is a direction of the weights (ddd_model_create layout): layer l adds
// conv(dW, act_prev) + db, act_prev re-formed from zs into the buffer the state part has
// just consumed, on the VALU in every layer.  The result, the tangent of the predictions
// [N][H], is left in r.gp (zero in the space-derivative channels of the time_derivative
// target).  Block-wide.
template <bool kReplicas = false>
__device__ __forceinline__ void forward_sample_tangent(const TrainParams& p, const Rows& r,
                                                       const float* zs, const float* net,
                                                       const float* tw, float* in, float* out) {
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const bool direct_time = p.target == TARGET_TIME_DERIVATIVE;
  const bool flux_diff = !direct_time && p.conservative;
  const int gl = p.G / 2, left = p.K / 2;
  const float* u = r.u;
  const float* tu = r.gdy;
  // ---- the tower: da_0 = tu / stddev, dz = conv(W, da) [+ conv(dW, a) + db], da = act'(z) dz
  for (int l = 0; l < p.L; ++l) {
    const int cin = p.cin[l], cout = p.cout[l];
    const float* z = l == p.L - 1 ? nullptr : zs + p.z_off[l];
    const float* z_now = tw == nullptr ? z : nullptr;   // with tw, act'(z) waits for its term
    if (p.wl_off[l] >= 0) conv_tangent_mfma(p, l, r.wl, in, out, z_now);
    else conv_tangent<kReplicas>(p, l, in, out, z_now);
    __syncthreads();
    if (tw != nullptr) {
      if (l == 0) {
        for (int i = tid; i < n; i += kThreads) in[i] = u[i] / p.stddev;
      } else {
        const float* zp = zs + p.z_off[l - 1];
        for (int i = tid; i < n * cin; i += kThreads) in[i] = apply_activation(zp[i], p.act);
      }
      __syncthreads();
      const float* __restrict__ dw = tw + p.w_off[l];
      const float* __restrict__ db = dw + (size_t)p.K * cin * cout;
      for (int idx = tid; idx < n * cout; idx += kThreads) {
        const int x = idx / cout, co = idx - x * cout;
        float acc = 0.0f;
        for (int k = 0; k < p.K; ++k) {
          const float* __restrict__ row = in + (size_t)wrap(x + k - left, n) * cin;
          const float* __restrict__ wk = dw + (size_t)k * cin * cout + co;
          for (int ci = 0; ci < cin; ++ci) acc = fmaf(row[ci], wk[(size_t)ci * cout], acc);
        }
        const float dz = out[idx] + (acc + db[co]);
        out[idx] = z != nullptr ? dz * activation_grad(z[idx], p.act) : dz;
      }
      __syncthreads();
    }
    float* t = in; in = out; out = t;
  }
  const float* dnet = in;   // [N][C_out]
  // ---- stencils (product rule) and the equation of motion
  for (int x = tid; x < n; x += kThreads) {
    float dr;
    if (direct_time) {
      for (int d = 0; d < D; ++d) r.gp[(size_t)x * H + d] = 0.0f;
      dr = dnet[x];
    } else {
      float dv[kMaxDerivs] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int d = 0; d < D; ++d) dv[d] = r.pred[(size_t)x * H + d];
      dr = rhs_state_partial(p.equation, dv) * tu[x];
      for (int d = 0; d < D; ++d) {
        float dsd = 0.0f;
        if (p.target == TARGET_SPACE_DERIVATIVES) {
          dsd = dnet[(size_t)x * p.C_out + d];
        } else {
          float mean = 0.0f, dmean = 0.0f;
          if (p.pao == 0 && p.unbiased) {
            for (int g = 0; g < p.G; ++g) {
              mean += net[(size_t)x * p.C_out + d * p.G + g];
              dmean += dnet[(size_t)x * p.C_out + d * p.G + g];
            }
            mean = mean / (float)p.G;
            dmean = dmean / (float)p.G;
          }
          for (int g = 0; g < p.G; ++g) {
            float coeff, dcoeff;
            if (p.pao == 0) {
              coeff = net[(size_t)x * p.C_out + d * p.G + g] - mean;
              dcoeff = dnet[(size_t)x * p.C_out + d * p.G + g] - dmean;
            } else {
              const float* __restrict__ ns = p.nullspace + p.ns_off[d];
              const float* __restrict__ nv = net + (size_t)x * p.C_out + p.in_start[d];
              const float* __restrict__ dnv = dnet + (size_t)x * p.C_out + p.in_start[d];
              float proj = 0.0f, dproj = 0.0f;
              for (int j = 0; j < p.in_size[d]; ++j) {
                proj = fmaf(nv[j], ns[j * p.G + g], proj);
                dproj = fmaf(dnv[j], ns[j * p.G + g], dproj);
              }
              coeff = p.bias[d * p.G + g] + proj;
              dcoeff = dproj;
            }
            const int xg = wrap(x + g - gl, n);
            dsd = fmaf(dcoeff, u[xg], dsd);
            dsd = fmaf(coeff, tu[xg], dsd);
          }
        }
        r.gp[(size_t)x * H + d] = dsd;
        dr = fmaf(rhs_partial(p.equation, d, u[x], dv, p.eta), dsd, dr);
      }
    }
    r.gfl[x] = dr;
  }
  __syncthreads();
  // (the flux difference is linear: the same difference of the flux tangent)
  for (int x = tid; x < n; x += kThreads)
    r.gp[(size_t)x * H + D] =
        flux_diff ? -(p.inv_dx * (r.gfl[x + 1 == n ? 0 : x + 1] - r.gfl[x])) : r.gfl[x];
  __syncthreads();
}

}  // namespace train
}  // namespace ddd
