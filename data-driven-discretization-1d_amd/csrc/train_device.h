// Device code shared by the kernels that differentiate one learned-stencil model
// evaluation: loss_grad_kernel (train.hip), vjp_kernel (vjp.hip),
// unrolled_loss_grad_kernel (train_unrolled.hip) and rollout_loss_grad_kernel
// (train_rollout.hip).  Activation and equation derivatives, the
// conv layers on the VALU and on v_mfma_f32_32x32x2_f32, the loss terms of one (point,
// head), the LDS plan of a workgroup and its prologue, the forward pass of one sample
// (forward_sample) and its backward pass from a cotangent of the predictions down to the
// weights and the state (evaluation_vjp, over tower_backward).  Each exists once, here;
// the kernels differ in where the cotangent comes from and where the state gradient goes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "train.h"

namespace ddd {
namespace train {

__device__ __forceinline__ int wrap(int i, int n) {
  i %= n;
  return i < 0 ? i + n : i;
}

__device__ __forceinline__ float activation_grad(float z, int act) {
  switch (act) {
    case ACT_RELU: return z > 0.0f ? 1.0f : 0.0f;
    case ACT_RELU6: return (z > 0.0f && z < 6.0f) ? 1.0f : 0.0f;
    case ACT_TANH: { const float t = tanhf(z); return 1.0f - t * t; }
    case ACT_SOFTPLUS: return 1.0f / (1.0f + expf(-z));
    case ACT_ELU: return z > 0.0f ? 1.0f : expf(z);
    default: return 1.0f;
  }
}

// d equation_rhs_or_flux / d derivative d (dev_params.h), at state y and derivatives dv
__device__ __forceinline__ float rhs_partial(int eq, int d, float y, const float (&dv)[kMaxDerivs],
                                             float eta) {
  switch (eq) {
    case EQ_BURGERS: return d == 0 ? -y : eta;
    case EQ_BURGERS_CONS: return d == 0 ? dv[0] : -eta;
    case EQ_KDV: return d == 0 ? -6.0f * y : -1.0f;
    case EQ_KDV_CONS: return d == 0 ? 6.0f * dv[0] : 1.0f;
    case EQ_KS: return d == 0 ? -y : -1.0f;
    case EQ_KS_CONS: return d == 0 ? dv[0] : 1.0f;
    default: return 0.0f;
  }
}

// d equation_rhs_or_flux / d y through its explicit state argument (dev_params.h): the
// non-conservative forms multiply the first derivative by y; fluxes do not read y
__device__ __forceinline__ float rhs_state_partial(int eq, const float (&dv)[kMaxDerivs]) {
  switch (eq) {
    case EQ_BURGERS: return -dv[0];
    case EQ_KDV: return -6.0f * dv[0];
    case EQ_KS: return -dv[0];
    default: return 0.0f;
  }
}

// The kernels of train_population.hip run R replicas on a grid (blocks, R): workgroup
// (b, r) is workgroup b of replica r, whose weights, slabs, minibatch and coefficient
// table lie r strides behind replica 0's (the pointers of p).  kReplicas is a template
// flag, false by default: every other kernel is one replica and compiles as before.
template <bool kReplicas>
__device__ __forceinline__ const float* weights_of(const TrainParams& p) {
  return kReplicas ? p.weights + (size_t)blockIdx.y * p.n_weights : p.weights;
}

// out[x][co] = bias[co] + sum_k sum_ci in[x + k - K/2][ci] w[k][ci][co]  (periodic), the
// pre-activation also stored to `z` (global) when non-null, out = act(pre-activation)
template <bool kReplicas = false>
__device__ inline void conv_forward(const TrainParams& p, int l, const float* in, float* out,
                                    float* z, int act) {
  const int n = p.N, cin = p.cin[l], cout = p.cout[l], left = p.K / 2;
  const float* __restrict__ w = weights_of<kReplicas>(p) + p.w_off[l];
  const float* __restrict__ b = w + (size_t)p.K * cin * cout;
  for (int idx = threadIdx.x; idx < n * cout; idx += kThreads) {
    const int x = idx / cout, co = idx - x * cout;
    float acc = 0.0f;
    for (int k = 0; k < p.K; ++k) {
      const float* __restrict__ row = in + (size_t)wrap(x + k - left, n) * cin;
      const float* __restrict__ wk = w + (size_t)k * cin * cout + co;
      for (int ci = 0; ci < cin; ++ci) acc = fmaf(row[ci], wk[(size_t)ci * cout], acc);
    }
    const float pre = acc + b[co];
    if (z != nullptr) z[idx] = pre;
    out[idx] = apply_activation(pre, act);
  }
}

// ---- the 32 -> 32 layers on v_mfma_f32_32x32x2_f32 (layout checked by
// ddd_selftest_mfma_layout, ops.h): A[i][k] from lane i + 32 k, B[k][j] from lane j + 32 k,
// register r of lane l holds D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31].  Each of the
// four wavefronts owns 32-row tiles (forward, backward-data) or taps (weight gradient).
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int mfma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// conv_forward for a staged layer: in [N][32] -> out / z [N][32]
template <bool kReplicas = false>
__device__ inline void conv_forward_mfma(const TrainParams& p, int l, const float* wl,
                                         const float* in, float* out, float* z, int act) {
  const int n = p.N, left = p.K / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const float* __restrict__ w = wl + p.wl_off[l];
  const float* __restrict__ b = weights_of<kReplicas>(p) + p.w_off[l] + (size_t)p.K * 32 * 32;
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
    const float bias = b[i];
    for (int r = 0; r < 16; ++r) {
      const int idx = (x0 + mfma_row(r, half)) * 32 + i;
      const float pre = acc[r] + bias;
      if (z != nullptr) z[idx] = pre;
      out[idx] = apply_activation(pre, act);
    }
  }
}

// d loss / d pre-activation of the layer below a staged layer:
// ga[y][ci] = sum_k sum_co gz[y - k + K/2][co] w[k][ci][co], times act'(z[y][ci])
__device__ inline void conv_backward_data_mfma(const TrainParams& p, int l, const float* wl,
                                               const float* gz, const float* z, float* out) {
  const int n = p.N, left = p.K / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  const float* __restrict__ w = wl + p.wl_off[l];
  for (int t = wave; t < n / 32; t += kThreads / 64) {
    const int y0 = 32 * t;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k = 0; k < p.K; ++k) {
      const float* __restrict__ g = gz + (size_t)wrap(y0 + i - k + left, n) * 32 + half;
      const float* __restrict__ wk = w + (size_t)(k * 32 + i) * 32 + half;
      for (int c = 0; c < 32; c += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g[c], wk[c], acc, 0, 0, 0);
    }
    for (int r = 0; r < 16; ++r) {
      const int idx = (y0 + mfma_row(r, half)) * 32 + i;
      out[idx] = acc[r] * activation_grad(z[idx], p.act);
    }
  }
}

// weight gradient of a staged layer: gw[k][ci][co] += sum_x a[x + k - K/2][ci] gz[x][co]
// (one wavefront per tap), gw[K][32][32 + co] (the bias) += sum_x gz[x][co]
__device__ inline void conv_weight_grad_mfma(const TrainParams& p, const float* a,
                                             const float* gz, float* gw) {
  const int n = p.N, left = p.K / 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 31, half = lane >> 5;
  for (int k = wave; k < p.K; k += kThreads / 64) {
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int x = half; x < n; x += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[(size_t)wrap(x + k - left, n) * 32 + i],
                                                 gz[(size_t)x * 32 + i], acc, 0, 0, 0);
    float* __restrict__ gk = gw + (size_t)k * 32 * 32;
    for (int r = 0; r < 16; ++r) gk[mfma_row(r, half) * 32 + i] += acc[r];
  }
  for (int co = threadIdx.x; co < 32; co += kThreads) {
    float acc = 0.0f;
    for (int x = 0; x < n; ++x) acc += gz[(size_t)x * 32 + co];
    gw[(size_t)p.K * 32 * 32 + co] += acc;
  }
}

struct HeadTerms { float abs_error, rel_error, cotangent; };

// abs_and_rel_error and the cotangent of the weighted loss at one (point, head)
__device__ __forceinline__ HeadTerms head_terms(float pv, float lv, float bv, float floor,
                                                float coef_abs, float coef_rel,
                                                float inv_count) {
  const float diff = lv - pv, base = lv - bv;
  const float me = diff * diff;
  const float den = base * base + floor;
  HeadTerms t;
  t.abs_error = me;
  t.rel_error = me / den;
  t.cotangent = ((2.0f * (pv - lv)) * (coef_abs + coef_rel / den)) * inv_count;
  return t;
}

// head_terms of head h with the loss constants of the call: the host values the kernel
// arguments carry (floor / coef_abs / coef_rel, TrainParams' or UnrolledParams'), or with
// kCoefTable the device table p.coef_table [3][heads] that clip_population_kernel
// (train_population.hip) wrote.
// A template flag, not a run-time null: the kernels of the host values compile as before.
template <bool kCoefTable, bool kReplicas = false>
__device__ __forceinline__ HeadTerms head_terms_of(const TrainParams& p, const float* floor,
                                                   const float* coef_abs, const float* coef_rel,
                                                   int heads, int h, float pv, float lv, float bv,
                                                   float inv_count) {
  if (kCoefTable) {
    const float* table =
        kReplicas ? p.coef_table + (size_t)blockIdx.y * (3 * heads) : p.coef_table;
    return head_terms(pv, lv, bv, table[h], table[heads + h], table[2 * heads + h], inv_count);
  }
  return head_terms(pv, lv, bv, floor[h], coef_abs[h], coef_rel[h], inv_count);
}

// The LDS rows of one workgroup.  The two [N][H] rows behind gp hold the error terms of
// the loss until their per-head sums are taken, and the space-derivative cotangents and
// the state gradient inside evaluation_vjp.
struct Rows {
  float* u;      // [N] the state of the current evaluation
  float* gdy;    // [N] cotangent of the time derivative
  float* gfl;    // [N] flux (forward) / cotangent of the flux (backward)
  float* pred;   // [N][H] one evaluation's predictions
  float* gp;     // [N][H] cotangent of the predictions
  float* gsd;    // [N][H] cotangents of the space derivatives / abs. error terms
  float* gu;     // [N][H] state gradient (a) + (b) (first N) / rel. error terms
  float* buf0;   // [N][cmax]
  float* buf1;   // [N][cmax]
  float* wl;     // staged 32 x 32 kernels (p.mfma)
  float* lam;    // [N] adjoint of the state (through time only)
  float* gmid;   // [N] state gradient of the midpoint evaluation (through time only)
};

// Rows over smem, in the order of the struct.  lds_floats (train.h) counts the rows
// before wl and unrolled_lds_floats (train_unrolled.h) the two behind it: a row added to
// the struct without its size fails to compile here.
__device__ __forceinline__ Rows carve_rows(const TrainParams& p, float* smem, bool through_time) {
  static_assert(offsetof(Rows, wl) / sizeof(float*) == kLdsRowsN + kLdsRowsNH + kLdsRowsNC &&
                    sizeof(Rows) / sizeof(float*) == kLdsRowsN + kLdsRowsNH + kLdsRowsNC + 1 + 2,
                "Rows and lds_floats / unrolled_lds_floats disagree");
  const int n = p.N, H = p.H;
  Rows r;
  r.u = smem;
  r.gdy = r.u + n;
  r.gfl = r.gdy + n;
  r.pred = r.gfl + n;
  r.gp = r.pred + (size_t)n * H;
  r.gsd = r.gp + (size_t)n * H;
  r.gu = r.gsd + (size_t)n * H;
  r.buf0 = r.gu + (size_t)n * H;
  r.buf1 = r.buf0 + (size_t)n * p.cmax;
  r.wl = r.buf1 + (size_t)n * p.cmax;
  r.lam = through_time ? r.wl + p.wl_floats : nullptr;
  r.gmid = through_time ? r.lam + n : nullptr;
  return r;
}

// A workgroup's prologue: the first n_zero floats of its slab cleared (the sums it adds
// into), the 32 x 32 kernels of the MFMA layers copied into wl.  Block-wide.
template <bool kReplicas = false>
__device__ __forceinline__ void stage_workgroup(const TrainParams& p, float* slab, int n_zero,
                                                float* wl) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n_zero; i += kThreads) slab[i] = 0.0f;
  for (int l = 0; l < p.L; ++l) {
    if (p.wl_off[l] < 0) continue;
    const float* src = weights_of<kReplicas>(p) + p.w_off[l];
    for (int i = tid; i < p.K * 32 * 32; i += kThreads) wl[p.wl_off[l] + i] = src[i];
  }
  __syncthreads();
}

// The forward pass of one sample whose state is staged in u (and u / stddev in *cur):
// the tower (model.py:420-513 / 551-615) ping-ponging between *cur and *nxt, the
// hidden layers' pre-activations to zs, then the stencils and the equation of motion
// into pred [N][H] (the flux / right-hand side passes through gfl).  On return *cur
// holds the net output [N][C_out].  Block-wide: every thread calls it.
template <bool kReplicas = false>
__device__ __forceinline__ void forward_sample(const TrainParams& p, const float* wl, float* zs,
                                               const float* u, float* gfl, float* pred,
                                               float*& cur, float*& nxt) {
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const bool direct_time = p.target == TARGET_TIME_DERIVATIVE;
  const bool flux_diff = !direct_time && p.conservative;
  const int gl = p.G / 2;
  for (int l = 0; l < p.L; ++l) {
    const bool last = l == p.L - 1;
    if (p.wl_off[l] >= 0)
      conv_forward_mfma<kReplicas>(p, l, wl, cur, nxt, last ? nullptr : zs + p.z_off[l],
                                   last ? ACT_NONE : p.act);
    else
      conv_forward<kReplicas>(p, l, cur, nxt, last ? nullptr : zs + p.z_off[l],
                              last ? ACT_NONE : p.act);
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
}

// The tower, top down, from gz = d / d net output [N][C_out]: per layer the weight
// gradient added into gw_base (the slab) when want_w, then the cotangent of the layer
// below over act_in.  With grad_y non-null, layer 0's transposed convolution down to its
// single input channel, times 1 / stddev, plus the LDS row gu, goes to grad_y [N] (the
// state gradient through the tower's input).  gz and act_in are overwritten.
template <bool kReplicas = false>
__device__ __forceinline__ void tower_backward(const TrainParams& p, const float* wl,
                                               const float* zs, const float* u, float* gz,
                                               float* act_in, float* gw_base, bool want_w,
                                               const float* gu, float* grad_y) {
  const int tid = threadIdx.x, n = p.N;
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
    if (want_w) {
      float* __restrict__ gw = gw_base + p.w_off[l];
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
    }
    if (l == 0) {
      if (grad_y != nullptr)   // cin = 1: w[k][0][co]
        for (int y = tid; y < n; y += kThreads) {
          float acc = 0.0f;
          for (int k = 0; k < p.K; ++k) {
            const float* __restrict__ g = gz + (size_t)wrap(y - k + left, n) * cout;
            const float* __restrict__ wk =
                weights_of<kReplicas>(p) + p.w_off[0] + (size_t)k * cout;
            for (int co = 0; co < cout; ++co) acc = fmaf(g[co], wk[co], acc);
          }
          grad_y[y] = gu[y] + acc / p.stddev;
        }
      break;
    }
    __syncthreads();
    // d loss / d pre-activation of layer l - 1 (transposed convolution), over act_in
    const float* __restrict__ w = weights_of<kReplicas>(p) + p.w_off[l];
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
}

// The vector-Jacobian product of the evaluation whose forward pass has just run, with the
// cotangent of its predictions in r.gp.  Contract with forward_sample: r.u and r.pred are
// that evaluation's, zs holds its pre-activations and cur its net output [N][C_out], which
// term (b) reads before tower_backward overwrites it; nxt is free.  From r.gp back through
// the equation of motion, the flux difference, the stencils and the projection to the net
// output, then the tower: the weight gradient is added into slab when want_w, and with
// grad_y non-null (LDS or global, [N]) the state gradient
//   grad_y[x] = (a) gfl[x] d r / d y (the explicit state terms of the equation)
//             + (b) sum_d sum_g gs[x - g + gl, d] coef[x - g + gl, d, g] (transposed
//                   stencils, gathered: coefficients target only)
//             + (c) layer 0's transposed convolution / stddev (the tower's input)
// is stored there, gs[x, d] being the cotangent of space derivative d at x.  r.gdy, r.gfl,
// r.gsd and r.gu are overwritten, the last two behind two barriers.  kStateGrad false
// (training: grad_y is null in every call) leaves gs and the state gradient unformed.
// Block-wide.
template <bool kStateGrad, bool kReplicas = false>
__device__ __forceinline__ void evaluation_vjp(const TrainParams& p, const Rows& r,
                                               const float* zs, float* cur, float* nxt,
                                               float* slab, bool want_w, float* grad_y) {
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const bool stencils = p.target == TARGET_COEFFICIENTS;
  const bool direct_time = p.target == TARGET_TIME_DERIVATIVE;
  const bool flux_diff = !direct_time && p.conservative;
  const int gl = p.G / 2;
  const float* u = r.u;
  // ---- backward through the equation of motion and the flux difference
  for (int x = tid; x < n; x += kThreads) r.gdy[x] = r.gp[(size_t)x * H + D];
  __syncthreads();
  for (int x = tid; x < n; x += kThreads)
    r.gfl[x] = flux_diff ? p.inv_dx * (r.gdy[x] - r.gdy[x == 0 ? n - 1 : x - 1]) : r.gdy[x];
  __syncthreads();
  // ---- ... the stencils and the projection: d / d net output, into nxt; gs and the
  // state gradient's term (a)
  float* gz = nxt;
  for (int x = tid; x < n; x += kThreads) {
    if (direct_time) {
      gz[x] = r.gfl[x];
      if (kStateGrad) r.gu[x] = 0.0f;
      continue;
    }
    float dv[kMaxDerivs] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int d = 0; d < D; ++d) dv[d] = r.pred[(size_t)x * H + d];
    if (kStateGrad) r.gu[x] = r.gfl[x] * rhs_state_partial(p.equation, dv);
    for (int d = 0; d < D; ++d) {
      const float gs = r.gp[(size_t)x * H + d] +
                       r.gfl[x] * rhs_partial(p.equation, d, u[x], dv, p.eta);
      if (kStateGrad) r.gsd[(size_t)x * H + d] = gs;
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
  if (kStateGrad && grad_y != nullptr && stencils) {
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
          acc = fmaf(r.gsd[(size_t)xs * H + d], coeff, acc);
        }
      }
      r.gu[x] += acc;
    }
    __syncthreads();
  }
  // ---- the tower, top down (the net output is no longer needed); term (c) and the
  // state gradient's store at layer 0
  tower_backward<kReplicas>(p, r.wl, zs, u, gz, cur, slab, want_w, r.gu,
                            kStateGrad ? grad_y : nullptr);
  __syncthreads();
}

}  // namespace train
}  // namespace ddd
