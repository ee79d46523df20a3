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
// The forward pass and the tower's backward pass are train_device.h's; the backward pass
// through the equation of motion and the stencils, and the state gradient's terms (a)
// and (b), are those of vjp_kernel (vjp.hip), restated here so that vjp_kernel's code
// stays what it was measured as.
#include <hip/hip_runtime.h>

#include "train_device.h"
#include "train_unrolled.h"

namespace ddd {
namespace train {

namespace {

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

// The LDS rows of one workgroup: the plan of loss_grad_kernel / vjp_kernel, then the
// adjoint of the state and the state gradient of the midpoint evaluation
struct Rows {
  float* u;      // [N] the state of the current evaluation
  float* gdy;    // [N] cotangent of the time derivative; g_s at the end of a product
  float* gfl;    // [N] flux (forward) / cotangent of the flux (backward)
  float* pred;   // [N][H] one evaluation's predictions
  float* gp;     // [N][H] cotangent of the predictions
  float* gsd;    // [N][H] cotangents of the space derivatives / abs. error terms
  float* gu;     // [N][H] state gradient (a) + (b) (first N) / rel. error terms
  float* buf0;   // [N][cmax]
  float* buf1;   // [N][cmax]
  float* wl;     // staged 32 x 32 kernels
  float* lam;    // [N] adjoint of the state
  float* gmid;   // [N] g_mid
};

// The vector-Jacobian product of the evaluation whose forward pass has just run
// (forward_sample: r.u, r.pred, the net output in cur, the pre-activations in zs) with
// the cotangent in r.gp: the weight gradient is added into slab, the state gradient goes
// to grad_y [N] (LDS) unless null.  vjp_kernel's backward pass.  Block-wide.
__device__ __forceinline__ void evaluation_vjp(const TrainParams& p, const Rows& r,
                                               const float* zs, float* cur, float* nxt,
                                               float* slab, float* grad_y) {
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
      r.gu[x] = 0.0f;
      continue;
    }
    float dv[kMaxDerivs] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int d = 0; d < D; ++d) dv[d] = r.pred[(size_t)x * H + d];
    r.gu[x] = r.gfl[x] * rhs_state_partial(p.equation, dv);
    for (int d = 0; d < D; ++d) {
      const float gs = r.gp[(size_t)x * H + d] +
                       r.gfl[x] * rhs_partial(p.equation, d, u[x], dv, p.eta);
      r.gsd[(size_t)x * H + d] = gs;
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
  if (grad_y != nullptr && stencils) {
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
  tower_backward(p, r.wl, zs, u, gz, cur, slab, true, r.gu, grad_y);
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(kThreads) void unrolled_loss_grad_kernel(UnrolledParams q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const int T = q.T, HT = q.HT, E = 2 * T;   // E evaluations: 2 s at y_s, 2 s + 1 at y_mid_s
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
  r.lam = r.wl + p.wl_floats;
  r.gmid = r.lam + n;
  float* slab = p.ws + (size_t)blockIdx.x * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* st = slab + q.st_off;   // [E][N] stage states
  float* gi = slab + q.gi_off;   // [T][N] loss cotangents of the integrated heads
  float* heads = slab + p.n_weights;   // [2][HT] sums of the error terms
  const float inv_count = 1.0f / ((float)p.batch * (float)n);
  const float dt = q.dt, half_dt = 0.5f * q.dt;

  for (int i = tid; i < p.n_slab; i += kThreads) slab[i] = 0.0f;
  for (int l = 0; l < p.L; ++l) {
    if (p.wl_off[l] < 0) continue;
    const float* src = p.weights + p.w_off[l];
    for (int i = tid; i < p.K * 32 * 32; i += kThreads) r.wl[p.wl_off[l] + i] = src[i];
  }
  __syncthreads();

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
          const HeadTerms t = head_terms(r.pred[i], p.labels[li], p.baseline[li], q.floor[h],
                                         q.coef_abs[h], q.coef_rel[h], inv_count);
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
          const HeadTerms t = head_terms(y_new, p.labels[li], p.baseline[li], q.floor[h],
                                         q.coef_abs[h], q.coef_rel[h], inv_count);
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
            g += head_terms(r.pred[(size_t)x * H + h], p.labels[li], p.baseline[li], q.floor[h],
                            q.coef_abs[h], q.coef_rel[h], inv_count).cotangent;
          }
          r.gp[(size_t)x * H + h] = g;
        }
      }
      __syncthreads();
      // g_mid to its own row; g_s to gdy (free once the product has read it); lam_0 is
      // not an output, so the last product skips the state gradient
      evaluation_vjp(p, r, zs, cur, nxt, slab, mid ? r.gmid : (e > 0 ? r.gdy : nullptr));
      if (!mid && e > 0) {
        for (int x = tid; x < n; x += kThreads)
          r.lam[x] = ((r.lam[x] + r.gmid[x]) + r.gdy[x]) + gi[(size_t)(step - 1) * n + x];
        __syncthreads();
      }
    }
  }
}

// grad[i] = sum over workgroups b (in order) of slab_b[i]; head_means = head sums / (batch N)
__global__ __launch_bounds__(kThreads) void unrolled_reduce_kernel(UnrolledParams q, int blocks) {
  const TrainParams& p = q.t;
  const int first = p.want_grad ? 0 : p.n_weights;
  const int total = p.n_weights + 2 * q.HT;
  for (int i = first + blockIdx.x * kThreads + threadIdx.x; i < total; i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += p.ws[(size_t)b * p.slab_stride + i];
    if (i < p.n_weights) p.grad[i] = acc;
    else p.head_means[i - p.n_weights] = acc / ((float)p.batch * (float)p.N);
  }
}

hipError_t launch_unrolled_loss_grad(const UnrolledParams& q, int blocks, size_t lds_bytes,
                                     hipStream_t stream) {
  hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(unrolled_loss_grad_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(unrolled_loss_grad_kernel, dim3(blocks), dim3(kThreads), lds_bytes, stream, q);
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  const int total = q.t.n_weights + 2 * q.HT;
  const int grid = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(unrolled_reduce_kernel, dim3(grid), dim3(kThreads), 0, stream, q, blocks);
  return hipGetLastError();
}

}  // namespace train
}  // namespace ddd
