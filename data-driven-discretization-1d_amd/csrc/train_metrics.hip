// ddd_eval_metrics' device code and launcher (train_metrics.h): metrics_kernel, forward only
// over the shared device code of train_device.h, and metrics_sum_kernel.
#include <hip/hip_runtime.h>

#include "train_device.h"
#include "train_metrics.h"

namespace ddd {
namespace train {

namespace {

// The eight terms of heads h0 .. h0 + hc - 1 at the sample's n points, summed per head in
// point order and added into the slab.  pv [n][pv_stride] holds the predictions of those
// heads (LDS); labels and baseline are read at loff + x HT + h.  Three passes over the three
// [N][H] rows behind r.gp (hc <= H): terms 0-2, 3-5, 6-7.  Pass 0's first two rows are the
// em / er of the loss kernels, summed by the same threads in the same order.  Block-wide;
// ends behind a barrier.
__device__ __forceinline__ void metric_sums(const UnrolledParams& q, const Rows& r, float* slab,
                                            const float* pv, int pv_stride, int h0, int hc,
                                            size_t loff, float inv_count) {
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, HT = q.HT;
  const size_t row_floats = (size_t)n * p.H;
  float* e0 = r.gp;
  float* e1 = e0 + row_floats;   // (= r.gsd)
  float* e2 = e1 + row_floats;   // (= r.gu)
  int* below = reinterpret_cast<int*>(slab + kMetricSums * HT);
  for (int pass = 0; pass < 3; ++pass) {
    const int nt = pass < 2 ? 3 : 2;
    for (int i = tid; i < n * hc; i += kThreads) {
      const int x = i / hc, hh = i - x * hc, h = h0 + hh;
      const size_t li = loff + (size_t)x * HT + h;
      const float pvv = pv[(size_t)x * pv_stride + hh];
      const float lv = p.labels[li], bv = p.baseline[li];
      const float diff = lv - pvv, base = lv - bv;
      if (pass == 0) {
        const HeadTerms t = head_terms_of<false, true>(p, q.floor, q.coef_abs, q.coef_rel, HT, h,
                                                       pvv, lv, bv, inv_count);
        e0[i] = t.abs_error;
        e1[i] = t.rel_error;
        e2[i] = fabsf(diff);
      } else if (pass == 1) {
        e0[i] = fabsf(base);
        e1[i] = diff * diff;
        e2[i] = base * base;
      } else {
        e0[i] = logf(fmaxf(fabsf(diff), 1e-8f)) - logf(fmaxf(fabsf(base), 1e-8f));
        const float d2 = diff * diff, b2 = base * base;
        e1[i] = d2 < b2 ? 1.0f : 0.0f;
      }
    }
    __syncthreads();
    if (tid < nt * hc) {   // per-(term, head) sums over the sample's points, in point order
      const int k = tid / hc, hh = tid - k * hc, term = 3 * pass + k;
      const float* e = e0 + (size_t)k * row_floats;
      if (term < kMetricSums) {
        float acc = 0.0f;
        for (int x = 0; x < n; ++x) acc += e[(size_t)x * hc + hh];
        slab[term * HT + h0 + hh] += acc;
      } else {
        int count = 0;
        for (int x = 0; x < n; ++x) count += e[(size_t)x * hc + hh] != 0.0f ? 1 : 0;
        below[h0 + hh] += count;
      }
    }
    __syncthreads();
  }
}

}  // namespace

// kThroughTime false: one evaluation per sample (q.T = 0, the forward pass of
// loss_grad_body); true: the forward sweep of unrolled_loss_grad_body, evaluations
// 0 .. 2 T - 1, in its arithmetic.  Always a replica grid (blockIdx.y).
template <bool kThroughTime>
__device__ __forceinline__ void metrics_body(const UnrolledParams& q) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const TrainParams& p = q.t;
  const int tid = threadIdx.x, n = p.N, H = p.H, D = p.D;
  const int T = kThroughTime ? q.T : 0, HT = q.HT, E = kThroughTime ? 2 * T : 1;
  const Rows r = carve_rows(p, smem, kThroughTime);
  float* slab = p.ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * p.slab_stride;
  float* zs = slab + p.n_slab;
  float* st = slab + q.st_off;   // [E][N] stage states (through time)
  int* flag = reinterpret_cast<int*>(slab + kMetricTerms * HT);
  float* predictions =
      p.predictions != nullptr ? p.predictions + (size_t)blockIdx.y * p.batch * n * HT : nullptr;
  const float inv_count = 1.0f / ((float)p.batch * (float)n);
  const float dt = q.dt, half_dt = 0.5f * q.dt;

  stage_workgroup<true>(p, slab, p.n_slab, r.wl);

  for (int s = blockIdx.x; s < p.batch; s += gridDim.x) {
    const int* index = p.sample_index + (size_t)blockIdx.y * p.index_stride;
    const int row = p.sample_index != nullptr ? index[s] : s;
    const size_t poff = (size_t)s * n * HT;
    if (row < 0 || row >= p.rows) {
      // an index outside [0, rows): no input read; the replica's sums and this sample's
      // predictions row become NaN, its counts -1 (the flag, metrics_sum_kernel)
      const float nan = __int_as_float(0x7fc00000);
      if (tid < kMetricSums * HT) slab[tid] = nan;
      if (tid == 0) *flag = 1;
      if (predictions != nullptr)
        for (int i = tid; i < n * HT; i += kThreads) predictions[poff + i] = nan;
      __syncthreads();   // (the sums are added to by other threads than wrote the NaNs)
      continue;          // (block-uniform)
    }
    const size_t loff = (size_t)row * n * HT;
    if (kThroughTime) {
      for (int i = tid; i < n; i += kThreads) st[i] = p.y[(size_t)row * n + i];
      __syncthreads();
    }
    for (int e = 0; e < E; ++e) {
      const int step = e >> 1;
      const bool mid = (e & 1) != 0;
      for (int i = tid; i < n; i += kThreads) {
        const float v = kThroughTime ? st[(size_t)e * n + i] : p.y[(size_t)row * n + i];
        r.u[i] = v;
        r.buf0[i] = v / p.stddev;
      }
      __syncthreads();
      float* cur = r.buf0;
      float* nxt = r.buf1;
      forward_sample<true>(p, r.wl, zs, r.u, r.gfl, r.pred, cur, nxt);
      if (e == 0) {
        // ---- the D + 1 heads of one evaluation
        if (predictions != nullptr)
          for (int i = tid; i < n * H; i += kThreads) {
            const int x = i / H, h = i - x * H;
            predictions[poff + (size_t)x * HT + h] = r.pred[i];
          }
        metric_sums(q, r, slab, r.pred, H, 0, H, loff, inv_count);
      }
      if (!kThroughTime) continue;
      if (!mid) {
        for (int x = tid; x < n; x += kThreads)
          st[(size_t)(e + 1) * n + x] = r.u[x] + half_dt * r.pred[(size_t)x * H + D];
      } else {
        // ---- y_{step + 1} = y_step + dt k2: the next stage state and head D + 1 + step
        const int h = H + step;
        for (int x = tid; x < n; x += kThreads) {
          const float y_new = st[(size_t)(e - 1) * n + x] + dt * r.pred[(size_t)x * H + D];
          if (step + 1 < T) st[(size_t)(e + 1) * n + x] = y_new;
          r.gdy[x] = y_new;
          if (predictions != nullptr) predictions[poff + (size_t)x * HT + h] = y_new;
        }
        __syncthreads();
        metric_sums(q, r, slab, r.gdy, 1, h, 1, loff, inv_count);
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kThreads) void metrics_kernel(UnrolledParams q) {
  metrics_body<false>(q);
}

__global__ __launch_bounds__(kThreads) void metrics_unrolled_kernel(UnrolledParams q) {
  metrics_body<true>(q);
}

static_assert(kMetricTerms * kMaxUnrolledHeads <= kThreads,
              "metrics_sum_kernel / the NaN rows: one thread per (term, head)");

// Workgroup r sums replica r's slabs in workgroup order: sums[r][term][h], the two loss rows
// over `count` = batch N as slab_sum_kernel (train.hip) forms head_means, and below[r][h],
// or -1 where a workgroup of the replica met an index out of range.
__global__ __launch_bounds__(kThreads) void metrics_sum_kernel(const float* ws, size_t stride,
                                                               int blocks, int heads, float count,
                                                               float* sums, int* below) {
  const size_t r = blockIdx.x;
  ws += r * (size_t)blocks * stride;
  const int i = threadIdx.x;
  if (i < kMetricSums * heads) {
    float acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += ws[(size_t)b * stride + i];
    sums[r * (size_t)(kMetricSums * heads) + i] = i < 2 * heads ? acc / count : acc;
  } else if (i < kMetricTerms * heads) {
    const int h = i - kMetricSums * heads;
    int acc = 0;
    bool poisoned = false;
    for (int b = 0; b < blocks; ++b) {
      const int* slab = reinterpret_cast<const int*>(ws + (size_t)b * stride);
      acc += slab[kMetricSums * heads + h];
      poisoned = poisoned || slab[kMetricTerms * heads] != 0;
    }
    below[r * (size_t)heads + h] = poisoned ? -1 : acc;
  }
}

hipError_t launch_eval_metrics(const MetricsParams& m, hipStream_t stream) {
  UnrolledParams q = m.q;
  const TrainParams& p = q.t;
  const void* kernel = q.T > 0 ? reinterpret_cast<const void*>(metrics_unrolled_kernel)
                               : reinterpret_cast<const void*>(metrics_kernel);
  hipError_t err = set_dynamic_lds(kernel, m.lds_bytes);
  if (err != hipSuccess) return err;
  void* args[] = {&q};
  err = hipLaunchKernel(kernel, dim3(m.blocks, m.replicas), dim3(kThreads), args, m.lds_bytes,
                        stream);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(metrics_sum_kernel, dim3(m.replicas), dim3(kThreads), 0, stream, p.ws,
                     p.slab_stride, m.blocks, q.HT, (float)p.batch * (float)p.N, m.sums, m.below);
  return hipGetLastError();
}

}  // namespace train
}  // namespace ddd
