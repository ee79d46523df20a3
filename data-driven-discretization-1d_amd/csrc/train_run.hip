// ddd_train_run's device code and launcher (train_run.h): slab_adam_kernel, the slab sum
// with the optimiser folded in; clip_kernel, error_max decided on the device; and the
// host loop that enqueues the steps.
#include <hip/hip_runtime.h>

#include <cmath>

#include "train_run.h"

namespace ddd {
namespace train {

struct AdamStep {
  const float* ws;         // [blocks][stride] the loss kernel's slabs
  size_t stride;
  int blocks, n_weights, total;   // total = n_weights + 2 heads
  float count;             // batch N
  float* weights;          // [n_weights], updated in place
  float* m;
  float* v;
  float* last_grad;        // [n_weights] or null
  float* head_means;       // [2][heads]: the step's row of the log
  float one_minus_beta1, beta2, one_minus_beta2, eps;
  float step_size;         // lr / (1 - beta1^t)
  float bias2_sqrt;        // sqrt(1 - beta2^t)
};

// slab_sum_kernel's sum (train.hip: same order, same arithmetic), then per index: Adam
// on the thread's weight, or the head mean to the log.  Plain vector loads and stores.
__global__ __launch_bounds__(kThreads) void slab_adam_kernel(AdamStep a) {
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < a.total; i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < a.blocks; ++b) acc += a.ws[(size_t)b * a.stride + i];
    if (i >= a.n_weights) {
      a.head_means[i - a.n_weights] = acc / a.count;
      continue;
    }
    const float g = acc;
    if (a.last_grad != nullptr) a.last_grad[i] = g;
    float m = a.m[i];
    m = m + (g - m) * a.one_minus_beta1;
    const float v = a.beta2 * a.v[i] + a.one_minus_beta2 * (g * g);
    const float denom = sqrtf(v) / a.bias2_sqrt + a.eps;
    a.m[i] = m;
    a.v[i] = v;
    a.weights[i] = a.weights[i] - a.step_size * (m / denom);
  }
}

struct ClipParams {
  int heads;
  double error_max;
  double scale_abs[kMaxUnrolledHeads], scale_rel[kMaxUnrolledHeads];
  float floor[kMaxUnrolledHeads], coef_abs[kMaxUnrolledHeads], coef_rel[kMaxUnrolledHeads];
  const float* head_means; // [2][heads] of the forward-only pass
  float* table;            // [3][heads]: floor, coef_abs, coef_rel
};

// Trainer.loss_and_grad's host decision (training.py), in its arithmetic: a term whose
// scaled mean (double) reaches error_max passes no gradient, so its coefficient is zero.
__global__ __launch_bounds__(64) void clip_kernel(ClipParams c) {
  const int i = threadIdx.x, H = c.heads;
  if (i < H) c.table[i] = c.floor[i];
  if (i < 2 * H) {
    const bool rel = i >= H;
    const int h = rel ? i - H : i;
    const double scaled = (double)c.head_means[i] * (rel ? c.scale_rel[h] : c.scale_abs[h]);
    const float coef = rel ? c.coef_rel[h] : c.coef_abs[h];
    c.table[H + i] = scaled >= c.error_max ? 0.0f : coef;
  }
}

static_assert(2 * kMaxUnrolledHeads <= 64, "clip_kernel: one thread per (term, head)");

hipError_t launch_train_run(const RunParams& r, hipStream_t stream) {
  UnrolledParams q = r.q;
  TrainParams& p = q.t;
  const bool through_time = q.T > 0;
  const bool clip = r.error_max > 0.0;
  const int total = p.n_weights + 2 * r.heads;
  const void* params = through_time ? static_cast<const void*>(&q) : static_cast<const void*>(&p);
  const void* kernel = through_time ? unrolled_loss_grad_kernel_entry(clip)
                                    : loss_grad_kernel_entry(clip);
  // (with clipping: the forward-only pass runs the kernel of the host values)
  const void* forward = through_time ? unrolled_loss_grad_kernel_entry(false)
                                     : loss_grad_kernel_entry(false);
  // the dynamic-LDS attribute once per kernel, not once per step
  hipError_t err = set_dynamic_lds(kernel, r.lds_bytes);
  if (err == hipSuccess && clip) err = set_dynamic_lds(forward, r.lds_bytes);
  if (err != hipSuccess) return err;

  AdamStep a;
  a.ws = p.ws;
  a.stride = p.slab_stride;
  a.blocks = r.blocks;
  a.n_weights = p.n_weights;
  a.total = total;
  a.count = (float)p.batch * (float)p.N;
  a.weights = r.weights;
  a.m = r.adam_m;
  a.v = r.adam_v;
  a.last_grad = r.last_grad;
  a.one_minus_beta1 = (float)(1.0 - r.beta1);
  a.beta2 = (float)r.beta2;
  a.one_minus_beta2 = (float)(1.0 - r.beta2);
  a.eps = (float)r.epsilon;

  ClipParams c;
  c.heads = r.heads;
  c.error_max = r.error_max;
  for (int h = 0; h < kMaxUnrolledHeads; ++h) {
    c.scale_abs[h] = r.scale_abs[h];
    c.scale_rel[h] = r.scale_rel[h];
    c.floor[h] = r.floor[h];
    c.coef_abs[h] = r.coef_abs[h];
    c.coef_rel[h] = r.coef_rel[h];
  }
  c.table = r.coef_table;

  const int grid = (total + kThreads - 1) / kThreads;
  for (int k = 0; k < r.num_steps; ++k) {
    float* row = r.head_means_log + (size_t)k * 2 * r.heads;
    p.sample_index = r.sample_index + (size_t)k * p.batch;
    p.grad = nullptr;
    p.head_means = row;
    if (clip) {
      // forward only on the host values, the head means to the log row, the table from them
      p.want_grad = 0;
      p.coef_table = nullptr;
      err = launch_prepared_then_sum(forward, params, p, r.blocks, r.lds_bytes, stream,
                                     p.n_weights, total);
      if (err != hipSuccess) return err;
      c.head_means = row;
      hipLaunchKernelGGL(clip_kernel, dim3(1), dim3(64), 0, stream, c);
      err = hipGetLastError();
      if (err != hipSuccess) return err;
      p.coef_table = r.coef_table;
    }
    p.want_grad = 1;
    // (an empty index range: the kernel alone; slab_adam_kernel is its sum)
    err = launch_prepared_then_sum(kernel, params, p, r.blocks, r.lds_bytes, stream, total,
                                   total);
    if (err != hipSuccess) return err;
    const double t = (double)r.first_step + k + 1;
    a.step_size = (float)(r.learning_rate[k] / (1.0 - std::pow(r.beta1, t)));
    a.bias2_sqrt = (float)std::sqrt(1.0 - std::pow(r.beta2, t));
    a.head_means = row;
    hipLaunchKernelGGL(slab_adam_kernel, dim3(grid), dim3(kThreads), 0, stream, a);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace train
}  // namespace ddd
