// The device code and launcher of ddd_train_run and ddd_train_population_run
// (train_population.h): the four loss kernels with a replica dimension,
// slab_adam_population_kernel (the slab sum with the optimiser folded in),
// slab_heads_population_kernel, clip_population_kernel (error_max decided on the device)
// and the host loop that enqueues the steps.
#include <hip/hip_runtime.h>

#include <cmath>

#include "train_body.h"
#include "train_population.h"
#include "train_unrolled_body.h"

namespace ddd {
namespace train {

// The bodies of loss_grad_kernel / unrolled_loss_grad_kernel with kReplicas
// (train_device.h: weights_of): workgroup (b, r) is workgroup b of gridDim.x on replica r's
// weights, slabs, index and table.  The parameter struct is replica 0's and is read from
// the kernel arguments as it is.  The *_table_* twins read the loss constants from
// p.coef_table instead of the host values.
__global__ __launch_bounds__(kThreads) void loss_grad_population_kernel(TrainParams p) {
  loss_grad_body<false, true>(p);
}

__global__ __launch_bounds__(kThreads) void loss_grad_table_population_kernel(TrainParams p) {
  loss_grad_body<true, true>(p);
}

__global__ __launch_bounds__(kThreads) void unrolled_loss_grad_population_kernel(
    UnrolledParams q) {
  unrolled_loss_grad_body<false, true>(q);
}

__global__ __launch_bounds__(kThreads) void unrolled_loss_grad_table_population_kernel(
    UnrolledParams q) {
  unrolled_loss_grad_body<true, true>(q);
}

struct AdamPopulationStep {
  const float* ws;         // [R][blocks][stride] the loss kernels' slabs
  size_t stride;
  int blocks, n_weights, total;   // total = n_weights + 2 heads
  float count;             // batch N
  float* weights;          // [R][n_weights], updated in place
  float* m;
  float* v;
  float* last_grad;        // [R][n_weights] or null
  float* head_means;       // [R][2][heads]: the step's rows of the log
  float one_minus_beta1, beta2, one_minus_beta2, eps;
  float bias2_sqrt;        // sqrt(1 - beta2^t), shared: t is
  float step_size[kMaxReplicas];   // lr[r] / (1 - beta1^t)
};

// slab_sum_kernel's sum (train.hip: same order, same arithmetic) on replica blockIdx.y,
// then per index: Adam on the thread's weight, or the head mean to the log.  Plain vector
// loads and stores.
__global__ __launch_bounds__(kThreads) void slab_adam_population_kernel(AdamPopulationStep a) {
  const size_t r = blockIdx.y;
  const float* ws = a.ws + r * (size_t)a.blocks * a.stride;
  const size_t w0 = r * (size_t)a.n_weights;
  float* head_means = a.head_means + r * (size_t)(a.total - a.n_weights);
  const float step_size = a.step_size[r];
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < a.total; i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < a.blocks; ++b) acc += ws[(size_t)b * a.stride + i];
    if (i >= a.n_weights) {
      head_means[i - a.n_weights] = acc / a.count;
      continue;
    }
    const float g = acc;
    if (a.last_grad != nullptr) a.last_grad[w0 + i] = g;
    float m = a.m[w0 + i];
    m = m + (g - m) * a.one_minus_beta1;
    const float v = a.beta2 * a.v[w0 + i] + a.one_minus_beta2 * (g * g);
    const float denom = sqrtf(v) / a.bias2_sqrt + a.eps;
    a.m[w0 + i] = m;
    a.v[w0 + i] = v;
    a.weights[w0 + i] = a.weights[w0 + i] - step_size * (m / denom);
  }
}

// The head part of slab_sum_kernel (train.hip) on replica blockIdx.y, behind the
// forward-only pass: head_means[r][i - n_weights] = the slabs' sum, in workgroup order,
// over count, for n_weights <= i < total
__global__ __launch_bounds__(kThreads) void slab_heads_population_kernel(
    const float* ws, size_t stride, int blocks, int n_weights, int total, float* head_means,
    float count) {
  const size_t r = blockIdx.y;
  ws += r * (size_t)blocks * stride;
  head_means += r * (size_t)(total - n_weights);
  for (int i = n_weights + blockIdx.x * kThreads + threadIdx.x; i < total;
       i += gridDim.x * kThreads) {
    float acc = 0.0f;
    for (int b = 0; b < blocks; ++b) acc += ws[(size_t)b * stride + i];
    head_means[i - n_weights] = acc / count;
  }
}

struct ClipPopulation {
  int heads;
  double error_max;
  double scale_abs[kMaxUnrolledHeads], scale_rel[kMaxUnrolledHeads];
  float floor[kMaxUnrolledHeads], coef_abs[kMaxUnrolledHeads], coef_rel[kMaxUnrolledHeads];
  const float* head_means; // [R][2][heads] of the forward-only pass
  float* table;            // [R][3][heads]: floor, coef_abs, coef_rel
};

// Trainer.loss_and_grad's host decision (training.py), in its arithmetic: a term whose
// scaled mean (double) reaches error_max passes no gradient, so its coefficient is zero.
// Workgroup r on replica r's means and table: the replicas clip independently.
__global__ __launch_bounds__(64) void clip_population_kernel(ClipPopulation c) {
  const int i = threadIdx.x, H = c.heads;
  const float* head_means = c.head_means + (size_t)blockIdx.x * (2 * H);
  float* table = c.table + (size_t)blockIdx.x * (3 * H);
  if (i < H) table[i] = c.floor[i];
  if (i < 2 * H) {
    const bool rel = i >= H;
    const int h = rel ? i - H : i;
    const double scaled = (double)head_means[i] * (rel ? c.scale_rel[h] : c.scale_abs[h]);
    const float coef = rel ? c.coef_rel[h] : c.coef_abs[h];
    table[H + i] = scaled >= c.error_max ? 0.0f : coef;
  }
}

static_assert(2 * kMaxUnrolledHeads <= 64, "clip_population_kernel: one thread per (term, head)");

namespace {

const void* population_loss_kernel(bool through_time, bool coef_table) {
  if (through_time)
    return coef_table
               ? reinterpret_cast<const void*>(unrolled_loss_grad_table_population_kernel)
               : reinterpret_cast<const void*>(unrolled_loss_grad_population_kernel);
  return coef_table ? reinterpret_cast<const void*>(loss_grad_table_population_kernel)
                    : reinterpret_cast<const void*>(loss_grad_population_kernel);
}

}  // namespace

hipError_t launch_train_population(const PopulationParams& pp, hipStream_t stream) {
  const RunParams& r = pp.r;
  const int R = pp.replicas;
  UnrolledParams q = r.q;
  TrainParams& p = q.t;
  const bool through_time = q.T > 0;
  const bool clip = r.error_max > 0.0;
  const int total = p.n_weights + 2 * r.heads;
  p.index_stride = pp.index_per_replica ? p.batch : 0;
  void* args[] = {through_time ? static_cast<void*>(&q) : static_cast<void*>(&p)};
  const void* kernel = population_loss_kernel(through_time, clip);
  // (with clipping: the forward-only pass runs the kernel of the host values)
  const void* forward = population_loss_kernel(through_time, false);
  // the dynamic-LDS attribute once per kernel, not once per step
  hipError_t err = set_dynamic_lds(kernel, r.lds_bytes);
  if (err == hipSuccess && clip) err = set_dynamic_lds(forward, r.lds_bytes);
  if (err != hipSuccess) return err;

  AdamPopulationStep a;
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
  for (int i = 0; i < kMaxReplicas; ++i) a.step_size[i] = 0.0f;

  ClipPopulation c;
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

  const dim3 loss_grid(r.blocks, R);
  const dim3 sum_grid((total + kThreads - 1) / kThreads, R);
  const size_t index_rows = pp.index_per_replica ? (size_t)R : 1;
  p.grad = nullptr;
  p.head_means = nullptr;   // (the loss kernels write slabs; the sums below write the log)
  for (int k = 0; k < r.num_steps; ++k) {
    float* rows = r.head_means_log + (size_t)k * R * 2 * r.heads;
    p.sample_index = r.sample_index + (size_t)k * index_rows * p.batch;
    if (clip) {
      // forward only on the host values, the head means to the log rows, the tables from them
      p.want_grad = 0;
      p.coef_table = nullptr;
      err = hipLaunchKernel(forward, loss_grid, dim3(kThreads), args, r.lds_bytes, stream);
      if (err != hipSuccess) return err;
      hipLaunchKernelGGL(slab_heads_population_kernel, dim3(1, R), dim3(kThreads), 0, stream,
                         p.ws, p.slab_stride, r.blocks, p.n_weights, total, rows, a.count);
      err = hipGetLastError();
      if (err != hipSuccess) return err;
      c.head_means = rows;
      hipLaunchKernelGGL(clip_population_kernel, dim3(R), dim3(64), 0, stream, c);
      err = hipGetLastError();
      if (err != hipSuccess) return err;
      p.coef_table = r.coef_table;
    }
    p.want_grad = 1;
    err = hipLaunchKernel(kernel, loss_grid, dim3(kThreads), args, r.lds_bytes, stream);
    if (err != hipSuccess) return err;
    const double t = (double)r.first_step + k + 1;
    const double bias1 = 1.0 - std::pow(r.beta1, t);
    for (int i = 0; i < R; ++i)
      a.step_size[i] = (float)(r.learning_rate[(size_t)i * r.num_steps + k] / bias1);
    a.bias2_sqrt = (float)std::sqrt(1.0 - std::pow(r.beta2, t));
    a.head_means = rows;
    hipLaunchKernelGGL(slab_adam_population_kernel, sum_grid, dim3(kThreads), 0, stream, a);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace train
}  // namespace ddd
