// The device code and launcher of ddd_train_rollout_run (train_rollout_population.h): the
// rollout loss kernel with a replica dimension, the slab sum that also forms the partial
// sums of g^2, the per-replica decision (norm, skip, clip factor, Adam's step count and
// bias corrections) and the Adam update, and the host loop that enqueues the steps.
#include <hip/hip_runtime.h>

#include <cmath>

#include "train_rollout_body.h"
#include "train_rollout_population.h"

namespace ddd {
namespace train {

// The body of rollout_loss_grad_kernel with kReplicas (train_device.h: weights_of):
// workgroup (b, r) is workgroup b of gridDim.x on replica r's weights, slabs and index.  The
// parameter struct is replica 0's and is read from the kernel arguments as it is.
__global__ __launch_bounds__(kThreads) void rollout_loss_grad_population_kernel(
    RolloutParams q) {
  rollout_loss_grad_body<true>(q);
}

struct RolloutSlabSum {
  const float* ws;         // [R][blocks][stride] the loss kernel's slabs
  size_t stride;
  int blocks, first, n_weights, total;   // indices [first, total); total = n_weights + n_saved
  float count;             // batch N
  float* grad_buf;         // [R][n_weights]
  float* last_grad;        // [R][n_weights] or null
  float* step_means;       // [R][n_saved]: the step's rows of the log
  double* partials;        // [R][gridDim.x] or null (first >= n_weights)
};

// The sum of 256 doubles in a fixed order (rk23.h: block_sum256): butterflies within a
// wavefront, then the four wavefronts in order
__device__ __forceinline__ double square_sum256(double v, double* red) {
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// slab_sum_kernel's sum (train.hip: same order, same arithmetic) on replica blockIdx.y, one
// slab index per thread: the gradient to the buffer, the step mean to the log, and the
// workgroup's sum of g^2 in float64.  Plain vector loads and stores.
__global__ __launch_bounds__(kThreads) void rollout_slab_sum_population_kernel(
    RolloutSlabSum a) {
  __shared__ double red[kThreads / 64];
  const size_t r = blockIdx.y;
  const float* ws = a.ws + r * (size_t)a.blocks * a.stride;
  const int i = a.first + blockIdx.x * kThreads + threadIdx.x;
  double square = 0.0;
  if (i < a.total) {
    float acc = 0.0f;
    for (int b = 0; b < a.blocks; ++b) acc += ws[(size_t)b * a.stride + i];
    if (i < a.n_weights) {
      const size_t at = r * (size_t)a.n_weights + i;
      a.grad_buf[at] = acc;
      if (a.last_grad != nullptr) a.last_grad[at] = acc;
      square = (double)acc * (double)acc;
    } else {
      a.step_means[r * (size_t)(a.total - a.n_weights) + (i - a.n_weights)] = acc / a.count;
    }
  }
  if (a.partials == nullptr) return;   // (uniform)
  const double sum = square_sum256(square, red);
  if (threadIdx.x == 0) a.partials[r * gridDim.x + blockIdx.x] = sum;
}

struct RolloutDecide {
  const double* partials;  // [R][sum_blocks]
  int sum_blocks;
  double clip_norm, beta1, beta2;
  int* adam_step;          // [R]
  float* grad_norm;        // [R]: the step's row of the log
  RolloutDecision* decisions;   // [R]
  double learning_rate[kMaxReplicas];   // the step's rate of every replica
};

// Workgroup r decides replica r's step: RolloutTrainer.step's host decision
// (training.py), with the norm, the clip factor and the bias corrections in double.
__global__ __launch_bounds__(64) void rollout_decide_population_kernel(RolloutDecide d) {
  if (threadIdx.x != 0) return;
  const int r = blockIdx.x;
  const double* partials = d.partials + (size_t)r * d.sum_blocks;
  double sum = 0.0;
  for (int b = 0; b < d.sum_blocks; ++b) sum += partials[b];
  const double norm = sqrt(sum);
  const float norm32 = (float)norm;
  d.grad_norm[r] = norm32;
  RolloutDecision out;
  out.skip = 1;
  out.scale = 0.0f;
  out.step_size = 0.0f;
  out.bias2_sqrt = 1.0f;
  if (isfinite(norm32)) {
    double scale = 1.0;
    if (d.clip_norm > 0.0) scale = fmin(1.0, d.clip_norm / (norm + 1e-12));
    const int t = d.adam_step[r] + 1;
    d.adam_step[r] = t;
    out.skip = 0;
    out.scale = (float)scale;
    out.step_size = (float)(d.learning_rate[r] / (1.0 - pow(d.beta1, (double)t)));
    out.bias2_sqrt = (float)sqrt(1.0 - pow(d.beta2, (double)t));
  }
  d.decisions[r] = out;
}

struct RolloutAdam {
  const float* grad_buf;   // [R][n_weights]
  const RolloutDecision* decisions;   // [R]
  int n_weights;
  float* weights;          // [R][n_weights], updated in place
  float* m;
  float* v;
  float one_minus_beta1, beta2, one_minus_beta2, eps;
};

// slab_adam_population_kernel's update (train_population.hip: its four statements, in their
// order, in float32) of replica blockIdx.y from the clipped gradient, or nothing at all for
// a skipped replica
__global__ __launch_bounds__(kThreads) void rollout_adam_population_kernel(RolloutAdam a) {
  const size_t r = blockIdx.y;
  const RolloutDecision d = a.decisions[r];
  if (d.skip) return;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n_weights) return;
  const size_t at = r * (size_t)a.n_weights + i;
  const float g = a.grad_buf[at] * d.scale;
  float m = a.m[at];
  m = m + (g - m) * a.one_minus_beta1;
  const float v = a.beta2 * a.v[at] + a.one_minus_beta2 * (g * g);
  const float denom = sqrtf(v) / d.bias2_sqrt + a.eps;
  a.m[at] = m;
  a.v[at] = v;
  a.weights[at] = a.weights[at] - d.step_size * (m / denom);
}

hipError_t launch_train_rollout_run(const RolloutRunParams& rr, hipStream_t stream) {
  const int R = rr.replicas;
  RolloutParams q = rr.q;
  TrainParams& p = q.t;
  const void* kernel = reinterpret_cast<const void*>(rollout_loss_grad_population_kernel);
  hipError_t err = set_dynamic_lds(kernel, rr.lds_bytes);
  if (err != hipSuccess) return err;
  void* args[] = {static_cast<void*>(&q)};
  const int total = p.n_weights + q.n_saved;
  const dim3 loss_grid(rr.blocks, R);
  p.index_stride = rr.index_per_replica && rr.sample_index != nullptr ? p.batch : 0;
  p.grad = nullptr;
  p.head_means = nullptr;   // (the loss kernel writes slabs; the sum below writes the log)
  q.trajectory = nullptr;

  RolloutSlabSum s;
  s.ws = p.ws;
  s.stride = p.slab_stride;
  s.blocks = rr.blocks;
  s.n_weights = p.n_weights;
  s.total = total;
  s.count = (float)p.batch * (float)p.N;
  s.grad_buf = rr.grad_buf;
  s.last_grad = rr.last_grad;

  if (rr.forward_only) {
    p.want_grad = 0;
    p.sample_index = rr.sample_index;
    err = hipLaunchKernel(kernel, loss_grid, dim3(kThreads), args, rr.lds_bytes, stream);
    if (err != hipSuccess) return err;
    s.first = p.n_weights;
    s.partials = nullptr;
    s.step_means = rr.step_means_log;
    hipLaunchKernelGGL(rollout_slab_sum_population_kernel,
                       dim3((q.n_saved + kThreads - 1) / kThreads, R), dim3(kThreads), 0, stream,
                       s);
    return hipGetLastError();
  }

  const int sum_blocks = rollout_sum_blocks(p.n_weights, q.n_saved);
  s.first = 0;
  s.partials = rr.partials;

  RolloutDecide d;
  d.partials = rr.partials;
  d.sum_blocks = sum_blocks;
  d.clip_norm = rr.clip_norm;
  d.beta1 = rr.beta1;
  d.beta2 = rr.beta2;
  d.adam_step = rr.adam_step;
  d.decisions = rr.decisions;
  for (int i = 0; i < kMaxReplicas; ++i) d.learning_rate[i] = 0.0;

  RolloutAdam a;
  a.grad_buf = rr.grad_buf;
  a.decisions = rr.decisions;
  a.n_weights = p.n_weights;
  a.weights = rr.weights;
  a.m = rr.adam_m;
  a.v = rr.adam_v;
  a.one_minus_beta1 = (float)(1.0 - rr.beta1);
  a.beta2 = (float)rr.beta2;
  a.one_minus_beta2 = (float)(1.0 - rr.beta2);
  a.eps = (float)rr.epsilon;

  const size_t index_rows = rr.index_per_replica ? (size_t)R : 1;
  const dim3 adam_grid((p.n_weights + kThreads - 1) / kThreads, R);
  p.want_grad = 1;
  for (int k = 0; k < rr.num_opt_steps; ++k) {
    p.sample_index = rr.sample_index + (size_t)k * index_rows * p.batch;
    err = hipLaunchKernel(kernel, loss_grid, dim3(kThreads), args, rr.lds_bytes, stream);
    if (err != hipSuccess) return err;
    s.step_means = rr.step_means_log + (size_t)k * R * q.n_saved;
    hipLaunchKernelGGL(rollout_slab_sum_population_kernel, dim3(sum_blocks, R), dim3(kThreads),
                       0, stream, s);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    for (int i = 0; i < R; ++i)
      d.learning_rate[i] = rr.learning_rate[(size_t)i * rr.num_opt_steps + k];
    d.grad_norm = rr.grad_norm_log + (size_t)k * R;
    hipLaunchKernelGGL(rollout_decide_population_kernel, dim3(R), dim3(64), 0, stream, d);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(rollout_adam_population_kernel, adam_grid, dim3(kThreads), 0, stream, a);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
  }
  return hipSuccess;
}

}  // namespace train
}  // namespace ddd
