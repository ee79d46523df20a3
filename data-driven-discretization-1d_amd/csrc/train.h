// Training: the loss of model.py:704-810 and its gradient with respect to the conv
// weights, for one minibatch, fused into one kernel (ddd_train_loss_grad, include/ddd1d.h).
// This header carries the kernel parameters and the host-side launchers; the kernel is in
// train.hip, the device code it shares with vjp.hip and train_unrolled.hip in
// train_device.h.
//
// One workgroup walks over samples s = blockIdx.x, blockIdx.x + gridDim.x, ... and, per
// sample, recomputes the forward pass (input scaling, the periodic conv tower, the
// projection, the stencils and the equation of motion), forms the elementwise loss
// cotangent and runs the backward pass down to the conv weights.  The weight gradient of
// every sample the workgroup owns is added, in sample order, into the workgroup's own
// partial slab of the caller's workspace; slab_sum_kernel then sums the slabs in workgroup
// order.  No atomics anywhere: equal inputs give equal bits.
//
// The pre-activations of the hidden layers go to the slab's scratch part (global memory,
// L2-resident at these sizes); the backward pass re-forms the layer inputs from them.
//
// Layers with 32 input and 32 output channels (the hidden layers of the default net) run
// their three GEMMs -- forward, backward-data, weight gradient -- on v_mfma_f32_32x32x2_f32
// (exact float32 products) when N is a multiple of 32; their kernels are copied into LDS
// once at kernel start.  Every other layer, and every net when the staged weights do not
// fit, runs on the VALU (fmaf chains over 256 threads).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dev_params.h"

namespace ddd {
namespace train {

constexpr int kThreads = 256;
constexpr int kMaxHeads = kMaxDerivs + 1;
constexpr int kMaxBlocks = 512;   // workgroups (= partial slabs) of a call: min(batch, this)

struct TrainParams {
  int equation, N, D, G, H, target, L, K, act, C_out, pao, unbiased, conservative;
  int cmax;        // widest activation row (max over layers of cin, cout)
  float eta, stddev, inv_dx;
  int in_start[kMaxDerivs], in_size[kMaxDerivs], ns_off[kMaxDerivs];
  int w_off[kMaxLayers], cin[kMaxLayers], cout[kMaxLayers], z_off[kMaxLayers];
  int mfma;        // 1: the 32 -> 32 layers on MFMA with their kernels staged in LDS
  int wl_off[kMaxLayers];   // LDS offset (floats, behind lds_floats) of layer l's staged
                            // kernel [K][32][32], or -1 (VALU layer)
  int wl_floats;   // floats of all staged kernels
  int n_weights;   // floats of the weight vector (kernels and biases of every layer)
  int n_slab;      // floats of a slab's gradient + head part (n_weights + 2 H, padded)
  size_t slab_stride;   // floats per workgroup: n_slab + the hidden layers' pre-activations
  const float* weights;    // [K][cin][cout] then bias [cout], per layer
  const float* nullspace;  // per derivative [in_size][G]
  const float* bias;       // [D][G]
  const float* y;          // [rows][N]
  const int* sample_index; // [batch] or null (rows 0 .. batch-1)
  int rows, batch;
  const float* labels;     // [rows][N][H]
  const float* baseline;   // [rows][N][H]
  float floor[kMaxHeads], coef_abs[kMaxHeads], coef_rel[kMaxHeads];
  float* predictions;      // [batch][N][H] or null
  float* ws;               // [blocks][slab_stride]
  int want_grad;
  int index_stride;        // entries between two replicas' rows of sample_index (population
                           // kernels, train_population.h: batch or 0); elsewhere not read
  float* grad;             // [n_weights] or null
  float* head_means;       // [2][H]
  const float* coef_table; // device [3][heads]: floor, coef_abs, coef_rel, read instead of the
                           // host values by the kernels built for it (train_population.h),
                           // or null
};

static_assert(offsetof(TrainParams, grad) == offsetof(TrainParams, index_stride) + 4 &&
                  offsetof(TrainParams, index_stride) == offsetof(TrainParams, want_grad) + 4,
              "index_stride fills the padding behind want_grad");

// The LDS plan of a workgroup (train_device.h: Rows): rows of [N] (the state, the
// time-derivative cotangent, the flux), of [N][H] (predictions, their cotangent, the two
// error-term rows) and of [N][cmax] (two activation buffers)
constexpr int kLdsRowsN = 3, kLdsRowsNH = 4, kLdsRowsNC = 2;
__host__ __device__ inline size_t lds_floats(const TrainParams& p) {
  return kLdsRowsN * (size_t)p.N + kLdsRowsNH * (size_t)p.N * p.H +
         kLdsRowsNC * (size_t)p.N * p.cmax;
}
// ... plus the staged 32 x 32 kernels of the MFMA layers
__host__ __device__ inline size_t lds_total_floats(const TrainParams& p) {
  return lds_floats(p) + (size_t)p.wl_floats;
}

// `kernel` (one by-value parameter struct at `params`, p its TrainParams) on `blocks`
// workgroups with lds_bytes of dynamic LDS, then, when first < total, slab_sum_kernel
// over the slab indices [first, total): grad below p.n_weights, head_means behind it
// (train.hip).  The one launcher of the three kernels below.
hipError_t launch_then_sum(const void* kernel, const void* params, const TrainParams& p,
                           int blocks, size_t lds_bytes, hipStream_t stream, int first,
                           int total);

// The dynamic-LDS attribute of `kernel`, for a caller that sets it once and then launches
// the kernel many times itself (train_population.hip, train_metrics.hip)
hipError_t set_dynamic_lds(const void* kernel, size_t lds_bytes);

// loss_grad_kernel on `blocks` workgroups, then the slab sum (train.hip)
hipError_t launch_loss_grad(const TrainParams& p, int blocks, size_t lds_bytes, hipStream_t stream);

// The vector-Jacobian product of one model evaluation (ddd_result_vjp, vjp.hip): the
// forward pass of training, then, with a cotangent, the same backward pass from that
// cotangent instead of the loss's, down to the weights and to the state.  Same
// configurations, workspace and LDS plan as training.
struct VjpParams {
  TrainParams t;           // configuration, weights, y (rows = batch, no sample_index),
                           // predictions, ws; want_grad / grad = the weight gradient
  const float* cotangent;  // [batch][N][H] or null: forward only
  float* grad_y;           // [batch][N] or null
};

// vjp_kernel on `blocks` workgroups, then (want_grad) the slab sum (vjp.hip)
hipError_t launch_vjp(const VjpParams& q, int blocks, size_t lds_bytes, hipStream_t stream);

// The tangent-linear model (train_tangent.h, jvp.hip): the Jacobian of one model evaluation
// applied to M tangents per sample (ddd_result_jvp), and M state tangents carried along a
// midpoint rollout (ddd_tangent_rollout).  Same configurations and LDS plan as training;
// the slab holds no sums, only scratch: the pre-activations, then at net_off the net output
// [N][C_out] of the primal pass, which the M tangents of a sample share.
constexpr int kMaxTangents = 32;

struct JvpParams {
  TrainParams t;           // configuration, weights, y (rows = batch), predictions, ws
  int M;                   // tangents per sample
  int net_off;             // slab offset (floats) of the saved net output
  const float* tangent_y;        // [batch][M][N] or null
  const float* tangent_weights;  // [M][n_weights] (shared by the batch) or null
  float* tangents_out;     // [batch][M][N][H]
};

struct TangentRolloutParams {
  TrainParams t;           // configuration, weights, y (the initial states, rows = batch), ws
  int M;                   // tangents per sample
  int net_off;             // slab offset (floats) of the saved net output
  int tan_off;             // slab offset of the tangents [M][N], then the midpoint's [M][N]
  int num_steps;
  float dt;
  const float* tangents;   // [batch][M][N] initial state tangents
  float* state_out;        // [batch][N]
  float* tangents_out;     // [batch][M][N]
};

// jvp_kernel / tangent_rollout_kernel on `blocks` workgroups (jvp.hip); no slab sum
hipError_t launch_jvp(const JvpParams& q, int blocks, size_t lds_bytes, hipStream_t stream);
hipError_t launch_tangent_rollout(const TangentRolloutParams& q, int blocks, size_t lds_bytes,
                                  hipStream_t stream);

}  // namespace train
}  // namespace ddd
