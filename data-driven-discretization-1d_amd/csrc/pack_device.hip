// Device packer of the population's weights (pack_device.h): one thread per output float,
// grid (ceil(kFloats / 256), replicas).  No LDS, no atomics, no dependence between threads;
// every float of a replica's three arrays is written, padding rows and dead lanes included.
#include <hip/hip_runtime.h>

#include "pack_device.h"

namespace ddd {
namespace packdev {

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void pack_population_kernel(
    const Tables t, const float* __restrict__ weights, long long n_weights,
    float* __restrict__ w_input, float* __restrict__ w_hidden, float* __restrict__ w_final4) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (i >= kFloats) return;
  const long long r = blockIdx.y;
  const float value = packed_slot(t, weights + r * n_weights, i);
  if (i < kInputFloats) w_input[r * kInputFloats + i] = value;
  else if (i < kInputFloats + kHiddenFloats) w_hidden[r * kHiddenFloats + (i - kInputFloats)] = value;
  else w_final4[r * kFinal4Floats + (i - kInputFloats - kHiddenFloats)] = value;
}

}  // namespace

void launch_pack(const Tables& t, const float* weights, long long n_weights, float* w_input,
                 float* w_hidden, float* w_final4, int count, hipStream_t stream) {
  const dim3 grid((kFloats + kThreads - 1) / kThreads, (unsigned)count);
  hipLaunchKernelGGL(pack_population_kernel, grid, dim3(kThreads), 0, stream, t, weights,
                     n_weights, w_input, w_hidden, w_final4);
}

}  // namespace packdev
}  // namespace ddd
