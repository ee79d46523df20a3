// ddd_rollout_reference / ddd_rollout_scores' device code and launchers (rollout_scores.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "rollout_scores.h"

namespace ddd {
namespace rollout {

namespace {

__global__ __launch_bounds__(kThreads) void reference_kernel(ReferenceParams p) {
  const size_t total = (size_t)p.T * p.S * p.N;
  const size_t o = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= total) return;
  const size_t ts = o / p.N;
  const int j = (int)(o - ts * p.N);
  const size_t t = ts / p.S, s = ts - t * p.S;
  const double* a = p.y_exact + ((s * p.T + t) * p.N + j) * (size_t)p.f;
  p.exact_low[o] = block_mean(a, p.f);
}

// Group g of the workgroup (lanes g G .. g G + G - 1, G = 1 << log_g <= 64) has row
// blockIdx.x (kThreads / G) + g.  Every thread reaches the butterfly: a row past the end
// contributes nothing and writes nothing.
template <typename Y>
__global__ __launch_bounds__(kThreads) void score_kernel(ScoreParams p, int log_g, size_t rows) {
  const int G = 1 << log_g;
  const int l = threadIdx.x & (G - 1);
  const size_t row = ((size_t)blockIdx.x << (8 - log_g)) + (threadIdx.x >> log_g);
  static_assert(kThreads == 256, "row: kThreads / G rows per workgroup");
  const bool live = row < rows;
  const size_t per_replica = (size_t)p.T * p.S;
  const size_t r = row / per_replica, ts = row - r * per_replica;
  double sum = 0.0;
  unsigned long long c0 = 0, c1 = 0;   // counts of q = 0 .. 3 and 4 .. 7, 16 bits each
  if (live) {
    const Y* y = static_cast<const Y*>(p.y_model) + row * p.N;
    const double* exact = p.exact_low + ts * p.N;
    for (int x = l; x < p.N; x += G) {
      const double e = fabs((double)y[x] - exact[x]);
      sum += e;
#pragma unroll
      for (int q = 0; q < kMaxQuantiles; ++q) {
        if (q < p.Q && e <= p.max_error[q]) {   // (false for a NaN)
          if (q < 4) c0 += 1ull << (16 * q);
          else c1 += 1ull << (16 * (q - 4));
        }
      }
    }
  }
  for (int m = G >> 1; m > 0; m >>= 1) {
    sum += __shfl_xor(sum, m);
    c0 += __shfl_xor(c0, m);
    c1 += __shfl_xor(c1, m);
  }
  if (!live || l != 0) return;
  p.row_abs_sum[row] = sum;
#pragma unroll
  for (int q = 0; q < kMaxQuantiles; ++q) {
    if (q < p.Q) {
      const unsigned long long word = q < 4 ? c0 >> (16 * q) : c1 >> (16 * (q - 4));
      const double frac = (double)(int)(word & 0xffffu) / (double)p.N;
      p.good[(r * p.Q + q) * per_replica + ts] = frac >= p.frac_good[q] ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(ScoreParams p) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)p.R * p.S) return;
  const size_t r = i / p.S, s = i - r * p.S;
  const size_t per_replica = (size_t)p.T * p.S;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int k = 0; k < p.K; ++k)   // NumPy's mean of nothing
    if (p.kept[k] == 0) p.mae[(r * p.K + k) * p.S + s] = nan;
  int first_bad[kMaxQuantiles];
#pragma unroll
  for (int q = 0; q < kMaxQuantiles; ++q) first_bad[q] = -1;
  double acc = 0.0;
  for (int t = 0; t < p.T; ++t) {
    acc += p.row_abs_sum[r * per_replica + (size_t)t * p.S + s];
    for (int k = 0; k < p.K; ++k)
      if (p.kept[k] == t + 1)
        p.mae[(r * p.K + k) * p.S + s] = acc / ((double)p.kept[k] * (double)p.N);
#pragma unroll
    for (int q = 0; q < kMaxQuantiles; ++q)
      if (q < p.Q && first_bad[q] < 0 &&
          p.good[(r * p.Q + q) * per_replica + (size_t)t * p.S + s] == 0)
        first_bad[q] = t;
  }
#pragma unroll
  for (int q = 0; q < kMaxQuantiles; ++q)
    if (q < p.Q)
      p.survival[(r * p.Q + q) * p.S + s] = p.times[first_bad[q] >= 0 ? first_bad[q] : p.T - 1];
}

// The caller's times may be gone before a copy from them runs, and a copy from pageable
// memory waits for the stream: they go through page-locked buffers owned by the library,
// each free again once the copy enqueued from it has run (as ddd_integrate_adaptive_f64's
// time slots, per process instead of per model).
struct TimeSlot {
  double* host = nullptr;
  size_t capacity = 0;
  hipEvent_t done = nullptr;
  int device = -1;
  bool in_flight = false;
};
constexpr int kTimeSlots = 8;
std::mutex g_mutex;
TimeSlot g_slots[kTimeSlots];
int g_next_slot = 0;

hipError_t upload_times(const double* times, int count, double* dst, hipStream_t stream) {
  std::lock_guard<std::mutex> lock(g_mutex);
  TimeSlot& slot = g_slots[g_next_slot];
  g_next_slot = (g_next_slot + 1) % kTimeSlots;
  hipError_t err;
  if (slot.in_flight) {   // only when kTimeSlots calls are still queued
    if ((err = hipEventSynchronize(slot.done)) != hipSuccess) return err;
    slot.in_flight = false;
  }
  int device = 0;
  if ((err = hipGetDevice(&device)) != hipSuccess) return err;
  if (slot.done != nullptr && slot.device != device) {
    (void)hipEventDestroy(slot.done);
    slot.done = nullptr;
  }
  if (slot.done == nullptr) {
    if ((err = hipEventCreateWithFlags(&slot.done, hipEventDisableTiming)) != hipSuccess)
      return err;
    slot.device = device;
  }
  if (slot.capacity < (size_t)count) {
    if (slot.host != nullptr) (void)hipHostFree(slot.host);
    slot.host = nullptr;
    slot.capacity = 0;
    err = hipHostMalloc(reinterpret_cast<void**>(&slot.host), (size_t)count * sizeof(double),
                        hipHostMallocPortable);
    if (err != hipSuccess) return err;
    slot.capacity = (size_t)count;
  }
  std::memcpy(slot.host, times, (size_t)count * sizeof(double));
  err = hipMemcpyAsync(dst, slot.host, (size_t)count * sizeof(double), hipMemcpyHostToDevice,
                       stream);
  if (err != hipSuccess) return err;
  if ((err = hipEventRecord(slot.done, stream)) != hipSuccess) return err;
  slot.in_flight = true;
  return hipSuccess;
}

}  // namespace

hipError_t launch_reference(const ReferenceParams& p, hipStream_t stream) {
  const size_t total = (size_t)p.T * p.S * p.N;
  const unsigned blocks = (unsigned)((total + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(reference_kernel, dim3(blocks), dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_scores(const ScoreParams& p, const double* times, hipStream_t stream) {
  hipError_t err = upload_times(times, p.T, const_cast<double*>(p.times), stream);
  if (err != hipSuccess) return err;
  int log_g = 0;
  while (log_g < 6 && (1 << log_g) < p.N) ++log_g;
  const size_t rows = (size_t)p.R * p.T * p.S;
  const size_t rows_per_block = (size_t)kThreads >> log_g;
  const unsigned blocks = (unsigned)((rows + rows_per_block - 1) / rows_per_block);
  if (p.f32)
    hipLaunchKernelGGL(score_kernel<float>, dim3(blocks), dim3(kThreads), 0, stream, p, log_g,
                       rows);
  else
    hipLaunchKernelGGL(score_kernel<double>, dim3(blocks), dim3(kThreads), 0, stream, p, log_g,
                       rows);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  const size_t pairs = (size_t)p.R * p.S;
  hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, stream, p);
  return hipGetLastError();
}

}  // namespace rollout
}  // namespace ddd
