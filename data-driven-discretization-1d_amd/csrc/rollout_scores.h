// Rollout scores on the device (ddd_rollout_reference, ddd_rollout_scores, include/ddd1d.h):
// what the reference computes per model on the host from whole trajectories --
// analysis.unify_x_coords (analysis.py:39-53), is_good / mostly_good / calculate_survival /
// mostly_good_survival (analysis.py:56-90) and the mean absolute error up to each stop time
// (scripts/run_evaluation.py:196-204) -- for R replicas at once, with the trajectories and
// the exact data staying where the integrators wrote them.  The kernels are in
// rollout_scores.hip.
//
// reference_kernel: one thread per output of exact_low [T][S][N], the mean of f consecutive
// values of y_exact [S][T][X] in the order NumPy's mean over a contiguous last axis adds them
// (block_mean below), so that it equals duckarray.resample_mean bit for bit.
//
// score_kernel: one GROUP of G lanes per row (r, t, s), G = min(64, N rounded up to a power
// of two), 256 / G rows per workgroup: rows shorter than a wavefront share one, and
// consecutive rows are consecutive in memory, so the loads of a wavefront stay dense.  Lane l
// of a group adds e = |y_model - exact_low| at x = l, l + G, ... in that order and counts
// e <= max_error[q] per q (four 16-bit counters per 64-bit word: a row has at most 1024
// points); the G partial results are combined by an xor butterfly over the group.  The order
// depends on N alone: equal inputs give equal bits, whatever R, T and S are.
//
// finish_kernel: one thread per (r, s) walks the T rows in time order: the first time that
// is not good per q, and the running sum of row_abs_sum, divided by kept[k] N where the
// prefix of kept[k] = #{t : times[t] <= stop_times[k]} rows ends (times increase, so the
// rows kept are a prefix; the launcher counts them on the host).
//
// No atomics, no scratch memory, no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddd {
namespace rollout {

constexpr int kThreads = 256;
constexpr int kMaxQuantiles = 8;     // Q
constexpr int kMaxStopTimes = 16;    // K
constexpr int kMaxPoints = 1024;     // N (the packed counters hold 16 bits)
constexpr int kMaxFactor = 128;      // f (NumPy's pairwise sum is one unrolled block up to here)

// Mean of a[0 .. f-1], 1 <= f <= 128, as numpy.mean adds a contiguous axis: below eight
// values left to right; else eight accumulators over the full groups of eight, combined as
// a balanced tree, then the remaining f mod 8 values left to right; one division.
__host__ __device__ inline double block_mean(const double* a, int f) {
  double res;
  if (f < 8) {
    res = a[0];
    for (int i = 1; i < f; ++i) res += a[i];
  } else {
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6],
           r7 = a[7];
    int i = 8;
    for (; i + 8 <= f; i += 8) {
      r0 += a[i];
      r1 += a[i + 1];
      r2 += a[i + 2];
      r3 += a[i + 3];
      r4 += a[i + 4];
      r5 += a[i + 5];
      r6 += a[i + 6];
      r7 += a[i + 7];
    }
    res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < f; ++i) res += a[i];
  }
  return res / (double)f;
}

// bytes of the row sums [R][T][S] (padded to 8), of good [R][Q][T][S] and of the times [T]
inline size_t row_sum_bytes(size_t R, size_t T, size_t S) { return R * T * S * sizeof(double); }
inline size_t good_bytes(size_t R, size_t T, size_t S, size_t Q) {
  return (R * Q * T * S + 7) & ~(size_t)7;
}
inline size_t workspace_bytes(size_t R, size_t T, size_t S, size_t Q) {
  return row_sum_bytes(R, T, S) + good_bytes(R, T, S, Q) + T * sizeof(double);
}

struct ReferenceParams {
  const double* y_exact;   // [S][T][X]
  double* exact_low;       // [T][S][N]
  int S, T, N, f;
};

struct ScoreParams {
  const void* y_model;     // [R][T][S][N] float64, or float32 with f32 != 0
  const double* exact_low; // [T][S][N]
  int f32;
  int R, T, S, N, Q, K;
  double max_error[kMaxQuantiles];
  double frac_good[kMaxQuantiles];
  int kept[kMaxStopTimes]; // rows with times[t] <= stop_times[k]
  double* row_abs_sum;     // [R][T][S]: the caller's, or in the workspace
  uint8_t* good;           // [R][Q][T][S]: the caller's, or in the workspace
  const double* times;     // device [T], in the workspace
  double* mae;             // out [R][K][S]
  double* survival;        // out [R][Q][S]
};

// Enqueue on `stream`; no synchronisation, no copy to the host, no graph capture.
hipError_t launch_reference(const ReferenceParams& p, hipStream_t stream);
// `times` is the caller's HOST array [T]: it is copied through a page-locked buffer that the
// library owns into p.times, ahead of the two launches.
hipError_t launch_scores(const ScoreParams& p, const double* times, hipStream_t stream);

}  // namespace rollout
}  // namespace ddd
