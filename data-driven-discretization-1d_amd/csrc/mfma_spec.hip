// Per-equation specialised MFMA kernels: this file is compiled once per
// equation id (-DDDD_EQ=<0..5>, __graft_entry__.build_hip); see launch.h.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "rhs_adaptive.h"
#include "rhs_mfma.h"

#ifndef DDD_EQ
#error "compile with -DDDD_EQ=<equation id 0..5>"
#endif

namespace ddd {
namespace launch {

template <>
void integrate_spec<DDD_EQ>(int rows, bool f64, bool traced, const DevParams& p,
                            const IntegrateArgs& a, int blocks, hipStream_t stream) {
  const dim3 grid(blocks);
  if (rows == 64) {
    if (f64) {
      hipLaunchKernelGGL((mfma::integrate_kernel<64, 64, double, true, DDD_EQ>), grid, dim3(64),
                         0, stream, p, a);
      return;
    }
#if DDD_EQ == 1 && defined(DDD_PROBES)   // probe build: the headline configuration carries phase stamps
    if (traced) {
      hipLaunchKernelGGL((mfma::integrate_kernel<64, 64, float, true, DDD_EQ, true>), grid,
                         dim3(64), 0, stream, p, a);
      return;
    }
#endif
    (void)traced;
    hipLaunchKernelGGL((mfma::integrate_kernel<64, 64, float, true, DDD_EQ>), grid, dim3(64), 0,
                       stream, p, a);
  } else if (f64) {
    // float64 state on four-wave groups (SciPy holds y in float64, integrate.py:154): round 6 --
    // these ran on the run-time kernel at 70.8 % where the float32 state runs at 83 %
    // (profiles/r6_adaptive_gap.txt)
    hipLaunchKernelGGL((mfma::integrate_kernel<256, 64, double, true, DDD_EQ>), grid, dim3(256),
                       0, stream, p, a);
  } else {
    hipLaunchKernelGGL((mfma::integrate_kernel<256, 64, float, true, DDD_EQ>), grid, dim3(256),
                       0, stream, p, a);
  }
}

template <>
void integrate_split_spec<DDD_EQ>(const DevParams& p, const IntegrateArgs& a, int blocks,
                                  hipStream_t stream) {
  hipLaunchKernelGGL((mfma::integrate_kernel<64, 32, float, true, DDD_EQ>), dim3(blocks), dim3(128),
                     0, stream, p, a);
}

template <>
void integrate_quad_spec<DDD_EQ>(const DevParams& p, const IntegrateArgs& a, int blocks,
                                 hipStream_t stream) {
  hipLaunchKernelGGL((mfma::integrate_kernel<64, 16, float, true, DDD_EQ>), dim3(blocks), dim3(256),
                     0, stream, p, a);
}

template <>
void adaptive_quad_spec<DDD_EQ>(const DevParams& p, const AdaptiveArgs& a, int blocks,
                                hipStream_t stream) {
  hipLaunchKernelGGL((mfma::adaptive_kernel<64, 16, true, DDD_EQ>), dim3(blocks), dim3(256), 0,
                     stream, p, a);
}

template <>
void substep_spec<DDD_EQ>(int rows, const DevParams& p, const SubstepArgs& a, int groups,
                          int grid, hipStream_t stream) {
  if (rows == 64)
    hipLaunchKernelGGL((mfma::substep_multi_kernel<64, 64, DDD_EQ>), dim3(grid), dim3(64), 0,
                       stream, p, a, groups);
  else
    hipLaunchKernelGGL((mfma::substep_multi_kernel<256, 64, DDD_EQ>), dim3(grid), dim3(256), 0,
                       stream, p, a, groups);
}

template <>
void step_spec<DDD_EQ>(int rows, const DevParams& p, const StepArgs& a, int groups,
                       int grid, hipStream_t stream) {
  if (rows == 64)
    hipLaunchKernelGGL((mfma::step_multi_kernel<64, 64, DDD_EQ>), dim3(grid), dim3(64), 0,
                       stream, p, a, groups);
  else
    hipLaunchKernelGGL((mfma::step_multi_kernel<256, 64, DDD_EQ>), dim3(grid), dim3(256), 0,
                       stream, p, a, groups);
}

// The four-wave adaptive kernels keep the whole tower resident (kHoist) where that fits 256
// VGPRs without a spill -- KdV and KS: 255 registers, 0 scratch, two workgroups per CU --;
// the Burgers kernels (forcing state on top: 21-28 spills when hoisted) fetch the hidden
// layer's operands per evaluation as before.  profiles/r6_adaptive_gap.txt: with the weights
// streamed, KS N = 256 ran at the rate of the float64-state run-time kernel (70.8 %), 12
// points below the resident fixed-step kernel.
constexpr bool kAdapt256Hoist = DDD_EQ >= 2;
template <>
void adaptive_spec<DDD_EQ>(int rows, const DevParams& p, const AdaptiveArgs& a, int blocks,
                           hipStream_t stream) {
  if (rows == 64)
    hipLaunchKernelGGL((mfma::adaptive_kernel<64, 64, true, DDD_EQ>), dim3(blocks), dim3(64), 0,
                       stream, p, a);
  else
    hipLaunchKernelGGL((mfma::adaptive_kernel<256, 64, kAdapt256Hoist, DDD_EQ>), dim3(blocks), dim3(256),
                       0, stream, p, a);
}

}  // namespace launch
}  // namespace ddd
