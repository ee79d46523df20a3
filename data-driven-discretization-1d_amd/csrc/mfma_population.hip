// Population forms of the per-equation one-wavefront integrators: this file is compiled once
// per equation id (-DDDD_EQ=<0..5>, __graft_entry__.build_hip); see launch.h.
//
// The kernels are adaptive_kernel<64, 64, true, kEq> and integrate_kernel<64, 64, float, true,
// kEq> themselves, instantiated with their trailing argument pack = PopulationStrides.  The
// grid is (groups, replicas).  Workgroup (g, r) is group g of a solo launch on `batch`
// samples, run with replica r's weights into replica r's part of the outputs: before the
// set-up loads the weights (once per wavefront, ahead of the time loop) the three packed
// weight arrays are read r strides further on (rhs_mfma.h: WeightShift, enter_replica;
// DevParams itself stays the read-only kernel-argument block) and the output pointers move
// on by r strides.  blockIdx.y is wave-uniform, so that is scalar arithmetic; nothing
// inside the time loop knows of it.
// y0, the output times, the forcing tables and the projection tables of the
// kernel-argument segment are shared by the replicas and read as in a solo launch.
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
void adaptive_population_spec<DDD_EQ>(const DevParams& p, const AdaptiveArgs& a,
                                      const PopulationStrides& s, int groups, int replicas,
                                      hipStream_t stream) {
  hipLaunchKernelGGL((mfma::adaptive_kernel<64, 64, true, DDD_EQ, false, mfma::DefaultTower,
                                           PopulationStrides>), dim3(groups, replicas), dim3(64),
                     0, stream, p, a, s);
}

template <>
void integrate_population_spec<DDD_EQ>(const DevParams& p, const IntegrateArgs& a,
                                       const PopulationStrides& s, int groups, int replicas,
                                       hipStream_t stream) {
  hipLaunchKernelGGL((mfma::integrate_kernel<64, 64, float, true, DDD_EQ, false, false, mfma::DefaultTower,
                                            PopulationStrides>), dim3(groups, replicas),
                     dim3(64), 0, stream, p, a, s);
}

}  // namespace launch
}  // namespace ddd
