// Layout constants of the MFMA path that the kernels (rhs_mfma.h, dev_params.h) and the
// host-side weight packing (pack_weights.h) share.  Plain C++: no HIP header, no builtin,
// so that g++ compiles the packing for the CPU test tier (oracle/pack_host.cpp).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define DDD_HD __host__ __device__
#else
#define DDD_HD
#endif

namespace ddd {

constexpr int kMaxLayers = 8;
constexpr int kGMax = 8;      // widest stencil of the default MFMA kernels (and the stream kernel)
// "wide" run-time-parameterised MFMA kernels (rhs_mfma.h, kWide): stencils up
// to 12 points and up to 24 output channels -- coefficient_grid_min_size = 9 and
// polynomial_accuracy_order = 0 with three derivatives (training_test.py:56-57)
constexpr int kGWide = 12;
constexpr int kChMax = 16, kChWide = 24;

// relu on the MFMA path = the VALU's [0, 1] output clamp on a PACKED add (v_pk_add_f32 x, 0
// clamp: two accumulator registers per instruction; gfx950 has no packed f32 max), on
// activations the host scaled by 2^-kReluShift: the input layer's weights and every
// bias row of the tower carry the factor, the output layer's weights carry its inverse
// (pack_weights.h).  Powers of two commute with every rounding of the fma
// chains, so the finite results are the bits of max(x, 0) for activations in
// [2^(-126 + kReluShift), 2^kReluShift] -- beyond 1.8e19 a state has diverged, below
// 2e-19 an activation contributes nothing float32 can see.  NaN -> 0 like v_max (DX10 clamp):
// rhs_mfma.h::eval_rhs re-creates the NaNs a propagating relu would have passed on (one
// v_cmp per evaluation; the rest only when a state holds a NaN).
// 64 relu instructions per wave-evaluation become 32 (profiles/r5_valu_census.txt).
constexpr int kReluShift = 64;

enum : int { ACT_NONE = -1, ACT_RELU = 0, ACT_RELU6 = 1, ACT_TANH = 2,
             ACT_SOFTPLUS = 3, ACT_ELU = 4 };
enum : int { TARGET_COEFFICIENTS = 0, TARGET_SPACE_DERIVATIVES = 1,
             TARGET_TIME_DERIVATIVE = 2, TARGET_FLUX = 3 };

namespace mfma {

constexpr int kF = 32;           // hidden channels
constexpr int kKW = 5;           // conv taps
constexpr int kInSteps = 3;      // (5 taps + bias) / 2
constexpr int kHidSteps = 81;    // 5*32/2 MFMA steps + 1 bias step
constexpr int kFin4K = kKW * kF + 1;   // output layer on 4x4x1 MFMAs: 160 reduction steps + bias
// Flavours of the run-time-parameterised kernels (template parameter kWide):
// default: stencils <= 8 points, <= 16 output channels; wide: <= 12 points,
// <= 24 channels of the net, projection always folded into the output layer.
DDD_HD constexpr int flavour_stencil(bool wide) { return wide ? kGWide : kGMax; }
DDD_HD constexpr int flavour_channels(bool wide) { return wide ? kChWide : kChMax; }
// Output channels the kernels carry in registers.  The wide flavour's output layer is ALWAYS
// folded (round 5): it emits coefficient g of derivative d as channel kGWide d + g -- slots
// of twelve, three channel groups per derivative, D <= 3 --, so the epilogue's register
// indices are compile-time constants and there is no projection left to run there.
constexpr int kWideDerivs = 3;
DDD_HD constexpr int flavour_net_channels(bool wide) {
  return wide ? kWideDerivs * kGWide : kChMax;
}
// ... coefficient g of derivative d = channel wide_slot(G) d + g: slots of 8 for stencils
// of up to 8 points, of exactly G above (27 channels = 7 channel groups for 9 points and
// three derivatives, where slots of 12 would issue 9).
DDD_HD constexpr int wide_slot(int G) { return G <= kGMax ? kGMax : G; }

constexpr int kT16InSteps = 2, kT16HidSteps = 4 * kKW + 1;   // A-operand rows of DevParams::w_quad in this mode

DDD_HD constexpr int fin4_regs(int groups) { return (kFin4K * groups + 15) / 16; }
// Run-time kernels issue their live channel groups as a head chunk followed by
// pairs: an even count has no head (0), a single group is its own head (1), any
// other odd count starts with three interleaved groups.
DDD_HD constexpr int rt_head_groups(int groups) {
  return groups % 2 == 0 ? 0 : groups == 1 ? 1 : 3;
}

// rows of a weight array in the storage order of rhs_mfma.h load_rows4
constexpr int padded_rows4(int rows) { return (rows + 3) / 4 * 4; }

constexpr int kQuadHidSteps = 41, kQuadFinSteps = 41, kQuadInSteps = 2;
constexpr int kQuadRows = 2 * kQuadInSteps + 2 * kQuadHidSteps + kQuadFinSteps;   // rows of w_quad (4 + 82 + 41)

}  // namespace mfma
}  // namespace ddd
