// The MFMA weight packing of pack_weights.h turned inside out, for the models the population
// kernels carry (capi.hip: plan_population): instead of walking a net and scattering its
// weights into the three arrays setup_weights reads (w_input, w_hidden, w_final4), every
// OUTPUT float computes its own source -- one natural-layout weight, a fold sum of at most
// five products, or zero -- so that a replica's arrays are packed by independent threads on
// the device (pack_device.hip) from the [n_weights] vector the trainers keep there.
//
// Plain C++ behind DDD_HD (mfma_layout.h): the kernel and the CPU test tier (g++,
// tests/pack_device_harness.cpp) run these very statements.  Bit for bit what
// pack::pack_weights uploads for the same values: the same float32 products with the relu
// scaling, the same double sums in the same order for the folded output layer, +0 wherever
// the host leaves its zero-initialised buffers untouched.
//
// Scope: three relu layers on the default tower (5 taps x 32 filters), a projected coefficient
// head, D <= 2 where the output layer is folded.  Nets of K <= 5 taps and F <= 32 filters are
// packed as their zero-padded embedding (pack_weights.h: embed_tower).
#pragma once
#include "mfma_layout.h"

namespace ddd {
namespace packdev {

constexpr int kLayers = 3;
constexpr int kDerivs = 4;   // DevParams' kMaxDerivs

// Everything the slot functions read that is not a weight: one by-value kernel argument,
// filled from the population's model 0 (capi.hip: pack_tables).
struct Tables {
  float ns8[kChWide][kGWide];     // DevParams::ns8 / bias8
  float bias8[kDerivs][kGWide];
  int in_start[kDerivs], in_size[kDerivs];
  int w_off[kLayers], b_off[kLayers];   // of the TRUE net (DevParams::w_off / b_off)
  int K, F, C_out;                      // its taps, filters and output channels
  int D, G;
  int fin4_groups;                      // channel groups of w_final4 (pack::Packed)
  int spec_folded;                      // w_final4 holds the folded output layer
};

// floats of a replica's three arrays (rows padded to fours, load_rows4's storage order)
constexpr int kInputFloats = mfma::padded_rows4(mfma::kInSteps) * 64;
constexpr int kHiddenFloats = mfma::padded_rows4(mfma::kHidSteps) * 64;
constexpr int kFinal4Floats = mfma::padded_rows4(mfma::fin4_regs(4)) * 64;
constexpr int kFloats = kInputFloats + kHiddenFloats + kFinal4Floats;

// relu scaling of mfma_layout.h kReluShift (pack_weights.h: dn, up); exact powers of two
DDD_HD inline float scale_dn() { return 0x1p-64f; }
DDD_HD inline float scale_up() { return 0x1p+64f; }
static_assert(kReluShift == 64, "scale_dn / scale_up spell out 2^-+kReluShift");

// inverse of pack::quad_rows: slot i of a quad-stored array is row `s` of lane `lane`
DDD_HD inline int slot_row(int i) { return 4 * (i >> 8) + (i & 3); }
DDD_HD inline int slot_lane(int i) { return (i >> 2) & 63; }

// Weight (tap, cin, cout) and bias cout of layer l of the net embedded in the tower: tap k of
// K sits at k + shift, channels beyond the net's are zero (pack::embed_tower).
DDD_HD inline float tower_weight(const Tables& t, const float* w, int l, int tap, int cin,
                                 int cout) {
  const int shift = (mfma::kKW - 1) / 2 - t.K / 2;
  const int cin_n = l == 0 ? 1 : t.F, cout_n = l == kLayers - 1 ? t.C_out : t.F;
  const int k = tap - shift;
  if (k < 0 || k >= t.K || cin >= cin_n || cout >= cout_n) return 0.0f;
  return w[t.w_off[l] + (k * cin_n + cin) * cout_n + cout];
}
DDD_HD inline float tower_bias(const Tables& t, const float* w, int l, int cout) {
  const int cout_n = l == kLayers - 1 ? t.C_out : t.F;
  return cout < cout_n ? w[t.b_off[l] + cout] : 0.0f;
}

// quad_rows(pack_input_stream(w0, b0, 5, 1, dn), kInSteps)
DDD_HD inline float input_slot(const Tables& t, const float* w, int i) {
  const int s = slot_row(i), lane = slot_lane(i);
  if (s >= mfma::kInSteps) return 0.0f;
  const int k = 2 * s + (lane >> 5), ch = lane & 31;
  return scale_dn() * (k < mfma::kKW ? tower_weight(t, w, 0, k, 0, ch)
                       : k == mfma::kKW ? tower_bias(t, w, 0, ch) : 0.0f);
}

// pack_hidden(w1, b1, dn)
DDD_HD inline float hidden_slot(const Tables& t, const float* w, int i) {
  const int s = slot_row(i), lane = slot_lane(i);
  if (s < 80) {
    const int tap = s / 16, jj = s % 16;
    return tower_weight(t, w, 1, tap, 16 * (lane >> 5) + jj, lane & 31);
  }
  if (s == 80 && lane < 32) return scale_dn() * tower_bias(t, w, 1, lane);
  return 0.0f;
}

// Row `row` (= 32 tap + cin; kFin4K - 1: the bias) and channel ch of the layer w_final4 is
// packed from: the net's last layer, or pack::fold_output_layer's W' = W @ nullspace,
// b' = bias8 + b @ nullspace (double sums in j order, rounded once).
DDD_HD inline float output_entry(const Tables& t, const float* w, int row, int ch) {
  const int last = kLayers - 1;
  const bool bias = row == mfma::kFin4K - 1;
  const int tap = row / mfma::kF, cin = row % mfma::kF;
  if (!t.spec_folded)
    return bias ? tower_bias(t, w, last, ch) : tower_weight(t, w, last, tap, cin, ch);
  const int d = ch / t.G, g = ch % t.G;
  const int start = t.in_start[d];
  double acc = bias ? (double)t.bias8[d][g] : 0.0;
  for (int j = 0; j < t.in_size[d]; ++j) {
    const float x = bias ? tower_bias(t, w, last, start + j)
                         : tower_weight(t, w, last, tap, cin, start + j);
    acc += (double)x * (double)t.ns8[start + j][g];
  }
  return (float)acc;
}

// quad_rows(pack_groups4(spec, up, kFin4K - 1, natural_row, 0, fin4_groups), fin4_regs(4))
DDD_HD inline float final4_slot(const Tables& t, const float* w, int i) {
  const int s = slot_row(i), lane = slot_lane(i);
  if (s >= mfma::fin4_regs(4)) return 0.0f;
  const int q = 16 * s + (lane >> 2), r = lane & 3;   // instruction q = k groups + gi
  const int k = q / t.fin4_groups, gi = q % t.fin4_groups;
  const int ch = 4 * gi + r;
  const int live = t.spec_folded ? t.D * t.G : t.C_out;
  if (k >= mfma::kFin4K || ch >= live) return 0.0f;
  const float x = output_entry(t, w, k, ch);
  return k < mfma::kFin4K - 1 ? scale_up() * x : x;
}

// Slot i of [0, kFloats): the three arrays one after the other.
DDD_HD inline float packed_slot(const Tables& t, const float* w, int i) {
  if (i < kInputFloats) return input_slot(t, w, i);
  if (i < kInputFloats + kHiddenFloats) return hidden_slot(t, w, i - kInputFloats);
  return final4_slot(t, w, i - kInputFloats - kHiddenFloats);
}

// ---- pack_device.hip ---------------------------------------------------------------------
#if defined(__HIP__) || defined(__HIPCC__)
// Packs `count` vectors weights[r][n_weights] into w_input / w_hidden / w_final4 (each
// [count][its floats], already offset to the first replica), on `stream`.
void launch_pack(const Tables& t, const float* weights, long long n_weights, float* w_input,
                 float* w_hidden, float* w_final4, int count, hipStream_t stream);
#endif

}  // namespace packdev
}  // namespace ddd
