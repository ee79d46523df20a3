// Reorders a net's conv weights into the MFMA A-operand layouts of rhs_mfma.h.  Plain host
// C++ (mfma_layout.h and the standard library only): capi.hip uploads what pack_weights()
// returns, and the CPU test tier runs this very header under g++ (oracle/pack_host.cpp,
// tests/test_cpu_mfma_emulation.py) -- the statements that feed the kernels, not a twin.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "mfma_layout.h"

namespace ddd {
namespace pack {

// Natural-layout description of the net the MFMA packing reads: the model's own
// ([K][cin][cout] + bias per layer, DevParams::w_off / b_off) or its zero-padded
// embedding in a tower (embed_tower).
struct NetLayout {
  const float* weights;
  int w_off[kMaxLayers], b_off[kMaxLayers];
};

struct Input {
  int L, D, G, C_out, cout0, act, target, pao;   // DevParams' (cout0: filters of the TRUE first layer)
  const int* in_start;                 // [D]
  const int* in_size;                  // [D]
  const float (*ns8)[kGWide];          // DevParams::ns8 / bias8 (capi.hip: upload_padded_tables)
  const float (*bias8)[kGWide];
  bool wide;                           // the wide flavour of the run-time kernels (rhs_mfma.h kWide)
  int tower_k, tower_cb;               // the tower `net` is laid out in (rhs_mfma.h Tower)
  bool no_fold;                        // (probes) keep the projection out of the output layer
  NetLayout net;
};

// One vector per device buffer of DevParams (empty: not built for this model) and the
// decisions the kernels are launched by.
struct Packed {
  std::vector<float> w_input, w_hidden, w_final4_rt, w_final4, w_final4_split, w_quad,
      w_final4_half, w_t16;
  int folded = 0, rt_groups = 0, fin4_groups = 0;
  bool spec_folded = false;            // w_final4 holds the folded output layer
  bool unsupported = false;            // a wide coefficient net that does not fold: nothing after
                                       // w_hidden is built (decide_mfma admits only what folds)
};

// [rows][64] -> the storage order of rhs_mfma.h load_rows4: four rows to a float4 per
// lane, rows zero-padded to a multiple of four.
inline std::vector<float> quad_rows(const float* rows64, int rows) {
  std::vector<float> out((size_t)ddd::mfma::padded_rows4(rows) * 64, 0.0f);
  for (int s = 0; s < rows; ++s)
    for (int lane = 0; lane < 64; ++lane)
      out[((size_t)(s >> 2) * 64 + lane) * 4 + (s & 3)] = rows64[(size_t)s * 64 + lane];
  return out;
}

// Nets between two towers ride the next tower up EXACTLY (rhs_mfma.h: Tower; the
// default one has 5 taps x 32 channels), embedded with
// zero weights: a K-tap kernel (K < 5) is the 5-tap kernel whose outer taps are
// zero (tap k of K sits at offset k - ceil((K-1)/2), the alignment of
// layers.pad_periodic(center=True), layers.py:76-79), F < 32 filters are 32
// filters whose extra rows / columns / biases are zero.  fma(0, x, acc) == acc
// for every finite x, and a padded channel is multiplied by zero weights in the
// next layer whatever the activation makes of its 0, so the finite results are
// bit-identical to the unpadded evaluation order-for-order; the matrix work
// grows by 5/K and (32/F)^2, still an order of magnitude ahead of the generic
// kernel.  (Algorithmic FLOPs -- ddd_fma_per_point -- keep counting the true net.)
// `dp`: DevParams, or anything with its L, K, C_out, w_off, b_off, cin and cout.
template <class Params>
void embed_tower(const Params& dp, const std::vector<float>& wv, int tower_k,
                 int tower_c, std::vector<float>* padded, NetLayout* net) {
  const int k5 = tower_k, f32 = tower_c;       // (the tower's taps and filters)
  const int shift = (k5 - 1) / 2 - dp.K / 2;   // ceil((k5-1)/2) - ceil((K-1)/2), k5 odd
  padded->clear();
  for (int l = 0; l < dp.L; ++l) {
    const int cin = l == 0 ? 1 : f32;
    const int cout = l == dp.L - 1 ? dp.C_out : f32;
    net->w_off[l] = (int)padded->size();
    padded->resize(padded->size() + (size_t)k5 * cin * cout, 0.0f);
    net->b_off[l] = (int)padded->size();
    padded->resize(padded->size() + (size_t)cout, 0.0f);
    const float* w = wv.data() + dp.w_off[l];
    const float* b = wv.data() + dp.b_off[l];
    for (int k = 0; k < dp.K; ++k)
      for (int ci = 0; ci < dp.cin[l]; ++ci)
        for (int co = 0; co < dp.cout[l]; ++co)
          (*padded)[(size_t)net->w_off[l] + ((size_t)(k + shift) * cin + ci) * cout + co] =
              w[((size_t)k * dp.cin[l] + ci) * dp.cout[l] + co];
    for (int co = 0; co < dp.cout[l]; ++co) (*padded)[(size_t)net->b_off[l] + co] = b[co];
  }
  net->weights = padded->data();
}

// ---- input and hidden layers on v_mfma_f32_32x32x2_f32 ---------------------------------
// (`dn`: the relu scaling of mfma_layout.h kReluShift, on the input layer's weights and on
// every bias row; 1 for the other activations)

// one hidden layer 32 -> 32 (rhs_mfma.h hidden_layer): step s = 16 tap + jj carries input
// channels jj (lanes 0..31) and 16 + jj (lanes 32..63); step 80: the bias in the first half
inline std::vector<float> pack_hidden(const float* w, const float* b, float dn) {   // w: [5][32][32]
  std::vector<float> packed((size_t)mfma::kHidSteps * 64, 0.0f);
  for (int s = 0; s < 80; ++s) {
    const int tap = s / 16, jj = s % 16;
    for (int lane = 0; lane < 64; ++lane) {
      const int cin = 16 * (lane >> 5) + jj, cout = lane & 31;
      packed[s * 64 + lane] = w[(tap * 32 + cin) * 32 + cout];
    }
  }
  for (int lane = 0; lane < 32; ++lane) packed[80 * 64 + lane] = dn * b[lane];
  return quad_rows(packed.data(), mfma::kHidSteps);   // every layer padded on its own (load_hidden)
}

// input layer 1 -> 32 tcb of a tower of tk taps, [block][step][lane]: k = 2 s + (lane >> 5) is
// the tap, k = tk the bias (rhs_mfma.h input_layer_big, streamed as it is; the default tower's
// input_layer reads the same three rows through load_rows4)
inline std::vector<float> pack_input_stream(const float* w, const float* b, int tk, int tcb,
                                            float dn) {   // w: [tk][1][tc]
  const int in_steps = (tk + 2) / 2, tc = 32 * tcb;
  std::vector<float> packed((size_t)tcb * in_steps * 64, 0.0f);
  for (int h = 0; h < tcb; ++h)
    for (int s = 0; s < in_steps; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int k = 2 * s + (lane >> 5), ch = 32 * h + (lane & 31);
        packed[((size_t)h * in_steps + s) * 64 + lane] =
            dn * (k < tk ? w[k * tc + ch] : k == tk ? b[ch] : 0.0f);
      }
  return packed;
}

// one hidden layer of a big tower (rhs_mfma.h hidden_layer_stream): [group][out block][lane]
// float4, then the bias rows [out block][lane] (stream_layer_floats), appended to `packed`
inline void pack_hidden_stream(const float* w, const float* b, int tk, int tcb, float dn,
                               std::vector<float>* packed) {   // w: [tk][tc][tc]
  const int tc = 32 * tcb, groups = tk * tc / 8;   // Tower::kHidGroups
  const size_t base = packed->size();
  packed->resize(base + (size_t)groups * tcb * 64 * 4 + (size_t)tcb * 64, 0.0f);
  float* dst = packed->data() + base;
  for (int g = 0; g < groups; ++g)
    for (int h = 0; h < tcb; ++h)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 4; ++e) {
          const int s = 4 * g + e;                       // reduction step of this output block
          const int tap = s / (16 * tcb), cb = (s / 16) % tcb, jj = s % 16;
          const int cin = 32 * cb + 16 * (lane >> 5) + jj, cout = 32 * h + (lane & 31);
          dst[(((size_t)g * tcb + h) * 64 + lane) * 4 + e] = w[((size_t)tap * tc + cin) * tc + cout];
        }
  float* bias = dst + (size_t)groups * tcb * 64 * 4;
  for (int h = 0; h < tcb; ++h)
    for (int lane = 0; lane < 32; ++lane) bias[h * 64 + lane] = dn * b[32 * h + lane];
}

// ---- the output layer ---------------------------------------------------------------------

// The matrix an output-layer packing reads: the net's own last layer or the folded one.
struct OutLayer {
  const float* w;   // [k = (tap, cin)][cols]
  const float* b;   // [cols]
  int cols;
  int live;         // channels >= live are left zero (<= cols)
};

// Fold coeff = bias + net[start:stop] @ nullspace into the output layer:
// W'[tap][cin][slot d + g] = sum_j W[tap][cin][start_d + j] * ns_d[j][g]
// (accumulated in double, rounded once to float32), same for the bias.
// The layer then emits the D x G coefficients directly and the epilogue's
// projection disappears.  Deviation from the reference's operation order:
// O(1 ulp) of the coefficient deltas, far inside the 1e-5 tolerance.
// The kernels' folded epilogue exists for two derivatives and 6..8 stencil points
// (default flavour: channel G d + g of 16) and -- always -- for the wide flavour's
// coefficient nets (channel wide_slot(G) d + g of 36, up to three derivatives: the wide
// kernels have no projection code at all).
struct Fold {
  std::vector<float> w, b;   // [kc][cols], [cols]; empty unless can_fold
  int cols = 0, slot = 0;
  bool can_fold = false;
  bool always = false;       // nothing to weigh: direct coefficients, or the wide flavour
  bool wide = false;
};

inline Fold fold_output_layer(const Input& in, const float* w_nat, const float* b_nat, int kc) {
  Fold f;
  const bool coeffs = in.target == TARGET_COEFFICIENTS;
  const bool projected = coeffs && in.pao > 0, direct_coeffs = coeffs && in.pao <= 0;
  f.wide = in.wide && coeffs;
  f.slot = f.wide ? mfma::wide_slot(in.G) : in.G;
  f.cols = f.wide ? mfma::flavour_net_channels(true) : 16;
  const bool fold_shape = f.wide ? in.D <= mfma::kWideDerivs
                                 : in.D <= 2 && in.G >= 6 && in.G <= kGMax && !in.wide;
  f.can_fold = fold_shape && (direct_coeffs || (projected && (!in.no_fold || f.wide)));
  f.always = direct_coeffs || f.wide;
  if (!f.can_fold) return f;
  f.w.assign((size_t)kc * f.cols, 0.0f);
  f.b.assign(f.cols, 0.0f);
  for (int d = 0; d < in.D; ++d)
    for (int g = 0; g < in.G; ++g) {
      const int oc = f.slot * d + g;
      if (direct_coeffs) {
        // the net emits the D x G coefficients themselves (model.py:460-475) in
        // exactly the folded layer's channel order: nothing to project
        const int c = in.G * d + g;
        for (int row = 0; row < kc; ++row)
          f.w[(size_t)row * f.cols + oc] = w_nat[(size_t)row * in.C_out + c];
        f.b[oc] = b_nat[c];
        continue;
      }
      const int start = in.in_start[d];
      for (int row = 0; row < kc; ++row) {
        double acc = 0.0;
        for (int j = 0; j < in.in_size[d]; ++j)
          acc += (double)w_nat[(size_t)row * in.C_out + start + j] * (double)in.ns8[start + j][g];
        f.w[(size_t)row * f.cols + oc] = (float)acc;
      }
      // bias row of the folded layer: the accuracy layer's standard
      // coefficients + the projected conv bias, rounded once
      double acc = (double)in.bias8[d][g];
      for (int j = 0; j < in.in_size[d]; ++j)
        acc += (double)b_nat[start + j] * (double)in.ns8[start + j][g];
      f.b[oc] = (float)acc;
    }
  return f;
}

// map from reduction step k to the row of OutLayer::w
inline int natural_row(int k) { return k; }
inline int tile16_row(int k) { return (k / 16) * 32 + k % 16; }   // k = 16 tap + cin of 32 filters

// Packing for the 4x4x1 broadcast MFMA (rhs_mfma.h: final_layer4): channels grouped by
// four; the channel groups [first_group, first_group + ng) are issued together, instruction
// q = k * ng + gi reads lanes 4 (q % 16) .. + 3 of weight register q / 16 (`rows`: row 0 of
// the chunk, [..][64]), lane 4 abid + r carrying channel 4 (first_group + gi) + r;
// k < kc: reduction step (row src_row(k) of the source, scaled by `up`), k = kc: the bias.
inline void pack_groups4(const OutLayer& src, float up, int kc, int (*src_row)(int),
                         int first_group, int ng, float* rows) {
  for (int k = 0; k <= kc; ++k)
    for (int gi = 0; gi < ng; ++gi) {
      const int q = k * ng + gi;
      for (int r = 0; r < 4; ++r) {
        const int ch = 4 * (first_group + gi) + r;
        if (ch >= src.live) continue;
        rows[(size_t)(q / 16) * 64 + 4 * (q % 16) + r] =
            k < kc ? up * src.w[(size_t)src_row(k) * src.cols + ch] : src.b[ch];
      }
    }
}

// Run-time-parameterised kernels: the head chunk (rt_head_groups: 0, 1 or 3 groups), then
// the pairs; + slack so that the kernels' fixed-size first fetch (three groups' rows)
// stays inside
inline std::vector<float> pack_final4_rt(const OutLayer& src, float up, int kc, int groups) {
  const auto regs = [kc](int ng) { return ((kc + 1) * ng + 15) / 16; };   // Tower::kFinK = kc + 1
  const int head = mfma::rt_head_groups(groups);
  const int total_rows = regs(head) + (groups - head) / 2 * regs(2) + regs(3);
  std::vector<float> packed((size_t)total_rows * 64, 0.0f);
  if (head > 0) pack_groups4(src, up, kc, natural_row, 0, head, packed.data());
  for (int g0 = head; g0 < groups; g0 += 2)
    pack_groups4(src, up, kc, natural_row, g0, 2,
                 packed.data() + (size_t)(regs(head) + (g0 - head) / 2 * regs(2)) * 64);
  return packed;
}

// ---- every layer on v_mfma_f32_16x16x4_f32: lane l supplies W[out = l & 15][slot l >> 4] ----

// input layer of output channels [c0, c0 + 16), two rows: step 0 = taps 0..3, step 1 = tap 4,
// bias, 0, 0 (input_layer's k order)
inline void pack_input16(const float* w0, const float* b0, float dn, int c0, float* rows) {
  for (int lane = 0; lane < 64; ++lane) {
    const int sg = lane >> 4, cout = c0 + (lane & 15);
    rows[lane] = dn * w0[sg * 32 + cout];
    rows[64 + lane] = sg == 0 ? dn * w0[4 * 32 + cout] : sg == 1 ? dn * b0[cout] : 0.0f;
  }
}

// The whole three-layer net for the integrators on FOUR 16-row wavefronts (rhs_mfma.h
// kQuad): [2 channel halves][2] input rows, [2][41] hidden rows, [41] output rows.
inline std::vector<float> pack_quad(const float* w0, const float* b0, const float* w1,
                                    const float* b1, const OutLayer& src, float dn, float up) {
  using namespace mfma;
  std::vector<float> quad((size_t)kQuadRows * 64, 0.0f);
  for (int chh = 0; chh < 2; ++chh) {
    pack_input16(w0, b0, dn, 16 * chh, quad.data() + (size_t)chh * kQuadInSteps * 64);
    // hidden layer: step 8 tap + i, slot sg -> cin = (sg >> 1) + 16 (sg & 1) + 2 i:
    // per tap c = 0, 16, 1, 17, ... -- hidden_layer's order (s = 16 tap + jj, half = l >> 5)
    float* hid = quad.data() + (size_t)(2 * kQuadInSteps + chh * kQuadHidSteps) * 64;
    for (int lane = 0; lane < 64; ++lane) {
      const int sg = lane >> 4, cout = 16 * chh + (lane & 15);
      for (int s2 = 0; s2 < 40; ++s2) {
        const int tap = s2 / 8, i = s2 % 8;
        const int cin = (sg >> 1) + 16 * (sg & 1) + 2 * i;
        hid[(size_t)s2 * 64 + lane] = w1[(tap * 32 + cin) * 32 + cout];
      }
      hid[(size_t)40 * 64 + lane] = sg == 0 ? dn * b1[cout] : 0.0f;
    }
  }
  // output layer: step s2, slot sg -> k = 4 s2 + sg in natural order (final_layer4's), k = 160: bias
  float* fin = quad.data() + (size_t)(2 * kQuadInSteps + 2 * kQuadHidSteps) * 64;
  for (int s2 = 0; s2 < kQuadFinSteps; ++s2)
    for (int lane = 0; lane < 64; ++lane) {
      const int k = 4 * s2 + (lane >> 4), ch = lane & 15;
      if (ch >= src.live || k > 160) continue;
      fin[(size_t)s2 * 64 + lane] = k < 160 ? up * src.w[(size_t)k * src.cols + ch] : src.b[ch];
    }
  return quad;
}

// Input and hidden layer of a net of up to 16 filters (rhs_mfma.h Tile16Tower), read from its
// embedding in 32 (channels >= 16 are zero there): 2 input rows; hidden layer: step 4 tap + e,
// slot sg -> input channel 4 e + sg; step 20: the bias in slot 0
inline std::vector<float> pack_t16(const float* w0, const float* b0, const float* w1,
                                   const float* b1, float dn) {
  using namespace mfma;
  std::vector<float> t16((size_t)(kT16InSteps + kT16HidSteps) * 64, 0.0f);
  pack_input16(w0, b0, dn, 0, t16.data());
  for (int lane = 0; lane < 64; ++lane) {
    const int sg = lane >> 4, cout = lane & 15;
    for (int s2 = 0; s2 < 20; ++s2) {
      const int tap = s2 / 4, e = s2 % 4;
      t16[(size_t)(kT16InSteps + s2) * 64 + lane] = w1[(tap * 32 + 4 * e + sg) * 32 + cout];
    }
    t16[(size_t)(kT16InSteps + 20) * 64 + lane] = sg == 0 ? dn * b1[cout] : 0.0f;
  }
  return t16;
}

// ---- the whole model ----------------------------------------------------------------------

inline Packed pack_weights(const Input& in) {
  Packed out;
  const NetLayout& net = in.net;
  const auto w = [&net](int l) { return net.weights + net.w_off[l]; };
  const auto b = [&net](int l) { return net.weights + net.b_off[l]; };
  const int hidden = in.L - 2;
  const int tk = in.tower_k, tcb = in.tower_cb;
  const bool big = tk != mfma::kKW || tcb != 1;
  const int kc = tk * 32 * tcb;                  // reduction length of the output layer
  const bool relu_clamp = in.act == ACT_RELU;    // mfma_layout.h kReluShift; exact: powers of two
  const float dn = relu_clamp ? std::ldexp(1.0f, -kReluShift) : 1.0f;
  const float up = relu_clamp ? std::ldexp(1.0f, kReluShift) : 1.0f;

  if (big) {
    out.w_input = pack_input_stream(w(0), b(0), tk, tcb, dn);
    for (int l = 1; l <= hidden; ++l) pack_hidden_stream(w(l), b(l), tk, tcb, dn, &out.w_hidden);
  } else {
    out.w_input = quad_rows(pack_input_stream(w(0), b(0), tk, tcb, dn).data(), mfma::kInSteps);
    for (int l = 1; l <= hidden; ++l) {
      const std::vector<float> q = pack_hidden(w(l), b(l), dn);
      out.w_hidden.insert(out.w_hidden.end(), q.begin(), q.end());
    }
  }

  const float* w_nat = w(in.L - 1);              // [tk][32 tcb][C_out]
  const float* b_nat = b(in.L - 1);
  const Fold fold = fold_output_layer(in, w_nat, b_nat, kc);
  const OutLayer plain{w_nat, b_nat, in.C_out, in.C_out};

  // Run-time-parameterised kernels: only the live channel groups are issued,
  // as interleaved accumulator chains (rhs_mfma.h: two or three chains run at
  // 8.1 cycles per MFMA, a lone group at 13.2).  Folding the projection trades the
  // epilogue's ~C_out x G FMAs (~2.5 units of 161 MFMA slots) for D x G
  // instead of C_out channels: fold only where the matrix work does not grow
  // by more than that (the same outcome as rhs_mfma.h: spec_folded for the six
  // default models, so the two kernel families stay bit-identical).
  // polynomial_accuracy_order = 0 has nothing to project.
  const auto issue_cost = [](int groups) { return groups == 1 ? 13.2 : 8.1 * groups; };
  const int groups_plain = (in.C_out + 3) / 4;
  const int groups_rt_folded = ((in.D - 1) * fold.slot + in.G + 3) / 4;
  const bool fold_rt = fold.can_fold && (fold.always || issue_cost(groups_rt_folded) <=
                                                            issue_cost(groups_plain) + 2.5);
  if (fold.wide && !fold_rt) {
    out.unsupported = true;
    return out;
  }
  out.folded = fold_rt ? 1 : 0;
  out.rt_groups = fold_rt ? groups_rt_folded : groups_plain;
  const OutLayer folded_rt{fold.w.data(), fold.b.data(), fold.cols, fold.cols};
  out.w_final4_rt = pack_final4_rt(fold_rt ? folded_rt : plain, up, kc, out.rt_groups);

  // specialised kernels: live channels only, renumbered contiguously (the folded columns
  // are contiguous already); folded only where that does not cost a channel group (same
  // rule as rhs_mfma.h: spec_folded)
  const int groups_folded = (in.D * in.G + 3) / 4;
  out.spec_folded = fold.can_fold && groups_folded <= groups_plain;
  out.fin4_groups = out.spec_folded ? groups_folded : groups_plain;
  // (they exist for the default tower and flavour, and hold at most four channel groups)
  if (in.wide || big || out.fin4_groups > 4) return out;
  const OutLayer folded_spec{fold.w.data(), fold.b.data(), fold.cols, in.D * in.G};
  const OutLayer& spec = out.spec_folded ? folded_spec : plain;
  const int groups = out.fin4_groups, rows4 = mfma::fin4_regs(4), kc5 = mfma::kFin4K - 1;
  {
    std::vector<float> rows((size_t)rows4 * 64, 0.0f);
    pack_groups4(spec, up, kc5, natural_row, 0, groups, rows.data());
    out.w_final4 = quad_rows(rows.data(), rows4);
  }
  // the same layer for the split integrators (rhs_mfma.h kSplit): two chunks of
  // channel groups, each packed on its own and quad-stored in 24 rows
  const int na = (groups + 1) / 2, chunk_rows = mfma::fin4_regs(2);
  for (int c = 0; c < 2; ++c) {
    std::vector<float> chunk((size_t)chunk_rows * 64, 0.0f);
    pack_groups4(spec, up, kc5, natural_row, c == 0 ? 0 : na, c == 0 ? na : groups - na,
                 chunk.data());
    const std::vector<float> q4 = quad_rows(chunk.data(), chunk_rows);
    out.w_final4_split.insert(out.w_final4_split.end(), q4.begin(), q4.end());
  }
  if (in.L != 3) return out;   // the per-equation kernels' nets only
  out.w_quad = pack_quad(w(0), b(0), w(1), b(1), spec, dn, up);
  // ... and, for nets of up to 16 filters (embedded here in 32), the packing of rhs_mfma.h
  // Tile16Tower: the output layer over 5 x 16 + 1 reduction steps
  if (in.cout0 <= 16) {
    std::vector<float> rows((size_t)rows4 * 64, 0.0f);
    pack_groups4(spec, up, 80, tile16_row, 0, groups, rows.data());
    out.w_final4_half = quad_rows(rows.data(), rows4);
    out.w_t16 = pack_t16(w(0), b(0), w(1), b(1), dn);
  }
  return out;
}

}  // namespace pack
}  // namespace ddd
