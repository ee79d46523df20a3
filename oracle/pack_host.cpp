// TEST INFRASTRUCTURE ONLY (CPU test tier; never part of the product).
//
// The PRODUCT header csrc/pack_weights.h -- the MFMA weight packing ddd_model_create uploads --
// compiled by g++ and called over flat arrays (tests/test_cpu_mfma_emulation.py): the CPU tests
// feed their emulated operand gathers from the buffers the kernels would read.
#include "../data-driven-discretization-1d_amd/csrc/pack_weights.h"

#include <cstring>
#include <string>

namespace {
struct Net {   // what embed_tower reads of DevParams
  int L, K, C_out, w_off[ddd::kMaxLayers], b_off[ddd::kMaxLayers], cin[ddd::kMaxLayers],
      cout[ddd::kMaxLayers];
};
}  // namespace

// cfg: L, K, F, C_out, D, G, act, target, pao, wide, tower_k, tower_cb, no_fold.
// weights: the net in its natural layout, per layer [K][cin][cout] then the bias.
// ns8: [kChWide][kGWide], bias8: [4][kGWide] (DevParams' tables), in_start / in_size: [D].
// Copies up to `capacity` floats of the buffer `name` to `out` and returns its length
// (0: not built); decisions: folded, rt_groups, fin4_groups, spec_folded, unsupported.
extern "C" int pack_host(const int* cfg, const float* weights, const int* in_start,
                         const int* in_size, const float* ns8, const float* bias8,
                         const char* name, float* out, int capacity, int* decisions) {
  Net dp{};
  dp.L = cfg[0]; dp.K = cfg[1]; dp.C_out = cfg[3];
  const int F = cfg[2];
  int n = 0;
  for (int l = 0; l < dp.L; ++l) {
    dp.cin[l] = l == 0 ? 1 : F;
    dp.cout[l] = l == dp.L - 1 ? dp.C_out : F;
    dp.w_off[l] = n; n += dp.K * dp.cin[l] * dp.cout[l];
    dp.b_off[l] = n; n += dp.cout[l];
  }
  const std::vector<float> wv(weights, weights + n);
  ddd::pack::Input in{};
  in.L = dp.L; in.C_out = dp.C_out; in.cout0 = dp.cout[0];
  in.D = cfg[4]; in.G = cfg[5]; in.act = cfg[6]; in.target = cfg[7]; in.pao = cfg[8];
  in.wide = cfg[9] != 0; in.tower_k = cfg[10]; in.tower_cb = cfg[11]; in.no_fold = cfg[12] != 0;
  in.in_start = in_start; in.in_size = in_size;
  in.ns8 = reinterpret_cast<const float (*)[ddd::kGWide]>(ns8);
  in.bias8 = reinterpret_cast<const float (*)[ddd::kGWide]>(bias8);
  in.net.weights = wv.data();
  for (int l = 0; l < dp.L; ++l) { in.net.w_off[l] = dp.w_off[l]; in.net.b_off[l] = dp.b_off[l]; }
  std::vector<float> padded;
  if (dp.K != in.tower_k || F != 32 * in.tower_cb)   // as ddd_model_create does
    ddd::pack::embed_tower(dp, wv, in.tower_k, 32 * in.tower_cb, &padded, &in.net);
  const ddd::pack::Packed p = ddd::pack::pack_weights(in);
  decisions[0] = p.folded; decisions[1] = p.rt_groups; decisions[2] = p.fin4_groups;
  decisions[3] = p.spec_folded; decisions[4] = p.unsupported;
  const std::string which(name);
  const std::vector<float>* buf =
      which == "w_input" ? &p.w_input : which == "w_hidden" ? &p.w_hidden :
      which == "w_final4_rt" ? &p.w_final4_rt : which == "w_final4" ? &p.w_final4 :
      which == "w_final4_split" ? &p.w_final4_split : which == "w_quad" ? &p.w_quad :
      which == "w_final4_half" ? &p.w_final4_half : which == "w_t16" ? &p.w_t16 : nullptr;
  if (buf == nullptr) return -1;
  const size_t count = buf->size() < (size_t)capacity ? buf->size() : (size_t)capacity;
  if (count > 0) std::memcpy(out, buf->data(), count * sizeof(float));
  return (int)buf->size();
}
