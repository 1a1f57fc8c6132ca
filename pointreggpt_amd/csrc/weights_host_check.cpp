// weights_host_check.cpp — weight preparation under AddressSanitizer / UBSan (make sanitize): the dim-16 U-Net and MaskUnet in
// every mode and under every switch setting, and single convs of odd shapes through pack_conv_host.  Stand-alone: CPU only.
#include <cstdio>

#include "weights_host.h"

using namespace prg;

static bool any_c(int) { return true; }                 // every shape "supported": all fused-attention / tail packings are built
static bool any_tail(int, int, int) { return true; }

static std::vector<float> noise(size_t n, uint32_t seed) {
  std::vector<float> v(n);
  uint32_t s = seed * 2654435761u + 1u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    v[i] = ((float)(s >> 8) * (1.0f / 8388608.0f) - 1.0f) * 0.1f;
  }
  return v;
}

int main() {
  size_t bytes = 0;
  for (int mask = 0; mask < 2; ++mask) {
    prg_unet_config cfg{};
    cfg.dim = 16; cfg.n_levels = 4;
    for (int i = 0; i < 4; ++i) cfg.dim_mults[i] = 1 << i;
    cfg.in_channels = mask ? 3 : 1; cfg.conditional = !mask; cfg.param_cond_dim = 4; cfg.groups = 8; cfg.sigmoid_out = mask;
    Layout L;
    std::string err;
    if (build_layout(cfg, L, err)) { std::printf("build_layout: %s\n", err.c_str()); return 1; }
    const std::vector<float> flat = noise((size_t)L.total, 7 + mask);
    for (int dtype = PRG_F32; dtype <= PRG_F16X3; ++dtype)
      for (int bits = 0; bits < 16; ++bits) {
        WeightOptions o;
        o.split_up2x2 = bits & 1; o.fused_attn = bits & 2; o.la_kshift = bits & 4; o.split_stem = bits & 8;
        o.linattn_fused_supported = any_c; o.resblock_tail_fused_supported = any_tail;
        UnetWeights w;
        if (build_unet_weights(cfg, flat.data(), L.total, dtype, o, w, err)) { std::printf("build_unet_weights: %s\n", err.c_str()); return 1; }
        bytes += w.packed_f32.size() * 4 + w.packed_bf16.size() * 2 + w.mx.size() + w.split.size() * 2 + w.attn.size() * 2;
      }
    UnetWeights w;
    if (build_unet_weights(cfg, flat.data(), L.total - 1, PRG_BF16, WeightOptions{}, w, err) != PRG_E_INVALID) return 1;   // size mismatch
    // default options: no predicate given = no fused shape supported, nothing in the fused arena
    if (build_unet_weights(cfg, flat.data(), L.total, PRG_BF16, WeightOptions{}, w, err) != PRG_OK || !w.attn.empty()) return 1;
  }
  // single convs: padding in both directions, every role, every mode (shapes the networks above do not have)
  const int shapes[][3] = {{72, 40, 3}, {8, 8, 1}, {64, 64, 3}, {128, 64, 3}, {64, 64, 4}, {5, 3, 4}, {1, 1, 1}, {200, 33, 3}};
  for (const auto& s : shapes) {
    std::vector<float> w = noise((size_t)s[0] * s[1] * s[2] * s[2], 99);
    for (int i = 0; i < s[1] * s[2] * s[2]; ++i) w[i] = 0.0f;                    // a dead output channel
    for (int dtype = PRG_F32; dtype <= PRG_F16X3; ++dtype)
      for (int role = 0; role < 4; ++role) {
        const ConvRole r{(role & 1) != 0, (role & 2) != 0};
        if (dtype == PRG_F32 || dtype == PRG_F16X3) bytes += pack_conv_host<float>(w.data(), s[0], s[1], s[2], dtype, r).main.size();
        else bytes += pack_conv_host<bf16_t>(w.data(), s[0], s[1], s[2], dtype, r).main.size();
      }
  }
  std::vector<bf16_t> sf;
  std::vector<uint16_t> ss;
  std::vector<float> sc;
  for (int cin : {1, 3}) {
    const std::vector<float> w = noise((size_t)64 * cin * 49, 5);
    pack_stem_mfma_weights(w.data(), cin, sf);
    pack_stem_mfma_weights_split(w.data(), cin, ss, sc);
    bytes += sf.size() + ss.size();
  }
  std::printf("weights_host_check OK (%zu bytes packed)\n", bytes);
  return 0;
}
