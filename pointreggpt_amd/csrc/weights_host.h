// weights_host.h — weight preparation of the U-Nets as host-only C++ (weights_host.cpp: no HIP runtime, no environment, linked
// into libprg_hip.so and libprg_cpu.so alike): the parameter layout and its one traversal, the shape rule of every optional weight
// packing, every packer, and build_unet_weights(): all that a handle holds, as host vectors.  unet_weights.hip uploads them.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/prg.h"
#include "bf16.h"

namespace prg {

constexpr int kHeads = 4, kDimHead = 32, kHidden = 128;   // sd:738, sd:773

// ---------------------------------------------------------------------------------------------
// parameter layout: the flat float32 array is the reference state_dict in order (weights.param_spec)
// ---------------------------------------------------------------------------------------------
struct ConvP {
  int Cout = 0, Cin = 0, KH = 0, KW = 0, CoutPad = 0, kchunks = 0;
  size_t w_off = 0;        // element offset into the packed-T arena
  int64_t b_off = -1;      // float offset of the bias in the flat array (-1: none)
  int64_t w_flat = -1;     // float offset of the raw OIHW weight in the flat array
  bool ws = false;         // weight-standardised (Block.proj)
  int64_t mx_off = -1;     // byte offset of the MX-fp8 copy of the weights (-1: none) and of its block scales
  int64_t mx_soff = -1;
  int64_t s2d_off = -1;    // 4x4 / stride 2 convs (bf16): element offset of the equivalent 2x2-tap packing (ConvLaunch::w_s2d)
  int s2d_kchunks = 0;
  int64_t sp_off = -1;     // f16x3 mode: element offset of the hi / lo f16 split packing (ConvLaunch::w_split)
  int sp_kchunks = 0;
  int64_t h16_off = -1;    // bf16 mode, second conv of a ResnetBlock: element offset of the f16 twin of the packing (ConvLaunch::w_f16)
  int64_t up_off = -1;     // bf16 mode, Upsample convs: element offset of the four pre-summed 2 x 2-tap packings (ConvLaunch::w_up)
  int64_t sp_scale_off = -1, up_sp_scale_off = -1;   // f16x3 mode: offsets into d_split_scale (ConvLaunch::split_scale / split_scale_up)
  int64_t up_sp_off = -1;  // f16x3 mode: the same in the split layout (ConvLaunch::w_up_split)
};
struct ResP {
  int cin = 0, cout = 0;
  int64_t mlp_w = -1, mlp_b = -1;  // Linear(2*emb -> 2*cout)
  int ss_off = 0;                  // column offset of this block's (scale|shift) in the conditioning row
  ConvP c1, c2, res;
  int64_t g1 = 0, b1 = 0, g2 = 0, b2 = 0;
  int64_t fw_res = -1;             // bf16 element offset of the raw res_conv weight in the fused-kernel arena (-1: unfused)
  bool has_res = false;
  int64_t pq1 = -1, pq2 = -1;      // float offsets into d_pq_static of (P = gamma | Q = beta) of norm 1 / 2, each cpad floats
  int cpad = 0;                    // cout rounded up to 4 floats (16-byte aligned rows)
};
struct AttnP {
  int C = 0;
  bool linear = true;
  ConvP qkv, out;
  int64_t out_g = -1, norm_g = -1;
  int64_t fw_qkv = -1, fw_out = -1;   // bf16 element offsets into the fused-attention weight arena (-1: unfused path)
  int64_t kshift = -1;                // float offset of the 128 static softmax shifts in d_kshift (-1: measure the maxima)
  int64_t sp_qkv = -1, sp_out = -1;   // f16x3 mode: element offsets into d_attn_split of the hi halves (the lo halves follow)
};
struct LevelP {
  ResP r0, r1;
  AttnP at;
  ConvP resample;
  bool strided = false;  // down: 4x4 s2 ; up: nearest x2 + 3x3
};

struct Layout {
  prg_unet_config cfg;
  int emb = 0, ss_total = 0, L = 0;
  std::vector<int> dims;
  int64_t stem_w = 0, stem_b = 0;
  int64_t tm1_w = 0, tm1_b = 0, tm3_w = 0, tm3_b = 0, pm0_w = 0, pm0_b = 0, pm2_w = 0, pm2_b = 0;
  std::vector<LevelP> downs, ups;
  ResP mid1, mid2, fin;
  AttnP mid_at;
  int64_t head_w = 0, head_b = 0;
  int64_t total = 0;
};

// walks the state dict in the reference's parameter order (downs, ups, mid, final).  Returns PRG_OK, or PRG_E_INVALID with the
// message in `err`: each library hands it to its own last-error slot.
int build_layout(const prg_unet_config& cfg, Layout& L, std::string& err);

// ---------------------------------------------------------------------------------------------
// the one traversal of the network's parts (Layout or const Layout): downs (r0, r1, attn, resample), ups likewise, then
// mid1, mid_at, mid2, fin.  Every weight arena is appended in this order; a loop over a subset filters inside its callback.
// ---------------------------------------------------------------------------------------------
struct ConvRole {
  bool conv2 = false;      // second conv of a ResnetBlock
  bool upsample = false;   // resample conv of an up level that is preceded by the nearest x2 Upsample
};

template <typename LayoutT, typename Fn>
void for_each_res(LayoutT& L, Fn&& fn) {
  for (auto& lv : L.downs) { fn(lv.r0); fn(lv.r1); }
  for (auto& lv : L.ups) { fn(lv.r0); fn(lv.r1); }
  fn(L.mid1); fn(L.mid2); fn(L.fin);
}
template <typename LayoutT, typename Fn>
void for_each_attn(LayoutT& L, Fn&& fn) {
  for (auto& lv : L.downs) fn(lv.at);
  for (auto& lv : L.ups) fn(lv.at);
  fn(L.mid_at);
}
template <typename LayoutT, typename Fn>
void for_each_conv(LayoutT& L, Fn&& fn) {   // fn(conv, ConvRole)
  auto res = [&](auto& r) { fn(r.c1, ConvRole{}); fn(r.c2, ConvRole{true, false}); if (r.has_res) fn(r.res, ConvRole{}); };
  auto at = [&](auto& a) { fn(a.qkv, ConvRole{}); fn(a.out, ConvRole{}); };
  for (auto& lv : L.downs) { res(lv.r0); res(lv.r1); at(lv.at); fn(lv.resample, ConvRole{}); }
  for (auto& lv : L.ups) { res(lv.r0); res(lv.r1); at(lv.at); fn(lv.resample, ConvRole{false, lv.strided}); }
  res(L.mid1); at(L.mid_at); res(L.mid2); res(L.fin);
}

// ---------------------------------------------------------------------------------------------
// shape rule of every optional packing (square K x K convs): what the kernels that read the packing cover
// ---------------------------------------------------------------------------------------------
inline bool s2d_eligible(int Cout, int Cin, int K) { return K == 4 && Cin % 64 == 0 && Cout % 64 == 0; }          // conv_w256.hip, 2 x 2-tap mode
inline bool up_eligible(int Cout, int Cin, int K) { return K == 3 && Cin % 64 == 0 && (Cout == 64 || Cout % 128 == 0); }   // conv_w256.hip MODE 2
inline bool mx_eligible(int Cout, int Cin, int K) { return K == 3 && Cin % 64 == 0 && Cout % 64 == 0; }           // conv3x3_mx_kernel
inline bool h16_eligible(int Cout, int Cin, int K) { return K == 3 && Cin == Cout && Cin % 64 == 0; }             // the h16 format, conv.h
inline bool up_split_eligible(int Cout, int Cin, int K) { return K == 3 && Cin % 32 == 0 && Cout % 128 == 0; }    // conv_split.hip, UP form

// ---------------------------------------------------------------------------------------------
// per-conv host packer: every packing one conv can have.  T = float (dtype PRG_F32 / PRG_F16X3) or bf16_t (PRG_BF16 / PRG_MXFP8).
// `w` is OIHW [Cout][Cin][K][K], already standardised where the Block standardises.  A vector is empty when the dtype, the
// role or the shape rule above says the conv has no such packing.  The layouts are stated at ConvLaunch (conv.h):
//   main     [tap = kh*KW+kw][chunk][CoutPad][BK] of T, BK = 64 bytes of T, zero padded in both Cout (to 64) and channel
//   h16      the same with BK = 32 as IEEE f16 bits, round to nearest even
//   split    [tap][32-channel chunk][CoutPad][32 hi | 32 lo] f16 bits; split_scale [CoutPad] exact powers of two the kernels
//            multiply the float32 totals by — the inverse of the per-output-channel scale the packer applied
//   mx       OCP microscaling fp8: per (tap, output channel) the input channels are cut into blocks of 32; block scale =
//            2^(floor(log2 max|w|) - 8) as an E8M0 byte (bias 127), elements = e4m3fn(w / scale), round to nearest even, saturating
//            at 448.  data [tap][ceil(Cin/64)][CoutPad][64], scales [tap][ceil(Cin/64)][CoutPad][2]
// ---------------------------------------------------------------------------------------------
template <typename T>
constexpr int kPackBK = 64 / (int)sizeof(T);   // elements per row of the main packing (= ConvTile<T>::BK, asserted in unet_weights.hip)
template <typename T>
struct PackedConv {
  std::vector<T> main;
  int CoutPad = 0, kchunks = 0;
  std::vector<T> s2d;                  // bf16, Downsample: ConvLaunch::w_s2d
  int s2d_kchunks = 0;
  std::vector<T> up;                   // bf16, Upsample: the four phases of ConvLaunch::w_up, concatenated
  std::vector<uint8_t> mx, mx_scale;   // PRG_MXFP8: ConvLaunch::w_mx / w_mx_scale
  std::vector<uint16_t> h16;           // bf16, conv2: ConvLaunch::w_f16
  std::vector<uint16_t> split;         // PRG_F16X3: ConvLaunch::w_split, split_scale
  std::vector<float> split_scale;
  int split_kchunks = 0;
  std::vector<uint16_t> up_split;      // PRG_F16X3, Upsample: the four phases of ConvLaunch::w_up_split; scales [phase][CoutPad]
  std::vector<float> up_split_scale;
};
template <typename T>
PackedConv<T> pack_conv_host(const float* w, int Cout, int Cin, int K, int dtype, ConvRole role);

// weight standardisation per output channel, biased variance, eps 1e-5 (sd:601-616); K = Cin * KH * KW
void standardize(const float* w, int Cout, int K, std::vector<float>& out);

// OIHW weights of the equivalent convolution described at ConvLaunch::w_s2d, from Conv2d(Cin, Cout, 4, 2, 1) weights
void s2d_equivalent_weights(const float* w_oihw, int Cout, int Cin, std::vector<float>& out);
// The four [Cout][Cin][2][2] tensors (phase-major) of ConvLaunch::w_up from Conv2d(Cin, Cout, 3, 1, 1) weights: for output sub-pixel
// dy the kernel rows {0 | 1, 2} (dy = 0) or {0, 1 | 2} (dy = 1) fall on the two source rows of its window (summed in float64)
void up_equivalent_weights(const float* w_oihw, int Cout, int Cin, std::vector<float>& out);

// host-side e4m3fn conversion used by the MX packer
uint8_t f32_to_e4m3(float v);
float e4m3_to_f32(uint8_t b);

// stem on MFMA (Cin 1 or 3 -> 64): w [64][Cin][7][7] as [Cin][2 row tiles][hi | lo][4 k-steps][64 lanes][8] A fragments, bf16 halves
void pack_stem_mfma_weights(const float* w, int Cin, std::vector<bf16_t>& out);
// f16x3 (round 5): the same fragments as f16 hi / lo halves; scale[64] = the inverse of the packer's per-channel power of two
void pack_stem_mfma_weights_split(const float* w, int Cin, std::vector<uint16_t>& out, std::vector<float>& scale);

// ---------------------------------------------------------------------------------------------
// What a handle packs for ONE fused Residual(PreNorm(LinearAttention)) block from the state dict's float32 tensors
// (the debug entry of unet_debug.hip packs through the same functions).  w_qkv [384][C], norm_g [C], w_out [C][128].
// ---------------------------------------------------------------------------------------------
struct FusedAttnPack {                 // bf16 (attn_fused.hip)
  std::vector<bf16_t> qkv;             // [384][C]: PreNorm gain folded in, q and k rows times log2 e
  std::vector<bf16_t> out;             // [C][128]
  float shifts[kHidden + kHeads];      // static softmax shifts: a bound on |k| per column, then on |q| per head (log2 units)
  bool ok = false;                     // every bound is small enough for the kernels to skip the measured maxima
};
void pack_fused_attention(const float* w_qkv, const float* norm_g, const float* w_out, int C, FusedAttnPack& p);
struct SplitAttnPack {                 // f16x3 (attn_split.hip): the f16 hi halves, then the lo halves
  std::vector<uint16_t> qkv;           // 2 x [384][C]
  std::vector<uint16_t> out;           // 2 x [C][128]
};
void pack_split_attention(const float* w_qkv, const float* norm_g, const float* w_out, int C, SplitAttnPack& p);

// appends `one` to `arena` at the next multiple of `align` elements (zero filled gap); returns its element offset
template <typename U>
size_t append_aligned(std::vector<U>& arena, const std::vector<U>& one, size_t align) {
  const size_t off = (arena.size() + align - 1) / align * align;
  arena.resize(off + one.size());
  if (!one.empty()) std::memcpy(arena.data() + off, one.data(), one.size() * sizeof(U));
  return off;
}

// ---------------------------------------------------------------------------------------------
// everything a handle holds, as a value
// ---------------------------------------------------------------------------------------------
// one entry per conditioned norm for cond_fold_kernel (blocks.h): (ss_off, C, gamma offset, beta offset into the flat array)
struct CondFoldEntry { int ss_off, C; long long gamma_off, beta_off; };

// The switches weight preparation depends on; the defaults are the library's.  unet_weights.hip fills them from the environment
// and from the shape rules of the fused kernels (attn_fused.hip), which this unit does not link.
struct WeightOptions {
  bool split_up2x2 = false;   // f16x3: build the Upsample convs' sub-pixel packings (PRG_SPLIT_UP2X2)
  bool fused_attn = true;     // bf16: build the fused-attention arena (PRG_FUSED_ATTN)
  bool split_stem = true;     // f16x3: build the split stem fragments (PRG_SPLIT_STEM)
  bool la_kshift = true;      // bf16: static softmax shifts where the bound allows (PRG_LA_KSHIFT)
  bool (*linattn_fused_supported)(int C) = nullptr;                                // null: no shape is supported
  bool (*resblock_tail_fused_supported)(int C0, int C1, int Cout) = nullptr;
};

struct UnetWeights {
  Layout lay;                                   // every offset filled in
  std::vector<float> packed_f32;                // packed conv weights of T: float (PRG_F32 / PRG_F16X3) ...
  std::vector<bf16_t> packed_bf16;              // ... or bf16_t (PRG_BF16 / PRG_MXFP8)
  std::vector<uint8_t> mx, mx_scale;
  std::vector<uint16_t> h16, split;
  std::vector<float> split_scale;
  std::vector<float> stem;                      // the direct stem kernel's [49 * Cin][dim] weights
  std::vector<bf16_t> stem_frag;                // bf16: MFMA stem fragments (Cin 1 / 3 -> 64)
  std::vector<uint16_t> stem_split;             // f16x3: the same as f16 hi / lo halves ...
  std::vector<float> stem_split_scale;          // ... and the inverse of the per-channel scale [64]
  std::vector<float> freqs;                     // SinusoidalPosEmb frequencies [dim / 2]
  std::vector<uint16_t> attn_split;             // f16x3: fused linear attention weights
  std::vector<float> pq_static;                 // bf16: (gamma | beta) rows of every norm
  std::vector<CondFoldEntry> cond_entries;
  std::vector<bf16_t> attn;                     // bf16: fused linear attention and fused ResnetBlock tail weights
  std::vector<float> kshift;
};

// build_layout + every weight arena of a handle of `dtype`.  Alignments: 128 elements (256-byte tiles of bf16) in the packed, h16
// and split arenas, 256 bytes for the MX data and scales, 64 elements in the attention arenas, shifts padded to 4 floats; the
// Upsample packings follow all the other packings of their arena.
int build_unet_weights(const prg_unet_config& cfg, const float* weights, int64_t n, int dtype, const WeightOptions& opt,
                       UnetWeights& out, std::string& err);

}  // namespace prg
