// unet_layout.h — what the three host units of the U-Nets share (unet.hip: forward pass, sampler, C-ABI; unet_weights.hip: state-dict
// walk and weight preparation; unet_debug.hip: the prg_debug_* entries): the parameter layout and its one traversal, the shape rule
// of every optional weight packing, the per-conv host packer, owned device buffers and the prg_unet handle.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "blocks.h"
#include "conv.h"

namespace prg {

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

// walks the state dict in the reference's parameter order (downs, ups, mid, final)
int build_layout(const prg_unet_config& cfg, Layout& L);

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
// role or the shape rule above says the conv has no such packing.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct PackedConv {
  std::vector<T> main;                 // pack_conv_weight<T>
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

// ---------------------------------------------------------------------------------------------
// What a handle packs for ONE fused Residual(PreNorm(LinearAttention)) block from the state dict's float32 tensors
// (unet_weights.hip; the debug entry of unet_debug.hip packs through the same functions).  w_qkv [384][C], norm_g [C], w_out [C][128].
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
// owned device allocations: freed when the owner goes (a handle, or the scope of a debug entry).  The first failure sticks in
// `rc` (and behind prg_last_error) and turns every later call into a no-op that returns null: check once after a group of calls.
// ---------------------------------------------------------------------------------------------
struct DeviceBuffers {
  std::vector<void*> ptrs;
  int rc = PRG_OK;
  DeviceBuffers() = default;
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;
  ~DeviceBuffers() { for (void* p : ptrs) (void)hipFree(p); }
  // uninitialised device memory; `nomem` is the whole PRG_E_NOMEM message.  count == 0: null
  template <typename U>
  U* alloc(size_t count, const char* nomem) {
    void* p = nullptr;
    if (rc != PRG_OK || count == 0) return nullptr;
    if (hipMalloc(&p, count * sizeof(U)) != hipSuccess) { rc = fail(PRG_E_NOMEM, nomem); return nullptr; }
    ptrs.push_back(p);
    return static_cast<U*>(p);
  }
  // hipMalloc + hipMemcpy of `count` host elements
  template <typename U>
  U* upload(const U* src, size_t count, const char* nomem) {
    U* p = alloc<U>(count, nomem);
    if (p) {
      const hipError_t e = hipMemcpy(p, src, count * sizeof(U), hipMemcpyHostToDevice);
      if (e != hipSuccess) { rc = fail(PRG_E_HIP, std::string("hipMemcpy (") + nomem + "): " + hipGetErrorString(e)); return nullptr; }
    }
    return p;
  }
  template <typename U>
  U* upload(const std::vector<U>& v, const char* nomem) { return upload(v.data(), v.size(), nomem); }
};

// ---------------------------------------------------------------------------------------------
// device stack arena (the workspace of a handle)
// ---------------------------------------------------------------------------------------------
struct Arena {
  char* base = nullptr;
  size_t cap = 0, top = 0, high = 0;
  bool dry = false;  // dry run: only measure
  void* alloc(size_t bytes) {
    size_t a = (top + 255) & ~(size_t)255;
    top = a + bytes;
    if (top > high) high = top;
    if (dry) return reinterpret_cast<void*>((uintptr_t)0x1000 + a);  // never dereferenced
    return (top <= cap) ? base + a : nullptr;
  }
  size_t mark() const { return top; }
  void reset(size_t m) { top = m; }
};

// conditioning source for the ResnetBlocks of one forward
struct CondSrc {
  const float* ss_a = nullptr;
  const float* ss_b = nullptr;
  int64_t ss_a_stride = 0, ss_b_stride = 0;
  const int* row = nullptr;
  int64_t row_stride = 0;
};

struct Tap {
  const void* ptr;
  int C, H, W, B;
  bool nchw_f32;
};

struct ProfileSink;   // per-launch conv timing (unet.hip)

}  // namespace prg

// ---------------------------------------------------------------------------------------------
// the U-Net handle.  `own` holds every weight buffer; the typed d_* members below are views into it (null: the handle has no such
// packing).  The workspace and d_gnacc are reallocated by reserve() and freed by prg_unet_destroy.
// ---------------------------------------------------------------------------------------------
struct prg_unet {
  prg::Layout lay;
  int dtype = PRG_F32;
  prg::DeviceBuffers own;
  float* d_flat = nullptr;      // the float32 state_dict on device (biases, norm gains, MLPs read in place)
  void* d_packed = nullptr;     // packed conv weights of T
  float* d_stem = nullptr;      // stem weights [49*Cin][dim]
  prg::bf16_t* d_stem_frag = nullptr; // stem weights as MFMA fragments (bf16 path, Cin 1 -> 64)
  uint16_t* d_stem_split = nullptr;    // f16x3 mode: the same fragments as f16 hi / lo halves (stem_mfma_kernel<CIN, true>)
  float* d_stem_split_scale = nullptr; // ... and the inverse of the packer's per-channel power-of-two scale [64]
  prg::bf16_t* d_attn = nullptr;     // fused linear attention: gain-folded to_qkv and to_out weights (bf16 path only)
  float* d_kshift = nullptr;    // fused linear attention: static softmax shifts of the k columns
  uint8_t* d_mx = nullptr;      // MX-fp8 conv weights (dtype PRG_MXFP8): e4m3 data and E8M0 block scales
  uint8_t* d_mx_scale = nullptr;
  uint16_t* d_attn_split = nullptr;   // f16x3 mode: fused linear attention weights as f16 hi / lo halves (attn_split.hip)
  float* d_split_scale = nullptr;   // f16x3 mode: the packer's per-output-channel power-of-two factors, undone in the epilogues
  uint16_t* d_split = nullptr;  // f16x3 mode (dtype PRG_F16X3): every conv weight as f16 hi / lo halves (conv_split.hip)
  uint16_t* d_h16 = nullptr;    // bf16 mode: f16 twins of the ResnetBlocks' second convs (the h16 format, conv.h)
  float* d_freqs = nullptr;     // SinusoidalPosEmb frequencies [dim/2] (sd:645-657), see prg_unet_set_time_freqs
  // fixed-point GroupNorm statistics (common.h, GnFold; bf16 / mxfp8 handles)
  long long* d_gnacc = nullptr; // [slots][resB][groups][2], zeroed by ONE memset at the start of every forward
  size_t gnacc_bytes = 0;
  int gn_slots = 0, gn_slot = 0;
  float* d_pq_static = nullptr; // (gamma | beta) of every norm, 16-byte aligned rows: P / Q of the unconditioned norms
  prg::CondFoldEntry* d_cond_entries = nullptr;   // one entry per conditioned norm (Block 1 of every ResnetBlock)
  int n_cond_entries = 0;
  prg::Arena arena;
  uint64_t arena_gen = 0;       // bumped whenever the workspace is reallocated: captured graphs bake its pointers in
  int resB = 0, resS = 0;
  bool taps_on = false;
  std::map<std::string, prg::Tap> taps;
  prg::ProfileSink* prof = nullptr;
  virtual ~prg_unet() {}
  virtual int measure(int B, int S, size_t* bytes) = 0;
  virtual int forward(const float* x_nchw, const prg::CondSrc& cond, float* out, int B, int S, hipStream_t s) = 0;
  virtual int cond_general(const int64_t* time, const float* param_cond, int B, prg::CondSrc* out, hipStream_t s) = 0;
  virtual int tap_copy(const prg::Tap& t, float* out, hipStream_t s) = 0;
};

namespace prg {
// build_layout + every weight arena of a fresh handle (its storage type is given by dtype: float for PRG_F32 / PRG_F16X3,
// bf16_t for PRG_BF16 / PRG_MXFP8).  On failure the caller deletes the handle, which frees what was uploaded.
int prepare_unet_weights(prg_unet& u, const prg_unet_config& cfg, const float* weights, int64_t n, int dtype);
}  // namespace prg
