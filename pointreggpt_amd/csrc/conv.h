// conv.h — launch interface of the MFMA convolutions and their weight packing.
#pragma once
#include <vector>

#include "common.h"
#include "conv_choose.h"   // ConvDesc, ConvFacts, ConvChoice: the host-only selection

namespace prg {

// K-chunk of the generic kernel (elements of one tap's channel range staged per main-loop iteration): 64 bytes
// per tile row.  The halo kernel consumes two of these per step (128-byte pixel rows).
template <typename T>
struct ConvTile {
  static constexpr int BK = 64 / (int)sizeof(T);  // bf16: 32, f32: 16
};

// Every weight pointer below is a packing that weights_host.cpp builds (pack_conv_host).
template <typename T>
struct ConvLaunch {
  ConvDesc d;
  const T* src0;
  const T* src1;
  const T* w;            // packed: [tap = kh*KW+kw][chunk][CoutPad][BK] of T, zero padded in both Cout and channel
  const float* bias;     // [Cout] or null
  const T* residual;     // NHWC (M, Cout) added in the epilogue, or null
  // Activated residual (1x1 convs on the implicit-GEMM kernel, bf16 mode): out = conv + bias + SiLU(residual * res_a[b][c]
  // + res_b[b][c]) — the ResnetBlock tail `SiLU(GroupNorm(h)) + res_conv(x)` (sd:731-734) in the res_conv's epilogue, where
  // `residual` is h and (res_a, res_b) are its folded GroupNorm coefficients.  out may alias residual.  null = plain add.
  const float* res_a;
  const float* res_b;
  T* out;                // NHWC (M, Cout)
  // fused GroupNorm statistics of the OUTPUT (before any activation): per (image, M-tile, group) (sum, sumsq)
  // written to gn_partials [B][gn_nsplit][gn_groups][2]; null = off.  launch_conv decides whether the shape
  // allows it and reports the slab count through *gn_nsplit_out (0 = caller must run the stats kernel).
  float* gn_partials;
  int gn_groups;
  // fused prologue on the INPUT (halo kernel, single source): x <- silu(x * pro_a[b][c] + pro_b[b][c]);
  // this is GroupNorm + (scale+1, shift) + SiLU of the previous Block folded into per-(image, channel) affine
  // coefficients (sd:690-696).  null = off.
  const float* pro_a;
  const float* pro_b;
  // Retired in-kernel coefficient folding of conv3x3_c64_kernel (conv_c64.hip keeps its device code): the workgroup that
  // completed an image's last tile turned the image's partial sums into gn_coef_a/b [B][Cout].  Never set: the launcher passes
  // gn_tickets = null.
  GnApply gn{};
  float* gn_coef_a = nullptr;
  float* gn_coef_b = nullptr;
  int* gn_tickets = nullptr;
  // Fixed-point statistics (common.h, GnFold): producers that support it add their wave totals into gn_acc [B][gn_groups][2]
  // (zeroed by the caller) INSTEAD of writing gn_partials slabs and report so through launch_conv's acc_done; consumers
  // with pro_fold.acc != null compute the prologue coefficients themselves (pro_a / pro_b then point to [B][C0] scratch
  // tables that kernels without the in-kernel fold fill with one gn_coeff_acc launch first).
  long long* gn_acc;
  GnFold pro_fold;
  // res_fold.acc != null (with `residual`, 1x1 convs on the implicit-GEMM kernel): the activated residual's coefficients are
  // folded in the epilogue from the accumulators (once per thread and image) instead of read from res_a / res_b
  GnFold res_fold;
  // MX-fp8 operands (handles of dtype PRG_MXFP8, 3x3 / s1 / p1 convs with 64-channel multiples): OCP e4m3 weights
  // [tap][64-channel chunk][CoutPad][64] with one E8M0 scale per 32 input channels [tap][chunk][CoutPad][2]; null = bf16.
  const uint8_t* w_mx;
  const uint8_t* w_mx_scale;
  int mx_pure;           // 1: never fall back to bf16 operands for shapes the 256-pixel MX kernel does not cover (unit tests)
  // Conv2d(C, Cout, 4, stride 2, pad 1) only: the same weights as the 3 x 3 packing of the equivalent 2 x 2-tap
  // convolution over the space-to-depth view of the shifted input ([Cout][4 C][3][3], taps (1..2, 1..2) non-zero; virtual
  // channel (2 dy + dx) C + c, tap (1 + by, 1 + bx) = W[.][c][2 by + dy][2 bx + dx]); null = not available.  conv_w256.hip
  const T* w_s2d;
  int s2d_kchunks;
  // Upsample convs (nn.Upsample(x2, nearest) + Conv2d(C, Cout, 3, pad 1), d.ups = 1; bf16): the four pre-summed 2 x 2-tap packings of
  // the sub-pixel decomposition (conv_w256.hip, MODE 2), [phase 2 dy + dx][tap 2 a + b][32-channel chunk][CoutPad][32]; null = the
  // nine-tap gather form.  up_equivalent_weights() builds the OIHW tensors.
  const T* w_up = nullptr;
  // f16x3 mode (handles of dtype PRG_F16X3, T = float; conv_split.hip): the weights split into f16 hi / lo halves,
  // [tap][32-channel chunk][CoutPad][32 hi | 32 lo]; null = the exact-f32 kernels
  const uint16_t* w_split;
  int split_kchunks;
  // f16x3, Upsample convs: the four sub-pixel 2 x 2-tap packings (up_equivalent_weights) in the split layout, phase-major:
  // [phase][tap 4][32-channel chunk][CoutPad][32 hi | 32 lo]; null = the nine-tap gather form
  const uint16_t* w_up_split = nullptr;
  // f16x3: [CoutPad] (w_split) / [4][CoutPad] (w_up_split, phase-major) exact power-of-two factors applied to the float32 totals
  // before the bias (the packer scaled every output channel's weights by the inverse); null = 1
  const float* split_scale = nullptr;
  const float* split_scale_up = nullptr;
  // h16 (bf16 mode, round 4): the tensor between the two convs of a ResnetBlock only ever feeds conv2's fused GroupNorm + SiLU
  // prologue, so it is stored as IEEE f16 instead of bf16 — the prologue then runs in PACKED f16 (v_pk_fma_f16, v_exp_f16,
  // v_rcp_f16: two channels per instruction, no unpack / repack) and conv2 contracts f16 operands
  // (v_mfma_f32_32x32x16_f16, the bf16 instruction's rate) against an f16 packing of its weights.
  //   out_f16: this launch stores f16 bit patterns into `out` (conv1);  in_f16: src0 holds f16, the prologue is pro_fold's and
  //   w_f16 is the f16 twin of `w`, same layout (conv2).  Only the kernels that conv_h16_pair_ok() accepts implement them.
  int out_f16 = 0, in_f16 = 0;
  int reserved = 0;      // unused (was a host-side probe flag): the struct is a kernel argument, its size and offsets are kept
  const uint16_t* w_f16 = nullptr;   // [tap][32-channel chunk][CoutPad][32] IEEE f16 bits, round to nearest even
};

// what the selection (conv_choose.h) reads of a launch
template <typename T>
inline ConvFacts conv_facts(const ConvLaunch<T>& L) {
  ConvFacts f{};
  f.d = L.d;
  f.f32 = sizeof(T) == 4;
  f.bias = L.bias != nullptr; f.residual = L.residual != nullptr; f.res_a = L.res_a != nullptr; f.pro_a = L.pro_a != nullptr;
  f.gn_partials = L.gn_partials != nullptr; f.gn_acc = L.gn_acc != nullptr; f.w_mx = L.w_mx && L.w_mx_scale;
  f.w_s2d = L.w_s2d != nullptr; f.w_up = L.w_up != nullptr; f.w_split = L.w_split != nullptr;
  f.w_up_split = L.w_up_split != nullptr; f.w_f16 = L.w_f16 != nullptr;
  f.res_fold_acc = L.res_fold.acc != nullptr;
  f.gn_groups = L.gn_groups;
  f.pro_fold_acc = L.pro_fold.acc != nullptr; f.pro_fold_pq = L.pro_fold.P && L.pro_fold.Q;
  f.pro_fold_G = L.pro_fold.G; f.pro_fold_cpg = L.pro_fold.cpg;
  f.in_f16 = L.in_f16; f.out_f16 = L.out_f16; f.mx_pure = L.mx_pure;
  return f;
}

// the PRG_* switches of the selection, read from the environment once
const ConvSwitches& conv_switches();

// true when conv1 (L1, asked to store f16) and conv2 (L2, asked to read f16 through its folded prologue) of a ResnetBlock would both
// run on kernels that implement the h16 format, L1 with fixed-point statistics; nothing is launched
bool conv_h16_pair_ok(const ConvLaunch<bf16_t>& L1, const ConvLaunch<bf16_t>& L2);

// Returns PRG_OK; *gn_nsplit_out (may be null) receives the number of statistic slabs per image written, or 0
// when statistics were requested but this shape cannot fuse them; *acc_done (may be null) 1 when they went to gn_acc instead;
// *chosen (may be null) what ran.  `allow_prologue` must be checked by the caller with conv_supports_prologue() before setting
// pro_a / pro_b.
template <typename T>
int launch_conv(const ConvLaunch<T>& L, hipStream_t s, int* gn_nsplit_out, int* acc_done = nullptr, ConvChoice* chosen = nullptr);

// The families' launchers: each owns the table of its instantiations (kernel, dynamic LDS bytes) and launches the one `c` names,
// with the geometry `c` holds.  launch_conv is their only caller.
int launch_conv_c64(const ConvChoice& c, const ConvLaunch<bf16_t>& L, hipStream_t s);          // conv_c64.hip
int launch_conv_ws(const ConvChoice& c, const ConvLaunch<bf16_t>& L, hipStream_t s);           // conv_ws.hip
int launch_conv_w256(const ConvChoice& c, const ConvLaunch<bf16_t>& L, hipStream_t s);         // conv_w256.hip (kConvW256, kConvW256Mx)
int launch_conv_split(const ConvChoice& c, const ConvLaunch<float>& L, hipStream_t s);         // conv_split.hip (the kConvSplit* families)
int launch_conv_split_w512(const ConvChoice& c, const ConvLaunch<float>& L, hipStream_t s);    // conv_split512.hip

#if defined(__HIPCC__)
// One instantiation in a family's table: the template parameters as a key, the kernel, its workgroup size and dynamic LDS bytes, and
// the MaxDynamicSharedMemorySize opt-in it needs (0 = none).  The same row serves the one-time hipFuncSetAttribute (per device:
// DeviceOnce is atomic, lanes launch from several host threads) and the launch.
template <typename Fn>
struct ConvKernel {
  int key;
  Fn fn;
  int block;
  size_t lds;
  int lds_attr;
  DeviceOnce attr;
};
constexpr int conv_key(int a, int b = 0, int c = 0, int d = 0) { return ((a * 512 + b) * 512 + c) * 8 + d; }
// the kernels that take (L, tiles_x, tiles_y, tiles_n, fuse_stats)
template <typename T>
using ConvTileKernel = void (*)(const ConvLaunch<T>, int, int, int, int);

template <typename Fn, size_t N>
inline int conv_kernel_find(ConvKernel<Fn> (&tab)[N], int key, const char* family, ConvKernel<Fn>** out) {
  for (ConvKernel<Fn>& e : tab) {
    if (e.key != key) continue;
    if (e.lds_attr && !e.attr.done()) {
      hipError_t err = hipFuncSetAttribute(reinterpret_cast<const void*>(e.fn), hipFuncAttributeMaxDynamicSharedMemorySize, e.lds_attr);
      if (err != hipSuccess) return fail(PRG_E_HIP, std::string("hipFuncSetAttribute(") + family + "): " + hipGetErrorString(err));
      e.attr.mark();
    }
    *out = &e;
    return PRG_OK;
  }
  return fail(PRG_E_STATE, std::string(family) + ": the selection named an instantiation this family does not have");
}
template <typename T, size_t N>
inline int launch_conv_tiles(ConvKernel<ConvTileKernel<T>> (&tab)[N], int key, const char* family, const ConvChoice& c,
                             const ConvLaunch<T>& L, hipStream_t s) {
  ConvKernel<ConvTileKernel<T>>* e = nullptr;
  if (int rc = conv_kernel_find(tab, key, family, &e)) return rc;
  e->fn<<<dim3(c.grid), e->block, e->lds, s>>>(L, c.tiles_x, c.tiles_y, c.tiles_n, c.fuse_stats);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}
#endif

// true when a single-source conv of this shape takes a fused input prologue (asked of the selection)
template <typename T>
inline bool conv_supports_prologue(const ConvDesc& d) { return choose_supports_prologue(d, sizeof(T) == 4); }

// conv_flops() is the ALGORITHMIC count (the reference's op); ConvChoice::exec_scale of the launch gives the executed share
inline double conv_flops(const ConvDesc& d) {
  return 2.0 * (double)d.B * d.Hout * d.Wout * d.Cout * (double)(d.C0 + d.C1) * d.KH * d.KW;
}

// Direct (VALU) stem conv 7x7 pad 3: float32 NCHW (B,Cin,H,W) with Cin in {1,3} -> T NHWC (B,H,W,Cout).
// wk = float32 [49*Cin][Cout] (tap-major, then cin), bias float32 [Cout].
// stem on MFMA (bf16 path, Cin 1 or 3 -> 64): fragments packed once by pack_stem_mfma_weights
bool stem_conv_mfma_supported(int Cin, int Cout, int H, int W);
int launch_stem_conv_mfma(const float* x, const bf16_t* wf, const float* bias, bf16_t* out, int B, int Cin, int H, int W, hipStream_t s);
// f16x3 (round 5): the same kernel on f16 hi / lo halves with a float32 output; scale[64] = the inverse of the packer's per-channel power of two
int launch_stem_conv_mfma_split(const float* x, const uint16_t* wf, const float* bias, const float* wscale, float* out, int B, int Cin,
                                int H, int W, hipStream_t s);
template <typename T>
int launch_stem_conv(const float* x, const float* wk, const float* bias, T* out, int B, int Cin, int H, int W,
                     int Cout, hipStream_t s);

// Head: 1x1 conv to ONE channel (+ optional sigmoid): T NHWC (M, C) -> float32 (M,).
template <typename T>
int launch_head_conv(const T* x, const float* w, const float* bias, float* out, int64_t M, int C, int sigmoid,
                     hipStream_t s);

}  // namespace prg
