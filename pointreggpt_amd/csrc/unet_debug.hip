// unet_debug.hip — the prg_debug_* entries (prg.h): single convolutions, one convolution of any storage mode with the fused options of its launch
// (two sources, statistics, prologue, residual) and a ResnetBlock's Block pair through the library's own packer (pack_conv_host:
// what a handle would pack for the same conv) and dispatch (launch_conv), on device buffers of their own;
// the attention cores, the channel LayerNorm, the fused linear-attention blocks (pack_fused_attention / pack_split_attention)
// and the fused ResnetBlock tail through the launch functions the forward calls, with the kernel chosen by argument;
// the GroupNorm passes (statistics, coefficients, the fold from accumulators, the affine + SiLU pass) and the conditioning kernels
// (cond_fold, linear, sinusoidal) of blocks.hip, each through its own launch function on buffers the hook owns.
#include <cstring>
#include <type_traits>

#include "unet_layout.h"

using namespace prg;

namespace {

// the launch of one single-source conv on the packings of `pk`; a packing the conv does not have leaves its pointer null
template <typename T>
struct DebugConv {
  ConvLaunch<T> L{};
  int Ho = 0, Wo = 0;
  DebugConv(DeviceBuffers& own, const PackedConv<T>& pk, int B, int Cin, int Cout, int H, int W, int K, int stride, int pad, int ups,
            int groups, const char* nomem) {
    Ho = ups ? 2 * H : (H + 2 * pad - K) / stride + 1;
    Wo = ups ? 2 * W : (W + 2 * pad - K) / stride + 1;
    L.d.B = B; L.d.Hin = H; L.d.Win = W; L.d.C0 = Cin; L.d.C1 = 0; L.d.ups = ups; L.d.KH = K; L.d.KW = K; L.d.stride = stride; L.d.pad = pad;
    L.d.Hout = Ho; L.d.Wout = Wo; L.d.Cout = Cout; L.d.CoutPad = pk.CoutPad; L.d.kchunks = pk.kchunks;
    L.gn_groups = groups;
    L.w = own.upload(pk.main, nomem);
    L.w_s2d = own.upload(pk.s2d, nomem); L.s2d_kchunks = pk.s2d_kchunks;
    L.w_up = own.upload(pk.up, nomem);
    L.w_mx = own.upload(pk.mx, nomem); L.w_mx_scale = own.upload(pk.mx_scale, nomem);
    L.w_f16 = own.upload(pk.h16, nomem);
    L.w_split = own.upload(pk.split, nomem); L.split_kchunks = pk.split_kchunks;
    L.split_scale = own.upload(pk.split_scale, nomem);
    L.w_up_split = own.upload(pk.up_split, nomem);
    L.split_scale_up = own.upload(pk.up_split_scale, nomem);
  }
};

// float32-storage handles (PRG_F32: the exact-f32 kernels; PRG_F16X3: the split-operand kernels of conv_split.hip) and the bf16
// ones (PRG_BF16, PRG_MXFP8).  pad = 1 except for the 1x1 convs.
template <typename T>
int debug_conv_t(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W, int dtype,
                 int K, int stride, hipStream_t s, int ups) {
  constexpr bool f32 = std::is_same<T, float>::value;
  const char* nomem = f32 ? "prg_debug_conv: hipMalloc failed" : "prg_debug_conv3x3: hipMalloc failed";
  if (dtype == PRG_MXFP8) PRG_CHECK(Cin % 64 == 0 && Cout % 64 == 0, "prg_debug_conv3x3: MX-fp8 needs 64-channel multiples");
  ConvRole role;
  role.upsample = ups != 0;
  const PackedConv<T> pk = pack_conv_host<T>(w, Cout, Cin, K, dtype, role);
  DeviceBuffers own;
  DebugConv<T> c(own, pk, B, Cin, Cout, H, W, K, stride, K == 1 ? 0 : 1, ups, 8, nomem);
  const std::vector<float> zb(Cout, 0.0f);
  T* d_in = own.alloc<T>((size_t)B * H * W * Cin, nomem);
  c.L.src0 = d_in;
  c.L.out = own.alloc<T>((size_t)B * c.Ho * c.Wo * Cout, nomem);
  c.L.bias = own.upload(bias ? bias : zb.data(), (size_t)Cout, nomem);
  c.L.mx_pure = f32 ? 0 : 1;
  if (own.rc) return own.rc;
  int rc = launch_nchw_f32_to_nhwc<T>(x, d_in, B, H * W, Cin, s);
  if (rc == PRG_OK) rc = launch_conv<T>(c.L, s, nullptr);
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<T>(c.L.out, out, B, c.Ho * c.Wo, Cout, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK)
    rc = fail(PRG_E_HIP, f32 ? "prg_debug_conv: stream synchronise failed" : "prg_debug_conv3x3: stream synchronise failed");
  return rc;
}

int debug_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W, int dtype, int K,
               int stride, void* stream, int ups = 0) {
  PRG_CHECK(x && w && out, "prg_debug_conv3x3: null pointer");
  PRG_CHECK(B > 0 && H > 0 && W > 0 && Cin % 8 == 0 && Cout % 8 == 0, "prg_debug_conv3x3: bad shape");
  PRG_CHECK(dtype == PRG_BF16 || dtype == PRG_MXFP8 || dtype == PRG_F32 || dtype == PRG_F16X3, "prg_debug_conv3x3: bad dtype");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PRG_F32 || dtype == PRG_F16X3) return debug_conv_t<float>(x, w, bias, out, B, Cin, Cout, H, W, dtype, K, stride, s, ups);
  return debug_conv_t<bf16_t>(x, w, bias, out, B, Cin, Cout, H, W, dtype, K, stride, s, ups);
}

// the attention cores on a qkv tensor of their own: T is the storage type, `mp` selects the matrix-pipe kernel of `dtype`
template <typename T>
int debug_attention_core_t(const float* qkv, float* out, int B, int N, int linear, int mp, hipStream_t s) {
  const char* nomem = "prg_debug_attention_core: hipMalloc failed";
  DeviceBuffers own;
  T* d_qkv = own.alloc<T>((size_t)B * N * 3 * kHidden, nomem);
  T* d_out = own.alloc<T>((size_t)B * N * kHidden, nomem);
  float* ws = linear ? own.alloc<float>(linattn_ws_floats(B, N), nomem) : nullptr;
  if (own.rc) return own.rc;
  int rc = launch_nchw_f32_to_nhwc<T>(qkv, d_qkv, B, N, 3 * kHidden, s);
  if (rc == PRG_OK) {
    if (linear) {
      rc = launch_linear_attention<T>(d_qkv, d_out, ws, B, N, s);
    } else if (!mp) {
      rc = launch_full_attention<T>(d_qkv, d_out, B, N, s);
    } else if constexpr (std::is_same<T, float>::value) {
      rc = launch_full_attention_split(d_qkv, d_out, B, N, s);
    } else {
      rc = launch_full_attention_mfma(d_qkv, d_out, B, N, s);
    }
  }
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<T>(d_out, out, B, N, kHidden, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_attention_core: stream synchronise failed");
  return rc;
}

// (M, C) float32 -> T and back without a change of layout: the NCHW <-> NHWC kernels with one channel are plain conversions
template <typename T>
int debug_layernorm_t(const float* x, const float* g, const float* residual, float* out, int64_t M, int C, hipStream_t s) {
  const char* nomem = "prg_debug_layernorm: hipMalloc failed";
  const size_t n = (size_t)M * C;
  DeviceBuffers own;
  T* d_x = own.alloc<T>(n, nomem);
  T* d_r = residual ? own.alloc<T>(n, nomem) : nullptr;
  T* d_o = own.alloc<T>(n, nomem);
  const float* d_g = own.upload(g, (size_t)C, nomem);
  if (own.rc) return own.rc;
  int rc = launch_nchw_f32_to_nhwc<T>(x, d_x, 1, (int)n, 1, s);
  if (rc == PRG_OK && residual) rc = launch_nchw_f32_to_nhwc<T>(residual, d_r, 1, (int)n, 1, s);
  if (rc == PRG_OK) rc = launch_layernorm<T>(d_x, d_g, d_r, d_o, M, C, s);
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<T>(d_o, out, 1, (int)n, 1, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_layernorm: stream synchronise failed");
  return rc;
}

// device-to-device copy of `count` elements on the stream
template <typename U>
bool copy_dd(U* dst, const U* src, size_t count, hipStream_t s) {
  return count == 0 || hipMemcpyAsync(dst, src, count * sizeof(U), hipMemcpyDeviceToDevice, s) == hipSuccess;
}

// what is wrong with a set of conditioning rows of `width` floats (GnApply's addressing), or null: every read stays inside its array
const char* cond_rows_bad(const float* ss_a, int64_t ss_a_stride, int64_t ss_a_floats, const float* ss_b, int64_t ss_b_stride,
                          int64_t ss_b_floats, const int* row, int64_t row_stride, int B, int64_t width) {
  const int64_t lim = (int64_t)1 << 28;
  if (!ss_a) return nullptr;
  if (ss_a_stride < 0 || ss_a_stride > lim || row_stride < 0 || row_stride > lim || ss_a_floats <= 0 || ss_a_floats > lim)
    return "ss_a strides and size out of range";
  if (row && (*row < 0 || *row > 1 << 20)) return "row out of range";
  if ((int64_t)(B - 1) * ss_a_stride + (row ? (int64_t)*row * row_stride : 0) + width > ss_a_floats) return "ss_a is read past its end";
  if (!ss_b) return nullptr;
  if (ss_b_stride < 0 || ss_b_stride > lim || ss_b_floats <= 0 || ss_b_floats > lim) return "ss_b stride and size out of range";
  if ((int64_t)(B - 1) * ss_b_stride + width > ss_b_floats) return "ss_b is read past its end";
  return nullptr;
}

int debug_gn_stats_t(const float* x, float* slabs, int* nsplit, int B, int C, int HW, int G, bool bf16, hipStream_t s) {
  const char* nomem = "prg_debug_gn_stats: hipMalloc failed";
  const size_t M = (size_t)B * HW * C;
  DeviceBuffers own;
  bf16_t* d_xb = bf16 ? own.alloc<bf16_t>(M, nomem) : nullptr;
  float* d_xf = bf16 ? nullptr : own.alloc<float>(M, nomem);
  float* d_slabs = own.alloc<float>((size_t)B * kGnMaxSplit * G * 2, nomem);
  if (own.rc) return own.rc;
  int ns = 0;
  int rc = bf16 ? launch_nchw_f32_to_nhwc<bf16_t>(x, d_xb, B, HW, C, s) : launch_nchw_f32_to_nhwc<float>(x, d_xf, B, HW, C, s);
  if (rc == PRG_OK) rc = bf16 ? launch_gn_stats<bf16_t>(d_xb, d_slabs, B, HW, C, G, &ns, s) : launch_gn_stats<float>(d_xf, d_slabs, B, HW, C, G, &ns, s);
  if (rc == PRG_OK && (ns < 1 || ns > kGnMaxSplit)) rc = fail(PRG_E_INVALID, "prg_debug_gn_stats: slab count out of range");
  if (rc == PRG_OK && !copy_dd(slabs, d_slabs, (size_t)B * ns * G * 2, s)) rc = fail(PRG_E_HIP, "prg_debug_gn_stats: copy failed");
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_gn_stats: stream synchronise failed");
  if (rc == PRG_OK) *nsplit = ns;
  return rc;
}

template <typename T>
int debug_affine_silu_t(const float* x, const float* A, const float* Bc, const float* residual, float* out, int B, int C, int HW,
                        int in_place, hipStream_t s) {
  const char* nomem = "prg_debug_affine_silu: hipMalloc failed";
  const size_t M = (size_t)B * HW * C, nc = (size_t)B * C;
  DeviceBuffers own;
  T* d_x = own.alloc<T>(M, nomem);
  T* d_r = residual ? own.alloc<T>(M, nomem) : nullptr;
  T* d_o = in_place ? d_x : own.alloc<T>(M, nomem);
  float* d_ab = own.alloc<float>(2 * nc, nomem);
  if (own.rc) return own.rc;
  if (!copy_dd(d_ab, A, nc, s) || !copy_dd(d_ab + nc, Bc, nc, s)) return fail(PRG_E_HIP, "prg_debug_affine_silu: copy failed");
  int rc = launch_nchw_f32_to_nhwc<T>(x, d_x, B, HW, C, s);
  if (rc == PRG_OK && d_r) rc = launch_nchw_f32_to_nhwc<T>(residual, d_r, B, HW, C, s);
  if (rc == PRG_OK) rc = launch_affine_silu<T>(d_x, d_ab, d_ab + nc, d_r, d_o, B, HW, C, s);
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<T>(d_o, out, B, HW, C, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_affine_silu: stream synchronise failed");
  return rc;
}

// prg_debug_conv_fused after its checks: T = bf16_t with packing dtype PRG_BF16, or float with PRG_F16X3 / PRG_F32, so the packer,
// DebugConv<T> and launch_conv<T> are those of a handle of that mode
template <typename T>
int debug_conv_fused_t(prg_conv_fused* a, const ConvDesc& d, int dtype, hipStream_t s) {
  const int B = a->B, C0 = a->C0, C1 = a->C1, Cout = a->Cout, H = a->H, W = a->W, K = a->K, G = a->groups;
  const int fold_C = a->prologue == PRG_CF_PRO_FOLD ? C0 : Cout;   // width of the tensor the folded norm belongs to
  const bool folds = a->prologue == PRG_CF_PRO_FOLD || a->residual_mode == PRG_CF_RES_FOLD;
  const char* nomem = "prg_debug_conv_fused: hipMalloc failed";
  const int cin = C0 + C1, HW = H * W;
  const size_t M = (size_t)B * HW;
  const PackedConv<T> pk = pack_conv_host<T>(a->w, Cout, cin, K, dtype, ConvRole{});
  DeviceBuffers own;
  DebugConv<T> c(own, pk, B, cin, Cout, H, W, K, 1, d.pad, 0, G, nomem);
  ConvLaunch<T>& L = c.L;
  L.d.C0 = C0; L.d.C1 = C1;
  T* d_x0 = own.alloc<T>(M * C0, nomem);
  T* d_x1 = own.alloc<T>(M * C1, nomem);
  T* d_res = a->residual ? own.alloc<T>(M * Cout, nomem) : nullptr;
  L.src0 = d_x0; L.src1 = d_x1;
  L.out = a->in_place ? d_res : own.alloc<T>(M * Cout, nomem);
  L.bias = a->bias ? own.upload(a->bias, (size_t)Cout, nomem) : nullptr;   // (null stays null: the generic kernels take it)
  L.residual = d_res;
  GnFold in_fold{};
  if (folds) {
    std::vector<float> pq(2 * (size_t)fold_C);
    for (int ch = 0; ch < fold_C; ++ch) { pq[ch] = a->fold_p[ch]; pq[fold_C + ch] = a->fold_q[ch]; }
    in_fold.acc = reinterpret_cast<const long long*>(a->fold_acc);
    in_fold.P = own.upload(pq, nomem); in_fold.Q = in_fold.P + fold_C; in_fold.pq_stride = 0;
    in_fold.G = G; in_fold.cpg = fold_C / G; in_fold.inv_n = 1.0f / ((float)HW * (float)in_fold.cpg);
  }
  if (a->prologue == PRG_CF_PRO_TABLES) { L.pro_a = a->pro_a; L.pro_b = a->pro_b; }
  if (a->prologue == PRG_CF_PRO_FOLD) {   // (the tables are scratch for kernels without the in-kernel fold, as in resblock())
    L.pro_fold = in_fold;
    L.pro_a = own.alloc<float>((size_t)2 * B * C0, nomem); L.pro_b = L.pro_a + (size_t)B * C0;
  }
  if (a->residual_mode == PRG_CF_RES_TABLES) { L.res_a = a->res_a; L.res_b = a->res_b; }
  if (a->residual_mode == PRG_CF_RES_FOLD) L.res_fold = in_fold;
  const size_t slab_floats = (size_t)B * kGnMaxSplit * G * 2, acc_count = (size_t)B * G * 2;
  GnApply apply{};
  GnFold out_fold{};
  if (a->stats != PRG_CF_STATS_OFF) {
    L.gn_partials = own.alloc<float>(slab_floats, nomem);
    std::vector<float> gb(2 * (size_t)Cout);
    for (int ch = 0; ch < Cout; ++ch) { gb[ch] = a->gamma[ch]; gb[Cout + ch] = a->beta[ch]; }
    apply.gamma = own.upload(gb, nomem); apply.beta = apply.gamma + Cout;
    if (a->stats == PRG_CF_STATS_ACC) {
      L.gn_acc = own.alloc<long long>(acc_count, nomem);
      out_fold.acc = L.gn_acc; out_fold.P = apply.gamma; out_fold.Q = apply.beta; out_fold.pq_stride = 0;
      out_fold.G = G; out_fold.cpg = Cout / G; out_fold.inv_n = 1.0f / ((float)HW * (float)out_fold.cpg);
    }
  }
  if (own.rc) return own.rc;
  const char* nocopy = "prg_debug_conv_fused: copy failed";
  if (L.gn_acc && hipMemsetAsync(L.gn_acc, 0, acc_count * sizeof(long long), s) != hipSuccess) return fail(PRG_E_HIP, nocopy);
  int rc = launch_nchw_f32_to_nhwc<T>(a->x0, d_x0, B, HW, C0, s);
  if (rc == PRG_OK && C1) rc = launch_nchw_f32_to_nhwc<T>(a->x1, d_x1, B, HW, C1, s);
  if (rc == PRG_OK && d_res) rc = launch_nchw_f32_to_nhwc<T>(a->residual, d_res, B, HW, Cout, s);
  int ns = 0, ad = 0, used = 0;
  ConvChoice chosen;
  if (rc == PRG_OK) rc = launch_conv<T>(L, s, a->stats ? &ns : nullptr, a->stats ? &ad : nullptr, &chosen);
  a->family = chosen.family; a->th = chosen.th; a->tw = chosen.tw; a->bm = chosen.bm; a->bn = chosen.bn;
  used = ns;
  if (rc == PRG_OK && a->stats && ns == 0) {   // (NormStats::complete: the conv fused no statistics)
    rc = launch_gn_stats<T>(L.out, L.gn_partials, B, HW, Cout, G, &used, s);
    a->stats_pass = 1;
  }
  if (rc == PRG_OK && a->stats)                // (NormStats::tables)
    rc = ad ? launch_gn_coeff_acc(out_fold, a->coef_a, a->coef_b, B, Cout, s)
            : launch_gn_coeff(L.gn_partials, used, apply, a->coef_a, a->coef_b, B, HW, Cout, G, s);
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<T>(L.out, a->out, B, HW, Cout, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_conv_fused: stream synchronise failed");
  if (rc != PRG_OK || !a->stats) return rc;
  a->nsplit = ns; a->acc_done = ad;
  std::vector<long long> acc(acc_count, 0);
  if (L.gn_acc && hipMemcpy(acc.data(), L.gn_acc, acc_count * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return fail(PRG_E_HIP, nocopy);
  if (a->acc_raw) for (size_t i = 0; i < acc_count; ++i) a->acc_raw[i] = acc[i];
  if (ad) {
    for (size_t i = 0; i < acc_count; ++i) a->sums[i] = (double)acc[i] * (i & 1 ? 1.0 / 1048576.0 : 1.0 / 16777216.0);
    return PRG_OK;
  }
  PRG_CHECK(used > 0 && used <= kGnMaxSplit, "prg_debug_conv_fused: slab count out of range");
  std::vector<float> slabs((size_t)B * used * G * 2);
  if (hipMemcpy(slabs.data(), L.gn_partials, slabs.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return fail(PRG_E_HIP, nocopy);
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g)
      for (int w = 0; w < 2; ++w) {
        double t = 0.0;
        for (int k = 0; k < used; ++k) t += (double)slabs[(((size_t)b * used + k) * G + g) * 2 + w];
        a->sums[((size_t)b * G + g) * 2 + w] = t;
      }
  if (a->slabs) {
    std::memcpy(a->slabs, slabs.data(), slabs.size() * sizeof(float));
    a->nslabs = used;
  }
  return PRG_OK;
}

}  // namespace

extern "C" {

// The linear-attention core and the three bottleneck attention cores on a given qkv (prg.h).
int prg_debug_attention_core(const float* qkv, float* out, int B, int N, int dtype, int linear, int kernel, void* stream) {
  PRG_CHECK(qkv && out, "prg_debug_attention_core: null pointer");
  PRG_CHECK(B > 0 && B <= 65535 && N > 0 && (int64_t)B * N <= (int64_t)1 << 22, "prg_debug_attention_core: bad shape");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16 || dtype == PRG_F16X3, "prg_debug_attention_core: bad dtype");
  PRG_CHECK((linear == 0 || linear == 1) && (kernel == 0 || kernel == 1), "prg_debug_attention_core: linear and kernel are 0 or 1");
  PRG_CHECK(!linear || (dtype != PRG_F16X3 && kernel == 0),
            "prg_debug_attention_core: the linear core has one kernel, in PRG_F32 and PRG_BF16");
  if (kernel) {
    PRG_CHECK(dtype != PRG_F32, "prg_debug_attention_core: PRG_F32 has no matrix-pipe kernel");
    PRG_CHECK(dtype == PRG_BF16 ? full_attention_mfma_supported(N) : full_attention_split_supported(N),
              "prg_debug_attention_core: the matrix-pipe kernel does not take this token count");
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PRG_BF16) return debug_attention_core_t<bf16_t>(qkv, out, B, N, linear, kernel, s);
  return debug_attention_core_t<float>(qkv, out, B, N, linear, kernel, s);
}

// Residual(PreNorm(LinearAttention)) through the fused bf16 kernels or the split-f16 ones, on what a handle would pack (prg.h).
int prg_debug_linear_attention_block(const float* x, const float* norm_g, const float* w_qkv, const float* w_out, const float* b_out,
                                     const float* out_g, float* out, int B, int C, int N, int dtype, int shift_mode, int psum,
                                     int* used_static, void* stream) {
  PRG_CHECK(x && norm_g && w_qkv && w_out && b_out && out_g && out, "prg_debug_linear_attention_block: null pointer");
  PRG_CHECK(dtype == PRG_BF16 || dtype == PRG_F16X3, "prg_debug_linear_attention_block: bad dtype");
  // (N <= 2^21: at most 4096 slabs of eight 64-pixel tiles, the limit of launch_linear_attention_fused)
  PRG_CHECK(B > 0 && B <= 65535 && N > 0 && N <= 1 << 21 && C > 0 && (int64_t)B * N <= (int64_t)1 << 22,
            "prg_debug_linear_attention_block: bad shape");
  PRG_CHECK(dtype == PRG_BF16 ? linattn_fused_supported(C) : linattn_split_supported(C, N),
            "prg_debug_linear_attention_block: the kernels of this dtype do not take this width and token count");
  PRG_CHECK(shift_mode >= -1 && shift_mode <= 1 && psum >= -1 && psum <= 1, "prg_debug_linear_attention_block: shift_mode and psum are -1, 0 or 1");
  PRG_CHECK(dtype == PRG_BF16 || (shift_mode == -1 && psum == -1),
            "prg_debug_linear_attention_block: shift_mode and psum choose among the bf16 kernels only");
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_linear_attention_block: hipMalloc failed";
  const char* nosync = "prg_debug_linear_attention_block: stream synchronise failed";
  const size_t M = (size_t)B * N;
  int rc;
  if (dtype == PRG_F16X3) {
    SplitAttnPack pk;
    pack_split_attention(w_qkv, norm_g, w_out, C, pk);
    if (used_static) *used_static = 0;
    DeviceBuffers own;
    const uint16_t* qh = own.upload(pk.qkv, nomem);
    const uint16_t* oh = own.upload(pk.out, nomem);
    const float* d_bias = own.upload(b_out, (size_t)C, nomem);
    const float* d_outg = own.upload(out_g, (size_t)C, nomem);
    float* d_x = own.alloc<float>(M * C, nomem);
    float* d_out = own.alloc<float>(M * C, nomem);
    float* ws = own.alloc<float>(linattn_split_ws_floats(B, N), nomem);
    if (own.rc) return own.rc;
    rc = launch_nchw_f32_to_nhwc<float>(x, d_x, B, N, C, s);
    if (rc == PRG_OK)
      rc = launch_linear_attention_split(d_x, qh, qh + (size_t)3 * kHidden * C, oh, oh + (size_t)C * kHidden, d_bias, d_outg, d_out, ws, B, N, C, s);
    if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<float>(d_out, out, B, N, C, s);
    if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, nosync);
    return rc;
  }
  FusedAttnPack pk;
  pack_fused_attention(w_qkv, norm_g, w_out, C, pk);
  PRG_CHECK(shift_mode != 1 || pk.ok, "prg_debug_linear_attention_block: the static softmax bound does not hold for these weights");
  // shift_mode -1: what a handle does with this block (unet_weights.hip)
  const bool stat = shift_mode == 1 || (shift_mode == -1 && pk.ok && env_int("PRG_LA_KSHIFT", 1) != 0);
  if (used_static) *used_static = stat ? 1 : 0;
  DeviceBuffers own;
  const bf16_t* d_wqkv = own.upload(pk.qkv, nomem);
  const bf16_t* d_wout = own.upload(pk.out, nomem);
  const float* d_shift = own.upload(pk.shifts, (size_t)(kHidden + kHeads), nomem);
  const float* d_bias = own.upload(b_out, (size_t)C, nomem);
  const float* d_outg = own.upload(out_g, (size_t)C, nomem);
  bf16_t* d_x = own.alloc<bf16_t>(M * C, nomem);
  bf16_t* d_out = own.alloc<bf16_t>(M * C, nomem);
  float* ws = own.alloc<float>(linattn_fused_ws_floats(B, N), nomem);
  if (own.rc) return own.rc;
  rc = launch_nchw_f32_to_nhwc<bf16_t>(x, d_x, B, N, C, s);
  if (rc == PRG_OK) rc = launch_linear_attention_fused(d_x, d_wqkv, d_wout, d_bias, d_outg, d_out, ws, B, N, C, stat ? d_shift : nullptr, s, psum);
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<bf16_t>(d_out, out, B, N, C, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, nosync);
  return rc;
}

// The fused ResnetBlock tail on tensors of its own, with the res_conv weight packed as a handle packs it (prg.h).
int prg_debug_resblock_tail(const float* h, const float* s0, const float* s1, const float* A, const float* Bc, const float* w_res,
                            const float* b_res, const float* head_w, const float* head_b, float* out, int B, int N, int C0, int C1,
                            int Cout, int head_sigmoid, int in_place, void* stream) {
  PRG_CHECK(h && s0 && s1 && A && Bc && w_res && b_res && out, "prg_debug_resblock_tail: null pointer");
  PRG_CHECK((head_w != nullptr) == (head_b != nullptr), "prg_debug_resblock_tail: head_w and head_b come together");
  PRG_CHECK(B > 0 && B <= 65535 && N > 0 && (int64_t)B * N <= (int64_t)1 << 22, "prg_debug_resblock_tail: bad shape");
  PRG_CHECK(C0 > 0 && C1 > 0 && Cout > 0 && resblock_tail_fused_supported(C0, C1, Cout),
            "prg_debug_resblock_tail: the kernel does not take these channel counts");
  PRG_CHECK(!head_w || Cout == 64, "prg_debug_resblock_tail: the head needs Cout = 64");
  PRG_CHECK((head_sigmoid == 0 || head_sigmoid == 1) && (in_place == 0 || in_place == 1),
            "prg_debug_resblock_tail: head_sigmoid and in_place are 0 or 1");
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_resblock_tail: hipMalloc failed";
  const size_t M = (size_t)B * N;
  const int cin = C0 + C1;
  std::vector<bf16_t> wb((size_t)Cout * cin);
  for (size_t i = 0; i < wb.size(); ++i) wb[i] = f32_to_bf16(w_res[i]);   // (upload_fused_attention: the raw weight as bf16)
  DeviceBuffers own;
  const bf16_t* d_w = own.upload(wb, nomem);
  const float* d_b = own.upload(b_res, (size_t)Cout, nomem);
  const float* d_hw = head_w ? own.upload(head_w, (size_t)Cout, nomem) : nullptr;
  const float* d_hb = head_b ? own.upload(head_b, (size_t)1, nomem) : nullptr;
  bf16_t* d_h = own.alloc<bf16_t>(M * Cout, nomem);
  bf16_t* d_s0 = own.alloc<bf16_t>(M * C0, nomem);
  bf16_t* d_s1 = own.alloc<bf16_t>(M * C1, nomem);
  bf16_t* d_o = in_place ? d_h : own.alloc<bf16_t>(M * Cout, nomem);
  if (own.rc) return own.rc;
  // (pixel-major already: the layout kernels with one channel are plain conversions)
  int rc = launch_nchw_f32_to_nhwc<bf16_t>(h, d_h, 1, (int)(M * Cout), 1, s);
  if (rc == PRG_OK) rc = launch_nchw_f32_to_nhwc<bf16_t>(s0, d_s0, 1, (int)(M * C0), 1, s);
  if (rc == PRG_OK) rc = launch_nchw_f32_to_nhwc<bf16_t>(s1, d_s1, 1, (int)(M * C1), 1, s);
  if (rc == PRG_OK)
    rc = launch_resblock_tail_fused(d_h, A, Bc, d_s0, C0, d_s1, C1, d_w, d_b, d_o, B, N, Cout, s, d_hw, d_hb, head_w ? out : nullptr,
                                    head_sigmoid, nullptr);
  if (rc == PRG_OK && !head_w) rc = launch_nhwc_to_nchw_f32<bf16_t>(d_o, out, 1, (int)(M * Cout), 1, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_resblock_tail: stream synchronise failed");
  return rc;
}

// Channel LayerNorm (+ residual) on pixel-major rows (prg.h).
int prg_debug_layernorm(const float* x, const float* g, const float* residual, float* out, int64_t M, int C, int dtype, void* stream) {
  PRG_CHECK(x && g && out, "prg_debug_layernorm: null pointer");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16, "prg_debug_layernorm: bad dtype");
  const int vec = dtype == PRG_F32 ? 4 : 8;
  // (launch_layernorm: at most four 16-byte vectors in each of 64 lanes)
  PRG_CHECK(C > 0 && C % vec == 0 && C / vec <= 256, "prg_debug_layernorm: C must be a multiple of the vector width, at most 256 vectors");
  PRG_CHECK(M > 0 && M <= (int64_t)0x7fffffff / C, "prg_debug_layernorm: bad row count");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PRG_BF16) return debug_layernorm_t<bf16_t>(x, g, residual, out, M, C, s);
  return debug_layernorm_t<float>(x, g, residual, out, M, C, s);
}

// The two convolutions of a ResnetBlock's Block pair in bf16 mode, through the library's own dispatch (prg.h).
int prg_debug_block_pair(const float* x, const float* w1, const float* b1, const float* gamma, const float* beta, const float* w2,
                         const float* b2, float* out, int B, int Cin, int C, int H, int W, int groups, int h16, void* stream) {
  PRG_CHECK(x && w1 && b1 && gamma && beta && w2 && b2 && out, "prg_debug_block_pair: null pointer");
  PRG_CHECK(B > 0 && H > 0 && W > 0 && Cin % 64 == 0 && C % 64 == 0 && groups > 0 && C % groups == 0 && (C / groups) % 8 == 0,
            "prg_debug_block_pair: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_block_pair: hipMalloc failed";
  const size_t M = (size_t)B * H * W;
  ConvRole conv2;
  conv2.conv2 = true;       // (with the f16 twin of its packing)
  const PackedConv<bf16_t> p1 = pack_conv_host<bf16_t>(w1, C, Cin, 3, PRG_BF16, ConvRole{});
  const PackedConv<bf16_t> p2 = pack_conv_host<bf16_t>(w2, C, C, 3, PRG_BF16, conv2);
  std::vector<float> pq(2 * (size_t)C);
  for (int c = 0; c < C; ++c) { pq[c] = gamma[c]; pq[C + c] = beta[c]; }
  DeviceBuffers own;
  DebugConv<bf16_t> c1(own, p1, B, Cin, C, H, W, 3, 1, 1, 0, groups, nomem), c2(own, p2, B, C, C, H, W, 3, 1, 1, 0, groups, nomem);
  ConvLaunch<bf16_t>&L1 = c1.L, &L2 = c2.L;
  const size_t acc_count = (size_t)B * groups * 2;
  bf16_t* d_x = own.alloc<bf16_t>(M * Cin, nomem);
  bf16_t* d_h = own.alloc<bf16_t>(M * C, nomem);
  L1.src0 = d_x; L1.out = d_h; L1.bias = own.upload(b1, (size_t)C, nomem);
  L1.gn_partials = own.alloc<float>((size_t)B * kGnMaxSplit * groups * 2, nomem);
  L1.gn_acc = own.alloc<long long>(acc_count, nomem);
  L2.src0 = d_h; L2.out = own.alloc<bf16_t>(M * C, nomem); L2.bias = own.upload(b2, (size_t)C, nomem);
  GnFold f{};
  f.acc = L1.gn_acc; f.P = own.upload(pq, nomem); f.Q = f.P + C; f.pq_stride = 0;
  f.G = groups; f.cpg = C / groups; f.inv_n = 1.0f / ((float)(H * W) * (float)f.cpg);
  L2.pro_fold = f;
  L2.pro_a = own.alloc<float>((size_t)2 * B * C, nomem); L2.pro_b = L2.pro_a + (size_t)B * C;
  if (own.rc) return own.rc;
  if (hipMemsetAsync(L1.gn_acc, 0, acc_count * sizeof(long long), s) != hipSuccess) return fail(PRG_E_HIP, "prg_debug_block_pair: upload failed");
  int rc = launch_nchw_f32_to_nhwc<bf16_t>(x, d_x, B, H * W, Cin, s);
  if (rc == PRG_OK && h16) {
    if (!conv_h16_pair_ok(L1, L2)) rc = fail(PRG_E_INVALID, "prg_debug_block_pair: the kernels this shape dispatches to do not implement the f16 format");
    L1.out_f16 = 1;
    L2.in_f16 = 1;
  }
  int ns = 0, ad = 0;
  if (rc == PRG_OK) rc = launch_conv<bf16_t>(L1, s, &ns, &ad);
  if (rc == PRG_OK && !ad) rc = fail(PRG_E_INVALID, "prg_debug_block_pair: conv1's kernel does not accumulate fixed-point statistics for this shape");
  if (rc == PRG_OK) rc = launch_conv<bf16_t>(L2, s, nullptr);
  if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<bf16_t>(L2.out, out, B, H * W, C, s);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_block_pair: stream synchronise failed");
  return rc;
}

// One convolution (bf16, or float storage: f16x3 / fp32) with the fused options of ConvLaunch, as the forward pass sets them (prg.h).
int prg_debug_conv_fused(prg_conv_fused* a, void* stream) {
  PRG_CHECK(a != nullptr, "prg_debug_conv_fused: null argument struct");
  a->nsplit = a->acc_done = a->stats_pass = 0;
  a->family = a->th = a->tw = a->bm = a->bn = a->nslabs = 0;
  const int B = a->B, C0 = a->C0, C1 = a->C1, Cout = a->Cout, H = a->H, W = a->W, K = a->K, G = a->groups;
  PRG_CHECK(a->x0 && a->w && a->out, "prg_debug_conv_fused: null pointer");
  PRG_CHECK(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)B * H * W <= (int64_t)1 << 22, "prg_debug_conv_fused: bad shape");
  PRG_CHECK(C0 > 0 && C1 >= 0 && Cout > 0 && C0 % 8 == 0 && C1 % 8 == 0 && Cout % 8 == 0 && C0 <= 4096 && C1 <= 4096 && Cout <= 4096,
            "prg_debug_conv_fused: channel counts are multiples of 8");
  PRG_CHECK((a->x1 != nullptr) == (C1 > 0), "prg_debug_conv_fused: x1 is given exactly when C1 > 0");
  PRG_CHECK(K == 1 || K == 3, "prg_debug_conv_fused: K is 1 or 3");
  PRG_CHECK(G > 0 && Cout % G == 0 && (Cout / G) % 8 == 0, "prg_debug_conv_fused: groups must cut Cout into multiples of 8 channels");
  PRG_CHECK(a->prologue >= PRG_CF_PRO_NONE && a->prologue <= PRG_CF_PRO_FOLD, "prg_debug_conv_fused: bad prologue mode");
  PRG_CHECK(a->residual_mode >= PRG_CF_RES_NONE && a->residual_mode <= PRG_CF_RES_FOLD, "prg_debug_conv_fused: bad residual mode");
  PRG_CHECK(a->stats >= PRG_CF_STATS_OFF && a->stats <= PRG_CF_STATS_ACC, "prg_debug_conv_fused: bad statistics mode");
  PRG_CHECK(a->in_place == 0 || a->in_place == 1, "prg_debug_conv_fused: in_place is 0 or 1");
  PRG_CHECK(a->storage >= PRG_CF_STORE_BF16 && a->storage <= PRG_CF_STORE_F32, "prg_debug_conv_fused: bad storage mode");
  const bool f32 = a->storage != PRG_CF_STORE_BF16;
  // float launches have no fixed-point accumulators (acc_on() is bf16-only) and choose_split declines the folds
  PRG_CHECK(!f32 || (a->prologue != PRG_CF_PRO_FOLD && a->residual_mode != PRG_CF_RES_FOLD && a->stats != PRG_CF_STATS_ACC),
            "prg_debug_conv_fused: the folds and the accumulators belong to bf16 storage");
  ConvDesc d{};
  d.B = B; d.Hin = H; d.Win = W; d.C0 = C0; d.C1 = C1; d.ups = 0; d.KH = K; d.KW = K; d.stride = 1; d.pad = K == 3 ? 1 : 0;
  d.Hout = H; d.Wout = W; d.Cout = Cout;
  const int fold_C = a->prologue == PRG_CF_PRO_FOLD ? C0 : Cout;   // width of the tensor the folded norm belongs to
  const bool folds = a->prologue == PRG_CF_PRO_FOLD || a->residual_mode == PRG_CF_RES_FOLD;
  if (a->prologue != PRG_CF_PRO_NONE) {
    PRG_CHECK(K == 3 && C1 == 0, "prg_debug_conv_fused: the prologue belongs to a single-source 3x3 conv");
    PRG_CHECK(f32 ? conv_supports_prologue<float>(d) : conv_supports_prologue<bf16_t>(d),
              "prg_debug_conv_fused: no kernel with a prologue takes this shape");
    PRG_CHECK(a->prologue != PRG_CF_PRO_TABLES || (a->pro_a && a->pro_b), "prg_debug_conv_fused: the table prologue needs pro_a and pro_b");
  }
  if (a->residual_mode != PRG_CF_RES_NONE) {
    PRG_CHECK(K == 1, "prg_debug_conv_fused: the residual belongs to a 1x1 conv");
    PRG_CHECK(a->residual != nullptr, "prg_debug_conv_fused: residual mode without a residual");
    PRG_CHECK(a->residual_mode != PRG_CF_RES_TABLES || (a->res_a && a->res_b), "prg_debug_conv_fused: the table residual needs res_a and res_b");
  } else {
    PRG_CHECK(a->residual == nullptr && a->in_place == 0, "prg_debug_conv_fused: residual and in_place need a residual mode");
  }
  if (folds) {
    PRG_CHECK(a->fold_acc && a->fold_p && a->fold_q, "prg_debug_conv_fused: fold mode needs fold_acc, fold_p and fold_q");
    PRG_CHECK(fold_C % G == 0 && (fold_C / G) % 8 == 0, "prg_debug_conv_fused: groups must cut the folded tensor into multiples of 8 channels");
  }
  if (a->stats != PRG_CF_STATS_OFF) {
    PRG_CHECK(K == 3, "prg_debug_conv_fused: statistics belong to a 3x3 conv");
    PRG_CHECK(G <= 64 && Cout <= 1024, "prg_debug_conv_fused: the coefficient kernels take at most 64 groups and 1024 channels");
    PRG_CHECK(a->gamma && a->beta && a->sums && a->coef_a && a->coef_b, "prg_debug_conv_fused: statistics need gamma, beta, sums, coef_a and coef_b");
    PRG_CHECK(a->stats != PRG_CF_STATS_ACC || a->acc_raw, "prg_debug_conv_fused: offered accumulators need acc_raw");
  }
  const int dtype = a->storage == PRG_CF_STORE_F16X3 ? PRG_F16X3 : a->storage == PRG_CF_STORE_F32 ? PRG_F32 : PRG_BF16;
  if (f32) return debug_conv_fused_t<float>(a, d, dtype, (hipStream_t)stream);
  return debug_conv_fused_t<bf16_t>(a, d, dtype, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// the GroupNorm passes and the conditioning kernels of blocks.hip, alone (prg.h)
// ---------------------------------------------------------------------------------------------
int prg_debug_gn_stats(const float* x, float* slabs, int* nsplit, int B, int C, int HW, int groups, int dtype, void* stream) {
  PRG_CHECK(x && slabs && nsplit, "prg_debug_gn_stats: null pointer");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16, "prg_debug_gn_stats: bad dtype");
  const int vec = dtype == PRG_F32 ? 4 : 8;
  PRG_CHECK(C > 0 && C % vec == 0 && C / vec <= 256 && ((C / vec) & (C / vec - 1)) == 0,
            "prg_debug_gn_stats: C / vec must be a power of two <= 256");
  PRG_CHECK(groups > 0 && groups <= 64 && C % groups == 0, "prg_debug_gn_stats: bad group count");
  PRG_CHECK(B > 0 && B <= 65535 && HW > 0 && (int64_t)B * HW * C <= (int64_t)1 << 26, "prg_debug_gn_stats: bad shape");
  *nsplit = 0;
  hipStream_t s = (hipStream_t)stream;
  return debug_gn_stats_t(x, slabs, nsplit, B, C, HW, groups, dtype == PRG_BF16, s);
}

int prg_debug_gn_coeff(const float* slabs, int nsplit, const float* gamma, const float* beta, const float* ss_a, int64_t ss_a_stride,
                       int64_t ss_a_floats, const float* ss_b, int64_t ss_b_stride, int64_t ss_b_floats, const int* row,
                       int64_t row_stride, float* A, float* Bc, int B, int HW, int C, int groups, void* stream) {
  PRG_CHECK(slabs && gamma && beta && A && Bc, "prg_debug_gn_coeff: null pointer");
  PRG_CHECK(B > 0 && B <= 65535 && HW > 0 && nsplit > 0 && nsplit <= kGnMaxSplit, "prg_debug_gn_coeff: bad shape");
  PRG_CHECK(C > 0 && C <= 1024 && groups > 0 && groups <= 64 && C % groups == 0, "prg_debug_gn_coeff: at most 1024 channels in at most 64 groups");
  PRG_CHECK(ss_a || (!ss_b && !row), "prg_debug_gn_coeff: ss_b and row come with ss_a");
  const char* why = cond_rows_bad(ss_a, ss_a_stride, ss_a_floats, ss_b, ss_b_stride, ss_b_floats, row, row_stride, B, 2 * (int64_t)C);
  PRG_CHECK(!why, std::string("prg_debug_gn_coeff: ") + (why ? why : ""));
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_gn_coeff: hipMalloc failed";
  DeviceBuffers own;
  const size_t nslab = (size_t)B * nsplit * groups * 2;
  float* d_slabs = own.alloc<float>(nslab, nomem);
  float* d_gb = own.alloc<float>(2 * (size_t)C, nomem);
  float* d_ssa = own.alloc<float>(ss_a ? (size_t)ss_a_floats : 0, nomem);
  float* d_ssb = own.alloc<float>(ss_b ? (size_t)ss_b_floats : 0, nomem);
  int* d_row = row ? own.upload(row, (size_t)1, nomem) : nullptr;
  float* d_ab = own.alloc<float>(2 * (size_t)B * C, nomem);
  if (own.rc) return own.rc;
  const char* nocopy = "prg_debug_gn_coeff: copy failed";
  if (!copy_dd(d_slabs, slabs, nslab, s) || !copy_dd(d_gb, gamma, (size_t)C, s) || !copy_dd(d_gb + C, beta, (size_t)C, s) ||
      (ss_a && !copy_dd(d_ssa, ss_a, (size_t)ss_a_floats, s)) || (ss_b && !copy_dd(d_ssb, ss_b, (size_t)ss_b_floats, s)))
    return fail(PRG_E_HIP, nocopy);
  GnApply p{};
  p.gamma = d_gb; p.beta = d_gb + C;
  p.ss_a = d_ssa; p.ss_a_stride = ss_a_stride; p.ss_b = d_ssb; p.ss_b_stride = ss_b_stride; p.ss_a_row = d_row; p.ss_a_row_stride = row_stride;
  int rc = launch_gn_coeff(d_slabs, nsplit, p, d_ab, d_ab + (size_t)B * C, B, HW, C, groups, s);
  if (rc == PRG_OK && (!copy_dd(A, d_ab, (size_t)B * C, s) || !copy_dd(Bc, d_ab + (size_t)B * C, (size_t)B * C, s))) rc = fail(PRG_E_HIP, nocopy);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_gn_coeff: stream synchronise failed");
  return rc;
}

int prg_debug_gn_fold(prg_gn_fold* a, void* stream) {
  PRG_CHECK(a != nullptr, "prg_debug_gn_fold: null argument struct");
  const int B = a->B, C = a->C, HW = a->HW, G = a->groups, n = a->n_entries;
  PRG_CHECK(a->output >= PRG_GF_NONE && a->output <= PRG_GF_APPLY, "prg_debug_gn_fold: bad output mode");
  PRG_CHECK(a->in_place == 0 || a->in_place == 1, "prg_debug_gn_fold: in_place is 0 or 1");
  PRG_CHECK(a->pq_per_image == 0 || a->pq_per_image == 1, "prg_debug_gn_fold: pq_per_image is 0 or 1");
  PRG_CHECK(B > 0 && B <= 65535, "prg_debug_gn_fold: bad batch");
  const bool cond = a->entries != nullptr;
  PRG_CHECK(cond || a->output != PRG_GF_NONE, "prg_debug_gn_fold: nothing to do");
  std::vector<CondFoldEntry> ent;
  if (cond) {
    PRG_CHECK(!a->p && !a->q && a->pq_per_image == 0, "prg_debug_gn_fold: p and q are given or folded from entries, not both");
    PRG_CHECK(n > 0 && n <= 256 && a->ss_total > 0 && a->flat && a->flat_floats > 0 && a->ss_a && a->pq && a->zero_out,
              "prg_debug_gn_fold: the conditioning fold needs entries, ss_total, flat, ss_a, pq and zero_out");
    PRG_CHECK(a->zero_words >= 0 && a->zero_words <= (int64_t)1 << 24, "prg_debug_gn_fold: zero_words out of range");
    const char* why = cond_rows_bad(a->ss_a, a->ss_a_stride, a->ss_a_floats, a->ss_b, a->ss_b_stride, a->ss_b_floats, a->row, a->row_stride,
                                    B, a->ss_total);
    PRG_CHECK(!why, std::string("prg_debug_gn_fold: ") + (why ? why : ""));
    for (int k = 0; k < n; ++k) {
      const int64_t* e = a->entries + 4 * (size_t)k;
      PRG_CHECK(e[1] > 0 && e[1] <= 4096 && e[0] >= 0 && e[0] + 2 * e[1] <= a->ss_total, "prg_debug_gn_fold: an entry leaves its conditioning row");
      PRG_CHECK(e[2] >= 0 && e[2] + e[1] <= a->flat_floats && e[3] >= 0 && e[3] + e[1] <= a->flat_floats, "prg_debug_gn_fold: an entry leaves flat");
      ent.push_back(CondFoldEntry{(int)e[0], (int)e[1], (long long)e[2], (long long)e[3]});
    }
    PRG_CHECK(a->output == PRG_GF_NONE || (a->use_entry >= 0 && a->use_entry < n && ent[a->use_entry].C == C),
              "prg_debug_gn_fold: use_entry names an entry of C channels");
  } else {
    PRG_CHECK(a->p && a->q, "prg_debug_gn_fold: p and q, or entries");
  }
  if (a->output != PRG_GF_NONE) {
    PRG_CHECK(a->acc != nullptr, "prg_debug_gn_fold: null accumulators");
    PRG_CHECK(C > 0 && C <= 4096 && G > 0 && C % G == 0 && HW > 0, "prg_debug_gn_fold: bad shape");
  }
  if (a->output == PRG_GF_TABLES) PRG_CHECK(a->coef_a && a->coef_b, "prg_debug_gn_fold: the tables need coef_a and coef_b");
  if (a->output == PRG_GF_APPLY) {
    PRG_CHECK(a->x && a->out, "prg_debug_gn_fold: the pass needs x and out");
    PRG_CHECK(C % 8 == 0 && C <= 1024 && (int64_t)B * HW * C <= (int64_t)1 << 26, "prg_debug_gn_fold: the pass takes multiples of 8 channels, at most 1024");
  } else {
    PRG_CHECK(!a->residual && a->in_place == 0, "prg_debug_gn_fold: residual and in_place belong to the pass");
  }
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_gn_fold: hipMalloc failed";
  const char* nocopy = "prg_debug_gn_fold: copy failed";
  DeviceBuffers own;
  GnFold f{};
  int rc = PRG_OK;
  const size_t nzero = cond ? (size_t)a->zero_words + 64 : 0;
  long long* d_zero = nullptr;
  if (cond) {
    const CondFoldEntry* d_ent = own.upload(ent, nomem);
    float* d_flat = own.alloc<float>((size_t)a->flat_floats, nomem);
    float* d_ssa = own.alloc<float>((size_t)a->ss_a_floats, nomem);
    float* d_ssb = own.alloc<float>(a->ss_b ? (size_t)a->ss_b_floats : 0, nomem);
    int* d_row = a->row ? own.upload(reinterpret_cast<const int*>(a->row), (size_t)1, nomem) : nullptr;
    float* d_pq = own.alloc<float>((size_t)B * a->ss_total, nomem);
    d_zero = own.alloc<long long>(nzero, nomem);
    if (own.rc) return own.rc;
    if (!copy_dd(d_flat, a->flat, (size_t)a->flat_floats, s) || !copy_dd(d_ssa, a->ss_a, (size_t)a->ss_a_floats, s) ||
        (a->ss_b && !copy_dd(d_ssb, a->ss_b, (size_t)a->ss_b_floats, s)) || !copy_dd(d_pq, a->pq, (size_t)B * a->ss_total, s) ||
        hipMemsetAsync(d_zero, 0x5a, nzero * sizeof(long long), s) != hipSuccess)
      return fail(PRG_E_HIP, nocopy);
    GnApply ss{};
    ss.ss_a = d_ssa; ss.ss_a_stride = a->ss_a_stride; ss.ss_b = d_ssb; ss.ss_b_stride = a->ss_b_stride; ss.ss_a_row = d_row; ss.ss_a_row_stride = a->row_stride;
    rc = launch_cond_fold(d_ent, n, d_flat, ss, d_pq, a->ss_total, B, s, d_zero, a->zero_words);
    if (rc == PRG_OK && (!copy_dd(a->pq, d_pq, (size_t)B * a->ss_total, s) || !copy_dd(reinterpret_cast<long long*>(a->zero_out), d_zero, nzero, s))) rc = fail(PRG_E_HIP, nocopy);
    if (a->output != PRG_GF_NONE) { f.P = d_pq + ent[a->use_entry].ss_off; f.Q = f.P + C; f.pq_stride = a->ss_total; }
  } else {
    const size_t rows = a->pq_per_image ? (size_t)B : 1;
    float* d_pq = own.alloc<float>(rows * 2 * C, nomem);   // image b: P at 2 C b, Q behind it
    if (own.rc) return own.rc;
    for (size_t b = 0; b < rows; ++b)
      if (!copy_dd(d_pq + 2 * C * b, a->p + C * b, (size_t)C, s) || !copy_dd(d_pq + 2 * C * b + C, a->q + C * b, (size_t)C, s)) return fail(PRG_E_HIP, nocopy);
    f.P = d_pq; f.Q = d_pq + C; f.pq_stride = a->pq_per_image ? 2 * (int64_t)C : 0;
  }
  if (rc == PRG_OK && a->output != PRG_GF_NONE) {
    const size_t nacc = (size_t)B * G * 2, M = (size_t)B * HW * C;
    long long* d_acc = own.alloc<long long>(nacc, nomem);
    if (own.rc) return own.rc;
    if (!copy_dd(d_acc, reinterpret_cast<const long long*>(a->acc), nacc, s)) return fail(PRG_E_HIP, nocopy);
    f.acc = d_acc; f.G = G; f.cpg = C / G; f.inv_n = 1.0f / ((float)HW * (float)f.cpg);
    if (a->output == PRG_GF_TABLES) {
      float* d_ab = own.alloc<float>(2 * (size_t)B * C, nomem);
      if (own.rc) return own.rc;
      rc = launch_gn_coeff_acc(f, d_ab, d_ab + (size_t)B * C, B, C, s);
      if (rc == PRG_OK && (!copy_dd(a->coef_a, d_ab, (size_t)B * C, s) || !copy_dd(a->coef_b, d_ab + (size_t)B * C, (size_t)B * C, s))) rc = fail(PRG_E_HIP, nocopy);
    } else {
      bf16_t* d_x = own.alloc<bf16_t>(M, nomem);
      bf16_t* d_r = a->residual ? own.alloc<bf16_t>(M, nomem) : nullptr;
      bf16_t* d_o = a->in_place ? d_x : own.alloc<bf16_t>(M, nomem);
      if (own.rc) return own.rc;
      rc = launch_nchw_f32_to_nhwc<bf16_t>(a->x, d_x, B, HW, C, s);
      if (rc == PRG_OK && d_r) rc = launch_nchw_f32_to_nhwc<bf16_t>(a->residual, d_r, B, HW, C, s);
      if (rc == PRG_OK) rc = launch_affine_silu_fold(d_x, f, d_r, d_o, B, HW, C, s);
      if (rc == PRG_OK) rc = launch_nhwc_to_nchw_f32<bf16_t>(d_o, a->out, B, HW, C, s);
    }
  }
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_gn_fold: stream synchronise failed");
  return rc;
}

int prg_debug_affine_silu(const float* x, const float* A, const float* Bc, const float* residual, float* out, int B, int C, int HW,
                          int dtype, int in_place, void* stream) {
  PRG_CHECK(x && A && Bc && out, "prg_debug_affine_silu: null pointer");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16, "prg_debug_affine_silu: bad dtype");
  PRG_CHECK(in_place == 0 || in_place == 1, "prg_debug_affine_silu: in_place is 0 or 1");
  PRG_CHECK(C > 0 && C % (dtype == PRG_F32 ? 4 : 8) == 0, "prg_debug_affine_silu: C must be a multiple of the vector width");
  PRG_CHECK(B > 0 && HW > 0 && (int64_t)B * HW * C <= (int64_t)1 << 28, "prg_debug_affine_silu: bad shape");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == PRG_BF16) return debug_affine_silu_t<bf16_t>(x, A, Bc, residual, out, B, C, HW, in_place, s);
  return debug_affine_silu_t<float>(x, A, Bc, residual, out, B, C, HW, in_place, s);
}

int prg_debug_linear(const float* x, int ldx, int xoff, const float* W, int ldw, int woff, const float* bias, float* y, int ldy,
                     int ycol, int R, int I, int O, int act_in, int act_out, void* stream) {
  PRG_CHECK(x && W && y, "prg_debug_linear: null pointer");
  PRG_CHECK(R > 0 && R <= 1 << 20 && I > 0 && I <= 1 << 16 && O > 0 && O <= 1 << 16, "prg_debug_linear: bad shape");
  PRG_CHECK(xoff >= 0 && ldx <= 1 << 20 && (int64_t)xoff + I <= ldx, "prg_debug_linear: x columns [xoff, xoff + I) leave the row");
  PRG_CHECK(woff >= 0 && ldw <= 1 << 20 && (int64_t)woff + I <= ldw, "prg_debug_linear: W columns [woff, woff + I) leave the row");
  PRG_CHECK(ycol >= 0 && ldy <= 1 << 20 && (int64_t)ycol + O <= ldy, "prg_debug_linear: y columns [ycol, ycol + O) leave the row");
  PRG_CHECK((int64_t)R * ldx <= (int64_t)1 << 28 && (int64_t)O * ldw <= (int64_t)1 << 28 && (int64_t)R * ldy <= (int64_t)1 << 28,
            "prg_debug_linear: operand too large");
  PRG_CHECK(act_in >= ACT_NONE && act_in <= ACT_GELU && act_out >= ACT_NONE && act_out <= ACT_GELU, "prg_debug_linear: bad activation");
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_linear: hipMalloc failed";
  const char* nocopy = "prg_debug_linear: copy failed";
  DeviceBuffers own;
  float* d_x = own.alloc<float>((size_t)R * ldx, nomem);
  float* d_w = own.alloc<float>((size_t)O * ldw, nomem);
  float* d_b = bias ? own.alloc<float>((size_t)O, nomem) : nullptr;
  float* d_y = own.alloc<float>((size_t)R * ldy, nomem);
  if (own.rc) return own.rc;
  if (!copy_dd(d_x, x, (size_t)R * ldx, s) || !copy_dd(d_w, W, (size_t)O * ldw, s) || (bias && !copy_dd(d_b, bias, (size_t)O, s)) ||
      !copy_dd(d_y, y, (size_t)R * ldy, s))
    return fail(PRG_E_HIP, nocopy);
  int rc = launch_linear(d_x, ldx, xoff, d_w, ldw, woff, d_b, d_y + ycol, ldy, R, I, O, act_in, act_out, s);
  if (rc == PRG_OK && !copy_dd(y, d_y, (size_t)R * ldy, s)) rc = fail(PRG_E_HIP, nocopy);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_linear: stream synchronise failed");
  return rc;
}

int prg_debug_sinusoidal(const void* t, const float* freqs, float* out, int R, int dim, int wide, void* stream) {
  PRG_CHECK(t && freqs && out, "prg_debug_sinusoidal: null pointer");
  PRG_CHECK(wide == 0 || wide == 1, "prg_debug_sinusoidal: wide is 0 (int32) or 1 (int64)");
  PRG_CHECK(R > 0 && dim >= 4 && dim % 2 == 0 && (int64_t)R * dim <= (int64_t)1 << 24, "prg_debug_sinusoidal: bad shape");
  hipStream_t s = (hipStream_t)stream;
  const char* nomem = "prg_debug_sinusoidal: hipMalloc failed";
  const char* nocopy = "prg_debug_sinusoidal: copy failed";
  DeviceBuffers own;
  const size_t tbytes = (size_t)R * (wide ? 8 : 4);
  char* d_t = own.alloc<char>(tbytes, nomem);
  float* d_f = own.alloc<float>((size_t)dim / 2, nomem);
  float* d_o = own.alloc<float>((size_t)R * dim, nomem);
  if (own.rc) return own.rc;
  if (!copy_dd(d_t, static_cast<const char*>(t), tbytes, s) || !copy_dd(d_f, freqs, (size_t)dim / 2, s)) return fail(PRG_E_HIP, nocopy);
  int rc = wide ? launch_sinusoidal(reinterpret_cast<const int64_t*>(d_t), d_f, d_o, R, dim, s)
                : launch_sinusoidal_i32(reinterpret_cast<const int32_t*>(d_t), d_f, d_o, R, dim, s);
  if (rc == PRG_OK && !copy_dd(out, d_o, (size_t)R * dim, s)) rc = fail(PRG_E_HIP, nocopy);
  if (hipStreamSynchronize(s) != hipSuccess && rc == PRG_OK) rc = fail(PRG_E_HIP, "prg_debug_sinusoidal: stream synchronise failed");
  return rc;
}

int prg_debug_conv3x3(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                      int dtype, void* stream) {
  return debug_conv(x, w, bias, out, B, Cin, Cout, H, W, dtype, 3, 1, stream);
}

int prg_debug_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                   int dtype, int K, int stride, void* stream) {
  PRG_CHECK((K == 1 || K == 3 || K == 4) && (stride == 1 || stride == 2), "prg_debug_conv: K must be 1, 3 or 4, stride 1 or 2");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_F16X3 || K != 1, "prg_debug_conv: 1x1 convs only in the float32-storage modes");
  PRG_CHECK(stride == 1 || (H % 2 == 0 && W % 2 == 0), "prg_debug_conv: odd image size");
  return debug_conv(x, w, bias, out, B, Cin, Cout, H, W, dtype, K, stride, stream);
}

int prg_debug_upsample_conv3x3(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                               void* stream) {
  return debug_conv(x, w, bias, out, B, Cin, Cout, H, W, PRG_BF16, 3, 1, stream, 1);
}

int prg_debug_upsample_conv(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                            int dtype, void* stream) {
  return debug_conv(x, w, bias, out, B, Cin, Cout, H, W, dtype, 3, 1, stream, 1);
}

int prg_debug_conv4x4s2(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int H, int W,
                        void* stream) {
  PRG_CHECK(H % 2 == 0 && W % 2 == 0, "prg_debug_conv4x4s2: odd image size");
  return debug_conv(x, w, bias, out, B, Cin, Cout, H, W, PRG_BF16, 4, 2, stream);
}

// prg_debug_conv_choice: the selection of conv_choose.h on plain values (no device)
static int conv_choice_facts(const int32_t* q, ConvFacts* f) {
  const int dtype = q[PRG_CQ_DTYPE];
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16 || dtype == PRG_MXFP8 || dtype == PRG_F16X3, "prg_debug_conv_choice: bad dtype");
  *f = ConvFacts{};
  ConvDesc& d = f->d;
  d.B = q[PRG_CQ_B]; d.Hin = q[PRG_CQ_HIN]; d.Win = q[PRG_CQ_WIN]; d.C0 = q[PRG_CQ_C0]; d.C1 = q[PRG_CQ_C1]; d.ups = q[PRG_CQ_UPS];
  d.KH = q[PRG_CQ_KH]; d.KW = q[PRG_CQ_KW]; d.stride = q[PRG_CQ_STRIDE]; d.pad = q[PRG_CQ_PAD]; d.Hout = q[PRG_CQ_HOUT];
  d.Wout = q[PRG_CQ_WOUT]; d.Cout = q[PRG_CQ_COUT]; d.CoutPad = q[PRG_CQ_COUTPAD]; d.kchunks = q[PRG_CQ_KCHUNKS];
  f->f32 = dtype == PRG_F32 || dtype == PRG_F16X3;
  const int vec = f->f32 ? 4 : 8;
  PRG_CHECK(d.B > 0 && d.Hin > 0 && d.Win > 0 && d.Hout > 0 && d.Wout > 0 && d.C0 > 0 && d.C1 >= 0 && d.Cout > 0 && d.KH > 0 && d.KW > 0 &&
                d.stride > 0 && d.pad >= 0 && d.kchunks > 0 && (d.ups == 0 || d.ups == 1),
            "prg_debug_conv_choice: bad descriptor");
  PRG_CHECK((int64_t)d.B * d.Hout * d.Wout < (int64_t)1 << 31 && (int64_t)d.B * d.Hin * d.Win < (int64_t)1 << 31, "prg_debug_conv_choice: M out of range");
  PRG_CHECK(d.C0 % vec == 0 && d.C1 % vec == 0, "prg_debug_conv_choice: channel counts must be multiples of the 16-byte vector");
  PRG_CHECK(d.CoutPad % 64 == 0 && d.CoutPad >= d.Cout, "prg_debug_conv_choice: bad CoutPad");
  const int p = q[PRG_CQ_PRESENT];
  PRG_CHECK(p >= 0 && p < 2 * PRG_CP_FOLD_PQ, "prg_debug_conv_choice: bad present bits");
  f->bias = (p & PRG_CP_BIAS) != 0; f->residual = (p & PRG_CP_RESIDUAL) != 0; f->res_a = (p & PRG_CP_RES_A) != 0;
  f->pro_a = (p & PRG_CP_PRO_A) != 0; f->gn_partials = (p & PRG_CP_GN_PARTIALS) != 0; f->gn_acc = (p & PRG_CP_GN_ACC) != 0;
  f->w_mx = (p & PRG_CP_MX) != 0; f->w_s2d = (p & PRG_CP_S2D) != 0; f->w_up = (p & PRG_CP_UP) != 0; f->w_split = (p & PRG_CP_SPLIT) != 0;
  f->w_up_split = (p & PRG_CP_UP_SPLIT) != 0; f->w_f16 = (p & PRG_CP_F16) != 0; f->res_fold_acc = (p & PRG_CP_RES_FOLD_ACC) != 0;
  f->pro_fold_acc = (p & PRG_CP_FOLD_ACC) != 0; f->pro_fold_pq = (p & PRG_CP_FOLD_PQ) != 0;
  f->gn_groups = q[PRG_CQ_GN_GROUPS]; f->pro_fold_G = q[PRG_CQ_FOLD_G]; f->pro_fold_cpg = q[PRG_CQ_FOLD_CPG];
  f->in_f16 = q[PRG_CQ_IN_F16] != 0; f->out_f16 = q[PRG_CQ_OUT_F16] != 0; f->mx_pure = q[PRG_CQ_MX_PURE] != 0;
  return PRG_OK;
}

int prg_debug_conv_choice(const int32_t* query, const int32_t* query2, int32_t* choice, float* exec_scale) {
  PRG_CHECK(query && choice && exec_scale, "prg_debug_conv_choice: null pointer");
  ConvFacts f1, f2;
  if (int rc = conv_choice_facts(query, &f1)) return rc;
  if (query2)
    if (int rc = conv_choice_facts(query2, &f2)) return rc;
  const int32_t* w = query + PRG_CQ_SWITCHES;
  ConvSwitches sw;
  sw.conv_ws = w[0]; sw.conv_c64 = w[1]; sw.conv_w256 = w[2]; sw.conv_down_w256 = w[3]; sw.conv_w256mx = w[4]; sw.w256_min_tiles = w[5];
  sw.up2x2 = w[6]; sw.h16 = w[7]; sw.mx_pure = w[8]; sw.split_up2x2 = w[9]; sw.split_p64 = w[10]; sw.split_w512 = w[11];
  const int num_cus = query[PRG_CQ_NUM_CUS];
  const ConvChoice c = choose_conv(f1, num_cus, sw);
  const int32_t out[PRG_CC_COUNT] = {c.family, c.th, c.tw, c.bm, c.bn, c.pro, c.mode, c.tiles_x, c.tiles_y, c.tiles_n, c.grid, c.fuse_stats,
                                     c.nsplit, c.acc_done, c.fill_tables, c.is_mx, choose_supports_prologue(f1.d, f1.f32),
                                     query2 && !f1.f32 && !f2.f32 && choose_h16_pair(f1, f2, num_cus, sw)};
  for (int i = 0; i < PRG_CC_COUNT; ++i) choice[i] = out[i];
  *exec_scale = (float)c.exec_scale;
  return PRG_OK;
}

}  // extern "C"
