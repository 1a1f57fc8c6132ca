// unet_weights.hip — host side of the U-Nets, load time: the state-dict walk (build_layout), the per-conv packer and the weight
// arenas of a handle.  Weight standardisation is folded into the packed weights here, once per conv; every arena is appended in
// the order of the one traversal (unet_layout.h) and uploaded into buffers the handle owns.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>

#include "unet_layout.h"

namespace prg {

// ---------------------------------------------------------------------------------------------
// parameter walk
// ---------------------------------------------------------------------------------------------
struct Cursor {
  int64_t pos = 0;
  int64_t take(int64_t n) {
    int64_t p = pos;
    pos += n;
    return p;
  }
};

static void walk_conv(Cursor& c, ConvP& p, int Cout, int Cin, int K, bool bias, bool ws) {
  p.Cout = Cout; p.Cin = Cin; p.KH = K; p.KW = K; p.ws = ws;
  p.w_flat = c.take((int64_t)Cout * Cin * K * K);
  p.b_off = bias ? c.take(Cout) : -1;
}
static void walk_res(Cursor& c, ResP& r, int cin, int cout, bool cond, int emb, int& ss_total) {
  r.cin = cin; r.cout = cout;
  if (cond) {
    r.mlp_w = c.take((int64_t)2 * cout * 2 * emb);
    r.mlp_b = c.take(2 * cout);
    r.ss_off = ss_total;
    ss_total += 2 * cout;
  }
  walk_conv(c, r.c1, cout, cin, 3, true, true);
  r.g1 = c.take(cout); r.b1 = c.take(cout);
  walk_conv(c, r.c2, cout, cout, 3, true, true);
  r.g2 = c.take(cout); r.b2 = c.take(cout);
  r.has_res = cin != cout;
  if (r.has_res) walk_conv(c, r.res, cout, cin, 1, true, false);
}
static void walk_attn(Cursor& c, AttnP& a, int C, bool linear) {
  a.C = C; a.linear = linear;
  walk_conv(c, a.qkv, 3 * kHidden, C, 1, false, false);
  walk_conv(c, a.out, C, kHidden, 1, true, false);
  if (linear) a.out_g = c.take(C);
  a.norm_g = c.take(C);
}

int build_layout(const prg_unet_config& cfg, Layout& L) {
  PRG_CHECK(cfg.dim >= 8 && cfg.dim % 8 == 0, "config: dim must be a multiple of 8");
  PRG_CHECK(cfg.n_levels >= 1 && cfg.n_levels <= 8, "config: n_levels out of range");
  PRG_CHECK(cfg.in_channels == 1 || cfg.in_channels == 3, "config: in_channels must be 1 or 3");
  PRG_CHECK(cfg.groups >= 1 && cfg.groups <= 64, "config: groups out of range");
  L.cfg = cfg;
  L.L = cfg.n_levels;
  L.emb = cfg.dim * 4;
  L.dims.assign(1, cfg.dim);
  for (int i = 0; i < cfg.n_levels; ++i) {
    PRG_CHECK(cfg.dim_mults[i] >= 1, "config: bad dim_mult");
    L.dims.push_back(cfg.dim * cfg.dim_mults[i]);
  }
  for (size_t i = 0; i < L.dims.size(); ++i) PRG_CHECK(L.dims[i] % cfg.groups == 0, "config: width not divisible by groups");
  for (size_t i = 0; i < L.dims.size(); ++i)
    if (L.dims[i] > 1024)
      return fail(PRG_E_INVALID, "config: dim * dim_mult = " + std::to_string(L.dims[i]) + " exceeds 1024 channels, the widest "
                  "GroupNorm the coefficient kernels handle (gn_coeff_kernel / affine_silu_fold_kernel: four channels per thread)");
  const bool cond = cfg.conditional != 0;
  Cursor c;
  const int d0 = cfg.dim, e = L.emb;
  L.stem_w = c.take((int64_t)d0 * cfg.in_channels * 49);
  L.stem_b = c.take(d0);
  if (cond) {
    L.tm1_w = c.take((int64_t)e * d0); L.tm1_b = c.take(e);
    L.tm3_w = c.take((int64_t)e * e);  L.tm3_b = c.take(e);
    L.pm0_w = c.take((int64_t)e * cfg.param_cond_dim); L.pm0_b = c.take(e);
    L.pm2_w = c.take((int64_t)e * e);  L.pm2_b = c.take(e);
  }
  L.downs.resize(L.L);
  L.ups.resize(L.L);
  for (int i = 0; i < L.L; ++i) {
    const int ci = L.dims[i], co = L.dims[i + 1];
    LevelP& lv = L.downs[i];
    walk_res(c, lv.r0, ci, ci, cond, e, L.ss_total);
    walk_res(c, lv.r1, ci, ci, cond, e, L.ss_total);
    walk_attn(c, lv.at, ci, true);
    lv.strided = i != L.L - 1;
    walk_conv(c, lv.resample, co, ci, lv.strided ? 4 : 3, true, false);
  }
  for (int i = 0; i < L.L; ++i) {
    const int ci = L.dims[L.L - 1 - i], co = L.dims[L.L - i];
    LevelP& lv = L.ups[i];
    walk_res(c, lv.r0, co + ci, co, cond, e, L.ss_total);
    walk_res(c, lv.r1, co + ci, co, cond, e, L.ss_total);
    walk_attn(c, lv.at, co, true);
    lv.strided = i != L.L - 1;  // here: "followed by x2 upsample"
    walk_conv(c, lv.resample, ci, co, 3, true, false);
  }
  const int mid = L.dims.back();
  walk_res(c, L.mid1, mid, mid, cond, e, L.ss_total);
  walk_attn(c, L.mid_at, mid, false);
  walk_res(c, L.mid2, mid, mid, cond, e, L.ss_total);
  walk_res(c, L.fin, 2 * d0, d0, cond, e, L.ss_total);
  L.head_w = c.take(d0);
  L.head_b = c.take(1);
  L.total = c.pos;
  return PRG_OK;
}

// ---------------------------------------------------------------------------------------------
// per-conv packing
// ---------------------------------------------------------------------------------------------
static void standardize(const float* w, int Cout, int K, std::vector<float>& out) {
  out.resize((size_t)Cout * K);
  for (int o = 0; o < Cout; ++o) {
    double m = 0;
    for (int k = 0; k < K; ++k) m += w[(size_t)o * K + k];
    m /= K;
    double v = 0;
    for (int k = 0; k < K; ++k) { double d = w[(size_t)o * K + k] - m; v += d * d; }
    v /= K;
    const double rs = 1.0 / std::sqrt(v + 1e-5);
    for (int k = 0; k < K; ++k) out[(size_t)o * K + k] = (float)((w[(size_t)o * K + k] - m) * rs);
  }
}

template <typename T>
PackedConv<T> pack_conv_host(const float* w, int Cout, int Cin, int K, int dtype, ConvRole role) {
  constexpr bool bf16 = std::is_same<T, bf16_t>::value;
  PackedConv<T> pk;
  int cp = 0, kc = 0;
  pack_conv_weight<T>(w, Cout, Cin, K, K, pk.main, &pk.CoutPad, &pk.kchunks);
  if (bf16 && s2d_eligible(Cout, Cin, K)) {
    std::vector<float> eq;
    s2d_equivalent_weights(w, Cout, Cin, eq);
    pack_conv_weight<T>(eq.data(), Cout, 4 * Cin, 3, 3, pk.s2d, &cp, &pk.s2d_kchunks);
  }
  if (dtype == PRG_MXFP8 && mx_eligible(Cout, Cin, K)) pack_conv_weight_mxfp8(w, Cout, Cin, 3, 3, pk.mx, pk.mx_scale, &cp, &kc);
  if (bf16 && role.conv2 && h16_eligible(Cout, Cin, K)) pack_conv_weight_f16(w, Cout, Cin, 3, 3, pk.h16);
  if (dtype == PRG_F16X3) pack_conv_weight_split(w, Cout, Cin, K, K, pk.split, &cp, &pk.split_kchunks, &pk.split_scale);
  // Upsample convs: the four [Cout][Cin][2][2] tensors of the sub-pixel decomposition, packed phase after phase
  const bool up = bf16 && role.upsample && up_eligible(Cout, Cin, K);
  const bool up_split = dtype == PRG_F16X3 && role.upsample && up_split_eligible(Cout, Cin, K);
  if (up || up_split) {
    std::vector<float> eq, sc1;
    std::vector<T> one;
    std::vector<uint16_t> one_split;
    up_equivalent_weights(w, Cout, Cin, eq);
    for (int ph = 0; ph < 4; ++ph) {
      const float* wp = eq.data() + (size_t)ph * Cout * Cin * 4;
      if (up) {
        pack_conv_weight<T>(wp, Cout, Cin, 2, 2, one, &cp, &kc);
        pk.up.insert(pk.up.end(), one.begin(), one.end());
      } else {
        pack_conv_weight_split(wp, Cout, Cin, 2, 2, one_split, &cp, &kc, &sc1);
        pk.up_split.insert(pk.up_split.end(), one_split.begin(), one_split.end());
        pk.up_split_scale.insert(pk.up_split_scale.end(), sc1.begin(), sc1.end());     // [phase][CoutPad]
      }
    }
  }
  return pk;
}
template PackedConv<float> pack_conv_host<float>(const float*, int, int, int, int, ConvRole);
template PackedConv<bf16_t> pack_conv_host<bf16_t>(const float*, int, int, int, int, ConvRole);

// ---------------------------------------------------------------------------------------------
// the weight arenas of a handle
// ---------------------------------------------------------------------------------------------
static bool fused_attention_enabled() {
  static const int on = env_int("PRG_FUSED_ATTN", 1);
  return on != 0;
}
// f16x3: the Upsample convs' sub-pixel packings are built only when the option is on — it is off by default
// (conv_split.hip: try_launch_conv_split)
static bool split_up2x2_enabled() {
  static const int on = env_int("PRG_SPLIT_UP2X2", 0);
  return on != 0;
}

// Every conv of the network through the packer.  Alignments: 128 elements (256-byte tiles of bf16) in the packed, h16 and split
// arenas, 256 bytes for the MX data and scales.  The Upsample packings follow all the other packings of their arena.
template <typename T>
static int upload_convs(prg_unet& u, const float* weights, int dtype) {
  std::vector<T> packed;
  std::vector<uint8_t> mx, mx_scale;
  std::vector<uint16_t> h16, split;
  std::vector<float> split_scale, tmp;
  std::vector<std::pair<ConvP*, PackedConv<T>>> upsample;
  for_each_conv(u.lay, [&](ConvP& p, ConvRole role) {
    const float* w = weights + p.w_flat;
    if (p.ws) { standardize(w, p.Cout, p.Cin * p.KH * p.KW, tmp); w = tmp.data(); }
    if (dtype == PRG_F16X3 && !split_up2x2_enabled()) role.upsample = false;
    PackedConv<T> pk = pack_conv_host<T>(w, p.Cout, p.Cin, p.KH, dtype, role);
    p.CoutPad = pk.CoutPad; p.kchunks = pk.kchunks;
    p.w_off = append_aligned(packed, pk.main, 128);
    if (!pk.s2d.empty()) { p.s2d_off = (int64_t)append_aligned(packed, pk.s2d, 128); p.s2d_kchunks = pk.s2d_kchunks; }
    if (!pk.mx.empty()) {
      p.mx_off = (int64_t)append_aligned(mx, pk.mx, 256);
      p.mx_soff = (int64_t)append_aligned(mx_scale, pk.mx_scale, 256);
    }
    if (!pk.h16.empty()) p.h16_off = (int64_t)append_aligned(h16, pk.h16, 128);
    if (!pk.split.empty()) {
      p.sp_off = (int64_t)append_aligned(split, pk.split, 128);
      p.sp_kchunks = pk.split_kchunks;
      p.sp_scale_off = (int64_t)append_aligned(split_scale, pk.split_scale, 1);
    }
    if (!pk.up.empty() || !pk.up_split.empty()) upsample.emplace_back(&p, std::move(pk));
  });
  for (auto& pu : upsample) {
    ConvP& p = *pu.first;
    const PackedConv<T>& pk = pu.second;
    if (!pk.up.empty()) p.up_off = (int64_t)append_aligned(packed, pk.up, 128);
    if (!pk.up_split.empty()) {
      p.up_sp_off = (int64_t)append_aligned(split, pk.up_split, 128);
      p.up_sp_scale_off = (int64_t)append_aligned(split_scale, pk.up_split_scale, 1);
    }
  }
  u.d_packed = u.own.upload(packed, "hipMalloc(packed weights)");
  u.d_mx = u.own.upload(mx, "hipMalloc(MX-fp8 weights)");
  u.d_mx_scale = u.own.upload(mx_scale, "hipMalloc(MX-fp8 weights)");
  u.d_h16 = u.own.upload(h16, "hipMalloc(h16 weights)");
  u.d_split_scale = u.own.upload(split_scale, "hipMalloc(split scales)");
  u.d_split = u.own.upload(split, "hipMalloc(split weights)");
  return u.own.rc;
}

// the direct stem kernel's [49 * Cin][dim] weights, and the fragments of the MFMA stem (bf16: Cin 1 / 3 -> 64; f16x3: the same as
// f16 hi / lo halves — PRG_SPLIT_STEM=0: the direct fmaf kernel of the parity mode)
static int upload_stems(prg_unet& u, const float* weights, int dtype) {
  const Layout& L = u.lay;
  std::vector<float> stem((size_t)49 * L.cfg.in_channels * L.cfg.dim);
  for (int o = 0; o < L.cfg.dim; ++o)
    for (int c = 0; c < L.cfg.in_channels; ++c)
      for (int t = 0; t < 49; ++t)
        stem[((size_t)t * L.cfg.in_channels + c) * L.cfg.dim + o] = weights[L.stem_w + ((size_t)o * L.cfg.in_channels + c) * 49 + t];
  u.d_stem = u.own.upload(stem, "hipMalloc(stem weights)");
  static const int split_stem_on = env_int("PRG_SPLIT_STEM", 1);
  const bool mfma_shape = (L.cfg.in_channels == 1 || L.cfg.in_channels == 3) && L.cfg.dim == 64;
  if ((dtype == PRG_BF16 || dtype == PRG_MXFP8) && mfma_shape) {
    std::vector<bf16_t> sf;
    pack_stem_mfma_weights(weights + L.stem_w, L.cfg.in_channels, sf);
    u.d_stem_frag = u.own.upload(sf, "hipMalloc(stem fragments)");
  }
  if (dtype == PRG_F16X3 && split_stem_on && mfma_shape) {
    std::vector<uint16_t> sf;
    std::vector<float> sc;
    pack_stem_mfma_weights_split(weights + L.stem_w, L.cfg.in_channels, sf, sc);
    u.d_stem_split = u.own.upload(sf, "hipMalloc(split stem fragments)");
    u.d_stem_split_scale = u.own.upload(sc, "hipMalloc(split stem scales)");
  }
  return u.own.rc;
}

// default frequency table: the reference's expression in float32 with this host's libm (the Python front-end
// replaces it with torch's own evaluation, which is what the reference would compute on the same host)
static int upload_time_freqs(prg_unet& u) {
  const int half = u.lay.cfg.dim / 2;
  std::vector<float> fr(half);
  const float stepf = -(float)(9.210340371976184 / (double)(half - 1));
  for (int i = 0; i < half; ++i) fr[i] = std::exp((float)i * stepf);
  u.d_freqs = u.own.upload(fr, "hipMalloc(time frequencies)");
  return u.own.rc;
}

// f16x3: fused linear attention (attn_split.hip): to_qkv with the PreNorm gain folded in (q and k rows times log2 e: both only ever
// enter a softmax, evaluated with exp2) and to_out, each as f16 hi halves followed by the lo halves
void pack_split_attention(const float* w_qkv, const float* norm_g, const float* w_out, int C, SplitAttnPack& p) {
  auto f16bits = [](float v, uint16_t& h, uint16_t& l) {
    const _Float16 a = (_Float16)v, b = (_Float16)(v - (float)a);
    std::memcpy(&h, &a, 2);
    std::memcpy(&l, &b, 2);
  };
  const size_t nq = (size_t)3 * kHidden * C;
  p.qkv.assign(2 * nq, 0);
  for (int o = 0; o < 3 * kHidden; ++o)
    for (int c = 0; c < C; ++c) {
      const float v = w_qkv[(size_t)o * C + c] * norm_g[c] * (o < 2 * kHidden ? 1.4426950408889634f : 1.0f);
      f16bits(v, p.qkv[(size_t)o * C + c], p.qkv[nq + (size_t)o * C + c]);
    }
  const size_t no = (size_t)C * kHidden;
  p.out.assign(2 * no, 0);
  for (size_t i = 0; i < no; ++i) f16bits(w_out[i], p.out[i], p.out[no + i]);
}

static int upload_split_attention(prg_unet& u, const float* weights) {
  std::vector<uint16_t> aw;
  SplitAttnPack one;
  for_each_attn(u.lay, [&](AttnP& a) {
    // mid_at is not linear; linattn_split_supported: C = 64 / 128 (the token count is checked per call)
    if (!a.linear || (a.C != 64 && a.C != 128)) return;
    pack_split_attention(weights + a.qkv.w_flat, weights + a.norm_g, weights + a.out.w_flat, a.C, one);
    a.sp_qkv = (int64_t)append_aligned(aw, one.qkv, 64);
    a.sp_out = (int64_t)append_aligned(aw, one.out, 64);
  });
  u.d_attn_split = u.own.upload(aw, "hipMalloc(split attention weights)");
  return u.own.rc;
}

// bf16: fixed-point GroupNorm statistics (common.h, GnFold): P = gamma, Q = beta of every norm in 16-byte aligned rows (what
// the unconditioned norms use directly) and the table cond_fold_kernel walks for the conditioned ones
static int upload_norm_rows(prg_unet& u, const float* weights) {
  std::vector<float> pq, row;
  std::vector<CondFoldEntry> ent;
  const bool conditional = u.lay.cfg.conditional != 0;
  for_each_res(u.lay, [&](ResP& r) {
    r.cpad = (r.cout + 3) & ~3;
    auto put = [&](int64_t g_off, int64_t b_off) {
      row.assign(2 * (size_t)r.cpad, 0.0f);
      std::memcpy(row.data(), weights + g_off, sizeof(float) * r.cout);
      std::memcpy(row.data() + r.cpad, weights + b_off, sizeof(float) * r.cout);
      return (int64_t)append_aligned(pq, row, 1);
    };
    r.pq1 = put(r.g1, r.b1);
    r.pq2 = put(r.g2, r.b2);
    if (conditional) ent.push_back(CondFoldEntry{r.ss_off, r.cout, (long long)r.g1, (long long)r.b1});
  });
  u.d_pq_static = u.own.upload(pq, "hipMalloc(norm gains)");
  u.d_cond_entries = u.own.upload(ent, "hipMalloc(cond entries)");
  u.n_cond_entries = (int)ent.size();
  return u.own.rc;
}

// bf16: fused linear attention (attn_fused.hip): to_qkv with the PreNorm gain folded in, to_out as is, both [out][in] bf16, and the
// static softmax shifts
void pack_fused_attention(const float* w_qkv, const float* norm_g, const float* w_out, int C, FusedAttnPack& p) {
  p.qkv.clear();
  for (int o = 0; o < 3 * kHidden; ++o)
    for (int c = 0; c < C; ++c)
      // q and k only ever enter a softmax: their rows carry log2(e), so the kernels exponentiate with a bare v_exp_f32
      p.qkv.push_back(f32_to_bf16(w_qkv[(size_t)o * C + c] * norm_g[c] * (o < 2 * kHidden ? 1.4426950408889634f : 1.0f)));
  // Softmax over pixels of k[n][d] = w_d . LN(x_n): a LayerNorm output has norm <= sqrt(C), so |k| <= ||w_d|| sqrt(C)
  // (Cauchy-Schwarz; w_d = the bf16 weights the kernel multiplies with, 2 % slack for the bf16 rounding of LN(x)).
  // exp(k - bound) >= exp(-2 bound): with bound <= 40 nothing underflows and the column maxima need not be measured.
  // (k, hence the bound, in units of 1 / log2(e): the rows above are pre-scaled.)
  p.ok = true;
  for (int d = 0; d < kHidden; ++d) {
    double n2 = 0;
    for (int c = 0; c < C; ++c) {
      const double w = bf16_to_f32(p.qkv[(size_t)(kHidden + d) * C + c]);
      n2 += w * w;
    }
    p.shifts[d] = (float)(1.02 * std::sqrt(n2 * C));
    p.ok = p.ok && p.shifts[d] <= 40.0f * 1.4426950408889634f;
  }
  // the same bound for the q rows (softmax over the 32 d of a head, per pixel): one shift per head
  for (int h = 0; h < kHeads; ++h) {
    double worst = 0;
    for (int d = 0; d < kDimHead; ++d) {
      double n2 = 0;
      for (int c = 0; c < C; ++c) {
        const double w = bf16_to_f32(p.qkv[(size_t)(h * kDimHead + d) * C + c]);
        n2 += w * w;
      }
      worst = std::max(worst, 1.02 * std::sqrt(n2 * C));
    }
    p.shifts[kHidden + h] = (float)worst;
    p.ok = p.ok && p.shifts[kHidden + h] <= 40.0f * 1.4426950408889634f;
  }
  p.out.clear();
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < kHidden; ++j) p.out.push_back(f32_to_bf16(w_out[(size_t)c * kHidden + j]));
}

// bf16: the fused linear-attention blocks and the raw res_conv weights of the fused ResnetBlock tail.  64-element alignment, shifts
// padded to 4 floats.
static int upload_fused_attention(prg_unet& u, const float* weights) {
  std::vector<bf16_t> aw, one;
  std::vector<float> ks;
  FusedAttnPack pk;
  // PRG_LA_KSHIFT=0 forces the measured column maxima (the la_kmax pass) for every block
  static const int kshift_on = env_int("PRG_LA_KSHIFT", 1);
  for_each_attn(u.lay, [&](AttnP& a) {
    if (!a.linear || !linattn_fused_supported(a.C)) return;   // (mid_at is not linear)
    pack_fused_attention(weights + a.qkv.w_flat, weights + a.norm_g, weights + a.out.w_flat, a.C, pk);
    a.fw_qkv = (int64_t)append_aligned(aw, pk.qkv, 64);
    if (kshift_on != 0 && pk.ok) {
      a.kshift = (int64_t)ks.size();
      ks.insert(ks.end(), pk.shifts, pk.shifts + kHidden + kHeads);
      ks.resize((ks.size() + 3) & ~(size_t)3);
    }
    a.fw_out = (int64_t)append_aligned(aw, pk.out, 1);
  });
  // fused ResnetBlock tail: raw res_conv weights [Cout][Cin] as bf16.  (has_res: the blocks of the up levels and the final one)
  for_each_res(u.lay, [&](ResP& r) {
    if (!r.has_res || r.res.b_off < 0 || !resblock_tail_fused_supported(r.cin / 2, r.cin - r.cin / 2, r.cout)) return;
    one.clear();
    for (size_t i = 0; i < (size_t)r.cout * r.cin; ++i) one.push_back(f32_to_bf16(weights[r.res.w_flat + i]));
    r.fw_res = (int64_t)append_aligned(aw, one, 64);
  });
  u.d_attn = u.own.upload(aw, "hipMalloc(attention weights)");
  u.d_kshift = u.own.upload(ks, "hipMalloc(softmax shifts)");
  return u.own.rc;
}

int prepare_unet_weights(prg_unet& u, const prg_unet_config& cfg, const float* weights, int64_t n, int dtype) {
  int rc = build_layout(cfg, u.lay);
  if (rc) return rc;
  if (u.lay.total != n)
    return fail(PRG_E_INVALID, "prg_unet_create: expected " + std::to_string(u.lay.total) + " floats, got " + std::to_string(n));
  const bool bf16 = dtype == PRG_BF16 || dtype == PRG_MXFP8;
  u.d_flat = u.own.upload(weights, (size_t)n, "hipMalloc(flat weights)");
  if ((rc = bf16 ? upload_convs<bf16_t>(u, weights, dtype) : upload_convs<float>(u, weights, dtype))) return rc;
  if ((rc = upload_stems(u, weights, dtype))) return rc;
  if ((rc = upload_time_freqs(u))) return rc;
  if (dtype == PRG_F16X3 && (rc = upload_split_attention(u, weights))) return rc;
  if (bf16 && (rc = upload_norm_rows(u, weights))) return rc;
  if (bf16 && fused_attention_enabled() && (rc = upload_fused_attention(u, weights))) return rc;
  u.dtype = dtype;
  return PRG_OK;
}

}  // namespace prg
