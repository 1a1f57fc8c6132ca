// weights_host.cpp — host side of the U-Nets, load time: the state-dict walk (build_layout), every weight packer and the weight
// arenas of a handle as a value (build_unet_weights).  Weight standardisation is folded into the packed weights here, once per
// conv; every arena is appended in the order of the one traversal (weights_host.h).  Plain C++: no HIP runtime, no environment.
// Compiled with -ffp-contract=off: the hi / lo splits compute v - (float)h behind a multiplication that must not fuse into it.
#include "weights_host.h"

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <utility>

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

#define LAYOUT_CHECK(cond, msg)                                          \
  do {                                                                   \
    if (!(cond)) { err = std::string(msg) + " [" #cond "]"; return PRG_E_INVALID; } \
  } while (0)

int build_layout(const prg_unet_config& cfg, Layout& L, std::string& err) {
  LAYOUT_CHECK(cfg.dim >= 8 && cfg.dim % 8 == 0, "config: dim must be a multiple of 8");
  LAYOUT_CHECK(cfg.n_levels >= 1 && cfg.n_levels <= 8, "config: n_levels out of range");
  LAYOUT_CHECK(cfg.in_channels == 1 || cfg.in_channels == 3, "config: in_channels must be 1 or 3");
  LAYOUT_CHECK(cfg.groups >= 1 && cfg.groups <= 64, "config: groups out of range");
  L.cfg = cfg;
  L.L = cfg.n_levels;
  L.emb = cfg.dim * 4;
  L.dims.assign(1, cfg.dim);
  for (int i = 0; i < cfg.n_levels; ++i) {
    LAYOUT_CHECK(cfg.dim_mults[i] >= 1, "config: bad dim_mult");
    L.dims.push_back(cfg.dim * cfg.dim_mults[i]);
  }
  for (size_t i = 0; i < L.dims.size(); ++i) LAYOUT_CHECK(L.dims[i] % cfg.groups == 0, "config: width not divisible by groups");
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
#undef LAYOUT_CHECK

// ---------------------------------------------------------------------------------------------
// equivalent weights of the resampling convs
// ---------------------------------------------------------------------------------------------
void up_equivalent_weights(const float* w, int Cout, int Cin, std::vector<float>& out) {
  out.assign((size_t)4 * Cout * Cin * 4, 0.0f);
  // tap a of phase dy collects kernel rows ky with source row offset (dy + ky - 1 floor-div 2) - (dy - 1) == a
  auto slot = [](int dphase, int k) { const int r = dphase + k - 1; return (r >= 0 ? r / 2 : -1) - (dphase - 1); };
  for (int dy = 0; dy < 2; ++dy)
    for (int dx = 0; dx < 2; ++dx)
      for (int o = 0; o < Cout; ++o)
        for (int c = 0; c < Cin; ++c) {
          double acc[2][2] = {{0, 0}, {0, 0}};
          for (int ky = 0; ky < 3; ++ky)
            for (int kx = 0; kx < 3; ++kx) acc[slot(dy, ky)][slot(dx, kx)] += (double)w[(((size_t)o * Cin + c) * 3 + ky) * 3 + kx];
          float* dst = out.data() + ((((size_t)(2 * dy + dx) * Cout + o) * Cin + c) * 4);
          dst[0] = (float)acc[0][0]; dst[1] = (float)acc[0][1]; dst[2] = (float)acc[1][0]; dst[3] = (float)acc[1][1];
        }
}

void s2d_equivalent_weights(const float* w, int Cout, int Cin, std::vector<float>& out) {
  out.assign((size_t)Cout * 4 * Cin * 9, 0.0f);
  for (int o = 0; o < Cout; ++o)
    for (int c = 0; c < Cin; ++c)
      for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx) {
          const int by = ky >> 1, dy = ky & 1, bx = kx >> 1, dx = kx & 1;
          const int cv = (2 * dy + dx) * Cin + c;
          out[(((size_t)o * 4 * Cin + cv) * 3 + 1 + by) * 3 + 1 + bx] = w[(((size_t)o * Cin + c) * 4 + ky) * 4 + kx];
        }
}

// ---------------------------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------------------------
static inline uint16_t f16_bits(_Float16 h) {
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}
// v = hi + lo as IEEE f16 bit patterns, each rounded to nearest even (compiler-rt / F16C)
static inline void f16_hi_lo(float v, uint16_t& hi, uint16_t& lo) {
  const _Float16 h = (_Float16)v;
  hi = f16_bits(h);
  lo = f16_bits((_Float16)(v - (float)h));
}

// The tiled layout every MFMA conv kernel reads: rows [tap = kh*KW+kw][chunk of BK channels][CoutPad = Cout rounded up to 64], each
// row holding its BK channels (the packers differ only in what a row's element is).  put(v, n, row, k) receives every weight
// W[n][c][kh][kw] with its output channel, its row index and its place k = c mod BK in the row; what is not visited stays as
// the caller zero-filled it.
struct Tiling {
  int CoutPad, kchunks;
  size_t rows;
};
static Tiling tiling(int Cout, int Cin, int KH, int KW, int BK) {
  const int cp = (Cout + 63) / 64 * 64, kcn = (Cin + BK - 1) / BK;
  return Tiling{cp, kcn, (size_t)KH * KW * kcn * cp};
}
template <typename Put>
static void tiled_walk(const float* w, int Cout, int Cin, int KH, int KW, int BK, const Tiling& t, Put&& put) {
  for (int kh = 0; kh < KH; ++kh)
    for (int kw = 0; kw < KW; ++kw)
      for (int kc = 0; kc < t.kchunks; ++kc)
        for (int n = 0; n < Cout; ++n)
          for (int k = 0; k < BK; ++k) {
            const int c = kc * BK + k;
            if (c >= Cin) break;
            put(w[(((size_t)n * Cin + c) * KH + kh) * KW + kw], n, (((size_t)(kh * KW + kw)) * t.kchunks + kc) * t.CoutPad + n, k);
          }
}

static inline void store_elem(float& dst, float v) { dst = v; }
static inline void store_elem(bf16_t& dst, float v) { dst = f32_to_bf16(v); }
static inline void store_elem(uint16_t& dst, float v) { dst = f16_bits((_Float16)v); }   // round to nearest even

// main packing: rows of 64 bytes of T (f32: 16, bf16: 32; T = uint16_t: the f16 twin of the bf16 packing, IEEE f16 bits)
template <typename T>
static void pack_conv_weight(const float* w, int Cout, int Cin, int KH, int KW, std::vector<T>& out, int* CoutPad, int* kchunks) {
  constexpr int BK = kPackBK<T>;
  const Tiling t = tiling(Cout, Cin, KH, KW, BK);
  out.assign(t.rows * BK, T{});
  tiled_walk(w, Cout, Cin, KH, KW, BK, t, [&](float v, int, size_t row, int k) { store_elem(out[row * BK + k], v); });
  *CoutPad = t.CoutPad;
  *kchunks = t.kchunks;
}

// Round 5: |a - hi - lo| <= 2^-22 |a| only holds while the lo half is a NORMAL f16; below |a| ~ 2^-3 it is
// subnormal with an absolute floor of 2^-25, so unstandardised weights of ~1 / sqrt(fan_in) (res_conv, Downsample, Upsample:
// 0.02-0.1; the stem's ~1/7-sized weights likewise) kept 18-20 bits.  Each output channel's weights are therefore multiplied by an
// exact power of two that brings max|w| into [2^9, 2^10) (hi exact to 2^-2, lo's 2^-25 floor = 2^-35 of the maximum; |w| < 2^10
// stays far from f16's 65504 with O(100) activations in the other operand being a float32-accumulated product), and the kernels
// multiply the float32 total by the inverse (exact) before the bias.
// w [Cout][per]; mul [Cout] = the factor; inv[0 .. Cout), which the caller filled with 1, = its inverse.
static void pow2_channel_scale(const float* w, int Cout, size_t per, std::vector<float>& mul, float* inv) {
  mul.assign((size_t)Cout, 1.0f);
  for (int n = 0; n < Cout; ++n) {
    float m = 0.0f;
    for (size_t i = 0; i < per; ++i) m = std::fmax(m, std::fabs(w[(size_t)n * per + i]));
    // (m < 2^-100: a dead / denormal channel — 2^k would overflow to +inf and 0 * inf = NaN: left unscaled,
    //  its halves flush to zero like the products they stand for)
    if (m >= 0x1p-100f && std::isfinite(m)) {
      int e = 0;
      (void)std::frexp(m, &e);                 // m = f * 2^e, f in [0.5, 1)
      const int k = 10 - e;                    // m * 2^k in [2^9, 2^10); |k| <= 110
      mul[n] = std::ldexp(1.0f, k);
      inv[n] = std::ldexp(1.0f, -k);
    }
  }
}

// split packing of the f16x3 mode: rows of [32 hi | 32 lo] f16 bit patterns of the scaled weights; oscale [CoutPad] undoes the scale
static void pack_conv_weight_split(const float* w, int Cout, int Cin, int KH, int KW, std::vector<uint16_t>& out, int* CoutPad,
                                   int* kchunks32, std::vector<float>& oscale) {
  const Tiling t = tiling(Cout, Cin, KH, KW, 32);
  out.assign(t.rows * 64, 0);
  oscale.assign((size_t)t.CoutPad, 1.0f);
  std::vector<float> mul;
  pow2_channel_scale(w, Cout, (size_t)Cin * KH * KW, mul, oscale.data());
  tiled_walk(w, Cout, Cin, KH, KW, 32, t,
             [&](float v, int n, size_t row, int k) { f16_hi_lo(v * mul[n], out[row * 64 + k], out[row * 64 + 32 + k]); });
  *CoutPad = t.CoutPad;
  *kchunks32 = t.kchunks;
}

// e4m3fn (OCP): 1-4-3, bias 7, max 448, no infinities; round to nearest even, saturating
uint8_t f32_to_e4m3(float v) {
  const uint8_t sign = std::signbit(v) ? 0x80 : 0;
  float a = std::fabs(v);
  if (!(a == a)) return sign | 0x7f;
  if (a >= 448.0f) return sign | 0x7e;
  if (a < 0.0009765625f) return sign;                       // < 2^-10: rounds to 0 (half of the smallest subnormal 2^-9, ties to even)
  int e;
  std::frexp(a, &e);                                         // a = m 2^e, m in [0.5, 1)
  int E = e - 1;                                             // floor(log2 a)
  if (E < -6) E = -6;                                        // subnormal range: fixed exponent, step 2^-9
  const float step = std::ldexp(1.0f, E - 3);
  float q = std::nearbyint(a / step);                        // round-half-even in the default rounding mode
  float r = q * step;
  if (r >= 448.0f) return sign | 0x7e;
  if (r < 0.015625f) return sign | (uint8_t)q;               // subnormal: q in 0..7
  int e2;
  const float m2 = std::frexp(r, &e2);                       // r may have carried into the next binade
  const int Eb = e2 - 1 + 7;
  const int man = (int)std::nearbyint((m2 * 2.0f - 1.0f) * 8.0f);
  return sign | (uint8_t)((Eb << 3) | man);
}
float e4m3_to_f32(uint8_t b) {
  const int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
  const float x = e == 0 ? std::ldexp((float)m, -9) : std::ldexp(1.0f + m / 8.0f, e - 7);
  return s ? -x : x;
}

// MX packing: 64-channel rows of two 32-channel blocks, one scale per block — not a row of the tiled walk above (a block's scale
// needs all of its 32 values, padding included, before any of them is stored)
static void pack_conv_weight_mxfp8(const float* w, int Cout, int Cin, int KH, int KW, std::vector<uint8_t>& data,
                                   std::vector<uint8_t>& scales, int* CoutPad, int* chunks64) {
  const int cp = (Cout + 63) / 64 * 64, kc = (Cin + 63) / 64;
  data.assign((size_t)KH * KW * kc * cp * 64, 0);
  scales.assign((size_t)KH * KW * kc * cp * 2, 0);
  for (int tap = 0; tap < KH * KW; ++tap)
    for (int c64 = 0; c64 < kc; ++c64)
      for (int n = 0; n < Cout; ++n)
        for (int blk = 0; blk < 2; ++blk) {
          float v[32], am = 0.0f;
          for (int k = 0; k < 32; ++k) {
            const int c = c64 * 64 + blk * 32 + k;
            v[k] = c < Cin ? w[((size_t)n * Cin + c) * KH * KW + tap] : 0.0f;
            am = std::fmax(am, std::fabs(v[k]));
          }
          uint32_t bits;
          std::memcpy(&bits, &am, 4);
          const int E = (int)((bits >> 23) & 0xff);
          const int S = E > 8 ? E - 8 : 0;
          const float mult = std::ldexp(1.0f, 127 - S);
          const size_t row = ((size_t)(tap * kc + c64) * cp + n);
          scales[row * 2 + blk] = (uint8_t)S;
          for (int k = 0; k < 32; ++k) {
            float g = v[k] * mult;
            g = g > 448.0f ? 448.0f : (g < -448.0f ? -448.0f : g);
            data[row * 64 + blk * 32 + k] = f32_to_e4m3(g);
          }
        }
  *CoutPad = cp;
  *chunks64 = kc;
}

// ---------------------------------------------------------------------------------------------
// stem fragments: w [64][Cin][7][7] as the A fragments [Cin][2 row tiles][hi | lo][4 k-steps][64 lanes][8] of the MFMA stem.
// put(v, co, hi, lo) receives every weight with its output channel and the indices of its hi and lo halves.
// ---------------------------------------------------------------------------------------------
constexpr size_t kStemFragElems = (size_t)2 * 2 * 4 * 64 * 8;   // per input channel
template <typename Put>
static void stem_fragment_walk(const float* w, int Cin, Put&& put) {
  for (int c = 0; c < Cin; ++c)
    for (int rt = 0; rt < 2; ++rt)
      for (int kk = 0; kk < 4; ++kk)
        for (int lane = 0; lane < 64; ++lane) {
          const int co = rt * 32 + (lane & 31), kh = 2 * kk + (lane >> 5);
          for (int j = 0; j < 7 && kh < 7; ++j)
            put(w[((size_t)co * Cin + c) * 49 + kh * 7 + j], co, (((((size_t)c * 2 + rt) * 2 + 0) * 4 + kk) * 64 + lane) * 8 + j,
                (((((size_t)c * 2 + rt) * 2 + 1) * 4 + kk) * 64 + lane) * 8 + j);
        }
}

void pack_stem_mfma_weights(const float* w, int Cin, std::vector<bf16_t>& outv) {
  outv.assign(Cin * kStemFragElems, f32_to_bf16(0.0f));
  stem_fragment_walk(w, Cin, [&](float v, int, size_t hi, size_t lo) {
    outv[hi] = f32_to_bf16(v);
    outv[lo] = f32_to_bf16(v - bf16_to_f32(outv[hi]));
  });
}

// f16 hi / lo halves of the same fragment layout, every output channel scaled by pow2_channel_scale; scale[co] = the inverse
void pack_stem_mfma_weights_split(const float* w, int Cin, std::vector<uint16_t>& outv, std::vector<float>& scale) {
  outv.assign(Cin * kStemFragElems, 0);
  scale.assign(64, 1.0f);
  std::vector<float> mul;
  pow2_channel_scale(w, 64, (size_t)Cin * 49, mul, scale.data());
  stem_fragment_walk(w, Cin, [&](float v, int co, size_t hi, size_t lo) { f16_hi_lo(v * mul[co], outv[hi], outv[lo]); });
}

// ---------------------------------------------------------------------------------------------
// per-conv packing
// ---------------------------------------------------------------------------------------------
void standardize(const float* w, int Cout, int K, std::vector<float>& out) {
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
  if (bf16 && role.conv2 && h16_eligible(Cout, Cin, K)) pack_conv_weight<uint16_t>(w, Cout, Cin, 3, 3, pk.h16, &cp, &kc);
  if (dtype == PRG_F16X3) pack_conv_weight_split(w, Cout, Cin, K, K, pk.split, &cp, &pk.split_kchunks, pk.split_scale);
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
        pack_conv_weight_split(wp, Cout, Cin, 2, 2, one_split, &cp, &kc, sc1);
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
// Every conv of the network through the packer.  Alignments: 128 elements (256-byte tiles of bf16) in the packed, h16 and split
// arenas, 256 bytes for the MX data and scales.  The Upsample packings follow all the other packings of their arena.
template <typename T>
static void build_convs(UnetWeights& u, std::vector<T>& packed, const float* weights, int dtype, const WeightOptions& opt) {
  std::vector<float> tmp;
  std::vector<std::pair<ConvP*, PackedConv<T>>> upsample;
  for_each_conv(u.lay, [&](ConvP& p, ConvRole role) {
    const float* w = weights + p.w_flat;
    if (p.ws) { standardize(w, p.Cout, p.Cin * p.KH * p.KW, tmp); w = tmp.data(); }
    if (dtype == PRG_F16X3 && !opt.split_up2x2) role.upsample = false;
    PackedConv<T> pk = pack_conv_host<T>(w, p.Cout, p.Cin, p.KH, dtype, role);
    p.CoutPad = pk.CoutPad; p.kchunks = pk.kchunks;
    p.w_off = append_aligned(packed, pk.main, 128);
    if (!pk.s2d.empty()) { p.s2d_off = (int64_t)append_aligned(packed, pk.s2d, 128); p.s2d_kchunks = pk.s2d_kchunks; }
    if (!pk.mx.empty()) {
      p.mx_off = (int64_t)append_aligned(u.mx, pk.mx, 256);
      p.mx_soff = (int64_t)append_aligned(u.mx_scale, pk.mx_scale, 256);
    }
    if (!pk.h16.empty()) p.h16_off = (int64_t)append_aligned(u.h16, pk.h16, 128);
    if (!pk.split.empty()) {
      p.sp_off = (int64_t)append_aligned(u.split, pk.split, 128);
      p.sp_kchunks = pk.split_kchunks;
      p.sp_scale_off = (int64_t)append_aligned(u.split_scale, pk.split_scale, 1);
    }
    if (!pk.up.empty() || !pk.up_split.empty()) upsample.emplace_back(&p, std::move(pk));
  });
  for (auto& pu : upsample) {
    ConvP& p = *pu.first;
    const PackedConv<T>& pk = pu.second;
    if (!pk.up.empty()) p.up_off = (int64_t)append_aligned(packed, pk.up, 128);
    if (!pk.up_split.empty()) {
      p.up_sp_off = (int64_t)append_aligned(u.split, pk.up_split, 128);
      p.up_sp_scale_off = (int64_t)append_aligned(u.split_scale, pk.up_split_scale, 1);
    }
  }
}

// the direct stem kernel's [49 * Cin][dim] weights, and the fragments of the MFMA stem (bf16: Cin 1 / 3 -> 64; f16x3: the same as
// f16 hi / lo halves — split_stem off: the direct fmaf kernel of the parity mode)
static void build_stems(UnetWeights& u, const float* weights, int dtype, const WeightOptions& opt) {
  const Layout& L = u.lay;
  u.stem.assign((size_t)49 * L.cfg.in_channels * L.cfg.dim, 0.0f);
  for (int o = 0; o < L.cfg.dim; ++o)
    for (int c = 0; c < L.cfg.in_channels; ++c)
      for (int t = 0; t < 49; ++t)
        u.stem[((size_t)t * L.cfg.in_channels + c) * L.cfg.dim + o] = weights[L.stem_w + ((size_t)o * L.cfg.in_channels + c) * 49 + t];
  const bool mfma_shape = (L.cfg.in_channels == 1 || L.cfg.in_channels == 3) && L.cfg.dim == 64;
  if ((dtype == PRG_BF16 || dtype == PRG_MXFP8) && mfma_shape) pack_stem_mfma_weights(weights + L.stem_w, L.cfg.in_channels, u.stem_frag);
  if (dtype == PRG_F16X3 && opt.split_stem && mfma_shape)
    pack_stem_mfma_weights_split(weights + L.stem_w, L.cfg.in_channels, u.stem_split, u.stem_split_scale);
}

// default frequency table: the reference's expression in float32 with this host's libm (the Python front-end
// replaces it with torch's own evaluation, which is what the reference would compute on the same host)
static void build_time_freqs(UnetWeights& u) {
  const int half = u.lay.cfg.dim / 2;
  u.freqs.resize(half);
  const float stepf = -(float)(9.210340371976184 / (double)(half - 1));
  for (int i = 0; i < half; ++i) u.freqs[i] = std::exp((float)i * stepf);
}

// f16x3: fused linear attention (attn_split.hip): to_qkv with the PreNorm gain folded in (q and k rows times log2 e: both only ever
// enter a softmax, evaluated with exp2) and to_out, each as f16 hi halves followed by the lo halves
void pack_split_attention(const float* w_qkv, const float* norm_g, const float* w_out, int C, SplitAttnPack& p) {
  const size_t nq = (size_t)3 * kHidden * C;
  p.qkv.assign(2 * nq, 0);
  for (int o = 0; o < 3 * kHidden; ++o)
    for (int c = 0; c < C; ++c) {
      const float v = w_qkv[(size_t)o * C + c] * norm_g[c] * (o < 2 * kHidden ? 1.4426950408889634f : 1.0f);
      f16_hi_lo(v, p.qkv[(size_t)o * C + c], p.qkv[nq + (size_t)o * C + c]);
    }
  const size_t no = (size_t)C * kHidden;
  p.out.assign(2 * no, 0);
  for (size_t i = 0; i < no; ++i) f16_hi_lo(w_out[i], p.out[i], p.out[no + i]);
}

static void build_split_attention(UnetWeights& u, const float* weights) {
  SplitAttnPack one;
  for_each_attn(u.lay, [&](AttnP& a) {
    // mid_at is not linear; linattn_split_supported: C = 64 / 128 (the token count is checked per call)
    if (!a.linear || (a.C != 64 && a.C != 128)) return;
    pack_split_attention(weights + a.qkv.w_flat, weights + a.norm_g, weights + a.out.w_flat, a.C, one);
    a.sp_qkv = (int64_t)append_aligned(u.attn_split, one.qkv, 64);
    a.sp_out = (int64_t)append_aligned(u.attn_split, one.out, 64);
  });
}

// bf16: fixed-point GroupNorm statistics (common.h, GnFold): P = gamma, Q = beta of every norm in 16-byte aligned rows (what
// the unconditioned norms use directly) and the table cond_fold_kernel walks for the conditioned ones
static void build_norm_rows(UnetWeights& u, const float* weights) {
  std::vector<float> row;
  const bool conditional = u.lay.cfg.conditional != 0;
  for_each_res(u.lay, [&](ResP& r) {
    r.cpad = (r.cout + 3) & ~3;
    auto put = [&](int64_t g_off, int64_t b_off) {
      row.assign(2 * (size_t)r.cpad, 0.0f);
      std::memcpy(row.data(), weights + g_off, sizeof(float) * r.cout);
      std::memcpy(row.data() + r.cpad, weights + b_off, sizeof(float) * r.cout);
      return (int64_t)append_aligned(u.pq_static, row, 1);
    };
    r.pq1 = put(r.g1, r.b1);
    r.pq2 = put(r.g2, r.b2);
    if (conditional) u.cond_entries.push_back(CondFoldEntry{r.ss_off, r.cout, (long long)r.g1, (long long)r.b1});
  });
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
static void build_fused_attention(UnetWeights& u, const float* weights, const WeightOptions& opt) {
  std::vector<bf16_t> one;
  FusedAttnPack pk;
  for_each_attn(u.lay, [&](AttnP& a) {
    if (!a.linear || !opt.linattn_fused_supported || !opt.linattn_fused_supported(a.C)) return;   // (mid_at is not linear)
    pack_fused_attention(weights + a.qkv.w_flat, weights + a.norm_g, weights + a.out.w_flat, a.C, pk);
    a.fw_qkv = (int64_t)append_aligned(u.attn, pk.qkv, 64);
    // la_kshift off forces the measured column maxima (the la_kmax pass) for every block
    if (opt.la_kshift && pk.ok) {
      a.kshift = (int64_t)u.kshift.size();
      u.kshift.insert(u.kshift.end(), pk.shifts, pk.shifts + kHidden + kHeads);
      u.kshift.resize((u.kshift.size() + 3) & ~(size_t)3);
    }
    a.fw_out = (int64_t)append_aligned(u.attn, pk.out, 1);
  });
  // fused ResnetBlock tail: raw res_conv weights [Cout][Cin] as bf16.  (has_res: the blocks of the up levels and the final one)
  for_each_res(u.lay, [&](ResP& r) {
    if (!r.has_res || r.res.b_off < 0 || !opt.resblock_tail_fused_supported ||
        !opt.resblock_tail_fused_supported(r.cin / 2, r.cin - r.cin / 2, r.cout)) return;
    one.clear();
    for (size_t i = 0; i < (size_t)r.cout * r.cin; ++i) one.push_back(f32_to_bf16(weights[r.res.w_flat + i]));
    r.fw_res = (int64_t)append_aligned(u.attn, one, 64);
  });
}

int build_unet_weights(const prg_unet_config& cfg, const float* weights, int64_t n, int dtype, const WeightOptions& opt,
                       UnetWeights& u, std::string& err) {
  u = UnetWeights{};
  const int rc = build_layout(cfg, u.lay, err);
  if (rc) return rc;
  if (u.lay.total != n) {
    err = "prg_unet_create: expected " + std::to_string(u.lay.total) + " floats, got " + std::to_string(n);
    return PRG_E_INVALID;
  }
  const bool bf16 = dtype == PRG_BF16 || dtype == PRG_MXFP8;
  if (bf16) build_convs(u, u.packed_bf16, weights, dtype, opt);
  else build_convs(u, u.packed_f32, weights, dtype, opt);
  build_stems(u, weights, dtype, opt);
  build_time_freqs(u);
  if (dtype == PRG_F16X3) build_split_attention(u, weights);
  if (bf16) build_norm_rows(u, weights);
  if (bf16 && opt.fused_attn) build_fused_attention(u, weights, opt);
  return PRG_OK;
}

}  // namespace prg
