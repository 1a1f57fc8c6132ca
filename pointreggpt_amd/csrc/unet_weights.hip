// unet_weights.hip — load time of a U-Net handle: read the switches, let weights_host.cpp build every arena as a host value,
// upload each into a buffer the handle owns.  Also the two host-only hooks that expose that value to the tests.
#include "unet_layout.h"

namespace prg {

// the packer's row length (weights_host.h) is the kernels' K-chunk (conv.h): this unit sees both
static_assert(kPackBK<float> == ConvTile<float>::BK && kPackBK<bf16_t> == ConvTile<bf16_t>::BK, "packer rows != kernel K-chunk");

// The switches weight preparation depends on.  PRG_SPLIT_UP2X2: the Upsample convs' sub-pixel packings of the f16x3 mode are off by
// default (conv_choose.cpp: choose_split); PRG_SPLIT_STEM=0: the direct fmaf stem kernel of the parity mode;
// PRG_LA_KSHIFT=0 forces the measured column maxima (the la_kmax pass) for every fused attention block.
static WeightOptions weight_options(bool split_up2x2, bool fused_attn, bool split_stem, bool la_kshift) {
  WeightOptions o;
  o.split_up2x2 = split_up2x2; o.fused_attn = fused_attn; o.split_stem = split_stem; o.la_kshift = la_kshift;
  o.linattn_fused_supported = linattn_fused_supported;
  o.resblock_tail_fused_supported = resblock_tail_fused_supported;
  return o;
}
static const WeightOptions& env_weight_options() {
  static const WeightOptions o = weight_options(env_int("PRG_SPLIT_UP2X2", 0) != 0, env_int("PRG_FUSED_ATTN", 1) != 0,
                                                env_int("PRG_SPLIT_STEM", 1) != 0, env_int("PRG_LA_KSHIFT", 1) != 0);
  return o;
}

int prepare_unet_weights(prg_unet& u, const prg_unet_config& cfg, const float* weights, int64_t n, int dtype) {
  // the kernels' limits first (the walk costs microseconds): a config they cannot run is refused before anything is packed
  int rc = build_layout_checked(cfg, u.lay);
  if (rc) return rc;
  if (u.lay.total != n)
    return fail(PRG_E_INVALID, "prg_unet_create: expected " + std::to_string(u.lay.total) + " floats, got " + std::to_string(n));
  DeviceBuffers& own = u.own;
  u.d_flat = own.upload(weights, (size_t)n, "hipMalloc(flat weights)");   // (before the build, as ever: measured 2-5 ms faster than after)
  UnetWeights w;
  std::string err;
  if ((rc = build_unet_weights(cfg, weights, n, dtype, env_weight_options(), w, err))) return fail(rc, err);
  u.lay = w.lay;
  // each host arena is given back as soon as it is on the device: held together they cost a few hundred MB of peak host memory
  // and, measured, 10-20 ms of prg_unet_create
  auto up = [&own](auto& v, const char* nomem) {
    auto* p = own.upload(v, nomem);
    std::decay_t<decltype(v)>().swap(v);
    return p;
  };
  u.n_cond_entries = (int)w.cond_entries.size();
  u.d_packed = w.packed_bf16.empty() ? (void*)up(w.packed_f32, "hipMalloc(packed weights)") : (void*)up(w.packed_bf16, "hipMalloc(packed weights)");
  u.d_mx = up(w.mx, "hipMalloc(MX-fp8 weights)");
  u.d_mx_scale = up(w.mx_scale, "hipMalloc(MX-fp8 weights)");
  u.d_h16 = up(w.h16, "hipMalloc(h16 weights)");
  u.d_split_scale = up(w.split_scale, "hipMalloc(split scales)");
  u.d_split = up(w.split, "hipMalloc(split weights)");
  u.d_stem = up(w.stem, "hipMalloc(stem weights)");
  u.d_stem_frag = up(w.stem_frag, "hipMalloc(stem fragments)");
  u.d_stem_split = up(w.stem_split, "hipMalloc(split stem fragments)");
  u.d_stem_split_scale = up(w.stem_split_scale, "hipMalloc(split stem scales)");
  u.d_freqs = up(w.freqs, "hipMalloc(time frequencies)");
  u.d_attn_split = up(w.attn_split, "hipMalloc(split attention weights)");
  u.d_pq_static = up(w.pq_static, "hipMalloc(norm gains)");
  u.d_cond_entries = up(w.cond_entries, "hipMalloc(cond entries)");
  u.d_attn = up(w.attn, "hipMalloc(attention weights)");
  u.d_kshift = up(w.kshift, "hipMalloc(softmax shifts)");
  if (own.rc) return own.rc;
  u.dtype = dtype;
  return PRG_OK;
}

// copies `bytes` of `src` behind a hook's (out, capacity, written) triple; out == null only reports the size
static int hook_copy(const void* src, size_t bytes, void* out, int64_t capacity, int64_t* written, const char* who) {
  if (written) *written = (int64_t)bytes;
  if (!out) return PRG_OK;
  if ((int64_t)bytes > capacity) return fail(PRG_E_INVALID, std::string(who) + ": output buffer too small");
  if (bytes) std::memcpy(out, src, bytes);
  return PRG_OK;
}
template <typename U>
static int hook_copy(const std::vector<U>& v, void* out, int64_t capacity, int64_t* written, const char* who) {
  return hook_copy(v.data(), v.size() * sizeof(U), out, capacity, written, who);
}

// every offset of the layout as int64: one row per conv, then per ResnetBlock, then per attention block, in traversal order
static std::vector<int64_t> layout_rows(const Layout& L) {
  std::vector<int64_t> r;
  for_each_conv(L, [&](const ConvP& p, ConvRole role) {
    r.insert(r.end(), {p.Cout, p.Cin, p.KH, p.KW, p.CoutPad, p.kchunks, (int64_t)p.w_off, p.b_off, p.w_flat, p.ws, p.mx_off, p.mx_soff,
                       p.s2d_off, p.s2d_kchunks, p.sp_off, p.sp_kchunks, p.h16_off, p.up_off, p.sp_scale_off, p.up_sp_scale_off,
                       p.up_sp_off, role.conv2, role.upsample});
  });
  for_each_res(L, [&](const ResP& p) { r.insert(r.end(), {p.cin, p.cout, p.ss_off, p.fw_res, p.pq1, p.pq2, p.cpad}); });
  for_each_attn(L, [&](const AttnP& a) { r.insert(r.end(), {a.C, a.fw_qkv, a.fw_out, a.kshift, a.sp_qkv, a.sp_out}); });
  return r;
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_debug_weight_arena(const prg_unet_config* cfg, const float* weights, int64_t n_floats, int dtype, int options, int arena,
                           void* out, int64_t capacity_bytes, int64_t* bytes) {
  const char* who = "prg_debug_weight_arena";
  PRG_CHECK(cfg && weights, "prg_debug_weight_arena: null pointer");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16 || dtype == PRG_MXFP8 || dtype == PRG_F16X3, "prg_debug_weight_arena: bad dtype");
  UnetWeights w;
  std::string err;
  const WeightOptions opt = weight_options(options & PRG_WOPT_SPLIT_UP2X2, options & PRG_WOPT_FUSED_ATTN, options & PRG_WOPT_SPLIT_STEM,
                                           options & PRG_WOPT_LA_KSHIFT);
  const int rc = build_unet_weights(*cfg, weights, n_floats, dtype, opt, w, err);
  if (rc) return fail(rc, err);
  const std::vector<int64_t> rows = layout_rows(w.lay);
  auto view = [&](int id) -> std::pair<const void*, size_t> {
    auto of = [](const auto& v) { return std::pair<const void*, size_t>(v.data(), v.size() * sizeof(v[0])); };
    switch (id) {
      case PRG_ARENA_LAYOUT: return of(rows);
      case PRG_ARENA_PACKED: return w.packed_bf16.empty() ? of(w.packed_f32) : of(w.packed_bf16);
      case PRG_ARENA_MX: return of(w.mx);
      case PRG_ARENA_MX_SCALE: return of(w.mx_scale);
      case PRG_ARENA_H16: return of(w.h16);
      case PRG_ARENA_SPLIT: return of(w.split);
      case PRG_ARENA_SPLIT_SCALE: return of(w.split_scale);
      case PRG_ARENA_STEM: return of(w.stem);
      case PRG_ARENA_STEM_FRAG: return of(w.stem_frag);
      case PRG_ARENA_STEM_SPLIT: return of(w.stem_split);
      case PRG_ARENA_STEM_SPLIT_SCALE: return of(w.stem_split_scale);
      case PRG_ARENA_FREQS: return of(w.freqs);
      case PRG_ARENA_ATTN_SPLIT: return of(w.attn_split);
      case PRG_ARENA_PQ_STATIC: return of(w.pq_static);
      case PRG_ARENA_COND_ENTRIES: return of(w.cond_entries);
      case PRG_ARENA_ATTN: return of(w.attn);
      case PRG_ARENA_KSHIFT: return of(w.kshift);
    }
    return {nullptr, 0};
  };
  if (arena == PRG_ARENA_ALL) {   // every arena in id order, each behind its int64 byte count
    std::vector<uint8_t> all;
    for (int id = 0; id < PRG_ARENA_COUNT; ++id) {
      const auto v = view(id);
      const int64_t nb = (int64_t)v.second;
      all.insert(all.end(), (const uint8_t*)&nb, (const uint8_t*)(&nb + 1));
      all.insert(all.end(), (const uint8_t*)v.first, (const uint8_t*)v.first + v.second);
    }
    return hook_copy(all, out, capacity_bytes, bytes, who);
  }
  if (arena >= 0 && arena < PRG_ARENA_COUNT) {
    const auto v = view(arena);
    return hook_copy(v.first, v.second, out, capacity_bytes, bytes, who);
  }
  return fail(PRG_E_INVALID, "prg_debug_weight_arena: no such arena");
}

int prg_debug_pack_conv(const float* w, int Cout, int Cin, int K, int dtype, int role_bits, int packing, void* out,
                        int64_t capacity_bytes, int64_t* bytes) {
  const char* who = "prg_debug_pack_conv";
  PRG_CHECK(w && Cout > 0 && Cin > 0 && K > 0, "prg_debug_pack_conv: bad arguments");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16 || dtype == PRG_MXFP8 || dtype == PRG_F16X3, "prg_debug_pack_conv: bad dtype");
  std::vector<float> eq;
  if (packing == PRG_PACK_S2D_OIHW) {
    PRG_CHECK(K == 4, "prg_debug_pack_conv: the space-to-depth form belongs to 4 x 4 convs");
    s2d_equivalent_weights(w, Cout, Cin, eq);
    return hook_copy(eq, out, capacity_bytes, bytes, who);
  }
  if (packing == PRG_PACK_UP_OIHW) {
    PRG_CHECK(K == 3, "prg_debug_pack_conv: the sub-pixel form belongs to 3 x 3 convs");
    up_equivalent_weights(w, Cout, Cin, eq);
    return hook_copy(eq, out, capacity_bytes, bytes, who);
  }
  ConvRole role;
  role.conv2 = (role_bits & PRG_ROLE_CONV2) != 0;
  role.upsample = (role_bits & PRG_ROLE_UPSAMPLE) != 0;
  auto pick = [&](const auto& pk) {
    switch (packing) {
      case PRG_PACK_MAIN: return hook_copy(pk.main, out, capacity_bytes, bytes, who);
      case PRG_PACK_S2D: return hook_copy(pk.s2d, out, capacity_bytes, bytes, who);
      case PRG_PACK_UP: return hook_copy(pk.up, out, capacity_bytes, bytes, who);
      case PRG_PACK_MX: return hook_copy(pk.mx, out, capacity_bytes, bytes, who);
      case PRG_PACK_MX_SCALE: return hook_copy(pk.mx_scale, out, capacity_bytes, bytes, who);
      case PRG_PACK_H16: return hook_copy(pk.h16, out, capacity_bytes, bytes, who);
      case PRG_PACK_SPLIT: return hook_copy(pk.split, out, capacity_bytes, bytes, who);
      case PRG_PACK_SPLIT_SCALE: return hook_copy(pk.split_scale, out, capacity_bytes, bytes, who);
      case PRG_PACK_UP_SPLIT: return hook_copy(pk.up_split, out, capacity_bytes, bytes, who);
      case PRG_PACK_UP_SPLIT_SCALE: return hook_copy(pk.up_split_scale, out, capacity_bytes, bytes, who);
    }
    return fail(PRG_E_INVALID, "prg_debug_pack_conv: no such packing");
  };
  if (dtype == PRG_F32 || dtype == PRG_F16X3) return pick(pack_conv_host<float>(w, Cout, Cin, K, dtype, role));
  return pick(pack_conv_host<bf16_t>(w, Cout, Cin, K, dtype, role));
}

}  // extern "C"
