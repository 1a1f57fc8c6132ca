// unet.hip — host side of the two U-Nets and of the sampler: forward pass, workspace, hipGraph, C-ABI.  (The parameter layout
// and the handle struct: unet_layout.h; weight preparation: unet_weights.hip; the prg_debug_* entries: unet_debug.hip.)
//
// Mirrors (structure only) Unet.forward sd:920-964, MaskUnet.forward dc:871-906, GaussianDiffusion.sample
// sd:1283-1409.  Activations live as NHWC tensors of T (bf16_t or float) in a stack arena owned by the handle;
// the skip `torch.cat` never materialises (two source pointers into the conv), `nn.Upsample` is folded into the
// following conv's gather, weight standardisation is folded into the packed weights at load time.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "sampler.h"
#include "unet_layout.h"

namespace prg {

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
int device_cu_count() {
  static std::atomic<int> cus[64];          // zero-initialised; per device ordinal
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::atomic<int>& c = cus[dev & 63];
  int n = c.load(std::memory_order_acquire);
  if (n <= 0) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
    n = p.multiProcessorCount;
    c.store(n, std::memory_order_release);
  }
  return n;
}
int fail(int code, const std::string& m) {
  g_err = m;
  return code;
}
const char* last_error() { return g_err.c_str(); }

static bool head_fuse_enabled() { static const int on = env_int("PRG_HEAD_FUSE", 1); return on != 0; }
static bool res_epilogue_enabled() { static const int on = env_int("PRG_RES_EPILOGUE", 1); return on != 0; }
// PRG_GN_ACC=0: GroupNorm statistics as per-tile slabs + one gn_coeff_kernel launch per norm (rounds 1-2) instead of the
// fixed-point accumulators folded by the consumers (common.h, GnFold).  bf16 / mxfp8 handles only; fp32 always uses slabs.
static bool gn_acc_enabled() { static const int on = env_int("PRG_GN_ACC", 1); return on != 0; }

struct ProfileSink {  // per-launch conv timing (bench roofline)
  bool on = false;
  // (start, stop) event pairs of the launches of one step: grown on demand, read and reused after every step
  struct Events {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
    size_t used = 0;
    Events() = default;
    Events(const Events&) = delete;   // (owns the events)
    ~Events() { for (auto& ev : pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); } }
    int start(hipStream_t s) {   // the next pair's start event
      if (used == pool.size()) {
        hipEvent_t a, b;
        PRG_HIP(hipEventCreate(&a));
        PRG_HIP(hipEventCreate(&b));
        pool.push_back({a, b});
      }
      PRG_HIP(hipEventRecord(pool[used++].first, s));
      return PRG_OK;
    }
    int stop(hipStream_t s) { PRG_HIP(hipEventRecord(pool[used - 1].second, s)); return PRG_OK; }   // ... and its stop event
    template <typename Fn>
    int harvest(Fn&& each) {     // each(i, ms) for the pairs recorded since the last harvest (the stream has drained)
      for (size_t i = 0; i < used; ++i) {
        float ms = 0;
        PRG_HIP(hipEventElapsedTime(&ms, pool[i].first, pool[i].second));
        each(i, ms);
      }
      used = 0;
      return PRG_OK;
    }
  };
  Events conv_ev;
  double conv_ms = 0, conv_flops = 0, conv_bytes = 0;   // conv_bytes: algorithmic input + output + weight bytes
  double conv_flops_exec = 0;                           // 2 * MACs the kernels executed (sub-pixel Upsample convs: 4 / 9 of the algorithmic count)
  int64_t launches = 0;
  // per-SHAPE table (round 5, bench.py roofline.per_kernel): what conv_ev.pool[i] timed, and the totals per distinct conv shape
  struct Rec { prg_profile_shape key; double flops, flops_exec; };
  std::vector<Rec> recs;                                       // recs[i] <-> conv_ev.pool[i] of the step being harvested
  std::vector<prg_profile_shape> shapes;                       // accumulated (launches, ms, flops) per distinct key
  void add_shape(const Rec& r, double ms) {
    for (auto& sh : shapes)
      if (sh.cin == r.key.cin && sh.cout == r.key.cout && sh.k == r.key.k && sh.stride == r.key.stride && sh.ups == r.key.ups &&
          sh.hout == r.key.hout && sh.wout == r.key.wout && sh.two_source == r.key.two_source && sh.prologue == r.key.prologue &&
          sh.mx == r.key.mx) {
        sh.launches += 1; sh.ms += ms; sh.flops += r.flops; sh.flops_executed += r.flops_exec;
        return;
      }
    prg_profile_shape sh = r.key;
    sh.launches = 1; sh.ms = ms; sh.flops = r.flops; sh.flops_executed = r.flops_exec;
    shapes.push_back(sh);
  }
  // the conv launch that conv_ev's last pair brackets; `c`: what launch_conv chose for it
  void add_conv(const ConvDesc& d, const ConvChoice& c, bool prologue, size_t elem_bytes) {
    Rec r{};
    r.key.cin = d.C0 + d.C1; r.key.cout = d.Cout; r.key.k = d.KH; r.key.stride = d.stride; r.key.ups = d.ups;
    r.key.hout = d.Hout; r.key.wout = d.Wout; r.key.two_source = d.C1 > 0; r.key.prologue = prologue;
    r.key.mx = c.is_mx;
    r.flops = prg::conv_flops(d); r.flops_exec = prg::conv_flops(d) * c.exec_scale;
    conv_flops += r.flops;
    conv_flops_exec += r.flops_exec;
    if (recs.size() < conv_ev.used) recs.resize(conv_ev.used);
    recs[conv_ev.used - 1] = r;
    conv_bytes += ((double)d.B * d.Hin * d.Win * (d.C0 + d.C1) + (double)d.B * d.Hout * d.Wout * d.Cout +
                   (double)d.Cout * (d.C0 + d.C1) * d.KH * d.KW) * elem_bytes;
    launches += 1;
  }
  Events step_ev;                                              // the per-transition update kernel (HBM-bound)
  double step_ms = 0;
  int64_t step_launches = 0;
  int harvest() {   // one step's events into the totals (keeps the pools small)
    int rc = conv_ev.harvest([&](size_t i, float ms) { conv_ms += ms; if (i < recs.size()) add_shape(recs[i], ms); });
    if (rc) return rc;
    return step_ev.harvest([&](size_t, float ms) { step_ms += ms; });
  }
  void reset() {    // start of a run: totals to zero, the pools are kept
    conv_ms = 0; conv_flops = 0; conv_flops_exec = 0; conv_bytes = 0; launches = 0; conv_ev.used = 0;
    step_ms = 0; step_launches = 0; step_ev.used = 0;
    shapes.clear(); recs.clear();
  }
};

template <typename T>
struct UnetImpl : prg_unet {
  // -------- storage modes --------
  // T = bf16_t: PRG_BF16 / PRG_MXFP8.  T = float: PRG_F32, or PRG_F16X3 (float storage, split-f16 weights for the MFMAs).
  static constexpr bool kBf16 = std::is_same<T, bf16_t>::value;
  bool f16x3() const { return !kBf16 && d_split != nullptr; }

  // -------- small helpers --------
  const float* F(int64_t off) const { return off < 0 ? nullptr : d_flat + off; }
  const T* W(const ConvP& p) const { return reinterpret_cast<const T*>(d_packed) + p.w_off; }
  template <typename U>
  U* alloc(size_t n) { return reinterpret_cast<U*>(arena.alloc(n * sizeof(U))); }

  // The one dry-run gate.  measure() walks forward() with arena.dry set: every allocation happens exactly as in a live
  // evaluation and nothing is launched.  Every launch goes through run() (or conv(), which asks live() itself, as does the h16 pair query).
  bool live() const { return !arena.dry; }
  template <typename Fn, typename... A>
  int run(Fn&& launch, A&&... a) { return live() ? launch(std::forward<A>(a)...) : PRG_OK; }
  struct Frame { Arena& a; size_t m; ~Frame() { a.reset(m); } };   // what a block allocates goes when the block returns
  static int no_kernel(const char* what) { return fail(PRG_E_STATE, std::string(what) + ": no kernel for this storage type"); }

  struct ConvOpt {           // optional fusions of one conv launch
    const T* residual = nullptr;
    const float* res_a = nullptr;   // activated residual: + SiLU(residual * res_a + res_b) (ConvLaunch::res_a)
    const float* res_b = nullptr;
    float* gn_partials = nullptr;   // fused GroupNorm statistics of the output
    int* gn_nsplit = nullptr;       // out: slabs written (0 = not fused for this shape)
    const float* pro_a = nullptr;   // fused GroupNorm+cond+SiLU on the input (halo kernel)
    const float* pro_b = nullptr;
    long long* gn_acc = nullptr;    // fixed-point statistics of the output (instead of gn_partials when the kernel can)
    int* acc_done = nullptr;        // out: 1 = the launch accumulated into gn_acc
    const GnFold* fold = nullptr;   // prologue coefficients folded by the consumer (pro_a / pro_b = scratch tables)
    const GnFold* res_fold = nullptr;   // activated residual folded in the 1x1 conv's epilogue (instead of res_a / res_b)
    bool out_f16 = false;           // h16 (conv.h): the output is stored as f16 / the input is f16 and the conv takes its f16 weights
    bool in_f16 = false;
  };

  ConvDesc make_desc(const ConvP& p, int C0, int C1, int B, int Hin, int Win, int stride, int pad, int ups) const {
    ConvDesc d;
    d.B = B; d.Hin = Hin; d.Win = Win; d.C0 = C0; d.C1 = C1; d.ups = ups;
    d.KH = p.KH; d.KW = p.KW; d.stride = stride; d.pad = pad;
    const int Hl = ups ? 2 * Hin : Hin, Wl = ups ? 2 * Win : Win;
    d.Hout = (Hl + 2 * pad - p.KH) / stride + 1;
    d.Wout = (Wl + 2 * pad - p.KW) / stride + 1;
    d.Cout = p.Cout; d.CoutPad = p.CoutPad; d.kchunks = p.kchunks;
    return d;
  }

  ConvLaunch<T> make_launch(const ConvP& p, const T* s0, int C0, const T* s1, int C1, int B, int Hin, int Win, int stride, int pad,
                            int ups, const ConvOpt& o, T* out) const {
    ConvLaunch<T> L;
    L.d = make_desc(p, C0, C1, B, Hin, Win, stride, pad, ups);
    L.src0 = s0; L.src1 = s1; L.w = W(p); L.bias = F(p.b_off); L.residual = o.residual; L.out = out;
    L.res_a = o.res_a; L.res_b = o.res_b;
    L.gn_partials = o.gn_partials; L.gn_groups = lay.cfg.groups; L.pro_a = o.pro_a; L.pro_b = o.pro_b;
    L.w_mx = (d_mx && p.mx_off >= 0) ? d_mx + p.mx_off : nullptr;
    L.w_mx_scale = (d_mx_scale && p.mx_soff >= 0) ? d_mx_scale + p.mx_soff : nullptr;
    L.mx_pure = 0;
    L.w_s2d = (p.s2d_off >= 0 && stride == 2 && pad == 1) ? reinterpret_cast<const T*>(d_packed) + p.s2d_off : nullptr;
    L.w_up = (p.up_off >= 0 && ups && stride == 1 && pad == 1) ? reinterpret_cast<const T*>(d_packed) + p.up_off : nullptr;
    L.s2d_kchunks = p.s2d_kchunks;
    L.w_split = (d_split && p.sp_off >= 0) ? d_split + p.sp_off : nullptr;
    L.w_up_split = (d_split && p.up_sp_off >= 0 && ups && stride == 1 && pad == 1) ? d_split + p.up_sp_off : nullptr;
    L.split_kchunks = p.sp_kchunks;
    L.split_scale = (L.w_split && d_split_scale && p.sp_scale_off >= 0) ? d_split_scale + p.sp_scale_off : nullptr;
    L.split_scale_up = (L.w_up_split && d_split_scale && p.up_sp_scale_off >= 0) ? d_split_scale + p.up_sp_scale_off : nullptr;
    L.gn_acc = o.gn_acc;
    L.pro_fold = o.fold ? *o.fold : GnFold{};
    L.res_fold = o.res_fold ? *o.res_fold : GnFold{};
    L.out_f16 = o.out_f16 ? 1 : 0;
    L.in_f16 = o.in_f16 ? 1 : 0;
    L.w_f16 = (d_h16 && p.h16_off >= 0) ? d_h16 + p.h16_off : nullptr;
    return L;
  }

  int conv(const ConvP& p, const T* s0, int C0, const T* s1, int C1, int B, int Hin, int Win, int stride, int pad,
           int ups, const ConvOpt& o, T* out, hipStream_t s) {
    const ConvLaunch<T> L = make_launch(p, s0, C0, s1, C1, B, Hin, Win, stride, pad, ups, o, out);
    PRG_CHECK(C0 + C1 == p.Cin, "conv: channel mismatch");
    if (o.gn_nsplit) *o.gn_nsplit = 0;
    if (o.acc_done) *o.acc_done = 0;
    if (!live()) return PRG_OK;
    if (!(prof && prof->on)) return launch_conv<T>(L, s, o.gn_nsplit, o.acc_done);
    int rc, e;
    if ((rc = prof->conv_ev.start(s))) return rc;
    ConvChoice chosen;
    rc = launch_conv<T>(L, s, o.gn_nsplit, o.acc_done, &chosen);
    if ((e = prof->conv_ev.stop(s))) return e;
    prof->add_conv(L.d, chosen, L.pro_a != nullptr || L.pro_fold.acc != nullptr, sizeof(T));
    return rc;
  }

  // -------- launchers that exist for one storage type only --------
  bool h16_pair(const ConvLaunch<T>& L1, const ConvLaunch<T>& L2) const {
    if constexpr (kBf16) return conv_h16_pair_ok(L1, L2);
    else return false;
  }
  int affine_silu_fold(const T* x, const GnFold& f, const T* skip, T* out, int B, int HW, int C, hipStream_t s) {
    if constexpr (kBf16) return run(launch_affine_silu_fold, x, f, skip, out, B, HW, C, s);
    else return no_kernel("affine_silu_fold");
  }
  // Residual(PreNorm(LinearAttention)) in one launch chain of its own: attn_fused.hip (bf16), attn_split.hip (f16x3)
  bool linattn_fused_ok(const AttnP& a, int N) const {
    return a.linear && (kBf16 ? a.fw_qkv >= 0 && d_attn : a.sp_qkv >= 0 && d_attn_split && linattn_split_supported(a.C, N));
  }
  int linattn_fused(const AttnP& a, const T* x, T* out, int B, int N, hipStream_t s) {
    float* ws = alloc<float>(kBf16 ? linattn_fused_ws_floats(B, N) : linattn_split_ws_floats(B, N));
    PRG_CHECK(arena.dry || ws, kBf16 ? "workspace exhausted (fused attention)" : "workspace exhausted (split attention)");
    if constexpr (kBf16) {
      return run([&] {
        return launch_linear_attention_fused(x, d_attn + a.fw_qkv, d_attn + a.fw_out, F(a.out.b_off), F(a.out_g), out, ws, B, N, a.C,
                                             a.kshift >= 0 ? d_kshift + a.kshift : nullptr, s);
      });
    } else {
      const uint16_t* qh = d_attn_split + a.sp_qkv;
      const uint16_t* oh = d_attn_split + a.sp_out;
      return run(launch_linear_attention_split, x, qh, qh + (size_t)3 * kHidden * a.C, oh, oh + (size_t)a.C * kHidden, F(a.out.b_off),
                 F(a.out_g), out, ws, B, N, a.C, s);
    }
  }
  int full_attention(const T* qkv, T* o, int B, int N, hipStream_t s) {   // MFMA core where one covers N, else the generic one
    if constexpr (kBf16) { if (full_attention_mfma_supported(N)) return run(launch_full_attention_mfma, qkv, o, B, N, s); }
    else { if (f16x3() && full_attention_split_supported(N)) return run(launch_full_attention_split, qkv, o, B, N, s); }
    return run(launch_full_attention<T>, qkv, o, B, N, s);
  }
  int stem(const float* x_nchw, T* x0, int B, int S, hipStream_t s) {
    const int cin = lay.cfg.in_channels, d0 = lay.cfg.dim;
    if constexpr (kBf16) {
      if (d_stem_frag && stem_conv_mfma_supported(cin, d0, S, S))
        return run(launch_stem_conv_mfma, x_nchw, d_stem_frag, F(lay.stem_b), x0, B, cin, S, S, s);
    } else {
      if (d_stem_split && stem_conv_mfma_supported(cin, d0, S, S))
        return run(launch_stem_conv_mfma_split, x_nchw, d_stem_split, F(lay.stem_b), d_stem_split_scale, x0, B, cin, S, S, s);
    }
    return run(launch_stem_conv<T>, x_nchw, d_stem, F(lay.stem_b), x0, B, cin, S, S, d0, s);
  }

  // ---- fixed-point GroupNorm statistics (bf16 path) ----
  const float* pq_dyn = nullptr;     // [B][ss_total] P | Q of the conditioned norms of THIS forward (cond_fold_kernel)
  bool acc_on() const { return kBf16 && d_gnacc && gn_acc_enabled(); }
  long long* next_acc(int B) {
    if (!acc_on() || gn_slot >= gn_slots) return nullptr;
    return d_gnacc + (size_t)(gn_slot++) * resB * lay.cfg.groups * 2;
  }
  GnFold make_fold(const long long* acc, int C, int HW, bool conditioned, int ss_off, int64_t pq_static) const {
    GnFold f{};
    f.acc = acc;
    f.G = lay.cfg.groups;
    f.cpg = C / f.G;
    f.inv_n = 1.0f / ((float)HW * (float)f.cpg);
    if (conditioned && pq_dyn) {
      f.P = pq_dyn + ss_off; f.Q = f.P + C; f.pq_stride = lay.ss_total;
    } else {
      f.P = d_pq_static + pq_static; f.Q = f.P + ((C + 3) & ~3); f.pq_stride = 0;
    }
    return f;
  }

  GnApply gn_params(int64_t g_off, int64_t b_off, const CondSrc* cs, int ss_off) const {
    GnApply p{};
    p.gamma = F(g_off); p.beta = F(b_off);
    if (cs && cs->ss_a) {
      p.ss_a = cs->ss_a + ss_off;
      p.ss_a_stride = cs->ss_a_stride;
      p.ss_b = cs->ss_b ? cs->ss_b + ss_off : nullptr;
      p.ss_b_stride = cs->ss_b_stride;
      p.ss_a_row = cs->row;
      p.ss_a_row_stride = cs->row_stride;
    }
    return p;
  }

  // One GroupNorm of a ResnetBlock: the statistics of a conv's output and the coefficients y = x * A + Bc they turn into.
  // The conv leaves the statistics in one of two forms and says which (nsplit / acc_done):
  //   slabs (fp32 and f16x3 always; bf16 under PRG_GN_ACC=0 or from a kernel without accumulators): per-tile partial sums,
  //     turned into the tables A / Bc by one gn_coeff launch;
  //   accumulators (bf16): fixed-point sums in this norm's slot of d_gnacc, folded into coefficients by the kernel that
  //     consumes them (GnFold); a consumer that cannot fold reads tables filled by one gn_coeff_acc launch.
  struct NormStats {
    UnetImpl* u;
    int B, HW, C;
    float* slabs;
    long long* acc;         // null: slabs only
    float *A, *Bc;          // [B][C] tables (scratch for a consumer that folds in-kernel)
    GnApply apply;          // gamma, beta and conditioning of the slab path
    GnFold f{};             // the same for the accumulator path (filled when acc is set)
    int nsplit = 0, acc_done = 0;
    bool tabled = false;
    void ask(ConvOpt& o) { o.gn_partials = slabs; o.gn_nsplit = &nsplit; o.gn_acc = acc; o.acc_done = &acc_done; }   // of the conv this norm follows
    int complete(const T* x, hipStream_t s) {   // the conv fused no statistics: one pass over its output
      return nsplit == 0 ? u->run(launch_gn_stats<T>, x, slabs, B, HW, C, u->lay.cfg.groups, &nsplit, s) : PRG_OK;
    }
    const GnFold* fold() const { return acc_done ? &f : nullptr; }   // for a consumer that folds in-kernel; null on the slab path
    int tables(hipStream_t s) {                 // A / Bc hold the coefficients from here on: at most one launch
      if (std::exchange(tabled, true)) return PRG_OK;
      if (acc_done) return u->run(launch_gn_coeff_acc, f, A, Bc, B, C, s);
      return u->run(launch_gn_coeff, slabs, nsplit, apply, A, Bc, B, HW, C, u->lay.cfg.groups, s);
    }
    // x <- SiLU(GroupNorm(x)) + skip as a pass of its own
    int pass(T* x, const T* skip, hipStream_t s) {
      if (fold()) return u->affine_silu_fold(x, f, skip, x, B, HW, C, s);
      int rc = tables(s);
      return rc ? rc : u->run(launch_affine_silu<T>, x, A, Bc, skip, x, B, HW, C, s);
    }
  };
  NormStats norm(float* slabs, float* A, float* Bc, const GnApply& apply, int B, int HW, int C, bool conditioned, int ss_off,
                 int64_t pq_static) {
    NormStats n{this, B, HW, C, slabs, next_acc(B), A, Bc, apply};
    if (n.acc) n.f = make_fold(n.acc, C, HW, conditioned, ss_off, pq_static);
    return n;
  }

  // The three forms of a block's tail, out <- SiLU(GroupNorm(out)) + res(cat[s0, s1]):
  //   Fused (bf16): one kernel with the 1x1 res_conv inside (resblock_tail.hip), which can also apply the network's head;
  //   ResEpilogue (bf16, f16x3): a res_conv the fused kernel does not cover (up levels 0-1: 768 -> 512, 384 -> 256) takes the
  //     tail into ITS epilogue, out = Wres . cat[s0, s1] + b + SiLU(GroupNorm(h)): one launch, `res` never materialised either;
  //   Plain: `res` from its own conv (or the identity skip), then one elementwise pass (exact fp32 keeps these passes).
  enum class Tail { Fused, ResEpilogue, Plain };
  Tail pick_tail(const ResP& r, int C0, int C1) const {
    if (!r.has_res) return Tail::Plain;
    if (kBf16 && r.fw_res >= 0 && d_attn && resblock_tail_fused_supported(C0, C1, r.cout)) return Tail::Fused;
    if ((kBf16 || f16x3()) && r.cout % 8 == 0 && res_epilogue_enabled()) return Tail::ResEpilogue;
    return Tail::Plain;
  }
  struct Head { const float *w, *b; float* out; int sigmoid; };   // the network's final 1x1 conv, offered to the last block's tail
  int tail_fused(const ResP& r, const NormStats& n, const T* s0, int C0, const T* s1, int C1, T* out, const Head* head, hipStream_t s) {
    if constexpr (kBf16)
      return run(launch_resblock_tail_fused, out, n.A, n.Bc, s0, C0, s1, C1, d_attn + r.fw_res, F(r.res.b_off), out, n.B, n.HW, n.C, s,
                 head ? head->w : nullptr, head ? head->b : nullptr, head ? head->out : nullptr, head ? head->sigmoid : 0, n.fold());
    else return no_kernel("resblock_tail_fused");
  }
  // `res`: room for the res_conv's output (Plain).  *head_applied: the fused tail wrote the network output instead of `out`.
  int tail(const ResP& r, NormStats& n2, const T* s0, int C0, const T* s1, int C1, T* res, T* out, int B, int H, int Wd,
           const Head* head, bool* head_applied, hipStream_t s) {
    int rc;
    switch (pick_tail(r, C0, C1)) {
      case Tail::Fused:
        if (!n2.fold() && (rc = n2.tables(s))) return rc;
        if (head_applied) *head_applied = head != nullptr;
        return tail_fused(r, n2, s0, C0, s1, C1, out, head, s);
      case Tail::ResEpilogue: {
        ConvOpt ro; ro.residual = out;
        if (n2.fold() && n2.f.cpg % 8 == 0) {
          ro.res_fold = n2.fold();                            // coefficients folded in the res_conv's epilogue
        } else {
          if ((rc = n2.tables(s))) return rc;
          ro.res_a = n2.A; ro.res_b = n2.Bc;
        }
        return conv(r.res, s0, C0, s1, C1, B, H, Wd, 1, 0, 0, ro, out, s);
      }
      default: break;
    }
    const T* skip = s0;
    if (r.has_res) {
      if ((rc = conv(r.res, s0, C0, s1, C1, B, H, Wd, 1, 0, 0, ConvOpt(), res, s))) return rc;
      skip = res;
    } else {
      PRG_CHECK(C1 == 0 && C0 == r.cout, "resblock: identity skip needs equal widths");
    }
    return n2.pass(out, skip, s);
  }

  // ResnetBlock (sd:700-734 / dc:726-740): out <- block2(block1(cat[s0,s1])) + res(cat[s0,s1]).
  //   conv1 (+ statistics) -> norm 1 reaches conv2 (folded prologue, table prologue, or a pass over h1) -> conv2 (+ statistics)
  //   -> tail.  head: the final block only.
  int resblock(const ResP& r, const T* s0, int C0, const T* s1, int C1, const CondSrc* cs, T* out, int B, int H, int Wd,
               hipStream_t s, const Head* head = nullptr, bool* head_applied = nullptr) {
    const Frame frame{arena, arena.mark()};
    const size_t M = (size_t)B * H * Wd;
    const int G = lay.cfg.groups, HW = H * Wd;
    T* h1 = alloc<T>(M * r.cout);
    T* res = r.has_res ? alloc<T>(M * r.cout) : nullptr;
    float* part1 = alloc<float>((size_t)B * kGnMaxSplit * G * 2);
    float* part2 = alloc<float>((size_t)B * kGnMaxSplit * G * 2);
    float* coefA = alloc<float>((size_t)B * r.cout);
    float* coefB = alloc<float>((size_t)B * r.cout);
    float* coefA2 = alloc<float>((size_t)B * r.cout);
    float* coefB2 = alloc<float>((size_t)B * r.cout);
    PRG_CHECK(arena.dry || (h1 && part1 && part2 && coefA && coefB && coefA2 && coefB2 && (!r.has_res || res)),
              "workspace exhausted (resblock)");
    const CondSrc* c1 = lay.cfg.conditional ? cs : nullptr;
    NormStats n1 = norm(part1, coefA, coefB, gn_params(r.g1, r.b1, c1, r.ss_off), B, HW, r.cout, c1 && c1->ss_a, r.ss_off, r.pq1);
    // conv2's own statistics turn into a second coefficient pair (coefA / coefB are still being read by its prologue)
    NormStats n2 = norm(part2, coefA2, coefB2, gn_params(r.g2, r.b2, nullptr, 0), B, HW, r.cout, false, 0, r.pq2);
    ConvOpt o1, o2;
    n1.ask(o1); n2.ask(o2);
    // conv2 applies GroupNorm + SiLU of h1 in its prologue wherever it supports one
    const bool fuse_pro = conv_supports_prologue<T>(make_desc(r.c2, r.cout, 0, B, H, Wd, 1, 1, 0));
    // h16 (conv.h): h1 only ever feeds conv2's fused prologue — stored as f16 when both launches land on kernels that implement it
    // (asked of the selection with the launches' own descriptors: PRG_H16=0, PRG_CONV_C64=0, ... and uncovered shapes fall back to bf16 h1)
    bool h16 = false;
    if (live() && n1.acc && fuse_pro && d_h16 && r.c2.h16_off >= 0) {
      ConvOpt p2 = o2;
      p2.fold = &n1.f; p2.pro_a = n1.A; p2.pro_b = n1.Bc;
      h16 = h16_pair(make_launch(r.c1, s0, C0, s1, C1, B, H, Wd, 1, 1, 0, o1, h1),
                      make_launch(r.c2, h1, r.cout, nullptr, 0, B, H, Wd, 1, 1, 0, p2, out));
    }
    o1.out_f16 = o2.in_f16 = h16;
    int rc;
    if ((rc = conv(r.c1, s0, C0, s1, C1, B, H, Wd, 1, 1, 0, o1, h1, s))) return rc;
    if ((rc = n1.complete(h1, s))) return rc;
    PRG_CHECK(!h16 || n1.acc_done, "resblock: the h16 pair query promised fixed-point statistics");
    if (!fuse_pro) {
      if ((rc = n1.pass(h1, nullptr, s))) return rc;
    } else {
      o2.fold = n1.fold();              // (then the tables are scratch for kernels without the in-kernel fold: nothing fills them)
      if (!o2.fold && (rc = n1.tables(s))) return rc;
      o2.pro_a = n1.A; o2.pro_b = n1.Bc;
    }
    if ((rc = conv(r.c2, h1, r.cout, nullptr, 0, B, H, Wd, 1, 1, 0, o2, out, s))) return rc;
    if ((rc = n2.complete(out, s))) return rc;
    return tail(r, n2, s0, C0, s1, C1, res, out, B, H, Wd, head, head_applied, s);
  }

  // Residual(PreNorm(LinearAttention | Attention)) (sd:583-589, 631-639, 737-796)
  int attention(const AttnP& a, const T* x, T* out, int B, int H, int Wd, hipStream_t s) {
    const Frame frame{arena, arena.mark()};
    const int N = H * Wd;
    const size_t M = (size_t)B * N;
    int rc;
    if (linattn_fused_ok(a, N)) return linattn_fused(a, x, out, B, N, s);
    T* xn = alloc<T>(M * a.C);
    T* qkv = alloc<T>(M * 3 * kHidden);
    T* o = alloc<T>(M * kHidden);
    T* y = a.linear ? alloc<T>(M * a.C) : nullptr;
    float* ws = a.linear ? alloc<float>(linattn_ws_floats(B, N)) : nullptr;
    PRG_CHECK(arena.dry || (xn && qkv && o && (!a.linear || (y && ws))), "workspace exhausted (attention)");
    if ((rc = run(launch_layernorm<T>, x, F(a.norm_g), nullptr, xn, (int64_t)M, a.C, s))) return rc;
    if ((rc = conv(a.qkv, xn, a.C, nullptr, 0, B, H, Wd, 1, 0, 0, ConvOpt(), qkv, s))) return rc;
    if (a.linear) {
      if ((rc = run(launch_linear_attention<T>, qkv, o, ws, B, N, s))) return rc;
      if ((rc = conv(a.out, o, kHidden, nullptr, 0, B, H, Wd, 1, 0, 0, ConvOpt(), y, s))) return rc;
      if ((rc = run(launch_layernorm<T>, y, F(a.out_g), x, out, (int64_t)M, a.C, s))) return rc;
    } else {
      if ((rc = full_attention(qkv, o, B, N, s))) return rc;
      ConvOpt ro; ro.residual = x;
      if ((rc = conv(a.out, o, kHidden, nullptr, 0, B, H, Wd, 1, 0, 0, ro, out, s))) return rc;
    }
    return PRG_OK;
  }

  void tap(const char* name, const void* p, int B, int C, int H, int Wd, bool nchw = false) {
    if (taps_on && !arena.dry) taps[name] = Tap{p, C, H, Wd, B, nchw};
  }

  // Start of an evaluation on the fixed-point path (bf16): the accumulators of every norm are cleared by one memset, and one
  // launch folds the conditioning (scale + 1, shift) of every ResnetBlock into P / Q — instead of one gn_coeff launch per norm.
  int begin_norms(const CondSrc* cs, int B, hipStream_t s) {
    gn_slot = 0; pq_dyn = nullptr;
    if (!(kBf16 && gn_acc_enabled())) return PRG_OK;
    const bool conditioned = lay.cfg.conditional && n_cond_entries > 0;
    // (the conditioned network clears the accumulators inside its cond_fold launch below: one launch fewer per evaluation)
    const bool fold = acc_on() && conditioned && cs && cs->ss_a;
    int rc;
    if (acc_on() && !fold && (rc = run([&] { PRG_HIP(hipMemsetAsync(d_gnacc, 0, gnacc_bytes, s)); return (int)PRG_OK; }))) return rc;
    if (!conditioned) return PRG_OK;
    float* pq = alloc<float>((size_t)B * lay.ss_total);
    PRG_CHECK(arena.dry || pq, "workspace exhausted (conditioning fold)");
    if (!fold) return PRG_OK;
    const GnApply ss = gn_params(-1, -1, cs, 0);   // the conditioning rows alone: no gamma / beta
    rc = run(launch_cond_fold, d_cond_entries, n_cond_entries, d_flat, ss, pq, lay.ss_total, B, s, d_gnacc,
             (int64_t)(gnacc_bytes / sizeof(long long)));
    if (!rc) pq_dyn = pq;
    return rc;
  }

  int forward(const float* x_nchw, const CondSrc& cond, float* out, int B, int S, hipStream_t s) override {
    const Layout& L = lay;
    const int nl = L.L;
    PRG_CHECK(S % (1 << (nl - 1)) == 0 && (S >> (nl - 1)) >= 2, "forward: image size too small for the level count");
    PRG_CHECK((S * S) % 4 == 0, "forward: H*W must be a multiple of 4");
    arena.reset(0);
    if (taps_on) taps.clear();
    const CondSrc* cs = L.cfg.conditional ? &cond : nullptr;
    int rc;
    const int d0 = L.cfg.dim;
    if ((rc = begin_norms(cs, B, s))) return rc;
    T* x0 = alloc<T>((size_t)B * S * S * d0);
    PRG_CHECK(arena.dry || x0, "workspace exhausted (stem)");
    if ((rc = stem(x_nchw, x0, B, S, s))) return rc;
    tap("init_conv", x0, B, d0, S, S);
    std::vector<std::pair<const T*, int>> skips;
    const T* x = x0;
    int H = S;
    for (int i = 0; i < nl; ++i) {
      const LevelP& lv = L.downs[i];
      const int C = L.dims[i], Co = L.dims[i + 1];
      const size_t M = (size_t)B * H * H;
      T* s1 = alloc<T>(M * C);
      PRG_CHECK(arena.dry || s1, "workspace exhausted (down)");
      if ((rc = resblock(lv.r0, x, C, nullptr, 0, cs, s1, B, H, H, s))) return rc;
      skips.push_back({s1, C});
      if (i == 0) tap("down0_block0", s1, B, C, H, H);
      T* s2 = alloc<T>(M * C);
      const size_t mk = arena.mark();
      T* t = alloc<T>(M * C);
      PRG_CHECK(arena.dry || (s2 && t), "workspace exhausted (down)");
      if ((rc = resblock(lv.r1, s1, C, nullptr, 0, cs, t, B, H, H, s))) return rc;
      if ((rc = attention(lv.at, t, s2, B, H, H, s))) return rc;
      arena.reset(mk);
      skips.push_back({s2, C});
      if (i == 0) tap("down0_attn", s2, B, C, H, H);
      const int Ho = lv.strided ? H / 2 : H;
      T* xd = alloc<T>((size_t)B * Ho * Ho * Co);
      PRG_CHECK(arena.dry || xd, "workspace exhausted (downsample)");
      if ((rc = conv(lv.resample, s2, C, nullptr, 0, B, H, H, lv.strided ? 2 : 1, 1, 0, ConvOpt(), xd, s))) return rc;
      if (i == 0) tap("down0_out", xd, B, Co, Ho, Ho);
      x = xd;
      H = Ho;
    }
    {
      const int C = L.dims.back();
      const size_t M = (size_t)B * H * H;
      T* m2 = alloc<T>(M * C);
      T* m3 = alloc<T>(M * C);
      const size_t mk = arena.mark();
      T* m1 = alloc<T>(M * C);
      PRG_CHECK(arena.dry || (m1 && m2 && m3), "workspace exhausted (mid)");
      if ((rc = resblock(L.mid1, x, C, nullptr, 0, cs, m1, B, H, H, s))) return rc;
      if ((rc = attention(L.mid_at, m1, m2, B, H, H, s))) return rc;
      arena.reset(mk);
      tap("mid_attn", m2, B, C, H, H);
      if ((rc = resblock(L.mid2, m2, C, nullptr, 0, cs, m3, B, H, H, s))) return rc;
      x = m3;
    }
    for (int i = 0; i < nl; ++i) {
      const LevelP& lv = L.ups[i];
      const int Ci = L.dims[nl - 1 - i], Co = L.dims[nl - i];  // block width Co, resample to Ci
      const size_t M = (size_t)B * H * H;
      const int Ho = lv.strided ? 2 * H : H;
      T* xu = alloc<T>((size_t)B * Ho * Ho * Ci);
      const size_t mk = arena.mark();
      T* u1 = alloc<T>(M * Co);
      T* u2 = alloc<T>(M * Co);
      T* u3 = alloc<T>(M * Co);
      PRG_CHECK(arena.dry || (xu && u1 && u2 && u3), "workspace exhausted (up)");
      auto sk = skips.back(); skips.pop_back();
      if ((rc = resblock(lv.r0, x, Co, sk.first, sk.second, cs, u1, B, H, H, s))) return rc;
      sk = skips.back(); skips.pop_back();
      if ((rc = resblock(lv.r1, u1, Co, sk.first, sk.second, cs, u2, B, H, H, s))) return rc;
      if ((rc = attention(lv.at, u2, u3, B, H, H, s))) return rc;
      if ((rc = conv(lv.resample, u3, Co, nullptr, 0, B, H, H, 1, 1, lv.strided ? 1 : 0, ConvOpt(), xu, s))) return rc;
      arena.reset(mk);
      if (i == 0) tap("up0_out", xu, B, Ci, Ho, Ho);
      x = xu;
      H = Ho;
    }
    {
      const size_t M = (size_t)B * H * H;
      T* fr = alloc<T>(M * d0);
      PRG_CHECK(arena.dry || fr, "workspace exhausted (final)");
      // the final block's fused tail applies the 1x1 head to its LDS tile and writes only the network output (bf16 path,
      // no taps requested): `fr` is then never written
      const Head head{F(L.head_w), F(L.head_b), out, L.cfg.sigmoid_out};
      const bool offer = !taps_on && d0 == 64 && head_fuse_enabled();
      bool head_applied = false;
      if ((rc = resblock(L.fin, x, d0, x0, d0, cs, fr, B, H, H, s, offer ? &head : nullptr, &head_applied))) return rc;
      tap("final_res", fr, B, d0, H, H);
      if (!head_applied && (rc = run(launch_head_conv<T>, fr, head.w, head.b, out, (int64_t)M, d0, head.sigmoid, s))) return rc;
    }
    return PRG_OK;
  }

  int measure(int B, int S, size_t* bytes) override {
    Arena saved = arena;
    arena = Arena();
    arena.dry = true;
    CondSrc cs;
    int rc = forward(nullptr, cs, nullptr, B, S, nullptr);
    // general-path conditioning scratch lives in the same arena, after the activations
    size_t extra = 0;
    if (lay.cfg.conditional) extra = ((size_t)B * (lay.cfg.dim + 5 * lay.emb + lay.ss_total) * sizeof(float) + 4096);
    if (lay.cfg.in_channels == 3) extra += (size_t)B * 3 * S * S * sizeof(float) + 4096;  // DepthAugment output
    *bytes = arena.high + extra + (1 << 20);
    arena = saved;
    return rc;
  }

  // general conditioning path (per-image timesteps): cond = cat[time_mlp(t), param_mlp(K)] -> every block's Linear
  int cond_general(const int64_t* time, const float* param_cond, int B, CondSrc* out, hipStream_t s) override {
    const Layout& L = lay;
    const int e = L.emb, d0 = L.cfg.dim;
    // placed at the top of the arena so the forward's stack (which starts at 0) cannot reach it
    size_t need = (size_t)B * (d0 + 5 * e + L.ss_total) * sizeof(float) + 4096;
    PRG_CHECK(arena.cap >= need, "workspace too small for conditioning");
    float* base = reinterpret_cast<float*>(arena.base + ((arena.cap - need) & ~(size_t)255));
    float* sinu = base;                       // [B][d0]
    float* h1 = sinu + (size_t)B * d0;        // [B][e]
    float* cat = h1 + (size_t)B * e;          // [B][2e]  = [t_emb | p_emb]
    float* h2 = cat + (size_t)B * 2 * e;      // [B][e]
    float* ss = h2 + (size_t)B * e;           // [B][ss_total]
    int rc;
    if ((rc = launch_sinusoidal(time, d_freqs, sinu, B, d0, s))) return rc;
    if ((rc = launch_linear(sinu, d0, 0, F(L.tm1_w), d0, 0, F(L.tm1_b), h1, e, B, d0, e, ACT_NONE, ACT_GELU, s))) return rc;
    if ((rc = launch_linear(h1, e, 0, F(L.tm3_w), e, 0, F(L.tm3_b), cat, 2 * e, B, e, e, ACT_NONE, ACT_NONE, s))) return rc;
    const int pc = L.cfg.param_cond_dim;
    if ((rc = launch_linear(param_cond, pc, 0, F(L.pm0_w), pc, 0, F(L.pm0_b), h2, e, B, pc, e, ACT_NONE, ACT_GELU, s))) return rc;
    if ((rc = launch_linear(h2, e, 0, F(L.pm2_w), e, 0, F(L.pm2_b), cat + e, 2 * e, B, e, e, ACT_NONE, ACT_NONE, s))) return rc;
    auto one = [&](const ResP& r) -> int {
      return launch_linear(cat, 2 * e, 0, F(r.mlp_w), 2 * e, 0, F(r.mlp_b), ss + r.ss_off, L.ss_total, B, 2 * e,
                           2 * r.cout, ACT_SILU, ACT_NONE, s);
    };
    rc = PRG_OK;
    for_each_res(L, [&](const ResP& r) { if (rc == PRG_OK) rc = one(r); });
    if (rc) return rc;
    out->ss_a = ss;
    out->ss_a_stride = L.ss_total;
    out->ss_b = nullptr;
    out->row = nullptr;
    return PRG_OK;
  }

  int tap_copy(const Tap& t, float* out, hipStream_t s) override {
    if (t.nchw_f32) {
      PRG_HIP(hipMemcpyAsync(out, t.ptr, (size_t)t.B * t.C * t.H * t.W * sizeof(float), hipMemcpyDeviceToDevice, s));
      return PRG_OK;
    }
    return launch_nhwc_to_nchw_f32<T>(reinterpret_cast<const T*>(t.ptr), out, t.B, t.H * t.W, t.C, s);
  }
};

static int reserve(prg_unet* h, int B, int S) {
  if (B <= h->resB && S <= h->resS && h->arena.base) return PRG_OK;
  size_t bytes = 0;
  const int nb = B > h->resB ? B : h->resB, ns = S > h->resS ? S : h->resS;
  int rc = h->measure(nb, ns, &bytes);
  if (rc) return rc;
  PRG_HIP(hipDeviceSynchronize());
  if (h->arena.base) PRG_HIP(hipFree(h->arena.base));
  h->arena = Arena();
  if (hipMalloc(reinterpret_cast<void**>(&h->arena.base), bytes) != hipSuccess) {
    h->arena.base = nullptr;
    h->resB = h->resS = 0;
    return fail(PRG_E_NOMEM, "hipMalloc(workspace " + std::to_string(bytes >> 20) + " MiB)");
  }
  h->arena.cap = bytes;
  ++h->arena_gen;
  h->resB = nb;
  h->resS = ns;
  if (h->d_pq_static) {   // (bf16 / mxfp8 handles only)
    // fixed-point GroupNorm accumulators: two norms per ResnetBlock, [slots][resB][groups][2] int64
    if (h->d_gnacc) PRG_HIP(hipFree(h->d_gnacc));
    h->d_gnacc = nullptr;
    h->gn_slots = 2 * (4 * h->lay.L + 3);
    h->gnacc_bytes = (size_t)h->gn_slots * nb * h->lay.cfg.groups * 2 * sizeof(long long);
    if (hipMalloc(reinterpret_cast<void**>(&h->d_gnacc), h->gnacc_bytes) != hipSuccess) {
      h->d_gnacc = nullptr;
      return fail(PRG_E_NOMEM, "hipMalloc(GroupNorm accumulators)");
    }
  }
  return PRG_OK;
}

}  // namespace prg

using namespace prg;

// =============================================================================================
// sampler handle
// =============================================================================================
struct prg_sampler {
  prg_unet* unet = nullptr;
  int B = 0, S = 0, n_steps = 0;
  std::vector<prg_step> steps;
  DeviceBuffers own;          // the d_* buffers below
  prg_step* d_steps = nullptr;
  float* d_tpart = nullptr;   // [n_steps][ss_total]  time half of every block's conditioning (+ bias)
  float* d_ppart = nullptr;   // [B][ss_total]        camera-parameter half
  float* d_scratch = nullptr; // embedding scratch
  float* d_x = nullptr;       // state (B, S*S)
  float* d_u = nullptr;       // network output
  int* d_step = nullptr;
  uint64_t* d_seeds = nullptr;
  float* d_keep = nullptr;         // (n_steps) DDNM keep thresholds: uploaded by every run that has a table (prg_sampler_set_keep)
  std::vector<float> keep;         // host copy; empty = no table: the kernel gets a null pointer
  const float* keep_u = nullptr;   // caller's stored keep-mask uniforms (keep_slabs, B, S, S), null = Philox
  int64_t keep_slabs = 0;
  float* d_obj = nullptr;          // (2, n_steps) the objective's p row and q row: uploaded by every run whose objective != 0
  std::vector<float> obj;          // host copy [p | q] (prg_sampler_set_objective); empty with objective 0
  int objective = 0;
  hipStream_t own_stream = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  const float* g_cond = nullptr;   // pointers baked into the captured graph
  const float* g_noise = nullptr;
  const float* g_keep = nullptr;   // d_keep or null
  const float* g_keep_u = nullptr;
  int g_objective = 0;             // the objective chooses the kernel instantiation the graph holds
  float* g_out = nullptr;
  hipStream_t g_stream = nullptr;
  uint64_t g_arena_gen = 0;        // workspace generation the graph was captured against
  bool use_graph = true;
  ProfileSink prof;
  double last_total_ms = 0;
  ~prg_sampler() {
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

namespace prg {

static void sampler_free(prg_sampler* h) {
  if (h->exec) (void)hipGraphExecDestroy(h->exec);
  if (h->graph) (void)hipGraphDestroy(h->graph);
  h->exec = nullptr;
  h->graph = nullptr;
}

static int sampler_one_step(prg_sampler* h, const float* cond, const float* noise, float* out, hipStream_t s) {
  CondSrc cs;
  cs.ss_a = h->d_tpart;
  cs.ss_a_stride = 0;
  cs.row = h->d_step;
  cs.row_stride = h->unet->lay.ss_total;
  cs.ss_b = h->d_ppart;
  cs.ss_b_stride = h->unet->lay.ss_total;
  int rc = h->unet->forward(h->d_x, cs, h->d_u, h->B, h->S, s);
  if (rc) return rc;
  SamplerStepArgs a;
  a.x = h->d_x; a.u = h->d_u; a.cond = cond; a.noise = noise; a.steps = h->d_steps; a.step_idx = h->d_step;
  a.seeds = h->d_seeds; a.final_out = out; a.B = h->B; a.HW = h->S * h->S; a.n_steps = h->n_steps;
  a.ticket = h->d_step + 1;
  a.keep_p = h->keep.empty() ? nullptr : h->d_keep;
  a.keep_u = h->keep_u;
  a.objective = h->objective;
  a.obj_p = h->objective ? h->d_obj : nullptr;
  a.obj_q = h->objective ? h->d_obj + h->n_steps : nullptr;
  ProfileSink& p = h->prof;
  if (!p.on) return launch_sampler_step(a, s);   // its last workgroup advances the step counter
  if ((rc = p.step_ev.start(s))) return rc;
  rc = launch_sampler_step(a, s);
  if (int e = p.step_ev.stop(s)) return e;
  p.step_launches += 1;
  return rc;
}

}  // namespace prg

// =============================================================================================
// C-ABI
// =============================================================================================
extern "C" {

int prg_abi_version(void) { return PRG_ABI_VERSION; }
const char* prg_last_error(void) { return prg::last_error(); }

int prg_device_info(char* name, size_t name_len, int* compute_units) {
  int dev = 0;
  PRG_HIP(hipGetDevice(&dev));
  hipDeviceProp_t p;
  PRG_HIP(hipGetDeviceProperties(&p, dev));
  if (name && name_len) {
    std::strncpy(name, p.gcnArchName, name_len - 1);
    name[name_len - 1] = 0;
  }
  if (compute_units) *compute_units = p.multiProcessorCount;
  return PRG_OK;
}

int64_t prg_unet_param_count(const prg_unet_config* cfg) {
  if (!cfg) return PRG_E_INVALID;
  Layout L;
  if (build_layout_checked(*cfg, L)) return PRG_E_INVALID;
  return L.total;
}

int prg_unet_create(const prg_unet_config* cfg, const float* weights, int64_t n_floats, int dtype, prg_unet** out) {
  PRG_CHECK(cfg && weights && out, "prg_unet_create: null pointer");
  PRG_CHECK(dtype == PRG_F32 || dtype == PRG_BF16 || dtype == PRG_MXFP8 || dtype == PRG_F16X3,
            "prg_unet_create: dtype must be PRG_F32, PRG_BF16, PRG_MXFP8 or PRG_F16X3");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PRG_E_HIP, "prg_unet_create: no HIP device");
  *out = nullptr;
  std::unique_ptr<prg_unet> u;
  if (dtype == PRG_F32 || dtype == PRG_F16X3) u.reset(new UnetImpl<float>());
  else u.reset(new UnetImpl<bf16_t>());
  int rc = prepare_unet_weights(*u, *cfg, weights, n_floats, dtype);
  if (rc) return rc;
  *out = u.release();
  return PRG_OK;
}

int prg_unet_destroy(prg_unet* h) {
  if (!h) return PRG_OK;
  (void)hipDeviceSynchronize();
  if (h->d_gnacc) (void)hipFree(h->d_gnacc);   // (reallocated by reserve, like the workspace; the weights: prg_unet::own)
  if (h->arena.base) (void)hipFree(h->arena.base);
  delete h;
  return PRG_OK;
}

int prg_unet_set_time_freqs(prg_unet* h, const float* freqs, int n) {
  PRG_CHECK(h && freqs, "prg_unet_set_time_freqs: null pointer");
  PRG_CHECK(n == h->lay.cfg.dim / 2, "prg_unet_set_time_freqs: need dim/2 frequencies");
  PRG_HIP(hipDeviceSynchronize());
  PRG_HIP(hipMemcpy(h->d_freqs, freqs, sizeof(float) * n, hipMemcpyHostToDevice));
  return PRG_OK;
}

int prg_unet_reserve(prg_unet* h, int B, int S) {
  PRG_CHECK(h && B > 0 && S > 0, "prg_unet_reserve: bad arguments");
  return reserve(h, B, S);
}

int prg_unet_set_taps(prg_unet* h, int enable) {
  PRG_CHECK(h, "prg_unet_set_taps: null handle");
  h->taps_on = enable != 0;
  return PRG_OK;
}

int prg_unet_get_tap(prg_unet* h, const char* name, float* out, int64_t cap, int* C, int* H, int* W, void* stream) {
  PRG_CHECK(h && name && out, "prg_unet_get_tap: null pointer");
  auto it = h->taps.find(name);
  if (it == h->taps.end()) return fail(PRG_E_STATE, std::string("no such tap recorded: ") + name);
  const Tap& t = it->second;
  PRG_CHECK((int64_t)t.B * t.C * t.H * t.W <= cap, "prg_unet_get_tap: output buffer too small");
  if (C) *C = t.C;
  if (H) *H = t.H;
  if (W) *W = t.W;
  return h->tap_copy(t, out, (hipStream_t)stream);
}

int prg_unet_forward(prg_unet* h, const float* x, const int64_t* time, const float* param_cond, float* out, int B,
                     int S, void* stream) {
  PRG_CHECK(h && x && out, "prg_unet_forward: null pointer");
  PRG_CHECK(h->lay.cfg.conditional && time && param_cond, "prg_unet_forward: handle is not a conditional U-Net");
  PRG_CHECK(h->lay.cfg.in_channels == 1, "prg_unet_forward: in_channels must be 1");
  PRG_CHECK(B > 0 && S > 0, "prg_unet_forward: bad shape");
  int rc = reserve(h, B, S);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  CondSrc cs;
  if ((rc = h->cond_general(time, param_cond, B, &cs, s))) return rc;
  return h->forward(x, cs, out, B, S, s);
}

int prg_maskunet_forward(prg_unet* h, const float* depth, float* prob, int B, int S, void* stream) {
  PRG_CHECK(h && depth && prob, "prg_maskunet_forward: null pointer");
  PRG_CHECK(!h->lay.cfg.conditional && h->lay.cfg.in_channels == 3, "prg_maskunet_forward: handle is not a MaskUnet");
  PRG_CHECK(B > 0 && S > 0, "prg_maskunet_forward: bad shape");
  int rc = reserve(h, B, S);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  // DepthAugment output (B,3,S,S) float32 sits at the top of the arena, out of the forward stack's reach
  const size_t aug_bytes = (size_t)B * 3 * S * S * sizeof(float);
  PRG_CHECK(h->arena.cap > aug_bytes + 4096, "workspace too small");
  float* aug = reinterpret_cast<float*>(h->arena.base + ((h->arena.cap - aug_bytes - 256) & ~(size_t)255));
  if ((rc = prg_depth_augment(depth, aug, B, S, S, stream))) return rc;
  CondSrc cs;
  rc = h->forward(aug, cs, prob, B, S, s);
  if (h->taps_on) h->taps["augment"] = Tap{aug, 3, S, S, B, true};
  return rc;
}

// ---------------------------------------------------------------------------------------------
int prg_sampler_create(prg_unet* unet, const prg_step* steps, int n_steps, int B, int S, prg_sampler** out) {
  PRG_CHECK(unet && steps && out, "prg_sampler_create: null pointer");
  PRG_CHECK(unet->lay.cfg.conditional && unet->lay.cfg.in_channels == 1, "prg_sampler_create: needs the conditional U-Net");
  PRG_CHECK(n_steps > 0 && B > 0 && S > 0, "prg_sampler_create: bad sizes");
  int rc = reserve(unet, B, S);
  if (rc) return rc;
  std::unique_ptr<prg_sampler> h(new prg_sampler());
  h->unet = unet; h->B = B; h->S = S; h->n_steps = n_steps;
  h->steps.assign(steps, steps + n_steps);
  const Layout& L = unet->lay;
  const int e = L.emb, d0 = L.cfg.dim, W = L.ss_total;
  const size_t HW = (size_t)S * S;
  const int R = n_steps > B ? n_steps : B;
  const char* nomem = "prg_sampler_create: hipMalloc failed";
  h->d_steps = h->own.upload(steps, (size_t)n_steps, nomem);
  h->d_tpart = h->own.alloc<float>((size_t)n_steps * W, nomem);
  h->d_ppart = h->own.alloc<float>((size_t)B * W, nomem);
  h->d_scratch = h->own.alloc<float>((size_t)R * (d0 + 2 * e) + n_steps, nomem);   // (+ n_steps int32 timesteps)
  h->d_x = h->own.alloc<float>(B * HW, nomem);
  h->d_u = h->own.alloc<float>(B * HW, nomem);
  h->d_step = h->own.alloc<int>(2, nomem);
  h->d_seeds = h->own.alloc<uint64_t>((size_t)B, nomem);
  h->d_keep = h->own.alloc<float>((size_t)n_steps, nomem);
  h->d_obj = h->own.alloc<float>(2 * (size_t)n_steps, nomem);
  if (h->own.rc) return h->own.rc;
  PRG_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault));
  // time half of the conditioning for every transition: Tpart[k] = W_t . SiLU(time_mlp(t_k)) + bias
  {
    hipStream_t s = h->own_stream;
    float* sinu = h->d_scratch;
    float* h1 = sinu + (size_t)R * d0;
    float* temb = h1 + (size_t)R * e;
    int32_t* tdev = reinterpret_cast<int32_t*>(temb + (size_t)R * e);
    std::vector<int32_t> tt(n_steps);
    for (int k = 0; k < n_steps; ++k) tt[k] = steps[k].t;
    PRG_HIP(hipMemcpyAsync(tdev, tt.data(), sizeof(int32_t) * n_steps, hipMemcpyHostToDevice, s));
    const float* F = unet->d_flat;
    if ((rc = launch_sinusoidal_i32(tdev, unet->d_freqs, sinu, n_steps, d0, s))) return rc;
    if ((rc = launch_linear(sinu, d0, 0, F + L.tm1_w, d0, 0, F + L.tm1_b, h1, e, n_steps, d0, e, ACT_NONE, ACT_GELU, s))) return rc;
    if ((rc = launch_linear(h1, e, 0, F + L.tm3_w, e, 0, F + L.tm3_b, temb, e, n_steps, e, e, ACT_NONE, ACT_NONE, s))) return rc;
    auto one = [&](const ResP& r) -> int {
      return launch_linear(temb, e, 0, F + r.mlp_w, 2 * e, 0, F + r.mlp_b, h->d_tpart + r.ss_off, W, n_steps, e,
                           2 * r.cout, ACT_SILU, ACT_NONE, s);
    };
    rc = PRG_OK;
    for_each_res(L, [&](const ResP& r) { if (rc == PRG_OK) rc = one(r); });
    if (rc) return rc;
    PRG_HIP(hipStreamSynchronize(s));
  }
  *out = h.release();
  return PRG_OK;
}

int prg_sampler_destroy(prg_sampler* h) {
  if (!h) return PRG_OK;
  (void)hipDeviceSynchronize();
  sampler_free(h);
  delete h;   // (events, stream and device buffers: ~prg_sampler)
  return PRG_OK;
}

int prg_sampler_set_graph(prg_sampler* h, int enable) {
  PRG_CHECK(h, "prg_sampler_set_graph: null handle");
  h->use_graph = enable != 0;
  return PRG_OK;
}

int prg_sampler_set_keep(prg_sampler* h, const float* keep_p, int n) {
  PRG_CHECK(h, "prg_sampler_set_keep: null handle");
  if (!keep_p) { h->keep.clear(); return PRG_OK; }
  PRG_CHECK(n == h->n_steps, "prg_sampler_set_keep: the table needs one threshold per transition");
  h->keep.assign(keep_p, keep_p + n);   // reaches d_keep on the stream of the next run, behind whatever still reads the old table
  return PRG_OK;
}

int prg_sampler_set_objective(prg_sampler* h, int objective, const float* p, const float* q, int n) {
  PRG_CHECK(h, "prg_sampler_set_objective: null handle");
  PRG_CHECK(objective >= 0 && objective <= 2, "prg_sampler_set_objective: unknown objective (0 = pred_x0, 1 = pred_noise, 2 = pred_v)");
  if (objective == 0) { h->objective = 0; h->obj.clear(); return PRG_OK; }
  PRG_CHECK(p && q, "prg_sampler_set_objective: pred_noise and pred_v need their p and q tables");
  PRG_CHECK(n == h->n_steps, "prg_sampler_set_objective: the table needs one (p, q) pair per transition");
  // like the keep table: reaches d_obj on the stream of the next run, behind whatever still reads the old one.  A captured graph
  // holds the instantiation of the objective it was captured with: prg_sampler_run captures again when the objective differs.
  h->obj.assign(p, p + n);
  h->obj.insert(h->obj.end(), q, q + n);
  h->objective = objective;
  return PRG_OK;
}

int prg_sampler_set_keep_draws(prg_sampler* h, const float* u, int64_t slabs) {
  PRG_CHECK(h, "prg_sampler_set_keep_draws: null handle");
  PRG_CHECK(!u || slabs > 0, "prg_sampler_set_keep_draws: stored uniforms need at least one slab");
  h->keep_u = u;
  h->keep_slabs = u ? slabs : 0;
  return PRG_OK;
}

int prg_sampler_set_profile(prg_sampler* h, int enable) {
  PRG_CHECK(h, "prg_sampler_set_profile: null handle");
  h->prof.on = enable != 0;
  return PRG_OK;
}

int prg_sampler_get_profile_executed(prg_sampler* h, double* conv_flops_executed) {
  PRG_CHECK(h && conv_flops_executed, "prg_sampler_get_profile_executed: null argument");
  *conv_flops_executed = h->prof.conv_flops_exec;
  return PRG_OK;
}

int prg_sampler_get_profile_bytes(prg_sampler* h, double* conv_bytes) {
  PRG_CHECK(h && conv_bytes, "prg_sampler_get_profile_bytes: null argument");
  *conv_bytes = h->prof.conv_bytes;
  return PRG_OK;
}

int prg_sampler_get_profile_shapes(prg_sampler* h, prg_profile_shape* rows, int32_t max_rows, int32_t* n_rows) {
  PRG_CHECK(h && n_rows && (rows || max_rows == 0), "prg_sampler_get_profile_shapes: null argument");
  const int n = (int)h->prof.shapes.size();
  *n_rows = n;
  for (int i = 0; i < n && i < max_rows; ++i) rows[i] = h->prof.shapes[i];
  return PRG_OK;
}

int prg_sampler_get_profile_step(prg_sampler* h, double* step_ms, int64_t* step_launches) {
  PRG_CHECK(h && step_ms && step_launches, "prg_sampler_get_profile_step: null argument");
  *step_ms = h->prof.step_ms;
  *step_launches = h->prof.step_launches;
  return PRG_OK;
}

int prg_sampler_get_profile(prg_sampler* h, double* conv_ms, int64_t* conv_launches, double* conv_flops,
                            double* total_ms) {
  PRG_CHECK(h, "prg_sampler_get_profile: null handle");
  if (conv_ms) *conv_ms = h->prof.conv_ms;
  if (conv_launches) *conv_launches = h->prof.launches;
  if (conv_flops) *conv_flops = h->prof.conv_flops;
  if (total_ms) *total_ms = h->last_total_ms;
  return PRG_OK;
}

int prg_sampler_run(prg_sampler* h, const float* param_cond, const float* img_cond, const float* noise,
                    int64_t noise_slabs, const uint64_t* seeds, float* out, void* stream) {
  PRG_CHECK(h && param_cond && out, "prg_sampler_run: null pointer");
  PRG_CHECK(noise || seeds, "prg_sampler_run: need stored noise or per-scene seeds");
  if (noise) {
    int64_t need = 1;
    for (int k = 0; k < h->n_steps; ++k)
      if (h->steps[k].sigma != 0.0f) need = k + 2;
    PRG_CHECK(noise_slabs >= need, "prg_sampler_run: stored noise has too few slabs for this transition table");
  }
  // rows that draw a keep mask: a threshold >= 0, a condition to thin out, not the refine row (sampler_step_kernel's own test)
  bool draws_keep = false;
  for (int k = 0; k < h->n_steps && img_cond && !h->keep.empty(); ++k)
    if (h->keep[k] >= 0.0f && !(h->steps[k].clip_pred & 4)) {
      draws_keep = true;
      PRG_CHECK(!h->keep_u || h->keep_slabs >= k + 1, "prg_sampler_run: stored keep-mask uniforms have too few slabs for this keep table");
    }
  PRG_CHECK(!draws_keep || h->keep_u || seeds, "prg_sampler_run: the keep mask needs stored uniforms or per-scene seeds");
  prg_unet* u = h->unet;
  PRG_CHECK(u->resB >= h->B && u->resS >= h->S, "prg_sampler_run: U-Net workspace was shrunk");
  hipStream_t s = stream ? (hipStream_t)stream : h->own_stream;
  const Layout& L = u->lay;
  const int e = L.emb, W = L.ss_total, B = h->B;
  int rc;
  if (seeds) PRG_HIP(hipMemcpyAsync(h->d_seeds, seeds, sizeof(uint64_t) * B, hipMemcpyHostToDevice, s));
  PRG_HIP(hipMemsetAsync(h->d_step, 0, 2 * sizeof(int), s));   // [step counter, arrival ticket]
  if (!h->keep.empty()) PRG_HIP(hipMemcpyAsync(h->d_keep, h->keep.data(), sizeof(float) * h->n_steps, hipMemcpyHostToDevice, s));
  if (h->objective) PRG_HIP(hipMemcpyAsync(h->d_obj, h->obj.data(), sizeof(float) * 2 * h->n_steps, hipMemcpyHostToDevice, s));
  // camera half of the conditioning: Ppart[b] = W_p . SiLU(param_mlp(K_b))
  {
    float* h2 = h->d_scratch;
    float* pemb = h2 + (size_t)B * e;
    const float* F = u->d_flat;
    const int pc = L.cfg.param_cond_dim;
    if ((rc = launch_linear(param_cond, pc, 0, F + L.pm0_w, pc, 0, F + L.pm0_b, h2, e, B, pc, e, ACT_NONE, ACT_GELU, s))) return rc;
    if ((rc = launch_linear(h2, e, 0, F + L.pm2_w, e, 0, F + L.pm2_b, pemb, e, B, e, e, ACT_NONE, ACT_NONE, s))) return rc;
    auto one = [&](const ResP& r) -> int {
      return launch_linear(pemb, e, 0, F + r.mlp_w, 2 * e, e, nullptr, h->d_ppart + r.ss_off, W, B, e, 2 * r.cout,
                           ACT_SILU, ACT_NONE, s);
    };
    rc = PRG_OK;
    for_each_res(L, [&](const ResP& r) { if (rc == PRG_OK) rc = one(r); });
    if (rc) return rc;
  }
  if ((rc = launch_sampler_init(h->d_x, noise, h->d_seeds, B, h->S * h->S, s))) return rc;

  const bool profiling = h->prof.on;
  h->prof.reset();
  // the U-Net reports its conv launches to this sampler for the length of this call only, whichever way the call ends
  struct ProfLink { prg_unet* u; ~ProfLink() { u->prof = nullptr; } } link{u};
  u->prof = profiling ? &h->prof : nullptr;
  struct ScopedEvent { hipEvent_t e = nullptr; ~ScopedEvent() { if (e) (void)hipEventDestroy(e); } } t0, t1;
  if (profiling) {
    PRG_HIP(hipEventCreate(&t0.e));
    PRG_HIP(hipEventCreate(&t1.e));
    PRG_HIP(hipEventRecord(t0.e, s));
  }
  if (h->use_graph && !profiling && !u->taps_on) {
    const float* keep_p = h->keep.empty() ? nullptr : h->d_keep;
    const bool stale = !h->exec || h->g_cond != img_cond || h->g_noise != noise || h->g_out != out || h->g_stream != s ||
                       h->g_arena_gen != u->arena_gen || h->g_keep != keep_p || h->g_keep_u != h->keep_u ||
                       h->g_objective != h->objective;
    if (stale) {
      sampler_free(h);
      PRG_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      rc = sampler_one_step(h, img_cond, noise, out, s);
      hipGraph_t g = nullptr;
      hipError_t ce = hipStreamEndCapture(s, &g);
      if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
      if (ce != hipSuccess) return fail(PRG_E_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
      h->graph = g;
      PRG_HIP(hipGraphInstantiate(&h->exec, h->graph, nullptr, nullptr, 0));
      h->g_cond = img_cond; h->g_noise = noise; h->g_out = out; h->g_stream = s; h->g_arena_gen = u->arena_gen;
      h->g_keep = keep_p; h->g_keep_u = h->keep_u; h->g_objective = h->objective;
    }
    for (int k = 0; k < h->n_steps; ++k) PRG_HIP(hipGraphLaunch(h->exec, s));
  } else {
    for (int k = 0; k < h->n_steps; ++k) {
      if ((rc = sampler_one_step(h, img_cond, noise, out, s))) return rc;
      if (profiling) {
        PRG_HIP(hipStreamSynchronize(s));
        if ((rc = h->prof.harvest())) return rc;
      }
    }
  }
  if (profiling) {
    PRG_HIP(hipEventRecord(t1.e, s));
    PRG_HIP(hipEventSynchronize(t1.e));
    float ms = 0;
    PRG_HIP(hipEventElapsedTime(&ms, t0.e, t1.e));
    h->last_total_ms = ms;
  }
  return PRG_OK;
}

}  // extern "C"
