// conv_choose.cpp — the selection of conv_choose.h.  Host-only C++: no HIP headers, no device, no environment.
#include "conv_choose.h"

#include <cstddef>
#include <cstdint>

namespace prg {
namespace {

// in-kernel GroupNorm fold of the prologue (common.h, GnFold): valid when an 8-channel unit lies inside one group
static bool fold_in_kernel(const ConvFacts& f) {
  return f.pro_fold_pq && f.pro_fold_cpg % 8 == 0 && f.pro_fold_G * f.pro_fold_cpg == f.d.C0 && f.d.C1 == 0;
}

// whether a launch of `total` tiles is large enough for the 256-pixel kernels (at least `dflt` tiles); PRG_W256_MIN_TILES=<n> > 0
// replaces the threshold (tests force small shapes onto them)
static bool w256_fills(long total, int dflt, const ConvSwitches& sw) {
  return total >= (sw.w256_min_tiles > 0 ? sw.w256_min_tiles : dflt);
}

// Fused GroupNorm statistics of the output, the two rules.  Kernels whose consumer wave rows each write a partial: a group must lie
// inside one wave's 64 channels, as a power-of-two run of 8-channel units.  Kernels that reduce a whole bn-channel tile: a group of
// 8-channel units whose width divides the tile.  Either way at most kGnMaxSplit slabs per image.
static int wave_rows_fuse(const ConvFacts& L, int slabs) {
  const int cpg = L.gn_groups > 0 ? L.d.Cout / L.gn_groups : 0;
  return L.gn_partials && cpg % 8 == 0 && cpg <= 64 && (cpg & (cpg - 1)) == 0 && slabs <= kGnMaxSplit;
}
static int tile_fuse(const ConvFacts& L, int bn, int slabs) {
  const int cpg = L.gn_groups > 0 ? L.d.Cout / L.gn_groups : 0;
  // bn % cpg: the tile reductions (conv_epi.h epilogue_stats, the split halo kernel's direct epilogue) give a tile bn / cpg whole
  // groups starting at its first channel; a width that does not divide the tile (24 channels: 192 / 8) would straddle two tiles
  return L.gn_partials && cpg % 8 == 0 && cpg <= bn && (cpg == 0 || bn % cpg == 0) && slabs <= kGnMaxSplit;
}

// th x tw-pixel tiles of an H x W image times bn-channel tiles, one workgroup each (the persistent kernels set their own grid)
static void set_tiles(ConvChoice* c, int family, int th, int tw, int bn, int H, int W, int Cout, int B) {
  c->family = family;
  c->th = th; c->tw = tw; c->bn = bn;
  c->tiles_x = W / tw; c->tiles_y = H / th; c->tiles_n = Cout / bn;
  c->grid = c->tiles_x * c->tiles_y * c->tiles_n * B;
}
// statistics of the output: `slabs` per image, or (kernels that can, when the launch offers gn_acc) the fixed-point accumulators
static void set_stats(ConvChoice* c, int fuse, int slabs, int gn_acc = 0) {
  c->fuse_stats = fuse;
  c->nsplit = fuse ? slabs : 0;
  c->acc_done = fuse && gn_acc;
}

// conv_c64.hip: the weights-stationary kernel for the 64 -> 64 convs
static bool choose_c64(const ConvFacts& L, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  constexpr int TH = 8, TW = 32;
  if (!sw.conv_c64) return false;
  const ConvDesc& d = L.d;
  if (!(d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1)) return false;
  if (d.C0 != 64 || d.C1 != 0 || d.Cout != 64 || d.CoutPad != 64 || d.kchunks != 2) return false;
  if (L.residual || !L.bias) return false;
  if (d.ups) return false;                                   // (no 64 -> 64 Upsample conv exists in the networks: not a tested shape)
  if (d.Wout % TW || d.Hout % TH) return false;
  // the producers address the input through ONE buffer descriptor with 32-bit byte offsets (pixel index * 128 in an SGPR,
  // num_records as an int): beyond 2 GiB of input the generic kernel (64-bit addressing) runs instead — B = 256 at 256x256
  if ((size_t)d.B * d.Hin * d.Win * 128 + 4096 >= ((size_t)1 << 31)) return false;
  const int tiles_x = d.Wout / TW, tiles_y = d.Hout / TH;
  const int total = tiles_x * tiles_y * d.B;
  if (num_cus <= 0) return false;
  int grid = (total < num_cus ? total : num_cus) & ~7;       // multiple of 8: XCD-contiguous tile runs
  if (grid < 8) return false;                                // tiny launches stay on the generic kernels
  const int cpg = L.gn_groups > 0 ? 64 / L.gn_groups : 0;
  const int split_n = cpg > 32 ? 2 : 1;
  const int fuse = wave_rows_fuse(L, tiles_x * tiles_y * 2 * split_n);
  if (L.gn_partials && !fuse) return false;
  const bool fold_ok = L.pro_fold_acc && L.pro_fold_pq && L.pro_fold_G * L.pro_fold_cpg == 64 && L.pro_fold_cpg % 8 == 0;
  if (L.pro_fold_acc && !fold_ok) return false;
  if (L.in_f16 && !(fold_ok && L.w_f16)) return false;       // h16 input: only through the folded prologue, with f16 weights
  const int pro = L.in_f16 ? 3 : fold_ok ? 2 : (L.pro_a ? 1 : 0);
  if (L.out_f16 && pro != 0) return false;                   // h16 output: conv1 of a ResnetBlock (no prologue)
  set_tiles(c, kConvC64, TH, TW, 64, d.Hout, d.Wout, 64, d.B);
  c->grid = grid;
  c->pro = pro;
  c->mode = L.out_f16 ? 1 : 0;
  set_stats(c, fuse, tiles_x * tiles_y * 2 * split_n, L.gn_acc);
  return true;
}

// What the four entries of conv_w256.hip share: 256-pixel tiles (32 x 8 or 16 x 16) of an H x W image and 128-channel tiles
// (Cout = 64: one, where `narrow` allows it), an XCD pinned to one channel tile (so 1, 2, 4 or 8 of them), one workgroup per CU of
// whole XCDs, and a launch of at least `fill(grid)` work items (`per_tile` of them per tile).
static bool w256_tiles(const ConvFacts& L, int H, int W, bool narrow, int per_tile, int num_cus, const ConvSwitches& sw, int fill_div,
                       ConvChoice* c) {
  constexpr int kCH = 64, BN = 128;
  const ConvDesc& d = L.d;
  if (d.C0 % kCH || d.C1 % kCH || d.C0 == 0 || d.CoutPad != d.Cout) return false;
  if (!(narrow && d.Cout == 64) && d.Cout % BN) return false;
  if (L.residual || !L.bias) return false;
  const int tiles_n = d.Cout == 64 ? 1 : d.Cout / BN;
  if (tiles_n != 1 && tiles_n != 2 && tiles_n != 4 && tiles_n != 8) return false;
  int tw = 0;
  if (W % 32 == 0 && H % 8 == 0) tw = 32;
  else if (W % 16 == 0 && H % 16 == 0) tw = 16;
  else return false;
  const int th = 256 / tw, tiles_x = W / tw, tiles_y = H / th;
  const long total = (long)tiles_x * tiles_y * tiles_n * d.B * per_tile;
  const int grid = num_cus & ~7;
  if (num_cus <= 0 || grid < 8 || !w256_fills(total, grid / fill_div, sw)) return false;
  c->th = th; c->tw = tw; c->bn = BN;
  c->tiles_x = tiles_x; c->tiles_y = tiles_y; c->tiles_n = tiles_n;
  c->grid = grid;
  return true;
}

// conv_w256.hip, 3x3 / stride 1 / pad 1 where the launch fills the chip: bf16 operands, or MX-fp8 ones (handles of dtype PRG_MXFP8)
static bool choose_w256(const ConvFacts& L, bool mx, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  if (mx ? !sw.conv_w256mx || !L.w_mx : !sw.conv_w256) return false;
  const ConvDesc& d = L.d;
  if (!(d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1)) return false;
  if (L.pro_a && d.C1) return false;                         // the fused prologue is defined for a single source
  if (d.ups && ((d.Hout | d.Wout) & 1)) return false;
  const bool fold = L.pro_fold_acc && fold_in_kernel(L);
  if (!mx) {
    if (L.in_f16 && !(fold && L.w_f16)) return false;        // h16 input: only through the in-kernel fold, with f16 weights
    if (L.out_f16 && (L.pro_a || L.pro_fold_acc)) return false;   // h16 output: conv1 of a ResnetBlock (no prologue)
  }
  // bf16, fewer tiles than CUs: the 128-pixel tiles of conv_ws.hip fill the chip better.
  // MX, round 5: a launch with fewer tiles than CUs stays on the bf16 kernels (the network's level-3 convs: 128 tiles on 256 CUs —
  // measured at the configs[4] shape, same box, same positions: 25 / 29 us on conv3x3_ws_kernel against 28-29 / 38-40 us here,
  // profiles/r05_configs4_conv_per_launch_bf16_vs_mxfp8.txt); mx_pure (the conv-level tests) keeps the old half-a-wave threshold
  ConvChoice t;
  if (!w256_tiles(L, d.Hout, d.Wout, false, 1, num_cus, sw, mx && L.mx_pure ? 2 : 1, &t)) return false;
  const int slabs = t.tiles_x * t.tiles_y * 2;
  const int fuse = wave_rows_fuse(L, slabs);
  if (L.gn_partials && !fuse) return false;
  *c = t;
  c->family = mx ? kConvW256Mx : kConvW256;
  c->fill_tables = L.pro_fold_acc && !fold;
  c->pro = (!mx && L.in_f16) ? 3 : fold ? 2 : (L.pro_a ? 1 : 0);
  set_stats(c, fuse, slabs, L.gn_acc);
  c->is_mx = mx;
  return true;
}

// conv_w256.hip MODE 2: Upsample (nearest x2) + 3x3 conv as four 2 x 2-tap sub-pixel convolutions of the source image
static bool choose_up_w256(const ConvFacts& L, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  if (!sw.up2x2 || !L.w_up) return false;
  const ConvDesc& d = L.d;
  if (!(d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.ups == 1 && d.C1 == 0)) return false;
  if (L.pro_a || L.pro_fold_acc || L.gn_partials || L.out_f16 || L.in_f16) return false;
  if (d.Hout != 2 * d.Hin || d.Wout != 2 * d.Win) return false;
  if ((size_t)d.B * d.Hin * d.Win * d.C0 * 2 >= ((size_t)1 << 31)) return false;   // (32-bit halo offsets, as the other modes)
  // tiles of 256 SOURCE pixels, four phases each (Cout = 64: two x-phases per tile)
  ConvChoice t;
  if (!w256_tiles(L, d.Hin, d.Win, true, d.Cout == 64 ? 2 : 4, num_cus, sw, 2, &t)) return false;
  *c = t;
  c->family = kConvW256;
  c->mode = 2;
  c->exec_scale = 4.0 / 9.0;                                 // (what the profile reports as EXECUTED work)
  return true;
}

// conv_w256.hip MODE 1: Conv2d(C, Cout, 4, stride 2, pad 1) as a 2 x 2-tap conv over the space-to-depth view
static bool choose_down_w256(const ConvFacts& L, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  if (!sw.conv_down_w256 || !L.w_s2d) return false;
  const ConvDesc& d = L.d;
  if (!(d.KH == 4 && d.KW == 4 && d.stride == 2 && d.pad == 1 && d.ups == 0 && d.C1 == 0)) return false;
  if (d.C0 > 128 || L.pro_a || L.gn_partials) return false;
  if (d.Hin != 2 * d.Hout || d.Win != 2 * d.Wout) return false;
  ConvChoice t;
  if (!w256_tiles(L, d.Hout, d.Wout, true, 1, num_cus, sw, 2, &t)) return false;   // the generic kernel for tiny launches
  *c = t;
  c->family = kConvW256;
  c->mode = 1;
  return true;
}

// conv_ws.hip: the wave-specialised kernel on 128-pixel tiles.  It reads coefficient tables (hand-counted loads): accumulators
// are folded into them first.
static bool choose_ws(const ConvFacts& L, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  constexpr int kCH = 64;
  if (!sw.conv_ws) return false;
  const ConvDesc& d = L.d;
  if (!(d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1)) return false;
  if (d.C0 % kCH || d.C1 % kCH || d.Cout % 64) return false;
  if (L.residual || !L.bias) return false;
  if (L.in_f16 || (L.out_f16 && L.pro_a)) return false;      // h16 (conv.h): f16 OUTPUT only, from a launch without prologue
  {
    const int tn128 = d.Cout % 128 == 0 ? d.Cout / 128 : d.Cout / 64;   // Cout tiles of the configuration chosen below
    if (tn128 != 1 && tn128 != 2 && tn128 != 4 && tn128 != 8) return false;  // every workgroup must own ONE channel tile
  }
  if (num_cus <= 0) return false;
  const int H = d.Hout, W = d.Wout;
  int TH, TW, BN;
  if (d.Cout % 128 == 0) {
    if (W % 32 == 0 && H % 4 == 0) { TH = 4; TW = 32; BN = 128; }
    else if (W % 16 == 0 && H % 8 == 0) { TH = 8; TW = 16; BN = 128; }
    else return false;
  } else {
    if (W % 32 == 0 && H % 8 == 0) { TH = 8; TW = 32; BN = 64; }
    else return false;
  }
  const int waves_m = 4 / (BN / 64);
  const int fuse = wave_rows_fuse(L, (W / TW) * (H / TH) * waves_m);   // one partial per (tile, consumer wave row)
  ConvChoice t;
  set_tiles(&t, kConvWs, TH, TW, BN, H, W, d.Cout, d.B);
  if (t.grid > num_cus) t.grid = num_cus;        // persistent: one workgroup per CU at the most
  if (t.grid >= 8) t.grid &= ~7;                 // multiple of 8: XCD-contiguous runs inside a round
  if (t.tiles_n > 1 && (t.grid & 7) != 0) return false;   // a workgroup must own one channel tile (bias in LDS)
  *c = t;
  c->fill_tables = L.pro_fold_acc;
  c->pro = L.pro_a ? 1 : 0;
  set_stats(c, fuse, t.tiles_x * t.tiles_y * waves_m, L.gn_acc);
  return true;
}

// the generic 3x3 / s1 / p1 kernels' tile (halo kernel, and the simple MX kernel of PRG_MX_PURE)
static bool pick_halo(const ConvDesc& d, int f32, ConvChoice* c) {
  const int CH = f32 ? 32 : 64;                              // 8 16-byte vectors
  if (!(d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1)) return false;
  if (d.C0 % CH || d.C1 % CH || d.Cout % 64) return false;
  const int H = d.Hout, W = d.Wout;
  if (d.Cout % 128 == 0) {
    if (W % 32 == 0 && H % 4 == 0) { c->th = 4; c->tw = 32; c->bn = 128; return true; }
    if (W % 16 == 0 && H % 8 == 0) { c->th = 8; c->tw = 16; c->bn = 128; return true; }
    return false;
  }
  if (W % 32 == 0 && H % 8 == 0) { c->th = 8; c->tw = 32; c->bn = 64; return true; }
  if (W % 16 == 0 && H % 8 == 0) { c->th = 8; c->tw = 16; c->bn = 64; return true; }
  return false;
}

static void halo_tiles(const ConvFacts& L, int family, ConvChoice* c) {
  set_tiles(c, family, c->th, c->tw, c->bn, L.d.Hout, L.d.Wout, L.d.Cout, L.d.B);
  set_stats(c, tile_fuse(L, c->bn, c->tiles_x * c->tiles_y), c->tiles_x * c->tiles_y);
}

// MX-fp8 operands when the handle carries them
static bool choose_mx(const ConvFacts& L, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  if (!L.w_mx) return false;
  // Round 5: the wide Upsample convs of an mxfp8 handle run the bf16 SUB-PIXEL form (four 2 x 2-tap convolutions, 4 / 9 of the MACs:
  // 64-67 us at the configs[4] shape) — the nine-tap MX launch took 77-81 us (same box, same positions:
  // profiles/r05_configs4_conv_per_launch_bf16_vs_mxfp8.txt); mx_pure keeps them on MX operands
  if (L.d.ups && !L.gn_partials && !L.mx_pure && !sw.mx_pure && choose_up_w256(L, num_cus, sw, c)) return true;
  if (choose_w256(L, true, num_cus, sw, c)) return true;     // 256-pixel x 128-channel tiles with MX operands
  // Shapes the 256-pixel MX kernel does not cover (the 64-channel convs, launches with few tiles): by default the bf16
  // kernels run them (those shapes are HBM- / VALU-bound: fp8 operands buy nothing there); PRG_MX_PURE=1 keeps every 3x3
  // conv on MX operands through the simple halo-tile kernel.
  if (!sw.mx_pure && !L.mx_pure) return false;
  if (L.residual || !pick_halo(L.d, 0, c)) return false;
  halo_tiles(L, kConvMxHalo, c);
  c->fill_tables = L.pro_fold_acc;
  c->is_mx = 1;
  return true;
}

static void igemm_tiles(const ConvFacts& L, int M, int BM, int BN, bool wide, ConvChoice* c) {
  const ConvDesc& d = L.d;
  c->bm = BM; c->bn = BN;
  c->tiles_x = (int)(((int64_t)M + BM - 1) / BM); c->tiles_y = 1; c->tiles_n = d.CoutPad / BN;
  c->grid = c->tiles_x * c->tiles_n;
  const int HWo = d.Hout * d.Wout;
  set_stats(c, wide && HWo % BM == 0 && tile_fuse(L, BN, HWo / BM), HWo / BM);
  c->mode = d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0 && !d.ups;
}

// f16x3 mode: the split-operand kernels (conv_split.hip, conv_split512.hip)
static bool choose_split(const ConvFacts& L, int num_cus, const ConvSwitches& sw, ConvChoice* c) {
  if (!L.w_split) return false;
  const ConvDesc& d = L.d;
  if (d.Cout % 8 || d.C0 % 8 || d.C1 % 8 || L.res_fold_acc || L.pro_fold_acc) return false;
  // the activated residual (ConvLaunch::res_a: the ResnetBlock tail in a 1x1 res_conv's epilogue) is the shared transposing
  // epilogue's feature: the gather kernel below has it, the 3x3 kernels do not
  if (L.res_a && !(d.KH == 1 && d.KW == 1)) return false;
  const int64_t M64 = (int64_t)d.B * d.Hout * d.Wout;
  if ((int64_t)d.B * d.Hin * d.Win >= ((int64_t)1 << 31) || M64 >= ((int64_t)1 << 31)) return false;
  const int M = (int)M64;
  const int want_stats = L.gn_partials;
  const bool halo = d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.C0 % 32 == 0 && d.C1 % 32 == 0 && d.Cout % 64 == 0;
  if (halo) {
    const int H = d.Hout, W = d.Wout;
    // The Upsample convs as four 2 x 2-tap sub-pixel convolutions (4 / 9 of their MFMAs: 0.3 ms = 2.5 % of an f16x3 evaluation): OFF by
    // default.  Per evaluation it is as accurate as the nine-tap form (test_split_upsample_conv_against_float64: rms 2.0e-7 against
    // torch-CPU's 2.9e-7), but every change of the rounding pattern RE-DRAWS the long chains' distance from the reference — over nine
    // equal-precision variants of the mode's arithmetic the 250-step 256 x 256 chain G21b sits anywhere in 3.7e-5 .. 8.8e-5 m at B = 1
    // (profiles/r05_chain_metric_spread_f16x3.txt; the reference's own 1-vs-8-thread spread is 4.7e-5 m) — and round 5 tried it as the
    // default: G21b drew 5.9e-5 m at B = 1 and 1.001e-4 m at B = 8 (the batch that selects the persistent 64-channel kernel).  The
    // mode's claim is the LITERAL 1e-4 m on that chain at the tested batches, so the nine-tap form stays.  PRG_SPLIT_UP2X2=1: on.
    if (sw.split_up2x2 && d.ups && L.w_up_split && d.C1 == 0 && d.Cout % 128 == 0 && d.Win % 16 == 0 && d.Hin % 8 == 0 && d.Hout == 2 * d.Hin &&
        d.Wout == 2 * d.Win && !L.residual && !L.pro_a && !want_stats) {
      set_tiles(c, kConvSplitWs, 8, 16, 128, d.Hin, d.Win, d.Cout, d.B * 4);   // tiles of the source image, four phases each
      c->mode = 1;
      return true;
    }
    // conv_split512.hip (round 6): one wave per SIMD, 128 x 64 wave tiles, for launches with a 256-pixel tile per CU; bit-identical to
    // the wave-specialised kernel below.  Default ON for launches with at least one 256-pixel x 128-channel tile per CU (same-box A/B,
    // profiles/r06_ab_split_w512.txt: -3 ... -5 % per launch against conv3x3_split_ws_kernel, the whole f16x3 pipeline +2.4 %; with
    // half as many workgroups as the 128-pixel kernel a launch below that size leaves CUs idle: 256 -> 256 @16x16 at B = 64 ran 83 us
    // against 52).  PRG_SPLIT_W512=0: never; =2: every shape it covers (tests).
    if (sw.split_w512 && d.Cout % 128 == 0 && W % 16 == 0 && H % 16 == 0 && !L.residual) {
      ConvChoice t;
      set_tiles(&t, kConvSplitW512, 16, 16, 128, H, W, d.Cout, d.B);
      const int slabs = t.tiles_x * t.tiles_y * 4;
      const int f = wave_rows_fuse(L, slabs);
      if ((sw.split_w512 == 2 || t.grid >= num_cus) && (f || !want_stats)) {
        *c = t;
        c->pro = L.pro_a ? 1 : 0;
        set_stats(c, f, slabs);
        return true;
      }
    }
    // Cout % 128 == 0: the wave-specialised kernel (128-pixel x 128-channel tiles, one workgroup per CU)
    if (d.Cout % 128 == 0 && W % 16 == 0 && H % 8 == 0 && !L.residual) {
      const int tiles = (W / 16) * (H / 8) * 2;
      const int f = wave_rows_fuse(L, tiles);
      if (f || !want_stats) {
        set_tiles(c, kConvSplitWs, 8, 16, 128, H, W, d.Cout, d.B);
        set_stats(c, f, tiles);
        return true;
      }
    }
    // Cout = 64 and a launch that fills the chip (>= one 16 x 16 tile per CU): the persistent kernel; PRG_SPLIT_P64=0: never,
    // PRG_SPLIT_P64=<n>: from n tiles (tests force it at small shapes)
    if (sw.split_p64 > 0 && d.Cout == 64 && W % 16 == 0 && H % 16 == 0 && !L.residual && !L.res_a && d.B * (W / 16) * (H / 16) >= sw.split_p64 &&
        (d.C0 + d.C1) >= 64) {
      const int tiles = (W / 16) * (H / 16) * 4;
      const int f = wave_rows_fuse(L, tiles);
      if (f || !want_stats) {
        set_tiles(c, kConvSplitP64, 16, 16, 64, H, W, 64, d.B);
        c->tiles_n = c->grid;                                // persistent: the kernel is told how many tiles there are in all
        if (c->grid > num_cus) c->grid = num_cus;            // (grid <= 0: no device properties, the launcher's error)
        if (c->grid >= 8) c->grid &= ~7;                     // multiple of 8: XCD-contiguous tile runs
        set_stats(c, f, tiles);
        return true;
      }
    }
    if ((W % 16 == 0 && H % 8 == 0) || (W % 32 == 0 && H % 4 == 0)) {
      const bool t8 = W % 16 == 0 && H % 8 == 0;
      set_tiles(c, kConvSplitHalo, t8 ? 8 : 4, t8 ? 16 : 32, 64, H, W, d.Cout, d.B);
      set_stats(c, tile_fuse(L, 64, c->tiles_x * c->tiles_y), c->tiles_x * c->tiles_y);
      return true;
    }
  }
  if (L.pro_a) return false;                   // (a fused prologue is only requested where pick_halo = the test above holds)
  c->family = kConvSplitIgemm;
  igemm_tiles(L, M, 128, d.CoutPad % 128 == 0 ? 128 : 64, true, c);
  return true;
}

static ConvChoice none(const char* why) {
  ConvChoice c;
  c.why = why;
  return c;
}

}  // namespace

ConvChoice choose_conv(const ConvFacts& L, int num_cus, const ConvSwitches& sw) {
  const ConvDesc& d = L.d;
  ConvChoice c;
  if (!L.f32) {
    if (choose_mx(L, num_cus, sw, &c)) return c;
    // persistent kernels of the bf16 throughput path
    if (choose_c64(L, num_cus, sw, &c)) return c;
    if (d.ups && !L.gn_partials && choose_up_w256(L, num_cus, sw, &c)) return c;
    if (choose_w256(L, false, num_cus, sw, &c)) return c;
    if (choose_ws(L, num_cus, sw, &c)) return c;
    if (!L.gn_partials && choose_down_w256(L, num_cus, sw, &c)) return c;
    // the generic kernels below read coefficient tables
    c = ConvChoice();
    c.fill_tables = L.pro_fold_acc;
  }
  if (L.out_f16 || L.in_f16) return none("conv: no kernel with the f16 format takes this launch");
  if (L.f32 && choose_split(L, num_cus, sw, &c)) return c;
  if (L.f32) c = ConvChoice();
  if (pick_halo(d, L.f32, &c)) {
    halo_tiles(L, kConvHalo, &c);
    return c;
  }
  if (L.pro_a) return none("conv: fused prologue requested on a shape the halo kernel does not cover");
  const int M = (int)((int64_t)d.B * d.Hout * d.Wout);
  const bool wide = d.Cout % 8 == 0;
  c.family = kConvIgemm;
  // 256 x 128 tiles (round 5): the 1x1 res_convs / projections of the coarse levels are bound by L2 -> LDS operand traffic
  // (M N K (1 / BM + 1 / BN) elements: 0.75x of the 128 x 128 tile's) and meet one barrier per 16 instead of 8 MFMAs per wave;
  // taken when the launch still has two workgroups per CU.
  if (!L.f32 && d.CoutPad % 128 == 0 && M % 256 == 0 && (int64_t)(M / 256) * (d.CoutPad / 128) >= (int64_t)2 * 256) igemm_tiles(L, M, 256, 128, wide, &c);
  else if (d.CoutPad % 128 == 0) igemm_tiles(L, M, 128, 128, wide, &c);
  else if (M >= 256 * 64) igemm_tiles(L, M, 256, 64, wide, &c);
  else igemm_tiles(L, M, 128, 64, wide, &c);
  return c;
}

bool choose_h16_pair(const ConvFacts& c1, const ConvFacts& c2, int num_cus, const ConvSwitches& sw) {
  if (!sw.h16) return false;                                 // PRG_H16=0: off (every ResnetBlock keeps its bf16 h1)
  // mxfp8 handles: a conv whose MX copy would run (the 256-pixel MX kernel takes Cout % 128 == 0; PRG_MX_PURE / mx_pure take every
  // 3x3 conv) never carries the f16 format — the 64-channel pairs, which the bf16 kernels run in that mode too, do
  auto mx_takes = [&](const ConvFacts& L) { return L.w_mx && (L.d.Cout % 128 == 0 || sw.mx_pure || L.mx_pure); };
  if (mx_takes(c1) || mx_takes(c2) || !c2.w_f16 || !c1.gn_acc || !c2.pro_fold_acc) return false;
  ConvFacts L1 = c1, L2 = c2;
  L1.out_f16 = 1;
  L2.in_f16 = 1;
  const ConvChoice r1 = choose_conv(L1, num_cus, sw);
  if (r1.family == kConvNone || !r1.acc_done) return false;
  return choose_conv(L2, num_cus, sw).family != kConvNone;
}

bool choose_supports_prologue(const ConvDesc& d, int f32) {
  if (d.C1 != 0) return false;
  ConvFacts L{};
  L.d = d;
  L.f32 = f32;
  L.bias = L.pro_a = 1;
  return choose_conv(L, 0, ConvSwitches()).family != kConvNone;
}

}  // namespace prg
