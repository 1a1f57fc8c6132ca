// conv_choose.h — which kernel runs a convolution: one pure function of plain values (conv_choose.cpp, host-only C++ without HIP
// headers, so it is tested and sanitised on the CPU).  launch_conv (conv.hip) asks it once and hands the answer to the chosen
// family's launcher; conv_h16_pair_ok and conv_supports_prologue are calls of the same function.
#pragma once

namespace prg {

constexpr int kGnMaxSplit = 1024;  // max GroupNorm (sum, sumsq) partial slabs per image (256x256: 8x32 tiles x 4 wave rows)

struct ConvDesc {
  int B, Hin, Win;          // source tensors' spatial size (before the optional x2 nearest upsample)
  int C0, C1;               // channels of src0 / src1 (virtual concat [src0, src1]); C1 = 0 when unused
  int ups;                  // 1: conv runs on the 2x nearest-upsampled image (Upsample, sd:592-594)
  int KH, KW, stride, pad;
  int Hout, Wout;
  int Cout, CoutPad;        // CoutPad = Cout rounded up to 64: packed weight rows (zeros beyond Cout)
  int kchunks;              // ceil((C0+C1) / BK)
};

// What the selection reads of a ConvLaunch<T> (conv.h: conv_facts): the descriptor, the storage type and which options are set.
struct ConvFacts {
  ConvDesc d;
  int f32;                  // storage type: 1 = float (handles of dtype PRG_F32 / PRG_F16X3), 0 = bf16 (PRG_BF16 / PRG_MXFP8)
  // present (non-null) pointers of the launch; w_mx stands for w_mx AND w_mx_scale
  int bias, residual, res_a, pro_a, gn_partials, gn_acc, w_mx, w_s2d, w_up, w_split, w_up_split, w_f16;
  int res_fold_acc;         // res_fold.acc present
  int gn_groups;
  int pro_fold_acc, pro_fold_pq, pro_fold_G, pro_fold_cpg;   // pro_fold: acc present, P and Q present, G, cpg
  int in_f16, out_f16, mx_pure;
};

// The PRG_* switches of the selection; conv_switches() in conv.hip reads them from the environment, once.
struct ConvSwitches {
  int conv_ws = 1;          // PRG_CONV_WS
  int conv_c64 = 1;         // PRG_CONV_C64
  int conv_w256 = 1;        // PRG_CONV_W256
  int conv_down_w256 = 1;   // PRG_CONV_DOWN_W256
  int conv_w256mx = 1;      // PRG_CONV_W256MX
  int w256_min_tiles = 0;   // PRG_W256_MIN_TILES
  int up2x2 = 1;            // PRG_UP2X2
  int h16 = 1;              // PRG_H16
  int mx_pure = 0;          // PRG_MX_PURE
  int split_up2x2 = 0;      // PRG_SPLIT_UP2X2
  int split_p64 = 256;      // PRG_SPLIT_P64
  int split_w512 = 1;       // PRG_SPLIT_W512
};

enum ConvFamily {
  kConvNone = 0,            // no kernel implements the request (ConvChoice::why says which)
  kConvIgemm,               // conv.hip: conv_igemm_kernel<T, bm, bn, mode = 1x1>
  kConvHalo,                // conv.hip: conv3x3_halo_kernel<T, th, tw, bn>
  kConvMxHalo,              // conv.hip: conv3x3_mx_kernel<th, tw, bn>
  kConvC64,                 // conv_c64.hip: conv3x3_c64_kernel<pro, mode = f16 output>
  kConvWs,                  // conv_ws.hip: conv3x3_ws_kernel<th, tw, bn, pro>
  kConvW256,                // conv_w256.hip: conv3x3_w256_kernel<tw, pro, mode> (mode 0: 3x3, 1: Downsample, 2: sub-pixel Upsample)
  kConvW256Mx,              // conv_w256.hip: conv3x3_w256mx_kernel<tw, pro>
  kConvSplitHalo,           // conv_split.hip: conv3x3_split_kernel<th, tw>
  kConvSplitWs,             // conv_split.hip: conv3x3_split_ws_kernel<mode = sub-pixel Upsample>
  kConvSplitP64,            // conv_split.hip: conv3x3_split_p64_kernel
  kConvSplitW512,           // conv_split512.hip: conv3x3_split_w512_kernel<pro>
  kConvSplitIgemm,          // conv_split.hip: conv_igemm_split_kernel<bm, bn, mode = 1x1>
};

struct ConvChoice {
  int family = kConvNone;
  int th = 0, tw = 0, bm = 0, bn = 0;   // tile of the instantiation (the family's comment above says which it has)
  int pro = 0;                          // prologue form: 0 none, 1 coefficient tables, 2 in-kernel fold, 3 in-kernel fold of f16 input
  int mode = 0;
  int tiles_x = 0, tiles_y = 0, tiles_n = 0;   // the kernel's arguments (implicit GEMM: tiles_x = tiles_m); p64: tiles_n = all tiles
  int grid = 0;                         // workgroups
  int fuse_stats = 0;                   // the kernel writes GroupNorm statistics of its output
  int nsplit = 0;                       // slabs per image it writes (launch_conv's gn_nsplit_out)
  int acc_done = 0;                     // it adds them to gn_acc instead
  int fill_tables = 0;                  // launch_gn_coeff_acc fills pro_a / pro_b from pro_fold first (the kernel reads tables)
  int is_mx = 0;                        // MX-fp8 operands
  double exec_scale = 1.0;              // executed / algorithmic MACs: 4 / 9 for the sub-pixel Upsample form of conv_w256.hip
  const char* why = nullptr;            // kConvNone: the reason
};

// The order of preference is the body of this function.  num_cus <= 0 (no device properties): the persistent kernels are out.
ConvChoice choose_conv(const ConvFacts& f, int num_cus, const ConvSwitches& sw);

// true when conv1 (asked to store f16) and conv2 (asked to read f16 through its folded prologue) of a ResnetBlock both land on
// kernels that implement the h16 format (conv.h), conv1 with fixed-point statistics
bool choose_h16_pair(const ConvFacts& c1, const ConvFacts& c2, int num_cus, const ConvSwitches& sw);

// true when a single-source conv of this shape takes a fused input prologue
bool choose_supports_prologue(const ConvDesc& d, int f32);

}  // namespace prg
