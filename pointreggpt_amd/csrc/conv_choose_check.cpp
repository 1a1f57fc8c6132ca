// conv_choose_check.cpp — the conv selection under AddressSanitizer and UBSan (make sanitize): a stand-alone program on the CPU.
// It asks choose_conv, choose_h16_pair and choose_supports_prologue over a grid of shapes, options, CU counts and switch settings,
// the zero and negative sizes that prg_debug_conv_choice rejects among them, and prints one OK line.
#include <cstdio>
#include <initializer_list>

#include "conv_choose.h"

using namespace prg;

int main() {
  const int sizes[] = {-16, 0, 1, 8, 12, 16, 24, 32, 40, 64, 128, 256, 512};
  const int chans[] = {-64, 0, 8, 16, 60, 64, 128, 192, 256, 384, 512, 1024};
  const int batches[] = {-1, 0, 1, 2, 16, 64, 256, 257};
  const int cus[] = {-8, 0, 7, 8, 64, 256, 304};
  const int groups[] = {-8, 0, 1, 8, 16, 64};
  struct Kind { int K, stride, pad, ups; } kinds[] = {{3, 1, 1, 0}, {3, 1, 1, 1}, {4, 2, 1, 0}, {1, 1, 0, 0}, {0, 0, 0, 0}, {7, 1, 3, 0}};
  ConvSwitches settings[16];
  settings[1].conv_ws = 0; settings[2].conv_c64 = 0; settings[3].conv_w256 = 0; settings[4].conv_down_w256 = 0;
  settings[5].conv_w256mx = 0; settings[6].w256_min_tiles = 1; settings[7].up2x2 = 0; settings[8].h16 = 0; settings[9].mx_pure = 1;
  settings[10].split_up2x2 = 1; settings[11].split_p64 = 0; settings[12].split_p64 = 1; settings[13].split_w512 = 0;
  settings[14].split_w512 = 2;
  settings[15].conv_ws = settings[15].conv_c64 = settings[15].conv_w256 = settings[15].conv_down_w256 = 0;
  long asked = 0, families[16] = {0}, pairs = 0, prologues = 0;
  unsigned long long mix = 1;                               // which options are present: a different mask for every query
  for (const Kind& k : kinds)
    for (int S : sizes)
      for (int cin : chans)
        for (int cout : chans)
          for (int B : batches)
            for (int f32 = 0; f32 < 2; ++f32) {
              ConvFacts f{};
              ConvDesc& d = f.d;
              d.B = B; d.Hin = d.Win = S; d.ups = k.ups; d.KH = d.KW = k.K; d.stride = k.stride; d.pad = k.pad;
              const int Sl = k.ups ? 2 * S : S;
              d.Hout = d.Wout = k.stride > 0 ? (Sl + 2 * k.pad - k.K) / k.stride + 1 : 0;
              mix = mix * 6364136223846793005ull + 1442695040888963407ull;
              const unsigned m = (unsigned)(mix >> 32);
              d.C0 = (m & 1) ? cin : cin / 2; d.C1 = cin - d.C0;
              d.Cout = cout; d.CoutPad = (cout + 63) / 64 * 64; d.kchunks = (cin + (f32 ? 15 : 31)) / (f32 ? 16 : 32);
              f.f32 = f32;
              f.bias = m >> 1 & 1; f.residual = (m >> 2 & 7) == 0; f.res_a = (m >> 5 & 7) == 0; f.pro_a = m >> 8 & 1; f.gn_partials = m >> 9 & 1;
              f.gn_acc = m >> 10 & 1; f.w_mx = m >> 11 & 1; f.w_s2d = m >> 12 & 1; f.w_up = m >> 13 & 1; f.w_split = m >> 14 & 1;
              f.w_up_split = m >> 15 & 1; f.w_f16 = m >> 16 & 1; f.res_fold_acc = (m >> 17 & 7) == 0; f.pro_fold_acc = m >> 20 & 1;
              f.pro_fold_pq = m >> 21 & 1; f.in_f16 = (m >> 22 & 3) == 0; f.out_f16 = (m >> 24 & 3) == 0; f.mx_pure = (m >> 26 & 3) == 0;
              f.gn_groups = groups[m % 6];
              f.pro_fold_G = groups[(m >> 3) % 6]; f.pro_fold_cpg = f.pro_fold_G > 0 ? d.C0 / f.pro_fold_G : (int)(m % 9) - 1;
              const ConvSwitches& sw = settings[(m >> 4) % 16];
              const int n = cus[(m >> 7) % 7];
              const ConvChoice c = choose_conv(f, n, sw);
              if (c.family < 0 || c.family > kConvSplitIgemm || (c.family == kConvNone) != (c.why != nullptr)) {
                std::printf("conv_choose_check: bad family %d\n", c.family);
                return 1;
              }
              families[c.family] += 1;
              ConvFacts f2 = f;
              f2.d.C0 = cout; f2.d.C1 = 0;
              pairs += choose_h16_pair(f, f2, n, sw);
              prologues += choose_supports_prologue(d, f32);
              asked += 1;
            }
  // the ResnetBlock pairs of the bf16 networks as the forward pass asks for them
  for (int S : {32, 64, 128})
    for (int C : {64, 128, 256})
      for (int B : {2, 16})
        for (int n : cus)
          for (const ConvSwitches& sw : settings) {
            ConvFacts c1{};
            c1.d = ConvDesc{B, S, S, C, 0, 0, 3, 3, 1, 1, S, S, C, C, C / 32};
            c1.bias = c1.gn_partials = c1.gn_acc = 1;
            c1.gn_groups = 8;
            ConvFacts c2 = c1;
            c2.pro_a = c2.pro_fold_acc = c2.pro_fold_pq = c2.w_f16 = 1;
            c2.pro_fold_G = 8; c2.pro_fold_cpg = C / 8;
            pairs += choose_h16_pair(c1, c2, n, sw);
          }
  if (!pairs) {
    std::printf("conv_choose_check: no ResnetBlock pair took the f16 format\n");
    return 1;
  }
  for (int fam = kConvNone; fam <= kConvSplitIgemm; ++fam)
    if (!families[fam]) {
      std::printf("conv_choose_check: family %d was never chosen\n", fam);
      return 1;
    }
  std::printf("conv_choose_check OK (%ld queries, %ld h16 pairs, %ld shapes with a prologue)\n", asked, pairs, prologues);
  return 0;
}
