// conv_split_common.h — device code shared by the f16x3 convolution kernels (conv_split.hip, conv_split512.hip): the on-the-fly
// hi / lo split of eight float32 channels, the three-product MFMA sequence and its flush, the scheduling pipeline that interleaves
// a consumer's fragment reads with its MFMAs, and what the four 3x3 halo kernels (conv3x3_split_kernel, _ws_, _p64_, _w512_) have
// in common: halo geometry, halo staging, weight-tile LDS-DMA, the consumers' fragment reads.  A piece is shared only where the
// gfx950 listing of the kernel stays what it was with the piece written out (profiles/split_ops_refactor_ab.txt, which also lists
// what therefore stays written out in the kernels: tile decode, fragment lane offsets, the producer and consumer wave loops and
// the statistics half of the direct epilogue).
#pragma once
#include "conv_epi.h"

namespace prg {

typedef h16x2 f16x2;   // (f16x8, f32x2: wave_ops.h, through conv_epi.h)

// 8 consecutive channels -> their hi and lo halves as two 16-byte MFMA operand units
template <bool MIX = true>
__device__ inline void split8(const float (&v)[8], uint4& hi, uint4& lo) {
  f16x8 h, l;
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const f32x2 p = {v[i], v[i + 1]};
    const f16x2 ph = __builtin_convertvector(p, f16x2);          // v_cvt_pk_f16_f32, round to nearest even
    // v - hi, exact in float32.  MIX (round 5): ONE mixed-precision fma per element — v_fma_mix_f32 reads the f16 half directly —
    // instead of a conversion back to float32 and a (packed, two-slot) subtraction: 16 instead of 24 issue slots per eight elements,
    // the same bits.  hipcc folds fma(float(h), -1, v) back into convert + subtract, hence two lines of inline asm (op_sel picks the
    // half).  Same-box A/B (profiles/r05_ab_split8_fma_mix.txt): the persistent 64-channel kernel 248-255 -> 229 us per level-0
    // launch (K = 1152: 460-470 -> 424); the launches with a fused GroupNorm + SiLU prologue got 3-4 % SLOWER with it (the asm
    // statements pin the schedule around the two transcendentals), so those keep the plain form (split8<false>).
    f32x2 r;
    if constexpr (MIX) {
      const uint32_t phw = __builtin_bit_cast(uint32_t, ph);
      asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r[0]) : "v"(phw), "v"(p[0]));
      asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r[1]) : "v"(phw), "v"(p[1]));
    } else {
      r = p - __builtin_convertvector(ph, f32x2);
    }
    const f16x2 pl = __builtin_convertvector(r, f16x2);
    h[i] = ph[0]; h[i + 1] = ph[1];
    l[i] = pl[0]; l[i + 1] = pl[1];
  }
  hi = __builtin_bit_cast(uint4, h);
  lo = __builtin_bit_cast(uint4, l);
}

__device__ inline f16x8 ld_frag(const uint4* p) { return __builtin_bit_cast(f16x8, *p); }

// scheduling pipeline of one k16 step of a consumer wave: (MFMA, ds_read) x 8, then 4 MFMAs  (sched_group_barrier masks: 0x008 = MFMA,
// 0x100 = DS read); placed behind the twelve MFMAs and the eight fragment reads of the OTHER register set it orders
__device__ inline void interleave_8_reads_12_mfmas() {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
  __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
}

template <int N>
struct IC {
  static constexpr int value = N;
};

// f(IC<0>()), f(IC<1>()), ... f(IC<N - 1>()): a loop whose index is a compile-time constant in the body
template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(IC<I>());
    static_for<N, I + 1>(f);
  }
}

// two consecutive channels -> packed hi and lo halves (one pair of split8: the same instructions, the same bits)
template <bool MIX>
__device__ inline void split2(float v0, float v1, uint32_t& hi, uint32_t& lo) {
  const f32x2 p = {v0, v1};
  const f16x2 ph = __builtin_convertvector(p, f16x2);
  f32x2 r;
  if constexpr (MIX) {
    const uint32_t phw = __builtin_bit_cast(uint32_t, ph);
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r[0]) : "v"(phw), "v"(p[0]));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r[1]) : "v"(phw), "v"(p[1]));
  } else {
    r = p - __builtin_convertvector(ph, f32x2);
  }
  const f16x2 pl = __builtin_convertvector(r, f16x2);
  hi = __builtin_bit_cast(uint32_t, ph);
  lo = __builtin_bit_cast(uint32_t, pl);
}

// ---------------------------------------------------------------------------------------------
// the three-product contraction
// ---------------------------------------------------------------------------------------------
// acc += a * w with split operands over TM x 2 MFMA tiles of one k16 step.  fa = (hi, lo) per row tile, fw = (hi, lo) per column
// tile.  Term-major, so that back-to-back MFMAs never wait on the same accumulator; the two cross terms first (small), then hi * hi
template <int TM>
__device__ inline void mfma3(const f16x8 (&fa)[2 * TM], const f16x8 (&fw)[4], f32x16 (&acc)[TM][2]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[2 * i + 1], fw[2 * j], acc[i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[2 * i], fw[2 * j + 1], acc[i][j], 0, 0, 0);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[2 * i], fw[2 * j], acc[i][j], 0, 0, 0);
}

// the partial of one accumulation chain (288 terms in the halo kernels, 256 in the gather kernel) joins the total.  `first`: a tile's
// first partial is assigned, not added to a zeroed total (0 + x = x).  CLEAR = false: the next chain starts from the MFMA's constant 0
template <int TM, bool CLEAR = true>
__device__ inline void flush_acc(f32x16 (&acc)[TM][2], f32x16 (&tot)[TM][2], bool first = false) {
  if (first) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) { tot[i][j][e] = acc[i][j][e]; acc[i][j][e] = 0.0f; }
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          tot[i][j][e] += acc[i][j][e];
          if constexpr (CLEAR) acc[i][j][e] = 0.0f;
        }
  }
}

// ---------------------------------------------------------------------------------------------
// 3x3 halo kernels: geometry
// ---------------------------------------------------------------------------------------------
// A TH x TW pixel tile with its one-pixel frame in LDS: 144-byte pixels (HaloGeom, wave_ops.h: conflict-free ds_read_b128 without
// an XOR swizzle) of one 32-channel chunk, units 0-3 the hi halves, 4-7 the lo halves.  NPT threads stage it, four per pixel (eight
// channels each), NH passes per chunk.
template <int TH, int TW, int NPT = 256>
struct SplitGeom : HaloGeom<TH, TW, NPT> {
  using H = HaloGeom<TH, TW, NPT>;
  static constexpr int PITCH = H::ROWB;
  // halo ROW stride: a multiple of 256 bytes (16 slots).  A 16-wide tile puts lanes 16-31 of a fragment load one halo row below
  // lanes 0-15; with the natural stride (18 x 144 B = 2 slots mod 16) two lanes of every ds_read_b128 lane group met on a bank
  // (SQ_LDS_BANK_CONFLICT above SQ_ACTIVE_INST_LDS); with a stride of 0 mod 16 slots the two half rows interleave exactly.
  static constexpr int RSTRIDE = (H::HP * PITCH + 255) / 256 * 256;
  static constexpr int HBYTES = (TH + 2) * RSTRIDE;              // one halo image; the kernels double-buffer it
  static constexpr int NH = (H::HALO * 4 + NPT - 1) / NPT;       // staging passes per chunk (NPT / 4 halo pixels each)
  static constexpr int at(int row, int col) { return row * RSTRIDE + col * PITCH; }   // byte offset of a halo position
  static constexpr int tap(int T) { return at(T / 3, T % 3); }                        // window of tap T of the 3 x 3 ...
  static constexpr int tap_up(int T) { return at(T / 2, T % 2); }                     // ... and of the 2 x 2 sub-pixel form (UP)
};

// ---------------------------------------------------------------------------------------------
// 3x3 halo kernels: halo staging
// ---------------------------------------------------------------------------------------------
// source pixel index of position (y, x) of the H x W image that the tiles cover, or -1: padding.  ups: the source is half that size
__device__ inline int halo_source(const ConvDesc& d, int b, int y, int x, int H, int W, bool ups) {
  int s = -1;
  if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
    if (ups) { y >>= 1; x >>= 1; }
    s = (b * d.Hin + y) * d.Win + x;
  }
  return s;
}

// which source tensor holds channel c of the concatenated input, its channel count and the channel's index in it
struct ChunkSrc {
  const float* base;
  int Cs, cc;
};
__device__ inline ChunkSrc chunk_source(const ConvLaunch<float>& L, int c) {
  const bool first = c < L.d.C0;
  return {first ? L.src0 : L.src1, first ? L.d.C0 : L.d.C1, first ? c : c - L.d.C0};
}
// eight channels of one halo pixel.  Always issued (padding lanes read the tensor's first bytes and are zeroed when written): the
// counted vmcnt waits need a fixed number of loads
__device__ inline void load_unit(const ChunkSrc& s, int hsrc, float4& g0, float4& g1) {
  const float4* p = reinterpret_cast<const float4*>(s.base + (hsrc >= 0 ? (size_t)hsrc * s.Cs + s.cc : (size_t)0));
  g0 = p[0];
  g1 = p[1];
}
// fused prologue coefficients of eight channels: a, b point at the first of them in the image's rows of L.pro_a, L.pro_b
__device__ inline void load_pro8(const float* a, const float* b, float (&pa)[8], float (&pb)[8]) {
  const float4* a4 = reinterpret_cast<const float4*>(a);
  const float4* b4 = reinterpret_cast<const float4*>(b);
  const float4 a0 = a4[0], a1 = a4[1], b0 = b4[0], b1 = b4[1];
  pa[0] = a0.x; pa[1] = a0.y; pa[2] = a0.z; pa[3] = a0.w; pa[4] = a1.x; pa[5] = a1.y; pa[6] = a1.z; pa[7] = a1.w;
  pb[0] = b0.x; pb[1] = b0.y; pb[2] = b0.z; pb[3] = b0.w; pb[4] = b1.x; pb[5] = b1.y; pb[6] = b1.z; pb[7] = b1.w;
}
// finishes one staged unit: the optional GroupNorm + SiLU prologue, zero if padding, hi / lo split, two 16-byte LDS writes
__device__ inline void finish_unit(float4 h0, float4 h1, bool pro, const float (&pa)[8], const float (&pb)[8],
                                            bool padding, char* p) {
  float v[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
  if (pro) {
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = fast_silu(fmaf(v[u], pa[u], pb[u]));
  }
  if (padding) {
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = 0.0f;
  }
  uint4 vh, vl;
  if (pro) split8<false>(v, vh, vl);
  else split8(v, vh, vl);
  *reinterpret_cast<uint4*>(p) = vh;
  *reinterpret_cast<uint4*>(p + 64) = vl;
}

// ---------------------------------------------------------------------------------------------
// 3x3 halo kernels: weight tiles
// ---------------------------------------------------------------------------------------------
// Weight tiles go global -> LDS directly (global_load_lds_dwordx4).  The LDS destination of such a wave-instruction is lane-linear
// (base + lane * 16 = eight 128-byte rows), so the XOR swizzle the fragment reads apply sits on the per-lane SOURCE address: LDS
// unit p of row n holds source unit p ^ ((n >> 1) & 7): a lane's source offset is swizzled_unit(its row, lane & 7).
__device__ inline int swizzled_unit(int row, int unit) { return row * 128 + ((unit ^ ((row >> 1) & 7)) << 4); }
__device__ inline void weight_dma_rows(const char* src, char* dst) {   // eight rows: one wave-instruction
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
template <int WPW>
__device__ inline void weight_dma(const char* tile, const int (&wsrc)[WPW], char* dst) {   // this wave's rows of one tile
#pragma unroll
  for (int r = 0; r < WPW; ++r) weight_dma_rows(tile + wsrc[r], dst + r * 1024);
}

// ---------------------------------------------------------------------------------------------
// 3x3 halo kernels: consumers
// ---------------------------------------------------------------------------------------------
// fragments of one k16 step of a 64-pixel x 64-channel consumer wave: A = halo image + tap window + step, Bb = ring slot
__device__ inline void consumer_reads(const char* A, const char* Bb, const int (&a_lane)[2], const int (&b_lane)[2],
                                               f16x8 (&fa)[4], f16x8 (&fw)[4]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    fa[2 * i] = ld_frag(reinterpret_cast<const uint4*>(A + a_lane[i]));
    fa[2 * i + 1] = ld_frag(reinterpret_cast<const uint4*>(A + a_lane[i] + 64));
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    fw[2 * j] = ld_frag(reinterpret_cast<const uint4*>(Bb + b_lane[0] + j * 4096));
    fw[2 * j + 1] = ld_frag(reinterpret_cast<const uint4*>(Bb + b_lane[1] + j * 4096));
  }
}
}  // namespace prg
