// wave_ops.h — device code that the MFMA kernels share (gfx950, wave = 64): the register vector types, bf16 / f16 packing, lane
// exchanges, the LDS-only barrier, the deterministic wave reductions of the GroupNorm partial sums, the paired 16-byte epilogue
// store, and the fused GroupNorm + SiLU prologue of one halo unit with its coefficients.  Everything is inlined: a kernel that
// calls these compiles to the instructions it had when it carried its own copy.
#pragma once
#include "common.h"

namespace prg {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) _Float16 h16x2;

// ---------------------------------------------------------------------------------------------
// packed bf16 / f16 words
// ---------------------------------------------------------------------------------------------
__device__ inline float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ inline float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
__device__ inline uint32_t pack_bf16(float a, float b) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  bf16x2 v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}
// two floats -> packed f16 (v_cvt_pk_f16_f32, round to nearest even); as a word: the h16 output format (conv.h)
__device__ inline h16x2 h16_pair(float a, float b) { return __builtin_convertvector((f32x2){a, b}, h16x2); }
__device__ inline uint32_t h16_pack(float a, float b) { return __builtin_bit_cast(uint32_t, h16_pair(a, b)); }

// ---------------------------------------------------------------------------------------------
// lane exchanges inside a wave without the LDS crossbar's address VGPR, and the barrier
// ---------------------------------------------------------------------------------------------
template <int CTRL>   // DPP quad permute
__device__ inline float dpp_f32(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int XOR>   // ds_swizzle: partner = lane ^ XOR, XOR < 32
__device__ inline float swz_xor(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), (XOR << 10) | 0x1F));
}
template <int BIT>   // partner = lane ^ (1 << BIT), by the cheapest exchange that reaches it
__device__ inline float lane_xor(float v) {
  if constexpr (BIT == 0) return dpp_f32<0xB1>(v);
  else if constexpr (BIT == 1) return dpp_f32<0x4E>(v);
  else if constexpr (BIT < 5) return swz_xor<(1 << BIT)>(v);
  else return __shfl_xor(v, 32, 64);
}

// Workgroup barrier that never waits for VMEM (loads and stores stay in flight across it).  LDS_DONE: this wave's own LDS
// operations are complete first — writers always must; a reader whose every LDS read has been consumed by an MFMA need not.
template <bool LDS_DONE = true>
__device__ __forceinline__ void lds_barrier() {
  if constexpr (LDS_DONE) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---------------------------------------------------------------------------------------------
// wave reductions of N = 16 or 8 values per lane (the GroupNorm partial sums of a tile: [sum | sumsq][chunk])
// ---------------------------------------------------------------------------------------------
// N full-wave sums with N + 1 lane exchanges: each butterfly round halves the values a lane carries (it keeps the half its
// lane bit selects and sends the other half to its partner); once one value is left the remaining lane bits are plain xor
// adds.  Fixed order: deterministic.  Afterwards lane l < N holds the total of value wave_sums_index<N>(l).
// Unrolled for N = 16: 8 values by lane bit 0, 4 by bit 1, 2 by bit 2, 1 by bit 3, then the xor adds of bits 4 and 5 — the
// text that w2_tile_stats (conv_w256.hip) carries written out.
template <int N, int BIT = 0>
__device__ inline float wave_sums(const float (&V)[N], int lane) {
  if constexpr (N == 1) {
    static_assert(BIT == 3 || BIT == 4, "called with N = 8 or 16 values");
    float D = V[0];
    if constexpr (BIT == 3) D += lane_xor<3>(D);
    D += lane_xor<4>(D);
    D += lane_xor<5>(D);
    return D;
  } else {
    const bool up = lane & (1 << BIT);
    float H[N / 2];
#pragma unroll
    for (int j = 0; j < N / 2; ++j) H[j] = (up ? V[N / 2 + j] : V[j]) + lane_xor<BIT>(up ? V[j] : V[N / 2 + j]);
    return wave_sums<N / 2, BIT + 1>(H, lane);
  }
}
// the value whose total lane l < N holds: lane bit k is bit log2(N) - 1 - k of the index
template <int N>
__device__ inline int wave_sums_index(int lane) {
  static_assert(N == 16 || N == 8, "two butterfly depths are in use");
  if constexpr (N == 16) return (lane & 1) * 8 + (lane & 2) * 2 + ((lane >> 2) & 1) * 2 + ((lane >> 3) & 1);
  else return (lane & 1) * 4 + (lane & 2) + ((lane >> 2) & 1);
}
// Values are [sum | sumsq][8-channel chunk]: folds the `per` (a power of two, at most N / 2) neighbouring chunks of one GroupNorm
// group, after which the lane of the group's FIRST chunk — (index & (N / 2 - 1) & (per - 1)) == 0 — holds the group's total.
template <int N>
__device__ inline float group_sums(float D, int per) {
  constexpr int LOG = N == 16 ? 4 : 3;
  if (per >= 2) D += lane_xor<LOG - 1>(D);
  if (per >= 4) D += lane_xor<LOG - 2>(D);
  if (N == 16 && per >= 8) D += lane_xor<1>(D);
  return D;
}

// ---------------------------------------------------------------------------------------------
// epilogue store: an MFMA 32x32 accumulator leaves lanes l and l + 32 with the two channel quads (packed: two words) of the same
// pixel and 8-channel chunk.  p0 p1 = this lane's words of chunk 2m, p2 p3 = of chunk 2m + 1: swapping the upper half of chunk 2m
// with the lower half of chunk 2m + 1 (one lane-half swap per word) leaves lane half 0 with all 8 channels of chunk 2m and half 1
// with those of chunk 2m + 1 — one 16-byte store each, at byte offset 16 * half from the address of chunk 2m.
// ---------------------------------------------------------------------------------------------
__device__ inline u32x4 pair_chunks(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  const auto s0 = __builtin_amdgcn_permlane32_swap(p0, p2, false, false);
  const auto s1 = __builtin_amdgcn_permlane32_swap(p1, p3, false, false);
  return u32x4{(uint32_t)s0[0], (uint32_t)s1[0], (uint32_t)s0[1], (uint32_t)s1[1]};
}

// ---------------------------------------------------------------------------------------------
// fused prologue of a halo: y = SiLU(x * A[c] + B[c]) on one 16-byte unit (8 channels of one pixel); the coefficients of the
// unit's channels as c[4] = {A0..3, A4..7, B0..3, B4..7}
// ---------------------------------------------------------------------------------------------
__device__ inline u32x4 silu_affine8(u32x4 v, const float (&a8)[8], const float (&b8)[8]) {   // bf16 channels
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float lo = fast_silu(fmaf(bf_lo(v[j]), a8[2 * j], b8[2 * j]));
    const float hh = fast_silu(fmaf(bf_hi(v[j]), a8[2 * j + 1], b8[2 * j + 1]));
    v[j] = pack_bf16(lo, hh);
  }
  return v;
}
// The same on four packed f16 channel pairs (the h16 input format).  Per pair: v_pk_fma_f16, v_pk_mul_f16, two v_exp_f16 (the
// second writes the upper half of the same register through SDWA: no repack), v_pk_add_f16, two v_rcp_f16, v_pk_mul_f16 — eight
// instructions against fourteen on the bf16 / float32 path.  exp2 overflow (y < -11) ends in rcp(inf) = 0 = SiLU's limit.  The
// transcendentals are inline asm (hipcc repacks with v_pack_b32_f16 otherwise), which hides them from the hazard recogniser:
// gfx950 needs one wait state between a transcendental / a dst_sel write and a VALU consumer of its result (LLVM:
// hasTransForwardingHazard, hasDstSelForwardingHazard) — the trailing s_nop of each block.
#define PRG_H16_TRANS4(OP)                                                                                             \
  asm(OP "_e32 %0, %4\n\t" OP "_e32 %1, %5\n\t" OP "_e32 %2, %6\n\t" OP "_e32 %3, %7\n\t"                            \
      OP "_sdwa %0, %4 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"                                  \
      OP "_sdwa %1, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"                                  \
      OP "_sdwa %2, %6 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\t"                                  \
      OP "_sdwa %3, %7 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_1\n\ts_nop 0"                           \
      : "=&v"(o0), "=&v"(o1), "=&v"(o2), "=&v"(o3)                                                                      \
      : "v"(i0), "v"(i1), "v"(i2), "v"(i3))
__device__ inline u32x4 h16_silu8(u32x4 x, const h16x2 (&a)[4], const h16x2 (&b)[4]) {
  const h16x2 nl2e = {(_Float16)-1.4426950408889634f, (_Float16)-1.4426950408889634f}, one = {(_Float16)1.0f, (_Float16)1.0f};
  h16x2 y[4];
  uint32_t i0, i1, i2, i3, o0, o1, o2, o3;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t w = x[j];   // (hipcc 7.2: __builtin_bit_cast of the vector ELEMENT x[j] reads element 0 for every j)
    y[j] = __builtin_elementwise_fma(__builtin_bit_cast(h16x2, w), a[j], b[j]);
  }
  i0 = __builtin_bit_cast(uint32_t, y[0] * nl2e); i1 = __builtin_bit_cast(uint32_t, y[1] * nl2e);
  i2 = __builtin_bit_cast(uint32_t, y[2] * nl2e); i3 = __builtin_bit_cast(uint32_t, y[3] * nl2e);
  PRG_H16_TRANS4("v_exp_f16");
  i0 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, o0) + one); i1 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, o1) + one);
  i2 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, o2) + one); i3 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(h16x2, o3) + one);
  PRG_H16_TRANS4("v_rcp_f16");
  u32x4 r;
  r[0] = __builtin_bit_cast(uint32_t, y[0] * __builtin_bit_cast(h16x2, o0));
  r[1] = __builtin_bit_cast(uint32_t, y[1] * __builtin_bit_cast(h16x2, o1));
  r[2] = __builtin_bit_cast(uint32_t, y[2] * __builtin_bit_cast(h16x2, o2));
  r[3] = __builtin_bit_cast(uint32_t, y[3] * __builtin_bit_cast(h16x2, o3));
  return r;
}
#undef PRG_H16_TRANS4

// The coefficients of 8 channels (16-byte aligned) from the tables A / B, or the P / Q of an in-kernel fold (common.h, GnFold) with
// the fixed-point statistics of the channels' group (8 | cpg): fold_coeffs turns those into A = rstd P, B = Q - mean A.
__device__ inline void load_coeffs(float4* c, const float* a, const float* b) {
  c[0] = *reinterpret_cast<const float4*>(a);
  c[1] = *reinterpret_cast<const float4*>(a + 4);
  c[2] = *reinterpret_cast<const float4*>(b);
  c[3] = *reinterpret_cast<const float4*>(b + 4);
}
__device__ inline const longlong2* group_stats(const GnFold& f, int img, int c0) {
  return reinterpret_cast<const longlong2*>(f.acc + ((size_t)img * f.G + c0 / f.cpg) * 2);
}
__device__ inline void fold_coeffs(float4* c, const float4* pq, longlong2 stats, float inv_n) {   // (c may be pq)
  float mean, rstd;
  gn_fold_stats_raw(stats.x, stats.y, inv_n, mean, rstd);
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    c[h2] = make_float4(rstd * pq[h2].x, rstd * pq[h2].y, rstd * pq[h2].z, rstd * pq[h2].w);
    c[2 + h2] = make_float4(fmaf(-mean, c[h2].x, pq[2 + h2].x), fmaf(-mean, c[h2].y, pq[2 + h2].y),
                            fmaf(-mean, c[h2].z, pq[2 + h2].z), fmaf(-mean, c[h2].w, pq[2 + h2].w));
  }
}
// the coefficients as packed f16 channel pairs, for h16_silu8
__device__ inline void pack_coeffs_h16(const float4* c, h16x2 (&a)[4], h16x2 (&b)[4]) {
#pragma unroll
  for (int h2 = 0; h2 < 2; ++h2) {
    a[2 * h2] = h16_pair(c[h2].x, c[h2].y);
    a[2 * h2 + 1] = h16_pair(c[h2].z, c[h2].w);
    b[2 * h2] = h16_pair(c[2 + h2].x, c[2 + h2].y);
    b[2 * h2 + 1] = h16_pair(c[2 + h2].z, c[2 + h2].w);
  }
}

// ---------------------------------------------------------------------------------------------
// halo geometry: a TH x TW pixel tile with its one-pixel frame as LDS rows of 64 bf16 channels, staged by NPT producer threads
// ---------------------------------------------------------------------------------------------
// Rows are padded from 128 to 144 bytes instead of XOR-swizzled: the 36-dword stride makes every ds_read_b128 lane group (16 rows,
// one 16-byte unit each) hit 64 distinct banks (9 r mod 16 is a permutation), and keeps addresses linear so taps, units and ring
// slots are immediate offsets.  A producer thread owns one 16-byte unit of a row in every pass of RPP rows: KU units per halo.
// (ROWB_ = 80: the same halo as rows of 64 fp8 channels, 64 bytes padded alike.)
template <int TH_, int TW_, int NPT_, int ROWB_ = 144>
struct HaloGeom {
  static constexpr int TH = TH_, TW = TW_, NPT = NPT_;
  static constexpr int ROWB = ROWB_;
  static constexpr int HP = TW + 2, HALO = (TH + 2) * HP;
  static constexpr int RPP = NPT / 8;                        // halo rows per pass (8 lanes per 128-byte row)
  static constexpr int KU = (HALO + RPP - 1) / RPP;          // halo units per producer thread
  static constexpr int HROWS = KU * RPP;                     // rows that the passes cover: the units past HALO need spare rows
};

}  // namespace prg
