// attn_fused.hip — Residual(PreNorm(LinearAttention)) of the U-Net (sd:583-589, 631-639, 737-769) as four kernels that
// never materialise q, k, v for the bf16 throughput path.
//
// The unfused path (blocks.hip) moves ~3 GB per instance at 128x128 / B=64 (LayerNorm out, the 384-channel qkv tensor
// written once and read three times, the 128-channel attention output, the to_out result): it is HBM-bound at 8x the
// bytes the block needs.  Here every pass re-reads only x (C channels per pixel) and recomputes what it needs with MFMA:
//
//   la_kmax   x -> LayerNorm -> k = Wk x^        column maxima per slab   (only when the static bound on |k| does not hold)
//   la_ctx    x -> LayerNorm -> k, v             p = exp(k [- max]);  sum_n p,  ctx[d][e] += p[n][d] v[n][e]   per slab
//   la_fin    slabs summed in fixed order, ctx / sum / N * 32^-1/2 -> bf16, stored in the k-slot order la_out's MFMA wants
//   la_out    x -> LayerNorm -> q -> softmax_d -> out = ctx^T q -> y = Wout out + b -> LayerNorm -> + x     -> store
//
// Tiles are 64 pixels; a block of four waves walks kTilesPerBlock tiles of one image.  Wave w owns head w and keeps its
// rows of the projection weights in registers as MFMA fragments (no LDS copy: 29-46 KB of LDS per block, several
// blocks per CU); the LDS tiles have rows padded to C+8 / 136 / 72 bf16 so the 16 lanes of a ds_read_b128 group hit
// distinct banks.
// MFMA: v_mfma_f32_32x32x16_bf16; its operand and accumulator layout is attn_common.h's.
// The LayerNorm gain of PreNorm is folded into the projection weights on the host (unet.hip).
#include <type_traits>

#include "attn_common.h"

namespace prg {

namespace {

__device__ inline float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

template <int C>
struct Geo {
  static constexpr int LDW = C + 8;       // LDS row stride of C-wide rows (bf16 elements)
  static constexpr int VPT = C / 32;      // 16-byte vectors per thread of a 64 x C tile (4 threads per pixel row)
  static constexpr int KK = C / 16;       // MFMA k-steps over C
};

// ---- x tile: global -> registers -> LayerNorm -> LDS ------------------------------------------------------------
// thread t: pixel row t >> 2, vectors (t & 3) + 4 i (interleaved so that a row's four threads read one contiguous run)
template <int C>
struct XTile {
  uint4 v[Geo<C>::VPT];
  __device__ inline void load(const bf16_t* x, int64_t pix0, int valid) {
    const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
#pragma unroll
    for (int i = 0; i < Geo<C>::VPT; ++i)
      v[i] = row < valid ? *reinterpret_cast<const uint4*>(x + (pix0 + row) * C + (part + 4 * i) * 8) : make_uint4(0, 0, 0, 0);
  }
  // (x - mean) * rstd as bf16 into xn[row][c]  (biased variance, two-pass on the registers, eps 1e-5)
  __device__ inline void normalize_to(__bf16* xn) const {
    const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
    float f[Geo<C>::VPT][8];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < Geo<C>::VPT; ++i) {
      const uint32_t w[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f[i][2 * j] = bf_lo(w[j]);
        f[i][2 * j + 1] = bf_hi(w[j]);
        s += f[i][2 * j] + f[i][2 * j + 1];
      }
    }
    s = quad_sum(s);                                     // a row's four threads are one quad: DPP, no LDS crossbar
    const float mean = s * (1.0f / C);
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < Geo<C>::VPT; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        f[i][j] -= mean;
        q = fmaf(f[i][j], f[i][j], q);
      }
    q = quad_sum(q);
    const float rstd = __builtin_amdgcn_rsqf(q * (1.0f / C) + kLnEps);   // (v_rsq_f32, 1 ulp: these tiles are rounded to bf16 next)
#pragma unroll
    for (int i = 0; i < Geo<C>::VPT; ++i) {
      uint4 o;
      o.x = pack_bf16(f[i][0] * rstd, f[i][1] * rstd);
      o.y = pack_bf16(f[i][2] * rstd, f[i][3] * rstd);
      o.z = pack_bf16(f[i][4] * rstd, f[i][5] * rstd);
      o.w = pack_bf16(f[i][6] * rstd, f[i][7] * rstd);
      *reinterpret_cast<uint4*>(xn + row * Geo<C>::LDW + (part + 4 * i) * 8) = o;
    }
  }
};

// rows [r0, r0 + nrows) of a row-major [.][C] bf16 matrix -> LDS rows of stride LD (all 256 threads)
template <int COLS, int LD>
__device__ inline void stage_rows(__bf16* dst, const bf16_t* src, int nrows) {
  constexpr int VR = COLS / 8;
  for (int i = threadIdx.x; i < nrows * VR; i += 256) {
    const int r = i / VR, v = i - r * VR;
    *reinterpret_cast<uint4*>(dst + r * LD + v * 8) = *reinterpret_cast<const uint4*>(src + (size_t)r * COLS + v * 8);
  }
}

// =====================================================================================================
// pass 1: column maxima of k per slab
// =====================================================================================================
template <int C>
__global__ __launch_bounds__(256) void la_kmax_fused_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wqkv,
                                                            float* __restrict__ pmax, int N, int nslab) {
  using G = Geo<C>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* xn = reinterpret_cast<__bf16*>(smem);      // [64][LDW]
  const int b = blockIdx.y, slab = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int ntiles = (N + kTP - 1) / kTP;
  const int tpb = tiles_per_block(ntiles), t0 = slab * tpb, t1 = min(t0 + tpb, ntiles);
  bf16x8 wk[G::KK];                                    // k rows 32 wave .. + 32 of the projection
  load_wfrags<C>(wk, wqkv, kHidden + 32 * wave, l31, hi);
  float m = -INFINITY;                                 // column 32 wave + l31, this lane's pixel rows
  XTile<C> xt;
  if (t0 < t1) xt.load(x, (int64_t)b * N + (int64_t)t0 * kTP, min(kTP, N - t0 * kTP));
  for (int t = t0; t < t1; ++t) {
    xt.normalize_to(xn);
    __syncthreads();
    if (t + 1 < t1) xt.load(x, (int64_t)b * N + (int64_t)(t + 1) * kTP, min(kTP, N - (t + 1) * kTP));
    f32x16 acc[2] = {zero16(), zero16()};
#pragma unroll
    for (int kk = 0; kk < G::KK; ++kk) {
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(xn + pt * 32 * G::LDW, G::LDW, l31, hi, kk), wk[kk], acc[pt], 0, 0, 0);
    }
    const int valid = min(kTP, N - t * kTP);
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int px = pt * 32 + acc_row(r, hi);
        if (px < valid) m = fmaxf(m, acc[pt][r]);
      }
    __syncthreads();
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  if (hi == 0) pmax[((size_t)b * nslab + slab) * kHidden + 32 * wave + l31] = m;
}

// =====================================================================================================
// pass 2: per-slab sums of p = exp(k - max) and of p v^T
// =====================================================================================================
// Both kernels of this file's attention are VALU-ISSUE bound (SQ counters, round 3: per tile and wave ~330 VALU instructions
// beside 24 MFMAs, VALU issue + matrix-pipe busy cycles ~ the kernel's duration, i.e. they barely overlap; neither occupancy
// 3 -> 4, nor the slab count, nor a deeper x prefetch moved it), so the loop is written to issue as few VALU instructions
// as possible:
//  * p and v go into the context MFMA STRAIGHT FROM THE ACCUMULATOR REGISTERS — the contraction index (pixels) may be
//    enumerated in any order as long as both operands use the same one, and lane (column, half hi) of the k / v
//    accumulators holds, in registers 8 i .. 8 i + 7, exactly the eight pixels that A's row / B's column `l31` supplies for
//    k-slots 8 hi .. 8 hi + 7 of k-step i (la_out's trick for q): no transposed LDS tiles;
//  * KSTAT (static bound on |k|, <= 57.7 in the log2 units the pre-scaled rows produce — unet.hip): NO shift at all.  The
//    softmax is shift-invariant, exp2(k) stays inside [2^-58, 2^58], the sums over at most 2^16 pixels inside 2^74, and
//    bf16 / fp32 relative precision does not depend on the scale: no splat, no subtraction, no maximum pass.  Otherwise
//    (measured maxima) the shift is the first MFMA's C operand, a loop-invariant register set;
//  * whole tiles take a branch without the per-pixel masks;
//  * PSUM_MFMA: sum_n p from the matrix pipe (pT times an all-ones operand: the SAME bf16-rounded p that feeds ctx) instead
//    of 32 float additions per tile and lane.
template <int C, bool PSUM_MFMA, bool KSTAT>
__global__ __launch_bounds__(256, C == 64 ? 3 : (C == 128 ? 2 : 1)) void la_ctx_fused_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wqkv,
                                                           const float* __restrict__ pmax, float* __restrict__ ctxp,
                                                           float* __restrict__ sump, int N, int nslab) {
  using G = Geo<C>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* xn = reinterpret_cast<__bf16*>(smem);      // [64][LDW]
  const int b = blockIdx.y, slab = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int ntiles = (N + kTP - 1) / kTP;
  const int tpb = tiles_per_block(ntiles), t0 = slab * tpb, t1 = min(t0 + tpb, ntiles);
  bf16x8 wk[G::KK], wv[G::KK];                         // k and v rows of head `wave`
  load_wfrags<C>(wk, wqkv, kHidden + 32 * wave, l31, hi);
  load_wfrags<C>(wv, wqkv, 2 * kHidden + 32 * wave, l31, hi);
  f32x16 kinit0 = zero16();                            // the k accumulators' initial value: minus the column maximum
  if constexpr (!KSTAT) {
    float m = -INFINITY;                               // (fixed-order reduce of la_kmax's slab maxima)
    for (int s2 = 0; s2 < nslab; ++s2) m = fmaxf(m, pmax[((size_t)b * nslab + s2) * kHidden + 32 * wave + l31]);
#pragma unroll
    for (int e = 0; e < 16; ++e) kinit0[e] = -m;
  }
  f32x16 ctx = zero16();                               // rows d, column e = l31 of head `wave`
  f32x16 psum = zero16();                              // rows d (any column)
  float ssum = 0.0f;
  bf16x8 ones;
#pragma unroll
  for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
  XTile<C> xt;
  if (t0 < t1) xt.load(x, (int64_t)b * N + (int64_t)t0 * kTP, min(kTP, N - t0 * kTP));
  for (int t = t0; t < t1; ++t) {
    xt.normalize_to(xn);
    __syncthreads();
    if (t + 1 < t1) xt.load(x, (int64_t)b * N + (int64_t)(t + 1) * kTP, min(kTP, N - (t + 1) * kTP));
    const int valid = min(kTP, N - t * kTP);
    // one 32-pixel half: k = x Wk^T (- shift) and v = x Wv^T, p = exp2(k), ctx += p^T v
    auto half = [&](const int pt, auto full_c) {
      constexpr bool FULL = decltype(full_c)::value;
      f32x16 k1, v1;
#pragma unroll
      for (int kk = 0; kk < G::KK; ++kk) {
        const bf16x8 xf = frag(xn + pt * 32 * G::LDW, G::LDW, l31, hi, kk);
        k1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, wk[kk], kk == 0 ? (KSTAT ? zero16() : kinit0) : k1, 0, 0, 0);
        v1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(xf, wv[kk], kk == 0 ? zero16() : v1, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        bf16x8 pa, vb;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const int r = 8 * i + s2;
          float pe = __builtin_amdgcn_exp2f(k1[r]);
          if constexpr (!FULL) pe = (pt * 32 + acc_row(r, hi)) < valid ? pe : 0.0f;
          if constexpr (!PSUM_MFMA) ssum += pe;
          pa[s2] = (__bf16)pe;
          vb[s2] = (__bf16)v1[r];
        }
        ctx = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, vb, ctx, 0, 0, 0);
        if constexpr (PSUM_MFMA) psum = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, ones, psum, 0, 0, 0);
      }
    };
    if (valid == kTP) {                                // (wave-uniform)
      half(0, std::true_type{});
      half(1, std::true_type{});
    } else {
      half(0, std::false_type{});
      half(1, std::false_type{});
    }
    __syncthreads();
  }
  const size_t ph = ((size_t)b * 4 + wave) * nslab + slab;
  if constexpr (PSUM_MFMA) {
    if (l31 == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sump[ph * 32 + acc_row(r, hi)] = psum[r];
    }
  } else {
    ssum += __shfl_xor(ssum, 32, 64);
    if (hi == 0) sump[ph * 32 + l31] = ssum;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) ctxp[ph * 1024 + acc_row(r, hi) * 32 + l31] = ctx[r];
}

// =====================================================================================================
// pass 3: ctx = sum_slabs(ctxp) / sum_slabs(sump) / N * 32^-1/2, as bf16 [b][h][e][slot(d)]
// slot(d) orders the 32 d of a row the way la_out's q registers supply them to the MFMA (see there)
// =====================================================================================================
__global__ __launch_bounds__(256) void la_fin_fused_kernel(const float* __restrict__ ctxp, const float* __restrict__ sump,
                                                           bf16_t* __restrict__ ctxT, int N, int nslab) {
  const int h = blockIdx.x, b = blockIdx.y;
  const size_t ph = ((size_t)b * 4 + h) * nslab;
  const float scale = 0.17677669529663687f / (float)N;    // 32^-1/2 (q) and 1/N (v)
  for (int idx = threadIdx.x; idx < 1024; idx += 256) {
    const int d = idx >> 5, e = idx & 31;
    float c = 0.0f, s = 0.0f;
    int s2 = 0;
    for (; s2 + 8 <= nslab; s2 += 8) {          // loads of a group issued together; the sums stay in slab order
      float cv[8], sv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        cv[u] = ctxp[(ph + s2 + u) * 1024 + idx];
        sv[u] = sump[(ph + s2 + u) * 32 + d];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        c += cv[u];
        s += sv[u];
      }
    }
    for (; s2 < nslab; ++s2) {
      c += ctxp[(ph + s2) * 1024 + idx];
      s += sump[(ph + s2) * 32 + d];
    }
    const int slot = kslot(d);
    ctxT[((size_t)b * 4 + h) * 1024 + e * 32 + slot] = f32_to_bf16(c / s * scale);
  }
}

// =====================================================================================================
// pass 4: q, softmax over d, ctx^T q, to_out conv + bias, LayerNorm, residual
// =====================================================================================================
template <int C, bool QSTAT>   // QSTAT: static bound on |q| (qshift != null is the flag; the value itself is not needed)
__global__ __launch_bounds__(256, C == 64 ? 3 : (C == 128 ? 2 : 1)) void la_out_fused_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ wqkv,
                                                           const bf16_t* __restrict__ wout, const float* __restrict__ bias,
                                                           const float* __restrict__ out_g, const bf16_t* __restrict__ ctxT,
                                                           bf16_t* __restrict__ out, int N, const float* __restrict__ qshift) {
  using G = Geo<C>;
  constexpr int RT = C / 32;                 // 32-channel row tiles of y
  constexpr int NA = RT / 2;                 // y accumulators per wave (RT x 2 pixel tiles over 4 waves)
  constexpr int NR = RT > 4 ? RT / 4 : 1;    // distinct row tiles per wave (C = 256: two, each with both pixel tiles)
  constexpr int RTL = RT > 4 ? RT : 4;       // row-tile pitch of the LayerNorm partial sums
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* xn = reinterpret_cast<__bf16*>(smem);      // [64][LDW]
  __bf16* ot = xn + kTP * G::LDW;                    // [64][kLdO]  attention output, pixel-major
  float* lnb = reinterpret_cast<float*>(ot + kTP * kLdO);   // [64][4][2] LayerNorm partial sums
  __bf16* yt = reinterpret_cast<__bf16*>(lnb + kTP * RTL * 2);   // [64][LDW] the normalised y tile (its own buffer: no barrier
                                                             // between a tile's last phase and the next tile's LayerNorm)
  // to_out's bias and the output LayerNorm's gain live in LDS: as global loads inside the tile loop they sat BEHIND the
  // next tile's x prefetch in the in-order vmcnt queue, so every tile waited for its successor's HBM latency
  float* bias_l = reinterpret_cast<float*>(yt + kTP * G::LDW);   // [C]
  float* outg_l = bias_l + C;                                    // [C]
  if (threadIdx.x < C) {
    bias_l[threadIdx.x] = bias[threadIdx.x];
    outg_l[threadIdx.x] = out_g[threadIdx.x];
  }                                                              // (visible after the first tile's barrier (1))
  const int b = blockIdx.y, slab = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int ntiles = (N + kTP - 1) / kTP;
  const int tpb = tiles_per_block(ntiles), t0 = slab * tpb, t1 = min(t0 + tpb, ntiles);
  bf16x8 wq[G::KK];                                    // q rows of head `wave`
  load_wfrags<C>(wq, wqkv, 32 * wave, l31, hi);
  // ctx^T rows e = l31 of head `wave`; k-slot s of half hi in k-step i is d = 16 i + 8 (s >> 2) + 4 hi + (s & 3):
  // exactly the d of q-accumulator register 8 i + s of a lane in half hi, so q feeds the MFMA without any shuffle
  bf16x8 ca[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    ca[i] = *reinterpret_cast<const bf16x8*>(ctxT + (((size_t)b * 4 + wave) * 32 + l31) * 32 + i * 16 + hi * 8);
  // y accumulators of this wave: row tile / pixel tile
  int yrt[NA], ypt[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    yrt[a] = y_row_tile<RT>(wave, a);
    ypt[a] = y_pix_tile<RT>(wave, a);
  }
  bf16x8 wo[NR][kHidden / 16];                            // to_out rows of this wave's y row tile(s)
#pragma unroll
  for (int r = 0; r < NR; ++r) load_wfrags<kHidden>(wo[r], wout, yrt[RT > 4 ? 2 * r : 0] * 32, l31, hi);
  XTile<C> xt;
  if (t0 < t1) xt.load(x, (int64_t)b * N + (int64_t)t0 * kTP, min(kTP, N - t0 * kTP));
  for (int t = t0; t < t1; ++t) {
    asm volatile("" ::: "memory");                     // (bias / out_g stay loads inside the loop: hoisted they cost 32 registers and a block per CU)
    const XTile<C> xraw = xt;                          // residual
    const int valid = min(kTP, N - t * kTP);
    xt.normalize_to(xn);
    __syncthreads();                                                                            // (1) xn ready
    if (t + 1 < t1) xt.load(x, (int64_t)b * N + (int64_t)(t + 1) * kTP, min(kTP, N - (t + 1) * kTP));
    // q^T[d][px] of head `wave`.  QSTAT (static bound |q| <= 57.7, see la_ctx's KSTAT): the softmax over d is
    // shift-invariant and exp2(q) stays inside [2^-58, 2^58], so there is no maximum, no shift and no subtraction.
    constexpr bool qstat = QSTAT;
    f32x16 qa[2];
#pragma unroll
    for (int kk = 0; kk < G::KK; ++kk) {
#pragma unroll
      for (int pt = 0; pt < 2; ++pt)
        qa[pt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wq[kk], frag(xn + pt * 32 * G::LDW, G::LDW, l31, hi, kk),
                                                         kk == 0 ? zero16() : qa[pt], 0, 0, 0);
    }
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
      f32x16 oa = zero16();
      if constexpr (qstat) {
        // e^q unnormalised into the contraction; sum_d e^q of pixel (column) l31 from the same operands against an
        // all-ones A (every row of `sa` holds it); the 1 / sum scales the 16 OUTPUTS of the lane instead of its 32 inputs
        f32x16 sa = zero16();
        bf16x8 ones;
#pragma unroll
        for (int e = 0; e < 8; ++e) ones[e] = (__bf16)1.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          bf16x8 qb;
#pragma unroll
          for (int s2 = 0; s2 < 8; ++s2) qb[s2] = (__bf16)__builtin_amdgcn_exp2f(qa[pt][8 * i + s2]);
          oa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ca[i], qb, oa, 0, 0, 0);      // rows e, column px
          sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones, qb, sa, 0, 0, 0);
        }
        const float inv = __builtin_amdgcn_rcpf(sa[0]);
        const f32x2 inv2 = {inv, inv};
#pragma unroll
        for (int r = 0; r < 16; r += 2) {                  // (v_pk_mul_f32)
          const f32x2 o2 = f32x2{oa[r], oa[r + 1]} * inv2;
          oa[r] = o2[0];
          oa[r + 1] = o2[1];
        }
      } else {
        // measured maximum (blocks whose static bound is too large): softmax over the 32 d of pixel pt*32 + l31, 16 in this
        // lane, 16 in lane ^ 32
        float mx = qa[pt][0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, qa[pt][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float sm = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          qa[pt][r] = __builtin_amdgcn_exp2f(qa[pt][r] - mx);   // q arrives times log2(e) (weights pre-scaled)
          sm += qa[pt][r];
        }
        sm += __shfl_xor(sm, 32, 64);
        const float inv = 1.0f / sm;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          bf16x8 qb;
#pragma unroll
          for (int s2 = 0; s2 < 8; ++s2) qb[s2] = (__bf16)(qa[pt][8 * i + s2] * inv);
          oa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ca[i], qb, oa, 0, 0, 0);      // rows e, column px
        }
      }
      const int px = pt * 32 + l31;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        uint2 w;
        w.x = pack_bf16(oa[4 * g4], oa[4 * g4 + 1]);
        w.y = pack_bf16(oa[4 * g4 + 2], oa[4 * g4 + 3]);
        *reinterpret_cast<uint2*>(ot + px * kLdO + 32 * wave + 8 * g4 + 4 * hi) = w;
      }
    }
    __syncthreads();                                                                            // (2) ot ready, xn free
    // y^T[c][px] = Wout[c][:] . o[px][:] + bias
    f32x16 ya[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) ya[a] = zero16();
#pragma unroll
    for (int kk = 0; kk < kHidden / 16; ++kk) {
#pragma unroll
      for (int a = 0; a < NA; ++a)
        ya[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wo[RT > 4 ? (a >> 1) : 0][kk],
                                                        frag(ot + ypt[a] * 32 * kLdO, kLdO, l31, hi, kk), ya[a], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = yrt[a] * 32 + acc_row(r, hi);
        ya[a][r] += bias_l[c];
        s1 += ya[a][r];
        s2 = fmaf(ya[a][r], ya[a][r], s2);
      }
      // v_permlane32_swap(s1, s2): lanes 0..31 end up with (s1 lower, s1 upper), lanes 32..63 with (s2 lower, s2 upper), so
      // one swap and one add leave the pixel's sum in the lower half and its sum of squares in the upper half
      const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, s1), __builtin_bit_cast(unsigned, s2), false, false);
      const float tot = __builtin_bit_cast(float, (unsigned)sw[0]) + __builtin_bit_cast(float, (unsigned)sw[1]);
      lnb[((ypt[a] * 32 + l31) * RTL + yrt[a]) * 2 + hi] = tot;
    }
    __syncthreads();                                                                            // (3) partial sums
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      const int px = ypt[a] * 32 + l31;
      float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        s1 += lnb[(px * RTL + rt) * 2];
        s2 += lnb[(px * RTL + rt) * 2 + 1];
      }
      const float mean = s1 * (1.0f / C);
      const float rstd = __builtin_amdgcn_rsqf(fmaxf(s2 * (1.0f / C) - mean * mean, 0.0f) + kLnEps);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int c0 = yrt[a] * 32 + 8 * g4 + 4 * hi;
        const float4 gg = *reinterpret_cast<const float4*>(outg_l + c0);
        uint2 w;
        w.x = pack_bf16((ya[a][4 * g4] - mean) * rstd * gg.x, (ya[a][4 * g4 + 1] - mean) * rstd * gg.y);
        w.y = pack_bf16((ya[a][4 * g4 + 2] - mean) * rstd * gg.z, (ya[a][4 * g4 + 3] - mean) * rstd * gg.w);
        *reinterpret_cast<uint2*>(yt + px * G::LDW + c0) = w;
      }
    }
    __syncthreads();                                                                            // (4) y tile ready
    {
      const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
      if (row < valid) {
#pragma unroll
        for (int i = 0; i < G::VPT; ++i) {
          const uint4 yv = *reinterpret_cast<const uint4*>(yt + row * G::LDW + (part + 4 * i) * 8);
          const uint4 xv = xraw.v[i];
          uint4 o;
          o.x = pack_bf16(bf_lo(yv.x) + bf_lo(xv.x), bf_hi(yv.x) + bf_hi(xv.x));
          o.y = pack_bf16(bf_lo(yv.y) + bf_lo(xv.y), bf_hi(yv.y) + bf_hi(xv.y));
          o.z = pack_bf16(bf_lo(yv.z) + bf_lo(xv.z), bf_hi(yv.z) + bf_hi(xv.z));
          o.w = pack_bf16(bf_lo(yv.w) + bf_lo(xv.w), bf_hi(yv.w) + bf_hi(xv.w));
          *reinterpret_cast<uint4*>(out + ((int64_t)b * N + (int64_t)t * kTP + row) * C + (part + 4 * i) * 8) = o;
        }
      }
    }
  }
}

// =====================================================================================================
// Bottleneck attention core (sd:789-795) on MFMA for N <= 256 tokens: one block per (image, head).
//   S^T[key][query] = K q^T (keys as MFMA rows: a lane owns ONE query and sees all its keys in registers, so the
//   softmax over keys is register-local plus one lane^32 exchange), P = exp(S/sqrt(32) - max), O^T = V^T P.
// K goes to LDS row-major, V transposed with the keys of each 32-key tile stored in the order the S^T accumulator
// registers supply them as the B operand (same trick as la_out): no shuffle between the two MFMAs.
// =====================================================================================================
// ---- what the two kernels of the core share ----
// K and V^T of one (image, head) into LDS (all 256 threads): K row-major [N][LDK]; V^T [32][LDV], each 32-key tile in k-slot order
template <int N, int LDK, int LDV>
__device__ inline void stage_kv(__bf16* Ks, __bf16* Vt, const bf16_t* base, int h) {
  for (int i = threadIdx.x; i < N * 4; i += 256) {
    const int key = i >> 2, u = i & 3;
    *reinterpret_cast<uint4*>(Ks + key * LDK + u * 8) =
        *reinterpret_cast<const uint4*>(base + (size_t)key * 3 * kHidden + kHidden + h * kDimHead + u * 8);
    const uint4 vv = *reinterpret_cast<const uint4*>(base + (size_t)key * 3 * kHidden + 2 * kHidden + h * kDimHead + u * 8);
    const int pos = (key & ~31) + kslot(key & 31);
    const uint32_t w[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      reinterpret_cast<uint16_t*>(Vt)[(u * 8 + 2 * j) * LDV + pos] = (uint16_t)(w[j] & 0xffffu);
      reinterpret_cast<uint16_t*>(Vt)[(u * 8 + 2 * j + 1) * LDV + pos] = (uint16_t)(w[j] >> 16);
    }
  }
}
// S^T of key tile kt (keys as rows) against the lane's query, whose two k-step fragments are q0 and q1; unscaled
template <int LDK>
__device__ inline f32x16 score_tile(const __bf16* Ks, int kt, const bf16x8& q0, const bf16x8& q1, int l31, int hi) {
  f32x16 sa = zero16();
  sa = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(Ks + kt * 32 * LDK, LDK, l31, hi, 0), q0, sa, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(Ks + kt * 32 * LDK, LDK, l31, hi, 1), q1, sa, 0, 0, 0);
}
// O^T / l of the lane's query: channels 8 g4 + {0..3} from op on (op already points at the head's 4 hi)
__device__ inline void store_out(bf16_t* op, const f32x16& oacc, float inv) {
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    uint2 w;
    w.x = pack_bf16(oacc[4 * g4] * inv, oacc[4 * g4 + 1] * inv);
    w.y = pack_bf16(oacc[4 * g4 + 2] * inv, oacc[4 * g4 + 3] * inv);
    *reinterpret_cast<uint2*>(op + 8 * g4) = w;
  }
}

template <int NT>   // key tiles of 32 (N = 32 NT)
__global__ __launch_bounds__(256) void full_attn_mfma_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out) {
  constexpr int N = 32 * NT, LDK = 40, LDV = N + 8;
  __shared__ __attribute__((aligned(16))) __bf16 Ks[N * LDK];
  __shared__ __attribute__((aligned(16))) __bf16 Vt[32 * LDV];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const bf16_t* base = qkv + (size_t)b * N * 3 * kHidden;
  stage_kv<N, LDK, LDV>(Ks, Vt, base, h);
  __syncthreads();
  for (int qt = wave; qt < NT; qt += 4) {
    const bf16_t* qp = base + (size_t)(qt * 32 + l31) * 3 * kHidden + h * kDimHead + hi * 8;
    const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(qp), q1 = *reinterpret_cast<const bf16x8*>(qp + 16);
    f32x16 sacc[NT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      sacc[kt] = score_tile<LDK>(Ks, kt, q0, q1, l31, hi);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sacc[kt][r] *= 0.17677669529663687f;
        m = fmaxf(m, sacc[kt][r]);
      }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.0f;
    f32x16 oacc = zero16();
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        bf16x8 pb;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const float pv = fast_exp(sacc[kt][8 * i + s2] - m);
          l += pv;
          pb[s2] = (__bf16)pv;
        }
        oacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(Vt + kt * 32, LDV, l31, hi, i), pb, oacc, 0, 0, 0);
      }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    store_out(out + ((size_t)b * N + qt * 32 + l31) * kHidden + h * kDimHead + 4 * hi, oacc, inv);
  }
}


// Same contraction for N up to 1024 tokens (the 256x256 bottleneck, 32 x 32): the score tile of a (query tile, key tile)
// pair no longer stays in registers for all key tiles, so the keys are walked twice — pass 1 the row maxima (2 MFMAs per
// key tile), pass 2 the scores again, exp, row sums and V^T P (4 MFMAs) — the reference's two-pass softmax order.  K and
// V^T of one (image, head) fill the LDS (146 KB at N = 1024: one block per CU); QS blocks share a head, each takes every
// QS-th query tile so the grid covers the chip at B = 16.
template <int NT, int QS>
__global__ __launch_bounds__(256) void full_attn_mfma_big_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ out) {
  constexpr int N = 32 * NT, LDK = 40, LDV = N + 8;
  extern __shared__ __attribute__((aligned(16))) char smem_attn[];
  __bf16* Ks = reinterpret_cast<__bf16*>(smem_attn);          // [N][LDK]
  __bf16* Vt = Ks + N * LDK;                                    // [32][LDV]
  const int h = blockIdx.x, b = blockIdx.y, qs = blockIdx.z, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const bf16_t* base = qkv + (size_t)b * N * 3 * kHidden;
  stage_kv<N, LDK, LDV>(Ks, Vt, base, h);
  __syncthreads();
  for (int qt = qs * 4 + wave; qt < NT; qt += 4 * QS) {
    const bf16_t* qp = base + (size_t)(qt * 32 + l31) * 3 * kHidden + h * kDimHead + hi * 8;
    const bf16x8 q0 = *reinterpret_cast<const bf16x8*>(qp), q1 = *reinterpret_cast<const bf16x8*>(qp + 16);
    float m = -INFINITY;
#pragma unroll 2
    for (int kt = 0; kt < NT; ++kt) {
      const f32x16 sa = score_tile<LDK>(Ks, kt, q0, q1, l31, hi);
#pragma unroll
      for (int r = 0; r < 16; ++r) m = fmaxf(m, sa[r] * 0.17677669529663687f);
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float l = 0.0f;
    f32x16 oacc = zero16();
#pragma unroll 2
    for (int kt = 0; kt < NT; ++kt) {
      const f32x16 sa = score_tile<LDK>(Ks, kt, q0, q1, l31, hi);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        bf16x8 pb;
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
          const float pv = fast_exp(sa[8 * i + s2] * 0.17677669529663687f - m);
          l += pv;
          pb[s2] = (__bf16)pv;
        }
        oacc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(Vt + kt * 32, LDV, l31, hi, i), pb, oacc, 0, 0, 0);
      }
    }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    store_out(out + ((size_t)b * N + qt * 32 + l31) * kHidden + h * kDimHead + 4 * hi, oacc, inv);
  }
}

template <int C>
size_t lds_kmax() { return (size_t)kTP * Geo<C>::LDW * 2; }
template <int C>
size_t lds_out() { return (size_t)2 * kTP * Geo<C>::LDW * 2 + (size_t)kTP * kLdO * 2 + (size_t)kTP * (C / 32 > 4 ? C / 32 : 4) * 2 * 4 + (size_t)2 * C * 4; }

template <int C>
constexpr bool kPsumDefault = C >= 128;   // (measured: C = 64 58 against 70 us with it, C = 128 21.4 against 22.8, C = 256 23.7 against 25.6)

template <int C>
int launch_c(const bf16_t* x, const bf16_t* wqkv, const bf16_t* wout, const float* bias, const float* out_g, bf16_t* out,
             float* ws, int B, int N, const float* kshift, hipStream_t s, int psum_override) {
  static DeviceOnce attr;   // one-time opt-in; atomic: lanes launch from several host threads (idempotent call)
  if (!attr.done()) {
    int rc;
    if ((rc = set_lds(&la_kmax_fused_kernel<C>, lds_kmax<C>()))) return rc;
    if ((rc = set_lds(&la_ctx_fused_kernel<C, false, false>, lds_kmax<C>()))) return rc;
    if ((rc = set_lds(&la_ctx_fused_kernel<C, false, true>, lds_kmax<C>()))) return rc;
    if ((rc = set_lds(&la_ctx_fused_kernel<C, true, false>, lds_kmax<C>()))) return rc;
    if ((rc = set_lds(&la_ctx_fused_kernel<C, true, true>, lds_kmax<C>()))) return rc;
    if ((rc = set_lds(&la_out_fused_kernel<C, false>, lds_out<C>()))) return rc;
    if ((rc = set_lds(&la_out_fused_kernel<C, true>, lds_out<C>()))) return rc;
    attr.mark();
  }
  const int nslab = slabs(N);
  float* pmax = ws;
  float* ctxp = pmax + (size_t)B * nslab * kHidden;
  float* sump = ctxp + (size_t)B * 4 * nslab * 1024;
  bf16_t* ctxT = reinterpret_cast<bf16_t*>(sump + (size_t)B * 4 * nslab * 32);
  const dim3 grid(nslab, B);
  if (!kshift) {
    la_kmax_fused_kernel<C><<<grid, 256, lds_kmax<C>(), s>>>(x, wqkv, pmax, N, nslab);
    PRG_LAUNCH_CHECK();
  }
  // PRG_LA_PSUM: sum_n p on the matrix pipe: -1 (default) where measured faster, 0 never, 1 always
  static const int psum_env = env_int("PRG_LA_PSUM", -1);
  const int psum_sel = psum_override >= 0 ? psum_override : psum_env;
  const bool psum = psum_sel > 0 || (psum_sel < 0 && kPsumDefault<C>);
  const auto la_ctx = kshift ? (psum ? &la_ctx_fused_kernel<C, true, true> : &la_ctx_fused_kernel<C, false, true>)
                             : (psum ? &la_ctx_fused_kernel<C, true, false> : &la_ctx_fused_kernel<C, false, false>);
  la_ctx<<<grid, 256, lds_kmax<C>(), s>>>(x, wqkv, pmax, ctxp, sump, N, nslab);
  PRG_LAUNCH_CHECK();
  la_fin_fused_kernel<<<dim3(4, B), 256, 0, s>>>(ctxp, sump, ctxT, N, nslab);
  PRG_LAUNCH_CHECK();
  // (the q shifts of the four heads follow the 128 k shifts)
  const int nt = ceil_div(N, kTP);
  const dim3 ogrid(ceil_div(nt, tiles_per_block(nt)), B);
  if (kshift) la_out_fused_kernel<C, true><<<ogrid, 256, lds_out<C>(), s>>>(x, wqkv, wout, bias, out_g, ctxT, out, N, kshift + kHidden);
  else la_out_fused_kernel<C, false><<<ogrid, 256, lds_out<C>(), s>>>(x, wqkv, wout, bias, out_g, ctxT, out, N, nullptr);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // namespace

bool full_attention_mfma_supported(int N) { return N == 64 || N == 128 || N == 256 || N == 512 || N == 1024; }

template <int NT, int QS>
static int launch_attn_big(const bf16_t* qkv, bf16_t* out, int B, hipStream_t s) {
  constexpr int N = 32 * NT;
  constexpr size_t lds = ((size_t)N * 40 + (size_t)32 * (N + 8)) * 2;
  static DeviceOnce attr;   // one-time opt-in; atomic: lanes launch from several host threads (idempotent call)
  if (!attr.done()) {
    int rc = set_lds(&full_attn_mfma_big_kernel<NT, QS>, lds);
    if (rc) return rc;
    attr.mark();
  }
  full_attn_mfma_big_kernel<NT, QS><<<dim3(4, B, QS), 256, lds, s>>>(qkv, out);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

// qkv (B, N, 384) bf16 -> out (B, N, 128) bf16
int launch_full_attention_mfma(const bf16_t* qkv, bf16_t* out, int B, int N, hipStream_t s) {
  PRG_CHECK(full_attention_mfma_supported(N) && qkv && out, "full attention (MFMA): unsupported token count");
  const dim3 grid(4, B);
  if (N == 1024) return B >= 32 ? launch_attn_big<32, 2>(qkv, out, B, s) : launch_attn_big<32, 4>(qkv, out, B, s);
  if (N == 512) return launch_attn_big<16, 2>(qkv, out, B, s);
  if (N == 64) full_attn_mfma_kernel<2><<<grid, 256, 0, s>>>(qkv, out);
  else if (N == 128) full_attn_mfma_kernel<4><<<grid, 256, 0, s>>>(qkv, out);
  else full_attn_mfma_kernel<8><<<grid, 256, 0, s>>>(qkv, out);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

bool linattn_fused_supported(int C) { return C == 64 || C == 128 || C == 256; }

size_t linattn_fused_ws_floats(int B, int N) {
  const size_t ns = slabs(N);
  return (size_t)B * ns * kHidden + (size_t)B * 4 * ns * 1024 + (size_t)B * 4 * ns * 32 + (size_t)B * 4 * 1024 / 2 + 64;
}

// x, out: (B, N, C) bf16.  wqkv: [384][C] with the PreNorm gain folded in (q | k | v rows, head-major); wout: [C][128].
int launch_linear_attention_fused(const bf16_t* x, const bf16_t* wqkv, const bf16_t* wout, const float* bias,
                                  const float* out_g, bf16_t* out, float* ws, int B, int N, int C, const float* kshift,
                                  hipStream_t s, int psum_override) {
  PRG_CHECK(linattn_fused_supported(C), "fused linear attention: unsupported width");
  PRG_CHECK(slabs(N) <= 4096, "fused linear attention: too many slabs");
  if (C == 64) return launch_c<64>(x, wqkv, wout, bias, out_g, out, ws, B, N, kshift, s, psum_override);
  if (C == 256) return launch_c<256>(x, wqkv, wout, bias, out_g, out, ws, B, N, kshift, s, psum_override);
  return launch_c<128>(x, wqkv, wout, bias, out_g, out, ws, B, N, kshift, s, psum_override);
}

}  // namespace prg
