// resblock_tail.hip — the fused tail of a ResnetBlock on the bf16 path: GroupNorm + SiLU of h, the 1x1 res_conv of the block's
// (concatenated) input on MFMA and the residual sum in one pass, optionally with the network's 1x1 head on the tile.
#include "attn_common.h"

namespace prg {

namespace {

// =====================================================================================================
// ResnetBlock tail with the 1x1 res_conv folded in (sd:731-734):
//   out = SiLU(h * A[b][c] + Bc[b][c]) + Wres . cat[s0, s1] + bres          (A, Bc: GroupNorm folded by gn_coeff)
// Unfused this is a 1x1 conv launch (reads both sources, writes res) plus the flat pass (reads h and res, writes out);
// fused, res never exists in HBM: -268 MB per level-0 block.  64-pixel tiles; the source tile and the h tile go
// through LDS (coalesced 16-byte global accesses on both sides), Wres lives in registers as MFMA fragments, the
// accumulator has pixels as columns so a lane owns four consecutive channels of one pixel.
// Reads in flight: two register sets per block (tiles t+1 and t+2 while tile t is worked on) and the per-channel
// coefficients in LDS instead of 48 registers per lane: 148 / 210 / 250 VGPRs, 3 / 2 / 2 blocks per CU, 144 / 160 / 192 KB
// of tile reads in flight per CU for <128,64> / <192,128> / <256,128> (one set and the coefficients in registers: 48 / 80 /
// 96 KB).  Measured: the launches do not get faster for it; only the head launch does, by its weights in LDS.
// =====================================================================================================
constexpr int kTailDepth = 2;        // register sets of a tail block = tiles of reads in flight per block
template <int CIN, int COUT>
__global__ __launch_bounds__(256, COUT == 64 ? 3 : 2) void resblock_tail_fused_kernel(
    const bf16_t* __restrict__ h, const float* __restrict__ A, const float* __restrict__ Bc, const bf16_t* __restrict__ s0, int C0,
    const bf16_t* __restrict__ s1, int C1, const bf16_t* __restrict__ wres, const float* __restrict__ bres, bf16_t* __restrict__ out,
    int N, const float* __restrict__ head_w, const float* __restrict__ head_b, float* __restrict__ head_out, int head_sigmoid,
    const GnFold fold) {
  constexpr int LDX = CIN + 8, LDH = COUT + 8;
  constexpr int RT = COUT / 32, NA = RT / 2;          // row tiles of 32 channels; accumulators per wave
  constexpr int XV = CIN / 32, HV = COUT / 32;        // 16-byte vectors per thread of the source / h tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* xs = reinterpret_cast<__bf16*>(smem);       // [64][LDX]
  __bf16* hs = xs + kTP * LDX;                        // [64][LDH]
  float* cf = reinterpret_cast<float*>(hs + kTP * LDH);   // [4][COUT]: A | Bc | bres of this image | head_w
  const int b = blockIdx.y, slab = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, hi = lane >> 5;
  const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
  const int ntiles = (N + kTP - 1) / kTP;
  const int t0 = slab * kTilesPerBlock, t1 = min(t0 + kTilesPerBlock, ntiles);
  const int yrt = y_row_tile<RT>(wave, 0);
  int ypt[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) ypt[a] = y_pix_tile<RT>(wave, a);
  bf16x8 wr[CIN / 16];
  load_wfrags<CIN>(wr, wres, yrt * 32, l31, hi);
  // The image's coefficients, one channel per thread, once per block into LDS (48 registers per lane as quads: the
  // third wave per SIMD); barrier (1) of the first tile publishes them.  Per channel the same operations as a handle's
  // gn_coeff pass: the GroupNorm fold from the image's fixed-point statistics, or the A / Bc tables.
  if (threadIdx.x < COUT) {
    const int c = threadIdx.x;
    float a, bb;
    if (fold.acc) {
      float mean, rstd;
      gn_fold_stats(fold, b, c / fold.cpg, mean, rstd);
      a = rstd * fold.P[(size_t)b * fold.pq_stride + c];
      bb = fmaf(-mean, a, fold.Q[(size_t)b * fold.pq_stride + c]);
    } else {
      a = A[(size_t)b * COUT + c];
      bb = Bc[(size_t)b * COUT + c];
    }
    cf[c] = a;
    cf[COUT + c] = bb;
    cf[2 * COUT + c] = bres[c];
    if (head_out) cf[3 * COUT + c] = head_w[c];        // (a global load inside the loop would wait for the tiles in flight)
  }
  const float hb = head_out ? head_b[0] : 0.0f;
  // Two register sets: while tile t is worked on, tiles t+1 and t+2 are on their way (two tiles of reads in flight per
  // block).  h of a later tile is never written before this block has read it: a block writes only its own tiles, after
  // reading them, so `out` may be `h`.
  struct Tile { u32x4 x[XV], h[HV]; };
  Tile ta, tb;
  // Every load is issued for every lane, so that the waits on a register set stay counted (a load under a branch makes the
  // compiler drain the whole queue): rows past the image's or the block's last pixel re-read that pixel (one line per
  // wave; their columns of the MFMA and their LDS rows are never stored).
  const int plast = min(t1 * kTP, N) - 1;
  auto load_tile = [&](Tile& T, int t) {
    const int64_t pix = (int64_t)b * N + min(t * kTP + row, plast);
#pragma unroll
    for (int i = 0; i < XV; ++i) {
      const int c = (part + 4 * i) * 8;
      const bf16_t* p = c < C0 ? s0 + pix * C0 + c : s1 + pix * C1 + (c - C0);
      T.x[i] = *reinterpret_cast<const u32x4*>(p);
    }
#pragma unroll
    for (int i = 0; i < HV; ++i) T.h[i] = *reinterpret_cast<const u32x4*>(h + pix * COUT + (part + 4 * i) * 8);
  };
  auto do_tile = [&](Tile& T, int t) {
    const int valid = t < t1 ? min(kTP, N - t * kTP) : 0;
#pragma unroll
    for (int i = 0; i < XV; ++i) *reinterpret_cast<u32x4*>(xs + row * LDX + (part + 4 * i) * 8) = T.x[i];
#pragma unroll
    for (int i = 0; i < HV; ++i) *reinterpret_cast<u32x4*>(hs + row * LDH + (part + 4 * i) * 8) = T.h[i];
    __syncthreads();                                                                            // (1) tiles staged
    load_tile(T, t + kTailDepth);
    // this lane's 16 channels: yrt*32 + 8 g4 + 4 hi + {0..3}; one 32-pixel half after the other (16 accumulators live)
#pragma unroll
    for (int a = 0; a < NA; ++a) {
      f32x16 ya = zero16();
#pragma unroll
      for (int kk = 0; kk < CIN / 16; ++kk)
        ya = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wr[kk], frag(xs + ypt[a] * 32 * LDX, LDX, l31, hi, kk), ya, 0, 0, 0);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int c0 = yrt * 32 + 8 * g4 + 4 * hi;
        const float4 ca = *reinterpret_cast<const float4*>(cf + c0);
        const float4 cb = *reinterpret_cast<const float4*>(cf + COUT + c0);
        const float4 cr = *reinterpret_cast<const float4*>(cf + 2 * COUT + c0);
        const float a4[4] = {ca.x, ca.y, ca.z, ca.w};
        const float b4[4] = {cb.x, cb.y, cb.z, cb.w};
        const float r4[4] = {cr.x, cr.y, cr.z, cr.w};
        __bf16* hp = hs + (ypt[a] * 32 + l31) * LDH + c0;
        const uint2 hw = *reinterpret_cast<const uint2*>(hp);
        const float hx[4] = {bf_lo(hw.x), bf_hi(hw.x), bf_lo(hw.y), bf_hi(hw.y)};
        float y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = Elem<bf16_t>::silu(fmaf(hx[j], a4[j], b4[j])) + (ya[4 * g4 + j] + r4[j]);
        uint2 w;
        w.x = pack_bf16(y[0], y[1]);
        w.y = pack_bf16(y[2], y[3]);
        *reinterpret_cast<uint2*>(hp) = w;            // each (pixel, channel quad) is owned by exactly one lane
      }
    }
    __syncthreads();                                                                            // (2) out tile in hs
    if (head_out) {
      // the network's last layer (1x1 conv to one channel) on the tile: four lanes share a pixel's channels
      float acc = 0.0f;
#pragma unroll
      for (int i = 0; i < HV; ++i) {
        const uint4 v = *reinterpret_cast<const uint4*>(hs + row * LDH + (part + 4 * i) * 8);
        const float* w = cf + 3 * COUT + (part + 4 * i) * 8;
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc = fmaf(bf_lo(q[j]), w[2 * j], acc);
          acc = fmaf(bf_hi(q[j]), w[2 * j + 1], acc);
        }
      }
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (part == 0 && row < valid) {
        const float y = acc + hb;
        head_out[(int64_t)b * N + (int64_t)t * kTP + row] = head_sigmoid ? 1.0f / (1.0f + expf(-y)) : y;
      }
    } else if (row < valid) {
#pragma unroll
      for (int i = 0; i < HV; ++i)
        *reinterpret_cast<uint4*>(out + ((int64_t)b * N + (int64_t)t * kTP + row) * COUT + (part + 4 * i) * 8) =
            *reinterpret_cast<const uint4*>(hs + row * LDH + (part + 4 * i) * 8);
    }
    __syncthreads();                                                                            // (3) tiles free
  };
  load_tile(ta, t0);
  load_tile(tb, t0 + 1);
  // (one back edge and no exit between the two halves, so that the compiler's waits stay counted: with an odd number of
  // tiles the second half runs once on a tile past the block's last one and stores nothing)
  for (int t = t0; t < t1; t += kTailDepth) {
    do_tile(ta, t);
    do_tile(tb, t + 1);
  }
}

int tail_slabs(int N) { return ceil_div(ceil_div(N, kTP), kTilesPerBlock); }

template <int CIN, int COUT>
int launch_tail(const bf16_t* h, const float* A, const float* Bc, const bf16_t* s0, int C0, const bf16_t* s1, int C1,
                const bf16_t* wres, const float* bres, bf16_t* out, int B, int N, hipStream_t s, const GnFold& fold,
                const float* head_w = nullptr, const float* head_b = nullptr, float* head_out = nullptr, int head_sigmoid = 0) {
  const size_t lds = (size_t)kTP * (CIN + 8 + COUT + 8) * 2 + (size_t)4 * COUT * 4;
  static DeviceOnce attr;   // one-time opt-in; atomic: lanes launch from several host threads (idempotent call)
  if (!attr.done()) {
    int rc = set_lds(&resblock_tail_fused_kernel<CIN, COUT>, lds);
    if (rc) return rc;
    attr.mark();
  }
  resblock_tail_fused_kernel<CIN, COUT><<<dim3(tail_slabs(N), B), 256, lds, s>>>(h, A, Bc, s0, C0, s1, C1, wres, bres, out, N, head_w, head_b,
                                                                                 head_out, head_sigmoid, fold);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // namespace

bool resblock_tail_fused_supported(int C0, int C1, int Cout) {
  const int cin = C0 + C1;
  return C0 % 8 == 0 && C1 % 8 == 0 && ((cin == 128 && Cout == 64) || (cin == 192 && Cout == 128) || (cin == 256 && Cout == 128));
}

// out (B, N, Cout) <- SiLU(h * A + Bc) + wres [Cout][C0+C1] . cat[s0 (B,N,C0), s1 (B,N,C1)] + bres.  out may alias h.
int launch_resblock_tail_fused(const bf16_t* h, const float* A, const float* Bc, const bf16_t* s0, int C0, const bf16_t* s1,
                               int C1, const bf16_t* wres, const float* bres, bf16_t* out, int B, int N, int Cout,
                               hipStream_t s,
                               const float* head_w, const float* head_b, float* head_out, int head_sigmoid, const GnFold* fold) {
  PRG_CHECK(resblock_tail_fused_supported(C0, C1, Cout) && bres, "fused resblock tail: unsupported shape");
  PRG_CHECK(!head_out || (Cout == 64 && head_w && head_b), "fused resblock tail: the head needs Cout = 64");
  GnFold f{};
  if (fold && fold->acc) {
    f = *fold;
    PRG_CHECK(f.cpg % 4 == 0 && f.G * f.cpg == Cout && f.P && f.Q, "fused resblock tail: bad GroupNorm fold");
  } else {
    PRG_CHECK(A && Bc, "fused resblock tail: no coefficients");
  }
  if (Cout == 64) return launch_tail<128, 64>(h, A, Bc, s0, C0, s1, C1, wres, bres, out, B, N, s, f, head_w, head_b, head_out, head_sigmoid);
  if (C0 + C1 == 192) return launch_tail<192, 128>(h, A, Bc, s0, C0, s1, C1, wres, bres, out, B, N, s, f);   // up level 2
  return launch_tail<256, 128>(h, A, Bc, s0, C0, s1, C1, wres, bres, out, B, N, s, f);
}

}  // namespace prg
