// conv_split.hip — the convolutions of the `f16x3` precision mode (round 4): float32 storage, every contraction on the
// f16 matrix pipe with BOTH operands split into two halves on the fly.
//
//   a = a_hi + a_lo,  a_hi = f16(a),  a_lo = f16(a - a_hi)      |a - a_hi - a_lo| <= 2^-22 |a|  (f16 subnormals are kept by
//   a * w ~= a_hi * w_hi + a_hi * w_lo + a_lo * w_hi            v_mfma_f32_32x32x16_f16: probed, tools/micro/f16_split_probe.hip)
//
// Three v_mfma_f32_32x32x16_f16 per product tile instead of eight v_mfma_f32_32x32x2_f32: 5.3x fewer matrix-pipe cycles
// than the exact-f32 parity kernels at 22-bit operands; the dropped a_lo * w_lo term is 2^-22 relative.  The fp32
// accumulation chain of the matrix pipe is cut at every 32-channel chunk (9 taps x 32 channels = 288 terms) and the partials
// are added in a second float32 accumulator set: measured on the part against float64 dot products, this sits 4-5x closer to
// exact than one K-long chain (K = 4608: rms 1.3e-5 vs 4.5e-5 on outputs of rms 62) and as close as a float64 sum of 32-term
// partials to within 1.5x — i.e. at the distance from exact arithmetic of the reference's own oneDNN convolution.
//
// Weights are split once at load (pack_conv_weight_split); activations while the halo / the gather tile is written to LDS
// (v_cvt_pk_f16_f32, one subtraction: 2.5 VALU instructions per element), after the optional fused GroupNorm + SiLU
// prologue.  In LDS a pixel's 32-channel chunk is 64 B of hi halves and 64 B of lo halves: the 3x3 halo kernels pad it to 144
// bytes (SplitGeom, conv_split_common.h) and store straight from the accumulator registers (direct epilogue); the gather kernel
// keeps 128-byte rows with the 16-byte XOR swizzle of conv.hip, and its epilogue is conv_epi.h's.  The GroupNorm statistics slabs
// are the parity kernels' own.  Reference: Block.proj / res_conv / to_qkv / to_out / Downsample / Upsample, sd:583-796.
#include "conv_split_common.h"

namespace prg {

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1: halo tile in LDS (structure of conv3x3_halo_kernel, conv.hip)
// ---------------------------------------------------------------------------------------------
// Tiles of 128 pixels x 64 channels, four waves, one 32-pixel x 64-channel wave tile each; two workgroups per CU.
//   * software pipeline: body(tap) = { wait + barrier | stage one pass of the NEXT chunk's halo | prefetch the weight tile
//     NS taps ahead | issue the twelve fragment loads of the NEXT tap into the other register set | twelve MFMAs of THIS tap };
//     the loads and the staging arithmetic do not feed the MFMAs behind them, so they run in the matrix pipe's shadow;
//   * the nine taps of a chunk are unrolled with the tap a compile-time constant: halo rows are 144 bytes (128 + 16 of
//     padding: conflict-free ds_read_b128 without an XOR swizzle, as in conv_w256.hip), so every fragment address is one
//     per-lane base register + an immediate; the weight ring slot (tap % 3) and the staging pass are constants too —
//     the instruction diet that took the loop from 8 VALU + 6 SALU per MFMA to ~2;
//   * the halo is DOUBLE-BUFFERED in LDS and staged incrementally (pass k of the next chunk loaded at tap k, converted and
//     written at tap k + 1): eight staging registers instead of the whole halo's 32-48;
//   * weight tiles go global -> LDS directly (global_load_lds_dwordx4: no staging registers, no ds_write pass) into a ring
//     of NS slots, with counted vmcnt waits so that the newest prefetch stays in flight across the barrier.
// History of the round (level-0 launch, 77 GFLOP): 64 x 64 wave tiles at 256 registers spilled the weight prefetch inside
// the loop (409 us); three workgroups per CU at 168 registers with just-in-time fragment loads 284 us — and 209 us with the
// MFMAs compiled out: MFMA 105 + LDS reads 53 + L1/TA 47 + split 21 + epilogue 48 us simply added up, identical workgroups
// run in lockstep and overlap nothing; the first pipelined version 345 us at 8 VALU + 6 SALU instructions per MFMA
// (rocprofv3 SQ_INSTS_*: address arithmetic and tap bookkeeping); this structure: DESIGN.md section 4.6.

template <int TH, int TW, int NS>
__global__ __launch_bounds__(256, 2) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3x3_split_kernel(
    const ConvLaunch<float> L, const int tiles_x, const int tiles_y, const int tiles_n, const int fuse_stats) {
  constexpr int NW = 4, BN = 64;
  constexpr int CH = 32;                       // channels per chunk: one LDS row = 64 B of hi halves + 64 B of lo halves
  using G = SplitGeom<TH, TW>;                 // 256 staging threads: NH passes of 64 halo pixels per chunk
  constexpr int HP = G::HP, HALO = G::HALO, PITCH = G::PITCH, RSTRIDE = G::RSTRIDE, HBYTES = G::HBYTES, NH = G::NH;
  constexpr int WPW = BN / 8 / NW;             // global_load_lds wave-instructions (8 rows each) per wave and weight tile
  constexpr int DIST = 8 - NH;                 // taps between a staging pass's load and its conversion / LDS write (last write at tap 7:
                                               // tap 8's body already issues the next chunk's first fragment loads)
  static_assert(TH * TW == 128 && NH <= 4 && (NS == 2 || NS == 3), "tile");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Ah = smem;                                 // [2][HALO] rows of PITCH bytes: units 0-3 hi, 4-7 lo
  char* const Bs = smem + 2 * HBYTES;                    // [NS][64][128 B], 16-byte units XOR-swizzled by (row >> 1) & 7

  const ConvDesc& d = L.d;
  const int nblk = tiles_x * tiles_y * tiles_n * d.B;
  // Tile decode (written out in halo, ws and w512: as a call it reorders the entry block's scalar code).  Workgroup b runs on XCD
  // b % 8 (observed).  With 2 / 4 / 8 output-channel tiles every XCD is pinned to ONE of them, so its 4 MB L2 holds that tile's
  // weight slice (512 -> 512: 1.2 MB of the 9.4 MB set) instead of streaming it all; otherwise contiguous runs of tiles (xcd_remap).
  int tn, lin;
  if (tiles_n > 1 && 8 % tiles_n == 0 && nblk % 8 == 0) {
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, per = 8 / tiles_n;
    tn = xcd % tiles_n;
    lin = idx * per + xcd / tiles_n;
  } else {
    lin = xcd_remap(blockIdx.x, nblk);
    tn = lin % tiles_n;
    lin /= tiles_n;
  }
  const int tx = lin % tiles_x; lin /= tiles_x;
  const int ty = lin % tiles_y;
  const int b = lin / tiles_y;
  const int y0 = ty * TH, x0 = tx * TW;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nchunks = (d.C0 + d.C1) / CH;
  const int Hl = d.Hout, Wl = d.Wout;
  const int q = tid & 3, prow = tid >> 2;      // this thread stages channels q * 8 .. + 7 of halo pixels prow + 64 k

  int hsrc[NH];                                // source pixel index (or -1: padding / beyond the halo)
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const int hp = prow + k * 64;
    hsrc[k] = -1;
    if (hp < HALO) {
      const int hy = hp / HP, hx = hp - hy * HP;
      hsrc[k] = halo_source(d, b, y0 - 1 + hy, x0 - 1 + hx, Hl, Wl, d.ups);
    }
  }
  // fragment addresses: one per-lane base each, everything else immediate
  const int pix = wave * 32 + l31;
  const int a_lane = (pix / TW) * RSTRIDE + (pix % TW) * PITCH + hi * 16;         // + buffer + tap offset + step * 32 (+ 64: lo)
  int b_lane[2][2];                                                                // [step][hi / lo], + ring slot + j * 4096
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const int sw = (l31 >> 1) & 7, unit = 2 * st + hi;
    b_lane[st][0] = l31 * 128 + ((unit ^ sw) << 4);
    b_lane[st][1] = l31 * 128 + (((4 + unit) ^ sw) << 4);
  }
  int w_lane[NH];                                                                  // staging write address of pass k (+ 64: lo)
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const int hp = prow + k * 64;
    w_lane[k] = (hp / HP) * RSTRIDE + (hp % HP) * PITCH + q * 16;
  }

  // one staging pass: load (global -> registers) and, one tap later, prologue + split + write (registers -> LDS)
  float4 hh0[NH], hh1[NH];                     // one register pair per pass: a pass is written DIST taps after its load
  auto halo_load = [&](int chunk, auto K) {   // (chunk_source + load_unit written out: as calls they reorder this kernel's listing)
    constexpr int k = decltype(K)::value;
    const int c = chunk * CH + q * 8;
    const bool first = c < d.C0;
    const float* base = first ? L.src0 : L.src1;
    const int Cs = first ? d.C0 : d.C1, cc = first ? c : c - d.C0;
    const float4* p = reinterpret_cast<const float4*>(base + (hsrc[k] >= 0 ? (size_t)hsrc[k] * Cs + cc : (size_t)0));
    hh0[k] = p[0];
    hh1[k] = p[1];
  };
  float pa[8], pb[8];                          // fused prologue coefficients of this thread's 8 channels (chunk being staged)
  auto pro_load = [&](int chunk) {
    if (L.pro_a) load_pro8(L.pro_a + (size_t)b * d.C0 + chunk * CH + q * 8, L.pro_b + (size_t)b * d.C0 + chunk * CH + q * 8, pa, pb);
  };
  auto halo_write = [&](int buf, auto K) {
    constexpr int k = decltype(K)::value;
    if (k * 64 + 63 < HALO || prow + k * 64 < HALO)
      finish_unit(hh0[k], hh1[k], L.pro_a != nullptr, pa, pb, hsrc[k] < 0, Ah + buf * HBYTES + w_lane[k]);
  };

  // weight tiles: LDS-DMA, lane-linear destination, the XOR swizzle on the per-lane source address (conv_split_common.h)
  const char* wtile = reinterpret_cast<const char*>(L.w_split + (size_t)tn * BN * 64);
  const size_t wstep = (size_t)d.CoutPad * 128;                                   // bytes between (tap, chunk) tiles
  int wsrc[WPW];
#pragma unroll
  for (int r = 0; r < WPW; ++r) {
    wsrc[r] = swizzled_unit((wave * WPW + r) * 8 + (lane >> 3), lane & 7);
  }
  auto gload_b = [&](int chunk, int tap, int slot) {
    const char* p = wtile + (size_t)(tap * L.split_kchunks + chunk) * wstep;
#pragma unroll
    for (int r = 0; r < WPW; ++r) weight_dma_rows(p + wsrc[r], Bs + (slot * BN + (wave * WPW + r) * 8) * 128);
  };

  f32x16 acc[1][2], tot[1][2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc[0][j][e] = 0.0f; tot[0][j][e] = 0.0f; }

  const int niter = nchunks * 9;
  // weight tiles 0 .. NS - 1 and chunk 0's halo (all passes in flight at once: one HBM latency per tile, not NH)
#pragma unroll
  for (int t = 0; t < NS; ++t)
    if (t < niter) gload_b(t / 9, t % 9, t);
  pro_load(0);
  {
    float4 g0[NH], g1[NH];
    const bool first = q * 8 < d.C0;
    const float* base = first ? L.src0 : L.src1;
    const int Cs = first ? d.C0 : d.C1, cc = first ? q * 8 : q * 8 - d.C0;
#pragma unroll
    for (int k = 0; k < NH; ++k) {
      if (hsrc[k] >= 0) {
        const float4* p = reinterpret_cast<const float4*>(base + (size_t)hsrc[k] * Cs + cc);
        g0[k] = p[0];
        g1[k] = p[1];
      } else {
        g0[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        g1[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    auto wr = [&](auto K) {
      hh0[decltype(K)::value] = g0[decltype(K)::value];
      hh1[decltype(K)::value] = g1[decltype(K)::value];
      halo_write(0, K);
    };
    wr(IC<0>()); wr(IC<1>()); wr(IC<2>());
    if constexpr (NH > 3) wr(IC<3>());
    if constexpr (NH > 4) wr(IC<4>());
    if constexpr (NH > 5) wr(IC<5>());
    if constexpr (NH > 6) wr(IC<6>());
  }

  f16x8 fa[2][2][2], fw[2][2][4];               // [register set][k16 step][A: hi, lo | W: (hi, lo) x column tile]
  // fragment loads of (chunk buffer cb, tap T) into register set S; ring slot T % NS (9 taps per chunk and NS = 3) or runtime
  auto reads = [&](auto SET, auto TAP, int cb, int slot) {
    constexpr int S = decltype(SET)::value, T = decltype(TAP)::value;
    const char* A = Ah + cb * HBYTES + a_lane + G::tap(T);
    const char* Bb = Bs + slot * (BN * 128);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      fa[S][st][0] = ld_frag(reinterpret_cast<const uint4*>(A + st * 32));
      fa[S][st][1] = ld_frag(reinterpret_cast<const uint4*>(A + st * 32 + 64));
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        fw[S][st][2 * j] = ld_frag(reinterpret_cast<const uint4*>(Bb + b_lane[st][0] + j * 4096));
        fw[S][st][2 * j + 1] = ld_frag(reinterpret_cast<const uint4*>(Bb + b_lane[st][1] + j * 4096));
      }
    }
  };
  auto mfmas = [&](auto SET) {
    constexpr int S = decltype(SET)::value;
#pragma unroll
    for (int st = 0; st < 2; ++st) mfma3<1>(fa[S][st], fw[S][st], acc);
  };

  // one tap of chunk c; P = parity of the chunk (register set of tap T = (T + P) & 1)
  auto body = [&](auto PAR, auto TAP, int c) {
    constexpr int P = decltype(PAR)::value, T = decltype(TAP)::value, S = (T + P) & 1;
    const int it = c * 9 + T;
    const bool more = c + 1 < nchunks;
    // (1) all but the newest weight prefetch (tile it + 2, issued by the previous body AFTER its halo pass) have landed — tile
    //     it + 1 in particular, and that halo pass; this wave's fragment loads of `it` and staging ds_writes are done.
    //     A RAW s_barrier: __syncthreads() makes hipcc drain vmcnt(0) in front of it while an LDS-DMA is in flight, i.e. a
    //     prefetch distance of zero.  The asm's memory clobber keeps LDS accesses on their side of it.  hipcc floats this
    //     tap's MFMAs (register-only) to just behind the barrier, in front of the staging code: measured the best order —
    //     pinning them in front of the wait (accumulators as asm operands) cost 20-35 % (355 / 395 us against 286 us at
    //     level 0): the wave then issues nothing else for 384 cycles and meets the barrier late.
    if (NS == 3 && (T + 2 < 9 || more)) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(WPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    // tile it + 1 is visible; nobody still reads tile it's ring slot or the previous chunk's halo
    if (more) {
      // (2) the next chunk's halo, one pass per tap: written one tap after its load, into the other halo buffer
      //     (loaded at taps 0 .. NH - 1, written DIST taps later: the loads come from HBM — ~2 us, two to four taps)
      if constexpr (T == 0) pro_load(c + 1);
      if constexpr (T >= DIST && T < DIST + NH) halo_write((c + 1) & 1, IC<T - DIST>());
      if constexpr (T < NH) halo_load(c + 1, IC<T>());
    }
    // (3) weight tile it + NS into the slot tile `it` just vacated
    if constexpr (T + NS < 9) gload_b(c, T + NS, NS == 3 ? T % 3 : it & 1);
    else if (more) gload_b(c + 1, T + NS - 9, NS == 3 ? T % 3 : it & 1);
    // (4) fragments of the next tap into the other register set, (5) the MFMAs of this tap
    if constexpr (T < 8) reads(IC<1 - S>(), IC<T + 1>(), c & 1, NS == 3 ? (T + 1) % 3 : (it + 1) & 1);
    else if (more) reads(IC<1 - S>(), IC<0>(), (c + 1) & 1, NS == 3 ? 0 : (it + 1) & 1);
    mfmas(IC<S>());
    if constexpr (T == 8) flush_acc<1>(acc, tot);   // the 288-term partial of this channel chunk
  };
  auto chunk_body = [&](auto PAR, int c) {
    body(PAR, IC<0>(), c); body(PAR, IC<1>(), c); body(PAR, IC<2>(), c);
    body(PAR, IC<3>(), c); body(PAR, IC<4>(), c); body(PAR, IC<5>(), c);
    body(PAR, IC<6>(), c); body(PAR, IC<7>(), c); body(PAR, IC<8>(), c);
  };

  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  reads(IC<0>(), IC<0>(), 0, 0);
  for (int c = 0; c < nchunks; c += 2) {
    chunk_body(IC<0>(), c);
    if (c + 1 < nchunks) chunk_body(IC<1>(), c + 1);
  }

  if (L.split_scale) {                         // undo the packer's per-channel power-of-two weight scale (exact)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float sc = L.split_scale[tn * BN + j * 32 + l31];
#pragma unroll
      for (int e = 0; e < 16; ++e) tot[0][j][e] *= sc;
    }
  }
  // DIRECT epilogue: the accumulator layout already has lanes 0-31 = 32 consecutive channels of ONE pixel (register e of half hi
  // is pixel row (e & 3) + 8 (e >> 2) + 4 hi), so a dword store per register writes two full 128-byte lines per wave-instruction —
  // no LDS transpose, no barrier; the GroupNorm partial sums come from lane reductions (a group's channels are adjacent lanes).
  {
    const int cpg = L.gn_groups > 0 ? d.Cout / L.gn_groups : 8;
    float sj[2], qj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch = tn * BN + j * 32 + l31;
      const float bv = L.bias ? L.bias[ch] : 0.0f;
      float s1 = 0.0f, q1 = 0.0f;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int p = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
        const size_t m = ((size_t)b * d.Hout + y0 + p / TW) * d.Wout + x0 + p % TW;
        const float v = tot[0][j][e] + bv;
        L.out[m * d.Cout + ch] = v;
        s1 += v;
        q1 = fmaf(v, v, q1);
      }
      sj[j] = s1;
      qj[j] = q1;
    }
    if (fuse_stats) {
      // a lane holds (sum, sumsq) of ONE channel over its 16 pixels: fold the two pixel halves, then the cpg adjacent channels
      double* red = reinterpret_cast<double*>(smem + 2 * HBYTES + NS * BN * 128);      // [4 waves][2 j][4][2] beyond the images
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        double sd = (double)sj[j], qd = (double)qj[j];
        sd += __shfl_xor(sd, 32, 64);
        qd += __shfl_xor(qd, 32, 64);
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {                 // the 8 channels of a granule are 8 adjacent lanes
          sd += __shfl_xor(sd, o, 64);
          qd += __shfl_xor(qd, o, 64);
        }
        if (hi == 0 && (l31 & 7) == 0) {                  // (8-channel granules: cpg is a multiple of 8 on this path)
          red[((wave * 2 + j) * 4 + (l31 >> 3)) * 2] = sd;
          red[((wave * 2 + j) * 4 + (l31 >> 3)) * 2 + 1] = qd;
        }
      }
      __syncthreads();
      // groups of this tile's 64 channels: 64 / cpg of them; thread g sums the four waves (fixed order) and the granules of a group
      const int ng = 64 / cpg;
      if (tid < ng) {
        const int gran0 = tid * (cpg / 8), ngran = cpg / 8;
        double ss = 0, qq = 0;
        for (int w = 0; w < 4; ++w)
          for (int k = 0; k < ngran; ++k) {
            const int gr = gran0 + k;                       // granule 0..7 of the tile: column tile gr >> 2, lanes 8 (gr & 3) .. + 7
            ss += red[((w * 2 + (gr >> 2)) * 4 + (gr & 3)) * 2];
            qq += red[((w * 2 + (gr >> 2)) * 4 + (gr & 3)) * 2 + 1];
          }
        const int nsplit = tiles_x * tiles_y;
        float* dst = L.gn_partials + ((size_t)b * nsplit + ty * tiles_x + tx) * L.gn_groups * 2;
        const int g = (tn * BN) / cpg + tid;
        dst[g * 2] = (float)ss;
        dst[g * 2 + 1] = (float)qq;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1, Cout % 128 == 0: the WAVE-SPECIALISED form (second half of round 4)
// ---------------------------------------------------------------------------------------------
// The symmetric kernel above is LDS-read bound at one ds_read_b128 per MFMA (32 x 64 wave tiles: larger ones do not fit its 256
// registers beside the staging state) and its two identical workgroups per CU run in lockstep.  Here a 512-thread workgroup owns
// a CU and its waves have DIFFERENT jobs, so the phases really overlap:
//   waves 0-3  CONSUMERS, one per SIMD: 64 pixels x 64 channels each (2 x 2 over the 128-pixel x 128-channel tile): per tap 16
//              fragment loads for 24 MFMAs (0.67 per MFMA), double-buffered per k16 step — step 1's fragments load beside step
//              0's MFMAs, the NEXT tap's step 0 beside step 1's; they never touch global memory, never convert, and their
//              barrier carries no wait at all;
//   waves 4-5  HALO producers: all passes of the next chunk's halo loaded at tap 0 (48 registers: they have no accumulators),
//              prologue + split + ds_write at taps 2-7 into the other halo buffer;
//   waves 6-7  WEIGHT producers: global_load_lds of tile t + 3 into a ring of four, `s_waitcnt vmcnt(8)` = tile t + 2 landed.
//              Their own waves because vmcnt retires IN ORDER: behind the halo's HBM loads a counted wait on the weight
//              prefetch would wait for HBM.
// One raw s_barrier per tap for the eight waves; invariant at barrier(t): weight tiles t and t + 1 are in LDS (so a consumer may
// fetch tile t + 1's first fragments before barrier(t + 1)), tile t - 1's slot is free.  The epilogue is wave-local (each
// consumer transposes its own tile through a private LDS stage; GroupNorm partial sums per (tile, pixel half) slab): no
// workgroup barrier after the one that ends the main loop.
// UP (round 4, second half): Upsample = nearest x2 + 3 x 3 conv as four 2 x 2-tap sub-pixel convolutions of the SOURCE image
// (conv_w256.hip MODE 2 / DESIGN 4.8 for the algebra): a tile is 128 source pixels x one phase (dy, dx) = the two low bits of the
// tile index, NT = 4 taps per chunk from the phase's own split packing (L.w_up_split), the phase's window starts at halo position
// (dy, dx), the epilogue stores to (2 y + dy, 2 x + dx).  With four taps per chunk a halo pass would have ONE tap between its
// load and its conversion, so the halo producers run two chunks ahead (two register sets).
template <int NS, bool UP>
__global__ __launch_bounds__(512, 1) void conv3x3_split_ws_kernel(const ConvLaunch<float> L, const int tiles_x, const int tiles_y,
                                                                  const int tiles_n, const int fuse_stats) {
  constexpr int TH = 8, TW = 16, BN = 128, CH = 32;
  constexpr int NT = UP ? 4 : 9;                         // taps per channel chunk
  using G = SplitGeom<TH, TW, 128>;                      // 128 halo-producer threads: six staging passes
  constexpr int HP = G::HP, HALO = G::HALO, PITCH = G::PITCH, RSTRIDE = G::RSTRIDE, HBYTES = G::HBYTES, NHP = G::NH;
  constexpr int WPW = BN / 8 / 2;                        // global_load_lds instructions per weight-producer wave and tile (8)
  static_assert(NS == 4 && NHP <= 6, "ring");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Ah = smem;                                 // [2][HALO] rows of PITCH bytes
  char* const Bs = smem + 2 * HBYTES;                    // [NS][128][128 B], units XOR-swizzled by (row >> 1) & 7

  const ConvDesc& d = L.d;
  const int nblk = tiles_x * tiles_y * tiles_n * d.B * (UP ? 4 : 1);
  int tn, lin;
  if (tiles_n > 1 && 8 % tiles_n == 0 && nblk % 8 == 0) {  // every XCD pinned to one output-channel tile (its weight slice stays in L2)
    const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, per = 8 / tiles_n;
    tn = xcd % tiles_n;
    lin = idx * per + xcd / tiles_n;
  } else {
    lin = xcd_remap(blockIdx.x, nblk);
    tn = lin % tiles_n;
    lin /= tiles_n;
  }
  const int ph = UP ? lin & 3 : 0;                       // sub-pixel phase 2 dy + dx
  if (UP) lin >>= 2;
  const int tx = lin % tiles_x; lin /= tiles_x;
  const int ty = lin % tiles_y;
  const int b = lin / tiles_y;
  const int y0 = ty * TH, x0 = tx * TW;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nchunks = (d.C0 + d.C1) / CH, niter = nchunks * NT;
  const size_t wstep = (size_t)d.CoutPad * 128;
  const char* wtile = UP ? reinterpret_cast<const char*>(L.w_up_split + (size_t)ph * 4 * L.split_kchunks * d.CoutPad * 64 + (size_t)tn * BN * 64)
                         : reinterpret_cast<const char*>(L.w_split + (size_t)tn * BN * 64);
  const int Hs = UP ? d.Hin : d.Hout, Ws = UP ? d.Win : d.Wout;   // the image the tiles cover (UP: the source)

  if (wave >= 6) {
    // ------------------------------------------------ weight producers ------------------------------------------------
    const int pw = wave - 6;
    int wsrc[WPW];
#pragma unroll
    for (int r = 0; r < WPW; ++r) {
      wsrc[r] = swizzled_unit((pw * WPW + r) * 8 + (lane >> 3), lane & 7);
    }
    auto gload_b = [&](int it) {
      const int c = it / NT, tap = it - NT * c;
      const char* p = wtile + (size_t)(tap * L.split_kchunks + c) * wstep;
      char* dst = Bs + ((it & (NS - 1)) * BN + pw * WPW * 8) * 128;
      weight_dma<WPW>(p, wsrc, dst);
    };
    gload_b(0);
    if (niter > 1) gload_b(1);
    if (niter > 2) gload_b(2);
    // tiles 0 and 1 landed (tile 2 may fly on)
    if (niter > 2) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(WPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    for (int it = 0; it < niter; ++it) {
      if (it + 3 < niter) {
        gload_b(it + 3);                                   // into tile it - 1's slot, free since barrier(it)
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(WPW) : "memory");   // tile it + 2 landed -> barrier(it + 1)
      } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      }
    }
    return;
  }
  if (wave >= 4) {
    // ------------------------------------------------- halo producers -------------------------------------------------
    const int pt = tid - 256, q = pt & 3, prow = pt >> 2;  // channels q * 8 .. + 7 of halo pixels prow + 32 k
    int hsrc[NHP];
#pragma unroll
    for (int k = 0; k < NHP; ++k) {
      const int hp = prow + k * 32;
      hsrc[k] = -1;
      if (hp < HALO) {
        const int hy = hp / HP, hx = hp - hy * HP;
        hsrc[k] = halo_source(d, b, y0 - 1 + hy, x0 - 1 + hx, Hs, Ws, !UP && d.ups);
      }
    }
    float4 gA0[NHP], gA1[NHP], gB0[NHP], gB1[NHP];        // (UP: two chunks in flight; otherwise only set A)
    auto load_chunk_set = [&](int chunk, float4 (&g0)[NHP], float4 (&g1)[NHP]) {
      const ChunkSrc s = chunk_source(L, chunk * CH + q * 8);
#pragma unroll
      for (int k = 0; k < NHP; ++k) load_unit(s, hsrc[k], g0[k], g1[k]);
    };
    auto load_chunk = [&](int chunk) { load_chunk_set(chunk, gA0, gA1); };
    float pa[8], pb[8];
    auto pro_load = [&](int chunk) {
      if (L.pro_a) load_pro8(L.pro_a + (size_t)b * d.C0 + chunk * CH + q * 8, L.pro_b + (size_t)b * d.C0 + chunk * CH + q * 8, pa, pb);
    };
    auto write_pass_set = [&](int buf, auto K, const float4 (&h0)[NHP], const float4 (&h1)[NHP]) {
      constexpr int k = decltype(K)::value;
      const int hp = prow + k * 32;
      if (hp < HALO) {                                     // (finish_unit written out: as a call + 9 / + 11 instructions in this kernel)
        float v[8] = {h0[k].x, h0[k].y, h0[k].z, h0[k].w, h1[k].x, h1[k].y, h1[k].z, h1[k].w};
        if (L.pro_a) {
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = fast_silu(fmaf(v[u], pa[u], pb[u]));
        }
        if (hsrc[k] < 0) {
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = 0.0f;
        }
        uint4 vh, vl;
        if (L.pro_a) split8<false>(v, vh, vl);
        else split8(v, vh, vl);
        char* p = Ah + buf * HBYTES + (hp / HP) * RSTRIDE + (hp % HP) * PITCH + q * 16;
        *reinterpret_cast<uint4*>(p) = vh;
        *reinterpret_cast<uint4*>(p + 64) = vl;
      }
    };
    auto write_pass = [&](int buf, auto K) { write_pass_set(buf, K, gA0, gA1); };
    if constexpr (UP) {
      // Upsample convs have no fused prologue (pro_a is null: checked by the launcher).  Chunk c + 2 is loaded at tap 0 of chunk c
      // into the register set of its parity, chunk c + 1 (loaded four taps earlier) is converted and written at taps 0-2, two
      // passes each; tap 3: nothing (the consumers fetch the next chunk's first fragments during it).
      load_chunk_set(0, gA0, gA1);
      if (nchunks > 1) load_chunk_set(1, gB0, gB1);
      write_pass_set(0, IC<0>(), gA0, gA1); write_pass_set(0, IC<1>(), gA0, gA1); write_pass_set(0, IC<2>(), gA0, gA1);
      write_pass_set(0, IC<3>(), gA0, gA1); write_pass_set(0, IC<4>(), gA0, gA1); write_pass_set(0, IC<5>(), gA0, gA1);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      auto chunk_taps = [&](int c, float4 (&n0)[NHP], float4 (&n1)[NHP], float4 (&f0)[NHP], float4 (&f1)[NHP]) {
        // n = the set holding chunk c + 1 (to be written now), f = the set chunk c held (free: reloaded with chunk c + 2)
        const bool more = c + 1 < nchunks;
        const int nb = (c + 1) & 1;
        if (c + 2 < nchunks) load_chunk_set(c + 2, f0, f1);
        if (more) { write_pass_set(nb, IC<0>(), n0, n1); write_pass_set(nb, IC<1>(), n0, n1); }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");         // -> barrier(4 c + 1)
        if (more) { write_pass_set(nb, IC<2>(), n0, n1); write_pass_set(nb, IC<3>(), n0, n1); }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");         // -> barrier(4 c + 2)
        if (more) { write_pass_set(nb, IC<4>(), n0, n1); write_pass_set(nb, IC<5>(), n0, n1); }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");         // -> barrier(4 c + 3)
        asm volatile("s_barrier" ::: "memory");                                   // -> barrier(4 c + 4)
      };
      for (int c = 0; c < nchunks; c += 2) {
        chunk_taps(c, gB0, gB1, gA0, gA1);
        if (c + 1 < nchunks) chunk_taps(c + 1, gA0, gA1, gB0, gB1);
      }
      return;
    }
    pro_load(0);
    load_chunk(0);
    write_pass(0, IC<0>()); write_pass(0, IC<1>()); write_pass(0, IC<2>());
    write_pass(0, IC<3>()); write_pass(0, IC<4>()); write_pass(0, IC<5>());
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    for (int c = 0; c < nchunks; ++c) {
      const bool more = c + 1 < nchunks;
      const int nb = (c + 1) & 1;
      // tap 0: the next chunk's coefficients and ALL its halo loads; taps 2 .. 7: one pass each converted and written (the
      // other halo buffer was last read during the previous chunk's tap 8, i.e. before barrier(9 c)); tap 8: nothing —
      // the consumers fetch the next chunk's first fragments during it
      if (more) { pro_load(c + 1); load_chunk(c + 1); }
      asm volatile("s_barrier" ::: "memory");                                   // -> barrier(9 c + 1)
      asm volatile("s_barrier" ::: "memory");                                   // -> barrier(9 c + 2)
      if (more) write_pass(nb, IC<0>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) write_pass(nb, IC<1>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) write_pass(nb, IC<2>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) write_pass(nb, IC<3>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) write_pass(nb, IC<4>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) write_pass(nb, IC<5>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");           // -> barrier(9 c + 8)
      asm volatile("s_barrier" ::: "memory");                                   // -> barrier(9 c + 9)
    }
    return;
  }
  // ---------------------------------------------------- consumers -----------------------------------------------------
  const int l31 = lane & 31, hi = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  int a_lane[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pix = wm * 64 + i * 32 + l31;
    a_lane[i] = (pix / TW) * RSTRIDE + (pix % TW) * PITCH + hi * 16;
  }
  int b_lane[2][2];
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const int sw = (l31 >> 1) & 7, unit = 2 * st + hi;
    b_lane[st][0] = wn * 8192 + l31 * 128 + ((unit ^ sw) << 4);
    b_lane[st][1] = wn * 8192 + l31 * 128 + (((4 + unit) ^ sw) << 4);
  }
  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.0f; tot[i][j][e] = 0.0f; }
  f16x8 fa[2][4], fw[2][4];                              // [k16 step][A: (hi, lo) x row tile | W: (hi, lo) x column tile]
  const int pho = UP ? (ph >> 1) * RSTRIDE + (ph & 1) * PITCH : 0;   // UP: the phase's 2 x 2 window starts at halo position (dy, dx)
  auto reads = [&](auto ST, auto TAP, int cb, int slot) {
    constexpr int st = decltype(ST)::value, T = decltype(TAP)::value;
    constexpr int toff = UP ? G::tap_up(T) : G::tap(T);
    consumer_reads(Ah + cb * HBYTES + toff + st * 32 + pho, Bs + slot * (BN * 128), a_lane, b_lane[st], fa[st], fw[st]);
  };
  auto mfmas = [&](auto ST) { mfma3<2>(fa[decltype(ST)::value], fw[decltype(ST)::value], acc); };
  auto body = [&](auto TAP, int c) {
    constexpr int T = decltype(TAP)::value;
    const int it = c * NT + T;
    const bool more = c + 1 < nchunks;
    // barrier #it (tap 0 runs straight after the prologue's barrier #0): weight tiles it, it + 1 are in LDS, tile it - 1's slot
    // is free for the producers, this chunk's halo is complete.  No wait: a consumer's outstanding fragment loads read only
    // images that stay valid for another tap.
    if (T > 0 || c > 0) asm volatile("s_barrier" ::: "memory");
    // one fragment read in each of the first eight MFMA shadows instead of eight reads in a row behind the twelfth MFMA: the four
    // consumers are barrier-aligned, so a burst is 32 ds_read_b128 at once on the CU's LDS port (4 cycles each) against one
    // 32-cycle MFMA of cover
    __builtin_amdgcn_sched_barrier(0);
    reads(IC<1>(), TAP, c & 1, it & (NS - 1));
    mfmas(IC<0>());
    interleave_8_reads_12_mfmas();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (T < NT - 1) reads(IC<0>(), IC<(T + 1) % NT>(), c & 1, (it + 1) & (NS - 1));
    else if (more) reads(IC<0>(), IC<0>(), (c + 1) & 1, (it + 1) & (NS - 1));
    mfmas(IC<1>());
    interleave_8_reads_12_mfmas();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (T == NT - 1) flush_acc<2>(acc, tot);
  };
  asm volatile("s_barrier" ::: "memory");                // the producers' prologue: chunk 0's halo, weight tiles 0 and 1
  reads(IC<0>(), IC<0>(), 0, 0);
  for (int c = 0; c < nchunks; ++c) {
    body(IC<0>(), c); body(IC<1>(), c); body(IC<2>(), c); body(IC<3>(), c);
    if constexpr (!UP) {
      body(IC<4>(), c); body(IC<5>(), c); body(IC<6>(), c); body(IC<7>(), c); body(IC<8>(), c);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(niter): every consumer is done with the LDS images
  // DIRECT epilogue (as in the symmetric kernel): register e of lane half hi is pixel row (e & 3) + 8 (e >> 2) + 4 hi, lanes 0-31
  // are 32 consecutive channels: a dword store per register writes two full 128-byte lines per wave-instruction; GroupNorm partial
  // sums by lane reductions (a group's channels are adjacent lanes), one slab per (tile, pixel half): no LDS, no barrier.
  {
    const int cpg = L.gn_groups > 0 ? d.Cout / L.gn_groups : 64;          // 16, 32 or 64 when the statistics are fused
    double sd[2], qd[2];
    // Addresses (round 5): pixel p = 64 wm + 32 i + (e & 3) + 8 (e >> 2) + 4 hi of the 16-wide tile is tile row 4 wm + 2 i + (e >> 3),
    // column (e & 3) + 8 ((e >> 2) & 1) + 4 hi: a WAVE-UNIFORM 64-bit tile base (scalar registers) + a 32-bit per-lane offset + uniform
    // per-store terms (row step, pixel step) — one vector add per store.  The generic form (m * d.Cout + ch per element in 64 bits)
    // cost ~350 of the epilogue's ~620 VALU instructions per wave, 140 of them quarter-rate integer multiplies.
    const size_t ps = (size_t)d.Cout * (UP ? 2 : 1);                       // floats between the lane's consecutive tile columns
    const size_t rs = (size_t)d.Wout * d.Cout * (UP ? 2 : 1);              // ... and tile rows
    float* const lbase = L.out + (UP ? (((size_t)b * d.Hout + 2 * (y0 + wm * 4) + (ph >> 1)) * d.Wout + 2 * x0 + (ph & 1)) * d.Cout
                                     : (((size_t)b * d.Hout + y0 + wm * 4) * d.Wout + x0) * d.Cout) + tn * BN + wn * 64 + (size_t)(4 * hi) * ps + l31;
    float bv[2], sc[2], s1[2] = {0.0f, 0.0f}, q1[2] = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch = tn * BN + wn * 64 + j * 32 + l31;
      bv[j] = L.bias ? L.bias[ch] : 0.0f;
      const float* scp = UP ? L.split_scale_up : L.split_scale;            // the packer's per-channel power of two, undone (exact)
      sc[j] = scp ? scp[(UP ? ph * d.CoutPad : 0) + ch] : 1.0f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        float* const cp = lbase + (size_t)(2 * i + (e >> 3)) * rs + (size_t)((e & 3) + 8 * ((e >> 2) & 1)) * ps;   // (uniform offsets)
#pragma unroll
        for (int j = 0; j < 2; ++j) {                                      // (per j the values are summed in the same (i, e) order as before)
          const float v = tot[i][j][e] * sc[j] + bv[j];
          cp[j * 32] = v;
          s1[j] += v;
          q1[j] = fmaf(v, v, q1[j]);
        }
      }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      sd[j] = (double)s1[j];
      qd[j] = (double)q1[j];
    }
    if (fuse_stats) {
      const int width = cpg < 32 ? cpg : 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sd[j] += __shfl_xor(sd[j], 32, 64);
        qd[j] += __shfl_xor(qd[j], 32, 64);
        for (int o = 1; o < width; o <<= 1) {
          sd[j] += __shfl_xor(sd[j], o, 64);
          qd[j] += __shfl_xor(qd[j], o, 64);
        }
      }
      const int nsplit = tiles_x * tiles_y * 2;
      float* slab = L.gn_partials + ((size_t)b * nsplit + (ty * tiles_x + tx) * 2 + wm) * L.gn_groups * 2;
      if (cpg == 64) {
        if (lane == 0) {
          const int g = (tn * BN + wn * 64) / 64;
          slab[g * 2] = (float)(sd[0] + sd[1]);
          slab[g * 2 + 1] = (float)(qd[0] + qd[1]);
        }
      } else if (hi == 0 && (l31 & (width - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int g = (tn * BN + wn * 64 + j * 32 + l31) / cpg;
          slab[g * 2] = (float)sd[j];
          slab[g * 2 + 1] = (float)qd[j];
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1, Cout = 64: the PERSISTENT wave-specialised form (round 5) — levels 0 / 1 and the narrow Upsample
// ---------------------------------------------------------------------------------------------
// The 64-channel convolutions (64 -> 64, the two-source 128 -> 64 of the up path, Upsample 128 -> 64: sixteen launches per
// evaluation, 29 % of the f16x3 mode's time) ran on the symmetric kernel at 0.33-0.41 MFMA-busy: with K = 576 a tile is 18 taps
// and a one-tile workgroup exposes its first halo's HBM latency and its epilogue, which only two co-resident (lock-step,
// LDS-read-bound) workgroups hid.  Here ONE 512-thread workgroup per CU walks a strided list of 16 x 16-pixel x 64-channel tiles
// with conv3x3_split_ws_kernel's division of labour, and the pipelines never drain between tiles:
//   waves 0-3  CONSUMERS, 64 pixels (four tile rows) x 64 channels each: per tap 16 fragment loads for 24 MFMAs, double-buffered
//              per k16 step; after a tile's last tap they run the direct epilogue (scale, bias, GroupNorm partial sums per
//              (tile, wave) slab, dword stores — no LDS, no barrier) while the producers are already a chunk / three taps ahead;
//   waves 4-5  HALO producers: chunk g + 1's 18 x 18 halo — of the NEXT tile when chunk g is a tile's last — loaded at tap 0 of
//              chunk g (eleven passes, 88 staging registers), prologue + split + ds_write two passes per tap at taps 2-7;
//   waves 6-7  WEIGHT producers: the (tap, chunk) tile sequence simply repeats per pixel tile (K = 576: 18 tiles of 8 KB, L2
//              resident), LDS-DMA three taps ahead into a ring of four, counted vmcnt.
// One raw s_barrier per tap for the eight waves, numbered through the whole tile list (invariants as in the kernel above);
// LDS = 2 x 50,688 (halos, 144-byte pixels, rows of 0 mod 16 slots) + 4 x 8,192 (weights) = 134,144 bytes.
// The arithmetic is the symmetric kernel's, term for term (same MFMA sequence per accumulator, 288-term partials, same epilogue
// expression): only the GroupNorm slab partition differs.
// (Round 5 also measured a MERGED-producer form — all four producer waves staging a quarter of the halo and a quarter of each weight
// tile — at 2-3 % slower, profiles/r05_p64_ablations.txt; removed in round 6.)
template <int NS>
__global__ __launch_bounds__(512, 1) void conv3x3_split_p64_kernel(const ConvLaunch<float> L, const int tiles_x, const int tiles_y,
                                                                   const int ntiles, const int fuse_stats) {
  constexpr int TH = 16, TW = 16, BN = 64, CH = 32, NT = 9;
  using G = SplitGeom<TH, TW, 128>;                      // 128 halo-producer threads: eleven staging passes
  constexpr int HP = G::HP, HALO = G::HALO, PITCH = G::PITCH, RSTRIDE = G::RSTRIDE, HBYTES = G::HBYTES, NHP = G::NH;
  constexpr int WPW = BN / 8 / 2;                        // global_load_lds instructions per weight-producer wave and tile (4)
  static_assert(NS == 4 && NHP == 11, "ring / passes");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Ah = smem;                                 // [2][18 rows of RSTRIDE bytes]
  char* const Bs = smem + 2 * HBYTES;                    // [NS][64][128 B], units XOR-swizzled by (row >> 1) & 7

  const ConvDesc& d = L.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int nchunks = (d.C0 + d.C1) / CH;
  // this workgroup's tiles: t_first + k * t_stride, k < t_count.  With a grid that is a multiple of 8, XCD x (workgroups b with
  // b % 8 = x: observed) owns a contiguous eighth of the tile list and its workgroups walk it interleaved, so tiles that share halo
  // rows run at the same time on one L2.
  int t_first, t_stride, t_count;
  {
    const int NG = (int)gridDim.x, bid = (int)blockIdx.x;
    if ((NG & 7) == 0) {
      const int xcd = bid & 7, idx = bid >> 3, per = NG >> 3;
      const int q = ntiles >> 3, r = ntiles & 7;
      const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
      const int cnt = q + (xcd < r ? 1 : 0);
      t_first = start + idx; t_stride = per; t_count = idx < cnt ? (cnt - idx + per - 1) / per : 0;
    } else {
      t_first = bid; t_stride = NG; t_count = bid < ntiles ? (ntiles - bid + NG - 1) / NG : 0;
    }
  }
  const int nchunks_total = t_count * nchunks, niter = nchunks_total * NT;
  if (niter == 0) return;                                // (uniform over the workgroup: no barrier is ever reached)
  const size_t wstep = (size_t)d.CoutPad * 128;
  const int Hs = d.Hout, Ws = d.Wout;
  const int tiles_img = tiles_x * tiles_y;

  if (wave >= 6) {
    // ------------------------------------------------ weight producers ------------------------------------------------
    const int pw = wave - 6;
    int wsrc[WPW];
#pragma unroll
    for (int r = 0; r < WPW; ++r) {
      wsrc[r] = swizzled_unit((pw * WPW + r) * 8 + (lane >> 3), lane & 7);
    }
    const char* wtile = reinterpret_cast<const char*>(L.w_split);
    int c_n = 0, tap_n = 0;                              // (chunk, tap) of the next tile to fetch: the sequence repeats per pixel tile
    auto gload_next = [&](int it) {
      const char* p = wtile + (size_t)(tap_n * L.split_kchunks + c_n) * wstep;
      char* dst = Bs + ((it & (NS - 1)) * BN + pw * WPW * 8) * 128;
      weight_dma<WPW>(p, wsrc, dst);
      if (++tap_n == NT) { tap_n = 0; if (++c_n == nchunks) c_n = 0; }
    };
    gload_next(0);
    gload_next(1);
    gload_next(2);                                       // (niter >= 18)
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(WPW) : "memory");     // tiles 0 and 1 landed -> barrier(0)
    for (int it = 0; it < niter; ++it) {
      if (it + 3 < niter) {
        gload_next(it + 3);                              // into tile it - 1's slot, free since barrier(it)
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(WPW) : "memory");   // tile it + 2 landed -> barrier(it + 1)
      } else {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      }
    }
    return;
  }
  if (wave >= 4) {
    // ------------------------------------------------- halo producers -------------------------------------------------
    const int pt = tid - 256, q = pt & 3, prow = pt >> 2;  // channels q * 8 .. + 7 of halo pixels prow + 32 k
    int hyx[NHP], wl[NHP];                               // tile-independent: halo coordinates and LDS address of pass k
#pragma unroll
    for (int k = 0; k < NHP; ++k) {
      const int hp = prow + k * 32;
      const int hy = hp / HP, hx = hp - hy * HP;
      hyx[k] = hp < HALO ? ((hy << 8) | hx) : -1;
      wl[k] = hy * RSTRIDE + hx * PITCH + q * 16;
    }
    int hsrc[NHP];                                       // source pixel index (or -1: padding / beyond the halo) for the tile being staged
    int img = 0;
    auto set_tile = [&](int kt) {
      int lin = t_first + kt * t_stride;
      const int tx = lin % tiles_x; lin /= tiles_x;
      const int ty = lin % tiles_y;
      img = lin / tiles_y;
      const int y0 = ty * TH, x0 = tx * TW;
#pragma unroll
      for (int k = 0; k < NHP; ++k) {
        hsrc[k] = -1;
        if (hyx[k] >= 0) {                               // (halo_source written out: as a call it reorders this kernel's listing)
          int y = y0 - 1 + (hyx[k] >> 8), x = x0 - 1 + (hyx[k] & 255);
          if ((unsigned)y < (unsigned)Hs && (unsigned)x < (unsigned)Ws) {
            if (d.ups) { y >>= 1; x >>= 1; }
            hsrc[k] = (img * d.Hin + y) * d.Win + x;
          }
        }
      }
    };
    float4 g0[NHP], g1[NHP];
    auto load_chunk = [&](int chunk) {
      const ChunkSrc s = chunk_source(L, chunk * CH + q * 8);
#pragma unroll
      for (int k = 0; k < NHP; ++k) load_unit(s, hsrc[k], g0[k], g1[k]);
    };
    float pa[8], pb[8];
    auto pro_load = [&](int chunk) {
      if (L.pro_a) load_pro8(L.pro_a + (size_t)img * d.C0 + chunk * CH + q * 8, L.pro_b + (size_t)img * d.C0 + chunk * CH + q * 8, pa, pb);
    };
    auto write_pass = [&](int buf, auto K) {
      constexpr int k = decltype(K)::value;
      if (hyx[k] >= 0) finish_unit(g0[k], g1[k], L.pro_a != nullptr, pa, pb, hsrc[k] < 0, Ah + buf * HBYTES + wl[k]);
    };
    set_tile(0);
    pro_load(0);
    load_chunk(0);
    write_pass(0, IC<0>()); write_pass(0, IC<1>()); write_pass(0, IC<2>()); write_pass(0, IC<3>());
    write_pass(0, IC<4>()); write_pass(0, IC<5>()); write_pass(0, IC<6>()); write_pass(0, IC<7>());
    write_pass(0, IC<8>()); write_pass(0, IC<9>()); write_pass(0, IC<10>());
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");               // -> barrier(0)
    int kt = 0, c = 0;
    for (int g = 0; g < nchunks_total; ++g) {
      const bool more = g + 1 < nchunks_total;
      int c1 = c + 1, kt1 = kt;
      if (c1 == nchunks) { c1 = 0; kt1 = kt + 1; }
      const int nb = (g + 1) & 1;
      // tap 0: the next chunk's (the next TILE's first chunk's) coordinates, coefficients and ALL its halo loads; taps 2 .. 7: two
      // passes each converted and written (the other halo buffer was last read during the previous chunk's tap 8, i.e. before
      // barrier(9 g)); tap 8: nothing — the consumers fetch the next chunk's first fragments during it
      if (more) {
        if (c1 == 0) set_tile(kt1);
        pro_load(c1);
        load_chunk(c1);
      }
      asm volatile("s_barrier" ::: "memory");                                     // -> barrier(9 g + 1)
      asm volatile("s_barrier" ::: "memory");                                     // -> barrier(9 g + 2)
      if (more) { write_pass(nb, IC<0>()); write_pass(nb, IC<1>()); }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) { write_pass(nb, IC<2>()); write_pass(nb, IC<3>()); }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) { write_pass(nb, IC<4>()); write_pass(nb, IC<5>()); }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) { write_pass(nb, IC<6>()); write_pass(nb, IC<7>()); }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) { write_pass(nb, IC<8>()); write_pass(nb, IC<9>()); }
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
      if (more) write_pass(nb, IC<10>());
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");             // -> barrier(9 g + 8)
      asm volatile("s_barrier" ::: "memory");                                     // -> barrier(9 g + 9)
      c = c1;
      kt = kt1;
    }
    return;
  }
  // ---------------------------------------------------- consumers -----------------------------------------------------
  const int l31 = lane & 31, hi = lane >> 5;
  int a_lane[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int pix = wave * 64 + i * 32 + l31;
    a_lane[i] = (pix / TW) * RSTRIDE + (pix % TW) * PITCH + hi * 16;
  }
  int b_lane[2][2];
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    const int sw = (l31 >> 1) & 7, unit = 2 * st + hi;
    b_lane[st][0] = l31 * 128 + ((unit ^ sw) << 4);
    b_lane[st][1] = l31 * 128 + (((4 + unit) ^ sw) << 4);
  }
  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.0f; tot[i][j][e] = 0.0f; }
  f16x8 fa[2][4], fw[2][4];                              // [k16 step][A: (hi, lo) x row tile | W: (hi, lo) x column tile]
  auto reads = [&](auto ST, auto TAP, int cb, int slot) {
    constexpr int st = decltype(ST)::value, T = decltype(TAP)::value;
    consumer_reads(Ah + cb * HBYTES + G::tap(T) + st * 32, Bs + slot * (BN * 128), a_lane, b_lane[st], fa[st], fw[st]);
  };
  auto mfmas = [&](auto ST) { mfma3<2>(fa[decltype(ST)::value], fw[decltype(ST)::value], acc); };
  // one tap of global chunk g (halo buffer g & 1); `more` = another chunk (of this or of the next tile) follows
  auto body = [&](auto TAP, int g, bool more, bool first) {
    constexpr int T = decltype(TAP)::value;
    const int it = g * NT + T;
    // barrier #it (the very first tap runs straight after the prologue's barrier #0): weight tiles it, it + 1 are in LDS, tile
    // it - 1's slot is free for the producers, this chunk's halo is complete.  No wait: a consumer's outstanding fragment loads
    // read only images that stay valid for another tap.
    if (it > 0) asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    reads(IC<1>(), TAP, g & 1, it & (NS - 1));
    mfmas(IC<0>());
    interleave_8_reads_12_mfmas();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (T < NT - 1) reads(IC<0>(), IC<(T + 1) % NT>(), g & 1, (it + 1) & (NS - 1));
    else if (more) reads(IC<0>(), IC<0>(), (g + 1) & 1, (it + 1) & (NS - 1));
    mfmas(IC<1>());
    interleave_8_reads_12_mfmas();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (T == NT - 1) {                         // the 288-term partial of this channel chunk
      // (a tile's FIRST partial is assigned, not added to a zeroed total: 0 + x = x, and the epilogue no longer zeroes 64 registers)
      flush_acc<2>(acc, tot, first);
    }
  };
  asm volatile("s_barrier" ::: "memory");                // barrier(0): the producers' prologue — tile 0's first halo, weight tiles 0 and 1
  reads(IC<0>(), IC<0>(), 0, 0);
  const int cpg = L.gn_groups > 0 ? d.Cout / L.gn_groups : 64;          // 8, 16, 32 or 64 when the statistics are fused
  const int nsplit = tiles_img * 4;
  int g = 0;
  for (int kt = 0; kt < t_count; ++kt) {
    for (int c = 0; c < nchunks; ++c, ++g) {
      const bool more = g + 1 < nchunks_total;
      const bool first = c == 0;
      body(IC<0>(), g, more, first); body(IC<1>(), g, more, first); body(IC<2>(), g, more, first); body(IC<3>(), g, more, first);
      body(IC<4>(), g, more, first); body(IC<5>(), g, more, first); body(IC<6>(), g, more, first); body(IC<7>(), g, more, first);
      body(IC<8>(), g, more, first);
    }
    // DIRECT epilogue of tile kt (as in the kernels above): register e of lane half hi is pixel row (e & 3) + 8 (e >> 2) + 4 hi of
    // the 32-pixel row tile, lanes 0-31 are 32 consecutive channels: a dword store per register writes two full 128-byte lines per
    // wave-instruction; GroupNorm partial sums by lane reductions, one slab per (tile, wave).  The next tile's first fragments are
    // already in flight, the producers are a chunk / three taps ahead.
    int lin = t_first + kt * t_stride;
    const int tx = lin % tiles_x; lin /= tiles_x;
    const int ty = lin % tiles_y;
    const int b = lin / tiles_y;
    const int y0 = ty * TH, x0 = tx * TW;
    double sd[2], qd[2];
    // Addresses (round 5): pixel p = 64 wave + 32 i + (e & 3) + 8 (e >> 2) + 4 hi of the 16-wide tile is tile row 4 wave + 2 i + (e >> 3),
    // column (e & 3) + 8 ((e >> 2) & 1) + 4 hi, and Cout is 64 here (the launcher's condition): ONE 64-bit base per lane and tile plus the
    // image's row step — every store is base (+ row step) + a compile-time offset.  The generic form (m * d.Cout + ch per element) cost
    // ~350 of the epilogue's 665 VALU instructions per tile and wave, 140 of them quarter-rate integer multiplies.
    float* const obase = L.out + (((size_t)b * d.Hout + y0 + wave * 4) * d.Wout + x0 + 4 * hi) * BN + l31;
    const size_t rowstep = (size_t)d.Wout * BN;                          // floats between image rows
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch = j * 32 + l31;
      const float bv = L.bias ? L.bias[ch] : 0.0f;
      const float sc = L.split_scale ? L.split_scale[ch] : 1.0f;         // the packer's per-channel power of two, undone (exact)
      float s1 = 0.0f, q1 = 0.0f;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        float* const r0 = obase + j * 32 + (size_t)(2 * i) * rowstep;
        float* const r1 = r0 + rowstep;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          // (sc is an exact power of two: the fused form rounds once, exactly where the product-then-sum form rounds — same bits)
          const float v = __builtin_fmaf(tot[i][j][e], sc, bv);
          ((e >> 3) ? r1 : r0)[((e & 3) + 8 * ((e >> 2) & 1)) * BN] = v;
          s1 += v;
          q1 = fmaf(v, v, q1);
        }
      }
      sd[j] = (double)s1;
      qd[j] = (double)q1;
    }
    if (fuse_stats) {
      const int width = cpg < 32 ? cpg : 32;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        sd[j] += __shfl_xor(sd[j], 32, 64);
        qd[j] += __shfl_xor(qd[j], 32, 64);
        for (int o = 1; o < width; o <<= 1) {
          sd[j] += __shfl_xor(sd[j], o, 64);
          qd[j] += __shfl_xor(qd[j], o, 64);
        }
      }
      float* slab = L.gn_partials + ((size_t)b * nsplit + (ty * tiles_x + tx) * 4 + wave) * L.gn_groups * 2;
      if (cpg == 64) {
        if (lane == 0) {
          slab[0] = (float)(sd[0] + sd[1]);
          slab[1] = (float)(qd[0] + qd[1]);
        }
      } else if (hi == 0 && (l31 & (width - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gr = (j * 32 + l31) / cpg;
          slab[gr * 2] = (float)sd[j];
          slab[gr * 2 + 1] = (float)qd[j];
        }
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // barrier(niter)
}

// ---------------------------------------------------------------------------------------------
// gather form (1x1, 4x4 stride 2, small / ragged shapes): structure of conv_igemm_kernel (conv.hip)
// ---------------------------------------------------------------------------------------------
template <int BM, int BN, bool ONE>
__global__ __launch_bounds__(256, 2) void conv_igemm_split_kernel(const ConvLaunch<float> L, const int M, const int tiles_m,
                                                                  const int tiles_n, const int fuse_stats) {
  constexpr int BK = 32;
  constexpr int AP = BM / 64, NB = BN * 8 / 256;
  constexpr int WAVES_N = BN / 64, WAVES_M = 4 / WAVES_N;
  constexpr int WM = BM / WAVES_M, TM = WM / 32;
  static_assert(TM >= 1, "wave tile");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* As = reinterpret_cast<uint4*>(smem);   // [2][BM][8]
  uint4* Bs = As + 2 * BM * 8;                  // [2][BN][8]
  float* stage = reinterpret_cast<float*>(smem);

  const ConvDesc& d = L.d;
  const int lin = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tn = lin % tiles_n, tm = lin / tiles_n;
  const int tid = threadIdx.x;
  const int lrow = tid >> 2, q = tid & 3;
  const int Cin = d.C0 + d.C1;
  const int Hl = d.ups ? 2 * d.Hin : d.Hin, Wl = d.ups ? 2 * d.Win : d.Win;
  const int HWo = d.Hout * d.Wout;

  int a_iy0[AP], a_ix0[AP], a_base[AP];
  bool a_ok[AP];
  const float* a_p0[AP];
  const float* a_p1[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int m = tm * BM + lrow + i * 64;
    a_ok[i] = m < M;
    const int mm = a_ok[i] ? m : 0;
    if constexpr (ONE) {
      a_p0[i] = L.src0 + (int64_t)mm * d.C0 + q * 8;
      a_p1[i] = d.C1 ? L.src1 + (int64_t)mm * d.C1 + q * 8 - d.C0 : a_p0[i];
    } else {
      const int bb = mm / HWo, rem = mm - bb * HWo;
      const int oy = rem / d.Wout, ox = rem - oy * d.Wout;
      a_iy0[i] = oy * d.stride - d.pad;
      a_ix0[i] = ox * d.stride - d.pad;
      a_base[i] = bb * d.Hin * d.Win;
    }
  }

  // Two register stages, branch-free loads, clamped re-issue past the end (conv.hip's conv_igemm_kernel, round 4): the loads of
  // iteration it + 2 are in flight while iteration it computes, and hipcc's s_waitcnt vmcnt(N) counts stay exact.
  typedef __attribute__((ext_vector_type(4))) unsigned int rb_t;   // (native vectors: hipcc kept an array of the uint4 STRUCT in scratch — every weight load waited on, stored, reloaded)
  typedef __attribute__((ext_vector_type(4))) float ra_t;
  ra_t ra0[AP][2], ra1[AP][2];
  rb_t rb0[NB], rb1[NB];
  unsigned ok0 = 0, ok1 = 0;
  const int niter = d.KH * d.KW * L.split_kchunks;
  auto gload = [&](ra_t(&ra)[AP][2], rb_t(&rb)[NB], unsigned& okm, int tap, int kc) {
    okm = 0;
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    const int c = kc * BK + q * 8;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const float* p = L.src0;
      bool ok;
      if constexpr (ONE) {
        ok = a_ok[i] && c < Cin;
        if (ok) p = (c < d.C0 ? a_p0[i] : a_p1[i]) + kc * BK;
      } else {
        int iy = a_iy0[i] + kh, ix = a_ix0[i] + kw;
        ok = a_ok[i] && (unsigned)iy < (unsigned)Hl && (unsigned)ix < (unsigned)Wl && c < Cin;
        if (d.ups) { iy >>= 1; ix >>= 1; }
        const int64_t pix = ok ? (int64_t)a_base[i] + (int64_t)iy * d.Win + ix : 0;
        const float* pp = (c < d.C0) ? L.src0 + pix * d.C0 + c : L.src1 + pix * d.C1 + (c - d.C0);
        if (ok) p = pp;
      }
      ra[i][0] = reinterpret_cast<const ra_t*>(p)[0];
      ra[i][1] = reinterpret_cast<const ra_t*>(p)[1];
      okm |= (ok ? 1u : 0u) << i;
    }
    const rb_t* wt = reinterpret_cast<const rb_t*>(L.w_split + ((size_t)(tap * L.split_kchunks + kc) * d.CoutPad + (size_t)tn * BN) * 64);
#pragma unroll
    for (int j = 0; j < NB; ++j) rb[j] = wt[tid + j * 256];
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l31 = lane & 31, hi = lane >> 5;

  f32x16 acc[TM][2], tot[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[i][j][e] = 0.0f; tot[i][j][e] = 0.0f; }

  int tap = 0, kc = 0, nxt = 0;                              // coordinates of the NEXT load to issue (clamped to the last chunk)
  auto advance = [&]() {
    const bool more = nxt + 1 < niter;
    nxt += more ? 1 : 0;
    const int k2 = kc + 1, wrap = k2 == L.split_kchunks;
    kc = more ? (wrap ? 0 : k2) : kc;
    tap = more ? tap + wrap : tap;
  };
  gload(ra0, rb0, ok0, tap, kc);
  advance();
  gload(ra1, rb1, ok1, tap, kc);
  advance();
  auto step = [&](ra_t(&ra)[AP][2], rb_t(&rb)[NB], unsigned& okm, int it) {
    uint4* Ab = As + (it & 1) * BM * 8;
    uint4* Bb = Bs + (it & 1) * BN * 8;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const int r = lrow + i * 64, sw = (r >> 1) & 7;
      const float z = ((okm >> i) & 1u) ? 1.0f : 0.0f;      // padding, rows past M, channels past Cin (the stand-in load is finite)
      const float v[8] = {ra[i][0][0] * z, ra[i][0][1] * z, ra[i][0][2] * z, ra[i][0][3] * z,
                          ra[i][1][0] * z, ra[i][1][1] * z, ra[i][1][2] * z, ra[i][1][3] * z};
      uint4 vh, vl;
      split8(v, vh, vl);
      Ab[r * 8 + (q ^ sw)] = vh;
      Ab[r * 8 + ((4 + q) ^ sw)] = vl;
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int u = tid + j * 256, n = u >> 3, slot = u & 7;
      *reinterpret_cast<rb_t*>(Bb + n * 8 + (slot ^ ((n >> 1) & 7))) = rb[j];
    }
    __syncthreads();
    gload(ra, rb, okm, tap, kc);
    advance();
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      const int unit = 2 * st + hi;
      f16x8 fa[2 * TM], fw[4];                               // (hi, lo) per row tile / per column tile
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int r = wm * WM + i * 32 + l31, sw = (r >> 1) & 7;
        fa[2 * i] = ld_frag(Ab + r * 8 + (unit ^ sw));
        fa[2 * i + 1] = ld_frag(Ab + r * 8 + ((4 + unit) ^ sw));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = wn * 64 + j * 32 + l31, sw = (n >> 1) & 7;
        fw[2 * j] = ld_frag(Bb + n * 8 + (unit ^ sw));
        fw[2 * j + 1] = ld_frag(Bb + n * 8 + ((4 + unit) ^ sw));
      }
      mfma3<TM>(fa, fw, acc);
    }
    if ((it & 7) == 7 || it + 1 == niter) flush_acc<TM>(acc, tot);   // 256-term partials
  };
  for (int it = 0; it + 1 < niter; it += 2) {
    step(ra0, rb0, ok0, it);
    step(ra1, rb1, ok1, it + 1);
  }
  if (niter & 1) step(ra0, rb0, ok0, niter - 1);

  double gs, gq;
  auto row_to_m = [&](int r) -> int64_t {
    const int m = tm * BM + wm * WM + r;
    return m < M ? (int64_t)m : (int64_t)-1;
  };
  if (L.split_scale) {                         // undo the packer's per-channel power-of-two weight scale (exact)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float sc = L.split_scale[tn * BN + wn * 64 + j * 32 + l31];      // [CoutPad]: padded columns read 1
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[i][j][e] *= sc;
    }
  }
  epilogue_store<float, TM>(L, tot, stage + wave * 32 * 68, lane, tn * BN + wn * 64, row_to_m, gs, gq);
  if (fuse_stats) {
    const int nsplit = HWo / BM;
    const int bimg = (tm * BM) / HWo, slab = tm - bimg * nsplit;
    float* dst = L.gn_partials + ((size_t)bimg * nsplit + slab) * L.gn_groups * 2;
    epilogue_stats<WAVES_M, WAVES_N>(reinterpret_cast<double*>(stage + 4 * 32 * 68), gs, gq, wave, lane, tn * BN, d.Cout,
                                     L.gn_groups, dst);
  }
}

// ---------------------------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------------------------
// conv3x3_split_kernel<TH, TW, NS> (weight ring slots NS: two workgroups must fit a CU)
template <int TH, int TW>
struct SplitHalo {
  static constexpr int HB = SplitGeom<TH, TW>::HBYTES;
  static constexpr int NS = (2 * HB + 3 * 8192) * 2 <= 160 * 1024 ? 3 : 2;
  static constexpr size_t lds0 = (size_t)2 * HB + NS * 8192 + 512;      // (+ the statistics scratch of the direct epilogue)
  static constexpr size_t lds = lds0 < kEpilogueLds ? kEpilogueLds : lds0;
};

// The f16x3 families of this file; when each is chosen: conv_choose.cpp, choose_split.  > 64 KB of dynamic LDS needs the opt-in.
int launch_conv_split(const ConvChoice& c, const ConvLaunch<float>& L, hipStream_t s) {
  constexpr int HB10 = SplitGeom<8, 16>::HBYTES, HB18 = SplitGeom<16, 16>::HBYTES;
  constexpr size_t ig128 = (size_t)2 * (128 + 128) * 8 * 16, ig64 = (size_t)2 * (128 + 64) * 8 * 16;
  static_assert(ig128 >= kEpilogueLds && ig64 >= kEpilogueLds, "the gather kernel's staging covers the epilogue scratch");
  static ConvKernel<ConvTileKernel<float>> tab[] = {
      {conv_key(kConvSplitWs, 1), &conv3x3_split_ws_kernel<4, true>, 512, (size_t)2 * HB10 + 4 * 128 * 128, 128 * 1024},   // sub-pixel Upsample
      {conv_key(kConvSplitWs, 0), &conv3x3_split_ws_kernel<4, false>, 512, (size_t)2 * HB10 + 4 * 128 * 128, 128 * 1024},
      // the persistent Cout = 64 kernel: 16 x 16-pixel tiles, one 512-thread workgroup per CU (tiles_n = all its tiles)
      {conv_key(kConvSplitP64), &conv3x3_split_p64_kernel<4>, 512, (size_t)2 * HB18 + 4 * 64 * 128, 136 * 1024},
      {conv_key(kConvSplitHalo, 8, 16), &conv3x3_split_kernel<8, 16, SplitHalo<8, 16>::NS>, 256, SplitHalo<8, 16>::lds, 80 * 1024},
      {conv_key(kConvSplitHalo, 4, 32), &conv3x3_split_kernel<4, 32, SplitHalo<4, 32>::NS>, 256, SplitHalo<4, 32>::lds, 80 * 1024}};
  using Ig = void (*)(const ConvLaunch<float>, int, int, int, int);   // (L, M, tiles_m, tiles_n, fuse_stats)
  static ConvKernel<Ig> igemm[] = {{conv_key(128, 128, 1), &conv_igemm_split_kernel<128, 128, true>, 256, ig128, 80 * 1024},
                                   {conv_key(128, 128, 0), &conv_igemm_split_kernel<128, 128, false>, 256, ig128, 80 * 1024},
                                   {conv_key(128, 64, 1), &conv_igemm_split_kernel<128, 64, true>, 256, ig64, 80 * 1024},
                                   {conv_key(128, 64, 0), &conv_igemm_split_kernel<128, 64, false>, 256, ig64, 80 * 1024}};
  switch (c.family) {
    case kConvSplitHalo: return launch_conv_tiles(tab, conv_key(c.family, c.th, c.tw), "split halo conv", c, L, s);
    case kConvSplitWs: return launch_conv_tiles(tab, conv_key(c.family, c.mode), "split ws conv", c, L, s);
    case kConvSplitP64:
      PRG_CHECK(c.grid > 0, "conv3x3_split_p64: no device properties");
      return launch_conv_tiles(tab, conv_key(c.family), "split p64 conv", c, L, s);
    default: break;
  }
  ConvKernel<Ig>* e = nullptr;
  if (int rc = conv_kernel_find(igemm, conv_key(c.bm, c.bn, c.mode), "split implicit-GEMM conv", &e)) return rc;
  e->fn<<<dim3(c.grid), e->block, e->lds, s>>>(L, L.d.B * L.d.Hout * L.d.Wout, c.tiles_x, c.tiles_n, c.fuse_stats);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // namespace prg

