// conv_c64.hip — weights-stationary 3x3 convolution for Cin = Cout = 64 (bf16 throughput path).
//
// The 64 -> 64 convs of the two full-resolution levels (down0/down1 blocks, the second conv of every up3 / final block,
// the last up conv) are the ones the wave-specialised kernel (conv_ws.hip) handles worst: one 64-channel chunk means a
// tile is finished after nine taps, so per 4608 MFMA cycles it re-stages the whole 72 KB weight set through LDS, meets
// nine workgroup barriers and pays one epilogue — 0.25-0.33 of the MFMA peak, while the shape itself is HBM-bound
// (256 B of activations per pixel against 73.7 kFLOP: 49 us of HBM time, 31 us of MFMA time at B = 64, 128 x 128).
//
// Here the weights never touch LDS again after the prologue: a consumer wave owns 32 output channels and keeps their
// 9 x 64 weights as 36 MFMA A-fragments in registers (144 VGPRs) for the whole launch; its B operands are the pixels of
// a 128-pixel half tile read from the halo (round 6: every fragment read once and used for the three taps of its column —
// 72 ds_read_b128 per 144 MFMAs; no weight reads, no weight ring, no per-tap barrier).  The workgroup (512 threads, 256 registers per lane) is
//
//   waves 0-3  CONSUMERS (2 pixel halves x 2 channel halves of a 8 x 32 pixel x 64 channel tile): 144 MFMAs per tile,
//              fragments prefetched three reads ahead; epilogue = bias, GroupNorm partial sums (wave_sums<8>, wave_ops.h:
//              the deterministic butterfly), bf16 and DIRECT stores: pair_chunks pairs the two lane halves' channel quads, so
//              every lane stores 16 contiguous bytes (no LDS stage, nothing for the producers to drain).  The four pixel
//              rows' accumulators finish one halo row apart (the row-reuse skew): rows 0-2 are packed, summed and stored
//              INSIDE the MFMA stream, in the shadows of the next halo row's MFMAs; only row 3, the butterfly and the
//              atomics come after the tile's last MFMA;
//   waves 4-7  PRODUCERS: write halo s+1 (loaded a whole step earlier; optional fused GroupNorm + (scale+1, shift) + SiLU
//              prologue of the previous Block, sd:690-696), re-issue the registers for halo s+2.  A step is ~5000 cycles,
//              so plain loads with compiler-managed waits are enough: every load has a full step to land.  (A third
//              register set, loads two steps ahead, was built and measured 9-22 % SLOWER per launch: at 254 registers
//              hipcc puts an s_waitcnt vmcnt(0) at the top of the three-step body.  DESIGN.md 4.1.)
//
// ONE barrier per tile, behind the consumers' MFMAs: "halo s+1 written; buffer s & 1 no longer read".  The step schedule
// (which halo is issued, written and read in which step, in which register set and LDS buffer, and how many barriers each
// wave class executes for a given step count) is c64_schedule.h; tests/test_c64_schedule.py proves it on the CPU.
// The rest of the epilogue of tile s runs while the producers already write halo s+2 (round 2 had two barriers and an LDS
// stage: producers idle during the epilogue, consumers idle during the drain — the two were additive, 81 / 122 us).
// LDS: 2 halos x 340 rows x 144 B (padded rows: conflict-free ds_read_b128 with immediate tap offsets).
#include <atomic>
#include <cstdlib>

#include "c64_schedule.h"
#include "conv.h"
#include "wave_ops.h"

namespace prg {

namespace {

using G = HaloGeom<8, 32, 256>;                                       // 8 x 32 pixel tiles, 256 producer threads: 340 halo rows, 11 units
constexpr int TH = G::TH, TW = G::TW, HP = G::HP, HALO = G::HALO, ROWB = G::ROWB, RPP = G::RPP, KU = G::KU;
constexpr size_t AH_BYTES = (size_t)G::HROWS * ROWB;                   // 352 rows: the units past the halo end land in spare rows
constexpr size_t C64_LDS = 2 * AH_BYTES + 64 * sizeof(float);          // + the bias

// tile t of this workgroup: XCD-contiguous runs (workgroup b runs on XCD b % 8; speed only), image-major
__device__ inline void c64_tile(int t, int tiles_x, int tiles_y, int& b, int& y0, int& x0) {
  const int tx = t % tiles_x;
  t /= tiles_x;
  const int ty = t % tiles_y;
  b = t / tiles_y;
  y0 = ty * TH;
  x0 = tx * TW;
}

// The per-image ticket fold below (c64_fold_coefficients, the `ticket` lambda, flags bit 1 = 0: contiguous tile runs) is retired:
// launch_conv_c64 never passes tickets and always asks for interleaved runs.  Its device code stays as it was because deleting
// it changes the producers' register allocation (conv3x3_c64_kernel<1 | 2> then spill to scratch) and measured 0.4 % slower end to end.
//
// What gn_coeff_kernel does in a launch of its own, for ONE image, by one wave (lane = channel of the 64): the image's
// (sum, sumsq) slabs summed in float64 — lanes of a group take slabs (c % cpg), + cpg, ... then a fixed xor tree —, mean /
// rstd, folded with the norm's gain / bias and the ResnetBlock conditioning into y = x * A + B.  The slabs were written by
// other CUs with agent-scope stores; they are read with agent-scope (L1-bypassing) loads.
__device__ inline void c64_fold_coefficients(const ConvLaunch<bf16_t>& L, int img, int nsplit, int lane) {
  const int G = L.gn_groups, cpg = 64 / G;
  const int c = lane, g = c / cpg, j = c % cpg;
  const GnApply& p = L.gn;
  const float* ssa = nullptr;
  const float* ssb = nullptr;
  if (p.ss_a) {
    ssa = p.ss_a + (size_t)img * p.ss_a_stride;
    if (p.ss_a_row) ssa += (size_t)(*p.ss_a_row) * p.ss_a_row_stride;
    if (p.ss_b) ssb = p.ss_b + (size_t)img * p.ss_b_stride;
  }
  const float gam = p.gamma[c], bet = p.beta[c];
  float s0 = 0.0f, s1 = 0.0f;
  if (ssa) {
    s0 = ssa[c];
    s1 = ssa[64 + c];
    if (ssb) { s0 += ssb[c]; s1 += ssb[64 + c]; }
  }
  const unsigned long long* pp =
      reinterpret_cast<const unsigned long long*>(L.gn_partials + ((size_t)img * nsplit * G + g) * 2);
  double ss = 0, qq = 0;
  for (int k0 = j; k0 < nsplit; k0 += 8 * cpg) {           // eight loads in flight per lane, summed in index order
    unsigned long long v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = k0 + i * cpg;
      v[i] = k < nsplit ? __hip_atomic_load(pp + (size_t)k * G, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      ss += (double)__uint_as_float((unsigned)(v[i] & 0xffffffffull));
      qq += (double)__uint_as_float((unsigned)(v[i] >> 32));
    }
  }
  for (int o = cpg >> 1; o > 0; o >>= 1) {
    ss += __shfl_xor(ss, o, 64);
    qq += __shfl_xor(qq, o, 64);
  }
  const double n = (double)L.d.Hout * L.d.Wout * cpg;
  const double mean = ss / n;
  double var = qq / n - mean * mean;
  if (var < 0) var = 0;
  const float fmean = (float)mean, frstd = (float)(1.0 / sqrt(var + 1e-5));
  float a = frstd * gam;
  float bb = bet - fmean * a;
  if (ssa) {
    a = a * (s0 + 1.0f);
    bb = fmaf(bb, s0 + 1.0f, s1);
  }
  L.gn_coef_a[(size_t)img * 64 + c] = a;
  L.gn_coef_b[(size_t)img * 64 + c] = bb;
}

// PRO 0: no prologue; 1: GroupNorm coefficient tables (pro_a / pro_b); 2: coefficients folded here from pro_fold; 3: as 2 on an
// f16 input with f16 weights (the h16 format, conv.h; h16_silu8: packed-f16 prologue, v_mfma_f32_32x32x16_f16).  O16: f16 output.
template <int PRO, bool O16>
__global__ __launch_bounds__(512) void conv3x3_c64_kernel(const ConvLaunch<bf16_t> L, const int tiles_x, const int tiles_y,
                                                          const int flags) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int fuse_stats = flags & 1;
  const ConvDesc& d = L.d;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int total = tiles_x * tiles_y * d.B;
  // XCD-contiguous tile runs (gridDim.x is a multiple of 8): XCD x owns tiles [x per, (x+1) per); inside, every workgroup
  // takes ONE contiguous run (stride 1): neighbouring tiles share halo rows in the XCD's L2 and a workgroup leaves an
  // image at most twice per launch (the per-image coefficient ticket below is one atomic per departure).
  const int xcd = blockIdx.x & 7, widx = blockIdx.x >> 3, wpx = gridDim.x >> 3;
  const int per = (total + 7) / 8;
  const int lo_t = min(xcd * per, total), hi_t = min((xcd + 1) * per, total);
  const int nx = hi_t - lo_t, qx = nx / wpx, rx = nx % wpx;
  // fuse_stats bit 1: interleaved assignment (workgroup w of the XCD takes tiles w, w + wpx, ...) instead of contiguous runs
  const bool inter = (flags & 2) != 0;
  const int first = inter ? lo_t + widx : lo_t + widx * qx + min(widx, rx);
  const int nsteps = inter ? (widx < nx ? (nx - widx + wpx - 1) / wpx : 0) : qx + (widx < rx ? 1 : 0);
  const int stride = inter ? wpx : 1;
  if (nsteps == 0) return;
  // halo register sets of the producers (c64_schedule.h).  A third set (loads two steps ahead) was built and measured slower:
  // profiles/c64_pipeline_stamps_and_variants.txt.
  constexpr int DEPTH = 2;

  // ---------------------------------------------------------------------------------------------------
  if (wave < 4) {
    __builtin_amdgcn_s_setprio(3);
    const int wm = wave >> 1, wn = wave & 1;              // pixel half (tile rows 4 wm .. 4 wm + 3), channel half
    const int l31 = lane & 31, hi = lane >> 5;
    // weights of channel wn*32 + l31: 9 taps x 4 k-steps; lane half hi takes k = 16 c + 8 hi .. + 7
    bf16x8 wf[9][4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16_t* const wsrc = PRO == 3 ? reinterpret_cast<const bf16_t*>(L.w_f16) : L.w;
        const bf16_t* p = wsrc + ((size_t)(tap * d.kchunks + (c >> 1)) * d.CoutPad + wn * 32 + l31) * 32 + (c & 1) * 16 + hi * 8;
        wf[tap][c] = *reinterpret_cast<const bf16x8*>(p);
      }
    float* const bias_lds = reinterpret_cast<float*>(smem + 2 * AH_BYTES);
    if (tid < 64) bias_lds[tid] = L.bias[tid];             // visible after the prologue barrier
    const float* const biasp = bias_lds + wn * 32 + 4 * hi;
    const int gn_per = fuse_stats ? (64 / L.gn_groups) >> 3 : 1;   // 8-channel chunks per group (1, 2, 4 or 8)
    // LDS byte offset of pixel (row 4 wm + pt, column l31), tap (0,0), k-step 0: rows are HP * ROWB apart
    const unsigned x0off = (unsigned)(((wm * 4) * HP + l31) * ROWB + hi * 16);
    auto mma = [](const bf16x8& a, const bf16x8& b, const f32x16& c) -> f32x16 {
      if constexpr (PRO == 3)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
      else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    };
    lds_barrier();                                         // halo 0 is in LDS (producers' prologue)
    for (int s = 0; s < nsteps; ++s) {
      const char* const xb = smem + (size_t)c64_lds_buf(s) * AH_BYTES + x0off;
      // Round 5: the accumulators START at the bias (16 values per lane, re-read from LDS per tile: they are dead again before the
      // fragment sets fill up) instead of at zero — the epilogue's 64 bias additions per tile and wave are gone; the sum's rounding
      // order changes (bias first), far below the bf16 / f16 output rounding.
      f32x16 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 b4 = *reinterpret_cast<const float4*>(biasp + 8 * q);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) { acc[pt][4 * q] = b4.x; acc[pt][4 * q + 1] = b4.y; acc[pt][4 * q + 2] = b4.z; acc[pt][4 * q + 3] = b4.w; }
      }
      // ---- epilogue state, ahead of the MFMAs: lane holds pixel (row 4 wm + pt, col l31), channels wn*32 + 8 q + 4 hi + {0..3}
      int tb, ty0, tx0;
      c64_tile(first + s * stride, tiles_x, tiles_y, tb, ty0, tx0);
      char* const obase = reinterpret_cast<char*>(L.out) +
                          ((((size_t)tb * d.Hout + ty0 + wm * 4) * d.Wout + tx0 + l31) * 64 + wn * 32 + 8 * hi) * 2;
      const size_t orow = (size_t)d.Wout * 128;          // output bytes per image row
      float V[8];                                          // [sum | sumsq][q]
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        V[q] = 0.0f;
        V[4 + q] = 0.0f;
      }
      uint32_t pk[8];
      // 8-channel chunk q of pixel row pt: statistics (per q the sums run pt-major, then r: the order they have always had, so the
      // float sums keep their bits) and packing.  `pin`: inside the MFMA stream the results are made opaque where they are
      // computed, or the compiler sinks the arithmetic behind the loop again (it did: 167 of 206 VALU instructions).
      auto pack_chunk = [&](const int pt, const int q, const bool pin) __attribute__((always_inline)) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[pt][4 * q + r];   // (the bias rode in as the accumulators' initial value)
          V[q] += v[r];
          V[4 + q] = fmaf(v[r], v[r], V[4 + q]);
        }
        pk[2 * q] = O16 ? h16_pack(v[0], v[1]) : pack_bf16(v[0], v[1]);
        pk[2 * q + 1] = O16 ? h16_pack(v[2], v[3]) : pack_bf16(v[2], v[3]);
        if (pin) asm volatile("" : "+v"(V[q]), "+v"(V[4 + q]), "+v"(pk[2 * q]), "+v"(pk[2 * q + 1]));
      };
      // chunks 2m and 2m + 1 of pixel row pt: one 16-byte store per lane (pair_chunks)
      auto store_half = [&](const int pt, const int m) __attribute__((always_inline)) {
        *reinterpret_cast<u32x4*>(obase + pt * orow + m * 32) = pair_chunks(pk[4 * m], pk[4 * m + 1], pk[4 * m + 2], pk[4 * m + 3]);
      };
      // Round 6: ROW REUSE.  Tap (dy, dx) of pixel row pt reads halo row pt + dy: the twelve (pt, dy) pairs of one (dx, k-step) touch
      // only SIX halo rows.  The four accumulators are independent chains, so they are skewed by one tap row: fragment (halo row r,
      // dx, c) is read ONCE and feeds acc[r] at tap (0, dx), acc[r-1] at (1, dx) and acc[r-2] at (2, dx) back to back — 72 reads
      // per tile instead of 144 (0.5 ds_read_b128 per MFMA), no extra registers, and every accumulator still sees its MFMAs in
      // tap-major order: the outputs are bit-identical.  Measured -1.0 ... -1.5 % per launch (profiles/r06_ab_c64_row_reuse.txt): the
      // fragment reads are a small term of this kernel (profiles/r06_c64_half_reads_bound.txt).  Ring of four fragments, three ahead.
      //
      // The skew also finishes the accumulators one halo row apart: acc[pt] has its last MFMA at the end of halo row pt + 2.  Its
      // epilogue (no LDS in it, so it needs no barrier) is issued in the MFMA shadows of halo row pt + 3: chunk q at fragments 1, 3,
      // 5, 7 of that row, the two stores at fragments 9 and 10.  Only acc[3] is finished behind the barrier.
      constexpr int FD = 3, FR = 4, NF = 72;
      bf16x8 fr[FR];
      auto foff = [](int n) { return ((n / 12) * HP + (n / 4) % 3) * ROWB + (n & 3) * 32; };   // n = (r * 3 + dx) * 4 + c
#pragma unroll
      for (int j = 0; j < FD && j < NF; ++j) fr[j] = *reinterpret_cast<const bf16x8*>(xb + foff(j));
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int r = n / 12, dx = (n / 4) % 3, c = n & 3;
        if (n + FD < NF) fr[(n + FD) % FR] = *reinterpret_cast<const bf16x8*>(xb + foff(n + FD));
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const int pt = r - dy;
          if (pt >= 0 && pt < 4) acc[pt] = mma(wf[dy * 3 + dx][c], fr[n % FR], acc[pt]);
        }
        if (r >= 3) {
          const int j = n % 12;
          if ((j & 1) && j < 8) pack_chunk(r - 3, j >> 1, true);
          if (j == 9) store_half(r - 3, 0);
          if (j == 10) store_half(r - 3, 1);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      // the partial sums of the previous tile have left this CU before the barrier its ticket is taken behind
      if (fuse_stats && L.gn_tickets) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      lds_barrier();                                       // halo s+1 is written; nobody reads buffer s & 1 any more
#pragma unroll
      for (int q = 0; q < 4; ++q) pack_chunk(3, q, false);
#pragma unroll
      for (int m = 0; m < 2; ++m) store_half(3, m);
      if (fuse_stats) {
        // lane (< 8) gets the wave total of value i = [sq][q]: 8-channel chunk q of this wave's 32 channels; then the chunks of
        // one group are folded (per = cpg / 8 <= 4 inside a wave; 8 = both channel halves: two slabs)
        float D = wave_sums<8>(V, lane);
        const int per = gn_per > 4 ? 4 : gn_per;
        D = group_sums<8>(D, per);
        const int i = wave_sums_index<8>(lane);
        const int q = i & 3;
        if (lane < 8 && (q & (per - 1)) == 0) {
          const int split_n = gn_per > 4 ? 2 : 1;
          const int nsplit = tiles_x * tiles_y * 2 * split_n;
          const int slab = (((ty0 / TH) * tiles_x + tx0 / TW) * 2 + wm) * split_n + (split_n == 2 ? wn : 0);
          const int grp = (wn * 4 + q) / gn_per;
          if (L.gn_acc) {
            // fixed-point accumulators (common.h): one no-return 64-bit integer atomic per wave total
            // (`which` made opaque here: its loop-invariant scale select otherwise lives in a VGPR across the MFMA loop — with the
            //  f16 epilogue that was the 257th register, and the spill's reload put an s_waitcnt vmcnt(0) behind the tile's stores)
            int which = i >> 2;
            asm volatile("" : "+v"(which));
            gn_acc_add(L.gn_acc, L.gn_groups, tb, grp, which, D);
          } else {
            // agent-scope (write-through, sc1) store: the workgroup that completes the image reads these from another CU
            __hip_atomic_store(&L.gn_partials[(((size_t)tb * nsplit + slab) * L.gn_groups + grp) * 2 + (i >> 2)], D,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
    if (fuse_stats && L.gn_tickets) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int p = c64_consumer_pad_barriers(nsteps, DEPTH); p > 0; --p) lds_barrier();   // the producers' padding steps
    lds_barrier();                                         // matches the producers' final barrier (ticket of the last tile)
    return;
  }

  // ---------------------------------------------------------------------------------------------------
  {
    const int ptid = tid - 256;
    const int slot = ptid & 7, row = ptid >> 3;           // 16-byte unit of a 128-byte pixel row; halo rows row + 32 k
    char* const ah = smem + row * ROWB + slot * 16;
    const int Hl = d.Hout, Wl = d.Wout;
    // Tile-independent halo geometry of this thread's units (round 3: the per-tile address arithmetic was ~27 VALU
    // instructions per unit — as many per tile as the consumers' whole epilogue).  Unit k sits at a fixed byte offset from
    // the tile's halo origin, and whether it is padding depends only on which image edges the tile touches: five bit masks
    // per thread, one AND-NOT per edge and tile.  The loads are raw BUFFER loads from a descriptor whose base lies one halo
    // row + one pixel before the tensor: every in-image unit has a non-negative offset, a padding unit gets offset
    // 0xffffffff and the hardware's range check returns zeros — no clamped stand-in address, no select after the load.
    int voffk[KU];
    unsigned m_valid = 0, m_top = 0, m_bot = 0, m_left = 0, m_right = 0;
#pragma unroll
    for (int k = 0; k < KU; ++k) {
      const int hp = k * RPP + row;
      const int hy = hp / HP, hx = hp - hy * HP;
      const bool valid = hp < HALO;
      // (tile origins are multiples of 8 / 32: (y0 - 1 + hy) >> ups = (y0 >> ups) + ((hy - 1) >> ups), arithmetic shift)
      const int dy = (hy - 1) >> d.ups, dx = (hx - 1) >> d.ups;
      voffk[k] = ((dy + 1) * d.Win + dx + 1) * 128 + slot * 16;
      m_valid |= (valid ? 1u : 0u) << k;
      m_top |= (valid && hy == 0 ? 1u : 0u) << k;
      m_bot |= (valid && hy == TH + 1 ? 1u : 0u) << k;
      m_left |= (valid && hx == 0 ? 1u : 0u) << k;
      m_right |= (valid && hx == HP - 1 ? 1u : 0u) << k;
    }
    const unsigned pad_bytes = (unsigned)(d.Win + 1) * 128u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(L.src0)) - pad_bytes, 0,
        (int)((size_t)d.B * d.Hin * d.Win * 128 + pad_bytes), 0x00020000);
    // Two register sets: halo h lives in set h & 1.  The loads of halo s+2 are issued BEFORE halo s+1 is transformed and
    // written, so HBM requests are in flight during the prologue arithmetic (with one set the re-issue had to wait for
    // the transform: every CU computed while HBM idled, then every CU loaded — the two times added up).
    u32x4 hA[KU], hB[KU];
    const int tpi = tiles_x * tiles_y;                     // tiles per image
    int done_in_img = 0;                                   // tiles of the current image this workgroup has finished
    unsigned okmask = 0, okmask_nxt = 0;
    float4 cf[4], nf[4];                                   // A0..3, A4..7, B0..3, B4..7 of the halo being written / issued
    h16x2 ah2[4], bh2[4];                                  // PRO == 3: the coefficients as packed f16 channel pairs
    longlong2 fs_n = make_longlong2(0, 0);                  // PRO == 2: (sum, sumsq) of the 8-channel unit's group, fixed point
    auto issue = [&](int s, u32x4(&h)[KU]) {           // loads of halo s (clamped to the last tile: harmless reloads)
      int b, y0, x0;
      c64_tile(first + c64_tile_of_halo(s, nsteps) * stride, tiles_x, tiles_y, b, y0, x0);
      okmask_nxt = m_valid & ~((y0 == 0 ? m_top : 0u) | (y0 + TH == Hl ? m_bot : 0u) | (x0 == 0 ? m_left : 0u) |
                               (x0 + TW == Wl ? m_right : 0u));
      const int soff = __builtin_amdgcn_readfirstlane((((b * d.Hin + (y0 >> d.ups)) * d.Win) + (x0 >> d.ups)) * 128);   // the SGPR offset
#pragma unroll
      for (int k = 0; k < KU; ++k)
        h[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, ((okmask_nxt >> k) & 1u) ? voffk[k] : -1, soff, 0);
      if constexpr (PRO == 1) load_coeffs(nf, L.pro_a + (size_t)b * 64 + slot * 8, L.pro_b + (size_t)b * 64 + slot * 8);
      if constexpr (PRO >= 2) {
        // the raw material of the coefficients: this unit's group statistics and its folded gain / bias (P, Q); the
        // arithmetic happens in adopt(), a step later, when the loads have long landed
        const GnFold& f = L.pro_fold;
        fs_n = *group_stats(f, b, slot * 8);
        load_coeffs(nf, f.P + (size_t)b * f.pq_stride + slot * 8, f.Q + (size_t)b * f.pq_stride + slot * 8);
      }
    };
    auto write = [&](int s, u32x4(&h)[KU]) {           // halo s -> LDS buffer s & 1
      char* dst = ah + (size_t)c64_lds_buf(s) * AH_BYTES;
      const float a8[8] = {cf[0].x, cf[0].y, cf[0].z, cf[0].w, cf[1].x, cf[1].y, cf[1].z, cf[1].w};
      const float b8[8] = {cf[2].x, cf[2].y, cf[2].z, cf[2].w, cf[3].x, cf[3].y, cf[3].z, cf[3].w};
#pragma unroll
      for (int k = 0; k < KU; ++k) {
        u32x4 v = h[k];
        if constexpr (PRO == 3) {
          v = h16_silu8(v, ah2, bh2);
        } else if constexpr (PRO) {
          v = silu_affine8(v, a8, b8);
        }
        if constexpr (PRO != 0) {                          // (PRO == 0: the padding units arrived as zeros)
          if (!((okmask >> k) & 1u)) v = u32x4{0u, 0u, 0u, 0u};
        }
        *reinterpret_cast<u32x4*>(dst + k * RPP * ROWB) = v;
      }
    };
    auto adopt = [&]() {                                   // the validity mask and coefficients of the halo about to be written
      okmask = okmask_nxt;
      if constexpr (PRO == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) cf[j] = nf[j];
      }
      if constexpr (PRO >= 2) fold_coeffs(cf, nf, fs_n, L.pro_fold.inv_n);   // A = rstd P, B = Q - mean A
      if constexpr (PRO == 3) pack_coeffs_h16(cf, ah2, bh2);
    };
    static_assert(c64_reg_set(0, DEPTH) == 0 && c64_reg_set(1, DEPTH) == 1 && c64_issued_in_step(0, DEPTH) == 2);
    issue(0, hA);                                          // (c64_schedule.h: halo 0, write 0, halo 1)
    adopt();
    write(0, hA);
    issue(1, hB);
    lds_barrier();                                         // halo 0 ready
    auto ticket = [&](int s) {                             // tile s is complete and its partial sums have left their CU
      if (fuse_stats && L.gn_tickets && ptid < 64) {       // first producer wave: per-image arrival ticket
        const int t = first + s * stride;
        const int img = t / tpi;
        ++done_in_img;
        const bool leave = s + 1 == nsteps || (t + stride) / tpi != img;
        if (leave) {
          int old = 0;
          if (ptid == 0) old = __hip_atomic_fetch_add(L.gn_tickets + img, done_in_img, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          old = __builtin_amdgcn_readfirstlane(old);
          if (old + done_in_img == tpi) {                  // this workgroup completed image `img`: fold its statistics
            if (ptid == 0) __hip_atomic_store(L.gn_tickets + img, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c64_fold_coefficients(L, img, tpi * 2 * (((64 / L.gn_groups) >> 3) > 4 ? 2 : 1), ptid);
          }
          done_in_img = 0;
        }
      }
    };
    // Two steps per iteration (the register set of a halo is a compile-time choice); an odd step count is padded with
    // one step of clamped reloads that nobody reads, so the loop body stays branch-free between a load and its use and
    // the compiler's s_waitcnt vmcnt(N) counts stay exact.  The consumers execute the padding step as a bare barrier.
    const int n2 = c64_padded_steps(nsteps, DEPTH);
#pragma unroll 1
    for (int s = 0; s < n2; s += 2) {
      // during the consumers' MFMAs of step s and their epilogue of step s-1: the loads of halo s+2, then halo s+1 into
      // the buffer they left before barrier s-1
      adopt();
      issue(s + 2, hA);
      write(s + 1, hB);
      lds_barrier();                                       // barrier s
      if (s > 0) ticket(s - 1);                            // the consumers stored tile s-1's partial sums before this barrier
      adopt();
      issue(s + 3, hB);
      write(s + 2, hA);
      lds_barrier();                                       // barrier s+1
      if (s < nsteps) ticket(s);
    }
    lds_barrier();
    if (n2 == nsteps) ticket(nsteps - 1);
  }
}

}  // namespace

// conv3x3_c64_kernel<PRO, OUT_F16>: pro 0-3, mode 1 = f16 output (conv1 of an h16 pair, no prologue)
int launch_conv_c64(const ConvChoice& c, const ConvLaunch<bf16_t>& L, hipStream_t s) {
  using Fn = void (*)(const ConvLaunch<bf16_t>, int, int, int);
#define PRG_C64(PRO, F16) {conv_key(PRO, F16), &conv3x3_c64_kernel<PRO, F16>, 512, C64_LDS, (int)C64_LDS}
  static ConvKernel<Fn> tab[] = {PRG_C64(0, false), PRG_C64(1, false), PRG_C64(2, false), PRG_C64(3, false), PRG_C64(0, true)};
#undef PRG_C64
  ConvKernel<Fn>* e = nullptr;
  if (int rc = conv_kernel_find(tab, conv_key(c.pro, c.mode), "c64 conv", &e)) return rc;
  ConvLaunch<bf16_t> Lk = L;
  Lk.gn_tickets = nullptr;                                   // (the in-kernel ticket fold is retired: never launched)
  if (!c.acc_done) Lk.gn_acc = nullptr;                      // slabs: the kernel takes a non-null gn_acc as "accumulate"
  // interleaved tile runs are ~2 % faster (neighbouring tiles run at the same time on neighbouring CUs of the XCD)
  const int flags = (c.fuse_stats ? 1 : 0) | 2;
  e->fn<<<dim3(c.grid), e->block, e->lds, s>>>(Lk, c.tiles_x, c.tiles_y, flags);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // namespace prg
