// conv.hip — convolutions of the two U-Nets as implicit GEMM on the CDNA4 matrix cores (MFMA roofline).
//
//   out[m][n] = bias[n] + sum_{tap,c} in[pixel(m) + tap][c] * w[n][tap][c]        m = (b, oy, ox), NHWC
//
// T = bf16_t uses v_mfma_f32_32x32x16_bf16 (fp32 accumulate); T = float uses v_mfma_f32_32x32x2_f32, an exact
// k-ordered fmaf chain — the parity mode.  Two kernels share one epilogue:
//
//  * conv3x3_halo_kernel — every 3x3 / stride 1 / pad 1 conv whose widths are multiples of 128 bytes (all of them
//    at dim = 64: Block.proj, the last down/up convs, Upsample's conv with the x2 nearest gather folded in, the
//    skip concat as two sources).  A workgroup owns a TH x TW pixel tile of ONE image: its (TH+2) x (TW+2) input
//    halo is staged into LDS once per 128-byte channel chunk and reused by all nine taps (9x less global->LDS
//    traffic than an im2col gather), weights stream through a double-buffered LDS tile one tap at a time, and
//    the next chunk's halo is prefetched into registers underneath the MFMAs.  LDS images are XOR-swizzled at
//    16-byte granularity (unit ^= (row >> 1) & 7) so the 32 rows of a ds_read_b128 fragment load hit distinct
//    bank quads.  Optional fused prologue: GroupNorm + (scale+1, shift) + SiLU of the previous Block applied
//    while the halo is written (each halo pixel transformed once, never the 9x im2col copies).
//  * conv_igemm_kernel — the general gather form (1x1, 4x4 stride 2, ragged widths, tiny images).
//
// Shared epilogue: accumulators are transposed through LDS so every lane stores 16 contiguous bytes (full 128-byte
// lines per 8 lanes) instead of 2-byte pieces, bias / residual are added on the way, and the per-(image, tile,
// group) GroupNorm partial sums of the output are emitted in a fixed order (deterministic) for the consumer.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "blocks.h"
#include "conv.h"
#include "conv_epi.h"

namespace prg {

// One "unit" = 16 bytes = Elem<T>::kVec channels.  A fragment step consumes one unit per lane.
template <typename T>
struct Mma;

template <>
struct Mma<bf16_t> {
  // per 2 units (hi = lane>>5 picks the unit): one K=16 MFMA
  static constexpr int UNITS_PER_CALL = 2;
  using Frag = bf16x8;
  __device__ static inline int unit_of(int call, int hi) { return call * 2 + hi; }
  __device__ static inline Frag load(const void* p) { return *reinterpret_cast<const Frag*>(p); }
  __device__ static inline void mma(const Frag& a, const Frag& b, f32x16& c, int /*hi*/) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};

template <>
struct Mma<float> {
  // per unit (both lane halves read the SAME 4 floats): two K=2 MFMAs, k = {0,1} then {2,3}
  static constexpr int UNITS_PER_CALL = 1;
  struct Frag {
    float4 v;
  };
  __device__ static inline int unit_of(int call, int /*hi*/) { return call; }
  __device__ static inline Frag load(const void* p) {
    Frag f;
    f.v = *reinterpret_cast<const float4*>(p);
    return f;
  }
  __device__ static inline void mma(const Frag& a, const Frag& b, f32x16& c, int hi) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(hi ? a.v.y : a.v.x, hi ? b.v.y : b.v.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(hi ? a.v.w : a.v.z, hi ? b.v.w : b.v.z, c, 0, 0, 0);
  }
};


// Parity mode (T = float): the reference's oneDNN kernels sum a convolution's K = 9 Cin products in short vector blocks;
// one K-long fp32 chain per output sits 2-3x further from exact arithmetic than that (measured per tap against a float64
// evaluation of the reference, tests/golden/G13).  So the exact-f32 MFMA chain is cut at every main-loop iteration (16 or 32
// terms) and the partials are summed in float64: the result is within 1 ulp of the correctly rounded fp32 value.
template <int TM>
__device__ inline void clear_acc(f32x16 (&acc)[TM][2]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
}
template <typename T, int TM = 1>
struct Wide {                      // bf16 path: nothing
  static constexpr bool on = false;
  __device__ inline void add(const f32x16 (&)[TM][2]) {}
  __device__ inline void finish(f32x16 (&)[TM][2]) {}
};
template <int TM>
struct Wide<float, TM> {
  static constexpr bool on = true;
  double tot[TM][2][16];
  __device__ inline Wide() {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[i][j][e] = 0.0;
  }
  __device__ inline void add(const f32x16 (&acc)[TM][2]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[i][j][e] += (double)acc[i][j][e];
  }
  __device__ inline void finish(f32x16 (&acc)[TM][2]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = (float)tot[i][j][e];
  }
};

// ---------------------------------------------------------------------------------------------
// 3x3 halo kernel
// ---------------------------------------------------------------------------------------------
template <typename T, int TH, int TW, int BN>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 1 : 2) void conv3x3_halo_kernel(const ConvLaunch<T> L, const int tiles_x,
                                                           const int tiles_y, const int tiles_n, const int fuse_stats) {
  constexpr int VEC = Elem<T>::kVec;
  constexpr int CH = 8 * VEC;                 // channels per 128-byte pixel row (bf16 64, f32 32)
  constexpr int BKG = ConvTile<T>::BK;        // packed-weight chunk (half a pixel row)
  constexpr int BM = TH * TW;
  constexpr int HP = TW + 2, HALO = (TH + 2) * HP;
  constexpr int NH = (HALO * 8 + 255) / 256;  // halo units per thread
  constexpr int NB = BN * 8 / 256;            // weight units per thread
  constexpr int WAVES_N = BN / 64, WAVES_M = 4 / WAVES_N;
  constexpr int WM = BM / WAVES_M, TM = WM / 32;
  constexpr int CALLS = 8 / Mma<T>::UNITS_PER_CALL;
  static_assert(WM % 32 == 0 && TM >= 1, "wave tile");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* Ah = reinterpret_cast<uint4*>(smem);            // [HALO][8] swizzled 16-byte units
  uint4* Bs = Ah + HALO * 8;                             // [2][BN][8]
  float* stage = reinterpret_cast<float*>(smem);         // epilogue scratch aliases the main-loop images

  const ConvDesc& d = L.d;
  const int nblk = tiles_x * tiles_y * tiles_n * d.B;
  int lin = xcd_remap(blockIdx.x, nblk);
  const int tn = lin % tiles_n; lin /= tiles_n;
  const int tx = lin % tiles_x; lin /= tiles_x;
  const int ty = lin % tiles_y;
  const int b = lin / tiles_y;
  const int y0 = ty * TH, x0 = tx * TW;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l31 = lane & 31, hi = lane >> 5;
  const int Cin = d.C0 + d.C1;
  const int nchunks = Cin / CH;
  const int Hl = d.Hout, Wl = d.Wout;         // 3x3 s1 p1: conv input extent == output extent (after upsample)
  const int slot = tid & 7;                    // this thread always stages unit `slot` of a row (256 % 8 == 0)

  // per-thread halo bookkeeping: source pixel offset (or -1) of each of its halo units
  int64_t hsrc[NH];
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const int hp = (tid >> 3) + k * 32;
    hsrc[k] = -1;
    if (hp < HALO) {
      const int hy = hp / HP, hx = hp - hy * HP;
      int y = y0 - 1 + hy, x = x0 - 1 + hx;
      if ((unsigned)y < (unsigned)Hl && (unsigned)x < (unsigned)Wl) {
        if (d.ups) { y >>= 1; x >>= 1; }
        hsrc[k] = ((int64_t)b * d.Hin + y) * d.Win + x;
      }
    }
  }
  // per-lane fragment rows: tile pixel p -> halo position of tap (0,0)
  int ahp[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int p = wm * WM + i * 32 + l31;
    ahp[i] = (p / TW) * HP + (p % TW);
  }

  Vec16<T> hreg[NH], breg[NB];
  auto gload_halo = [&](int chunk) {
    const int c = chunk * CH + slot * VEC;
    const bool first = c < d.C0;
    const T* base = first ? L.src0 : L.src1;
    const int Cs = first ? d.C0 : d.C1, cc = first ? c : c - d.C0;
#pragma unroll
    for (int k = 0; k < NH; ++k) hreg[k] = hsrc[k] >= 0 ? vec_load(base + hsrc[k] * Cs + cc) : vec_zero<T>();
  };
  auto gload_b = [&](int chunk, int tap) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int n = (tid >> 3) + j * 32;
      const T* p = L.w + ((size_t)(tap * d.kchunks + 2 * chunk + (slot >> 2)) * d.CoutPad + tn * BN + n) * BKG +
                   (slot & 3) * VEC;
      breg[j] = vec_load(p);
    }
  };

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  Wide<T, TM> wacc;
  const int niter = nchunks * 9;
  gload_halo(0);
  gload_b(0, 0);
  int tap = 0, chunk = 0;
  for (int it = 0; it < niter; ++it) {
    if (tap == 0) {
      if (it > 0) __syncthreads();            // every wave is done reading the previous chunk's halo
      // prologue coefficients of this thread's 8 channels (only when fused)
      float pa[VEC], pb[VEC];
      if (L.pro_a) {
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
          pa[u] = L.pro_a[(size_t)b * d.C0 + chunk * CH + slot * VEC + u];
          pb[u] = L.pro_b[(size_t)b * d.C0 + chunk * CH + slot * VEC + u];
        }
      }
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        const int hp = (tid >> 3) + k * 32;
        if (hp < HALO) {
          Vec16<T> v = hreg[k];
          if (L.pro_a && hsrc[k] >= 0) {
#pragma unroll
            for (int u = 0; u < VEC; ++u) v.e[u] = Elem<T>::store(Elem<T>::silu(fmaf(Elem<T>::load(v.e[u]), pa[u], pb[u])));
          }
          Ah[hp * 8 + (slot ^ ((hp >> 1) & 7))] = *reinterpret_cast<const uint4*>(&v);
        }
      }
    }
    uint4* Bb = Bs + (it & 1) * BN * 8;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int n = (tid >> 3) + j * 32;
      Bb[n * 8 + (slot ^ ((n >> 1) & 7))] = *reinterpret_cast<const uint4*>(&breg[j]);
    }
    __syncthreads();
    // next iteration's operands: in flight underneath the MFMAs
    const int ntap = tap == 8 ? 0 : tap + 1, nchunk = tap == 8 ? chunk + 1 : chunk;
    if (it + 1 < niter) gload_b(nchunk, ntap);
    if (tap == 0 && chunk + 1 < nchunks) gload_halo(chunk + 1);

    const int kh = tap / 3, kw = tap - kh * 3;
    const int toff = kh * HP + kw;
    if constexpr (Wide<T>::on) clear_acc<TM>(acc);   // parity mode: this (tap, chunk)'s 32-term partial, then summed in float64
#pragma unroll
    for (int call = 0; call < CALLS; ++call) {
      const int unit = Mma<T>::unit_of(call, hi);
      typename Mma<T>::Frag fa[TM], fb[2];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int hp = ahp[i] + toff;
        fa[i] = Mma<T>::load(Ah + hp * 8 + (unit ^ ((hp >> 1) & 7)));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = wn * 64 + j * 32 + l31;
        fb[j] = Mma<T>::load(Bb + n * 8 + (unit ^ ((n >> 1) & 7)));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) Mma<T>::mma(fa[i], fb[j], acc[i][j], hi);
    }
    wacc.add(acc);
    tap = ntap;
    chunk = nchunk;
  }
  wacc.finish(acc);

  StatAcc<T> gs, gq;
  auto row_to_m = [&](int r) -> int64_t {
    const int p = wm * WM + r;
    return ((int64_t)b * d.Hout + y0 + p / TW) * d.Wout + x0 + p % TW;
  };
  epilogue_store<T, TM>(L, acc, stage + wave * 32 * 68, lane, tn * BN + wn * 64, row_to_m, gs, gq);
  if (fuse_stats) {
    const int nsplit = tiles_x * tiles_y;
    float* dst = L.gn_partials + ((size_t)b * nsplit + ty * tiles_x + tx) * L.gn_groups * 2;
    epilogue_stats<WAVES_M, WAVES_N>(reinterpret_cast<StatAcc<T>*>(stage + 4 * 32 * 68), gs, gq, wave, lane, tn * BN, d.Cout,
                                     L.gn_groups, dst);
  }
}

// ---------------------------------------------------------------------------------------------
// 3x3 halo kernel with MX-fp8 operands (BASELINE configs[4]: "fp8 UNet weights on CDNA4 MFMA")
// ---------------------------------------------------------------------------------------------
// Same tiling as conv3x3_halo_kernel, but both MFMA operands are OCP e4m3 with one E8M0 scale per 32 channels and the
// contraction runs on v_mfma_scale_f32_32x32x64_f8f6f4 (K = 64 = one channel chunk of one tap per instruction: a quarter of
// the bf16 instruction count at twice the rate).  Weights arrive pre-quantised (pack_conv_weight_mxfp8); the bf16
// activations are quantised while the halo is written to LDS, after the optional fused GroupNorm+SiLU prologue: the four
// lanes that hold one pixel's 32 consecutive channels agree on the block maximum with two lane exchanges, the block scale
// is 2^(floor(log2 max) - 8), the elements are rounded by v_cvt_pk_fp8_f32 (saturated at +-448 first).
// Operand layout of the instruction (probed, tools/micro/mx_layout_probe.hip): lane l holds row/column l & 31; its 32
// bytes are k = 16 h + (0..15) and 32 + 16 h + (0..15) with h = l >> 5; lane l's scale covers k in [32 h, 32 h + 32).
// LDS rows are 64 data bytes padded to 80 (conflict-free ds_read_b128), scales sit in a byte array beside them.
typedef __attribute__((ext_vector_type(8))) int mx_i32x8;

__device__ inline uint32_t mx_cvt4(float a, float b, float c, float d) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

template <int TH, int TW, int BN>
__global__ __launch_bounds__(256, 2) void conv3x3_mx_kernel(const ConvLaunch<bf16_t> L, const int tiles_x, const int tiles_y,
                                                            const int tiles_n, const int fuse_stats) {
  using T = bf16_t;
  constexpr int CH = 64;                       // channels per chunk = K of one MFMA
  constexpr int ROWB = 80;                     // LDS row: 64 fp8 + 16 pad
  constexpr int BM = TH * TW;
  constexpr int HP = TW + 2, HALO = (TH + 2) * HP;
  constexpr int NH = (HALO * 8 + 255) / 256;   // halo units (8 channels) per thread
  constexpr int NB = BN * 4 / 256;             // 16-byte weight units per thread (BN rows x 64 B)
  constexpr int WAVES_N = BN / 64, WAVES_M = 4 / WAVES_N;
  constexpr int WM = BM / WAVES_M, TM = WM / 32;
  static_assert(WM % 32 == 0 && TM >= 1 && NB >= 1, "wave tile");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ah = smem;                                        // [HALO][80]
  char* Bw = Ah + HALO * ROWB;                            // [2][BN][80]
  unsigned char* As = reinterpret_cast<unsigned char*>(Bw + 2 * BN * ROWB);   // [HALO][2] block scales
  unsigned char* Bsc = As + ((HALO * 2 + 15) & ~15);      // [2][BN][2]
  float* stage = reinterpret_cast<float*>(smem);          // epilogue scratch aliases the main-loop images

  const ConvDesc& d = L.d;
  const int nblk = tiles_x * tiles_y * tiles_n * d.B;
  int lin = xcd_remap(blockIdx.x, nblk);
  const int tn = lin % tiles_n; lin /= tiles_n;
  const int tx = lin % tiles_x; lin /= tiles_x;
  const int ty = lin % tiles_y;
  const int b = lin / tiles_y;
  const int y0 = ty * TH, x0 = tx * TW;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nchunks = (d.C0 + d.C1) / CH;
  const int Hl = d.Hout, Wl = d.Wout;
  const int slot = tid & 7;

  int64_t hsrc[NH];
#pragma unroll
  for (int k = 0; k < NH; ++k) {
    const int hp = (tid >> 3) + k * 32;
    hsrc[k] = -1;
    if (hp < HALO) {
      const int hy = hp / HP, hx = hp - hy * HP;
      int y = y0 - 1 + hy, x = x0 - 1 + hx;
      if ((unsigned)y < (unsigned)Hl && (unsigned)x < (unsigned)Wl) {
        if (d.ups) { y >>= 1; x >>= 1; }
        hsrc[k] = ((int64_t)b * d.Hin + y) * d.Win + x;
      }
    }
  }
  int ahp[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int p = wm * WM + i * 32 + l31;
    ahp[i] = (p / TW) * HP + (p % TW);
  }

  Vec16<T> hreg[NH];
  uint4 breg[NB];
  uint16_t bsreg = 0;
  auto gload_halo = [&](int chunk) {
    const int c = chunk * CH + slot * 8;
    const bool first = c < d.C0;
    const T* base = first ? L.src0 : L.src1;
    const int Cs = first ? d.C0 : d.C1, cc = first ? c : c - d.C0;
#pragma unroll
    for (int k = 0; k < NH; ++k) hreg[k] = hsrc[k] >= 0 ? vec_load(base + hsrc[k] * Cs + cc) : vec_zero<T>();
  };
  auto gload_b = [&](int chunk, int tap) {
    const size_t tile = (size_t)(tap * nchunks + chunk) * d.CoutPad + (size_t)tn * BN;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int u = tid + j * 256;                          // unit u: row u >> 2, 16-byte piece u & 3
      breg[j] = *reinterpret_cast<const uint4*>(L.w_mx + (tile + (u >> 2)) * 64 + (u & 3) * 16);
    }
    if (tid < BN) bsreg = *reinterpret_cast<const uint16_t*>(L.w_mx_scale + (tile + tid) * 2);
  };

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  const int niter = nchunks * 9;
  gload_halo(0);
  gload_b(0, 0);
  int tap = 0, chunk = 0;
  for (int it = 0; it < niter; ++it) {
    if (tap == 0) {
      if (it > 0) __syncthreads();            // every wave is done reading the previous chunk's halo
      float pa[8], pb[8];
      if (L.pro_a) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          pa[u] = L.pro_a[(size_t)b * d.C0 + chunk * CH + slot * 8 + u];
          pb[u] = L.pro_b[(size_t)b * d.C0 + chunk * CH + slot * 8 + u];
        }
      }
#pragma unroll
      for (int k = 0; k < NH; ++k) {
        const int hp = (tid >> 3) + k * 32;           // (all 8 lanes of a row take the same branch: shuffles are safe)
        if (hp < HALO) {
          float f[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) f[u] = Elem<T>::load(hreg[k].e[u]);
          if (L.pro_a && hsrc[k] >= 0) {
#pragma unroll
            for (int u = 0; u < 8; ++u) f[u] = Elem<T>::load(Elem<T>::store(Elem<T>::silu(fmaf(f[u], pa[u], pb[u]))));
          }
          float am = 0.0f;
#pragma unroll
          for (int u = 0; u < 8; ++u) am = fmaxf(am, fabsf(f[u]));
          am = fmaxf(am, __shfl_xor(am, 1, 64));
          am = fmaxf(am, __shfl_xor(am, 2, 64));      // maximum over the 32 channels of this block (slots 4q .. 4q+3)
          const int E = (int)((__float_as_uint(am) >> 23) & 0xffu);
          const int S = E > 8 ? E - 8 : 0;              // E8M0 scale 2^(S - 127); am == 0 -> S = 0 (elements are 0)
          const float mult = __uint_as_float((uint32_t)(254 - S) << 23);   // 2^(127 - S)
          float g[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) g[u] = fminf(fmaxf(f[u] * mult, -448.0f), 448.0f);
          uint2 w;
          w.x = mx_cvt4(g[0], g[1], g[2], g[3]);
          w.y = mx_cvt4(g[4], g[5], g[6], g[7]);
          *reinterpret_cast<uint2*>(Ah + hp * ROWB + slot * 8) = w;
          if ((slot & 3) == 0) As[hp * 2 + (slot >> 2)] = (unsigned char)S;
        }
      }
    }
    char* Bb = Bw + (it & 1) * BN * ROWB;
    unsigned char* Sb = Bsc + (it & 1) * BN * 2;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int u = tid + j * 256;
      *reinterpret_cast<uint4*>(Bb + (u >> 2) * ROWB + (u & 3) * 16) = breg[j];
    }
    if (tid < BN) *reinterpret_cast<uint16_t*>(Sb + tid * 2) = bsreg;
    __syncthreads();
    const int ntap = tap == 8 ? 0 : tap + 1, nchunk = tap == 8 ? chunk + 1 : chunk;
    if (it + 1 < niter) gload_b(nchunk, ntap);
    if (tap == 0 && chunk + 1 < nchunks) gload_halo(chunk + 1);

    const int kh = tap / 3, kw = tap - kh * 3;
    const int toff = kh * HP + kw;
    mx_i32x8 fa[TM], fb[2];
    int sa[TM], sb[2];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int hp = ahp[i] + toff;
      const uint4 lo = *reinterpret_cast<const uint4*>(Ah + hp * ROWB + hi * 16);
      const uint4 up = *reinterpret_cast<const uint4*>(Ah + hp * ROWB + 32 + hi * 16);
      fa[i] = mx_i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)up.x, (int)up.y, (int)up.z, (int)up.w};
      sa[i] = As[hp * 2 + hi];
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = wn * 64 + j * 32 + l31;
      const uint4 lo = *reinterpret_cast<const uint4*>(Bb + n * ROWB + hi * 16);
      const uint4 up = *reinterpret_cast<const uint4*>(Bb + n * ROWB + 32 + hi * 16);
      fb[j] = mx_i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)up.x, (int)up.y, (int)up.z, (int)up.w};
      sb[j] = Sb[n * 2 + hi];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
    tap = ntap;
    chunk = nchunk;
  }

  StatAcc<T> gs, gq;
  auto row_to_m = [&](int r) -> int64_t {
    const int p = wm * WM + r;
    return ((int64_t)b * d.Hout + y0 + p / TW) * d.Wout + x0 + p % TW;
  };
  epilogue_store<T, TM>(L, acc, stage + wave * 32 * 68, lane, tn * BN + wn * 64, row_to_m, gs, gq);
  if (fuse_stats) {
    const int nsplit = tiles_x * tiles_y;
    float* dst = L.gn_partials + ((size_t)b * nsplit + ty * tiles_x + tx) * L.gn_groups * 2;
    epilogue_stats<WAVES_M, WAVES_N>(reinterpret_cast<StatAcc<T>*>(stage + 4 * 32 * 68), gs, gq, wave, lane, tn * BN, d.Cout,
                                     L.gn_groups, dst);
  }
}

// ---------------------------------------------------------------------------------------------
// generic gather kernel (1x1, 4x4 s2, ragged shapes)
// ---------------------------------------------------------------------------------------------
// ONE: 1x1, stride 1, no padding, no upsampling (the res_convs and the attention projections): output row m reads input
// pixel m, so a thread's gather address is a constant of the thread plus the chunk's channel offset — no coordinates, no
// bounds, no 64-bit multiplies per load (round 3: the gather form issued ~20 VALU instructions per MFMA on these shapes).
template <typename T, int BM, int BN, bool ONE>
__global__ __launch_bounds__(256, sizeof(T) == 4 ? 1 : 2) void conv_igemm_kernel(const ConvLaunch<T> L, const int M, const int tiles_m,
                                                         const int tiles_n, const int fuse_stats, const int wide) {
  constexpr int BK = ConvTile<T>::BK;
  constexpr int VEC = Elem<T>::kVec;
  constexpr int UPR = BK / VEC;              // 16-byte units per tile row (4)
  constexpr int RPP = 256 / UPR;             // rows staged per pass (64)
  constexpr int AP = BM / RPP, BP = BN / RPP;
  constexpr int WAVES_N = BN / 64, WAVES_M = 4 / WAVES_N;
  constexpr int WM = BM / WAVES_M, TM = WM / 32;
  constexpr int CALLS = UPR / Mma<T>::UNITS_PER_CALL;
  static_assert(TM >= 1, "wave tile");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS rows are 64 bytes (4 units), unit u of row r stored at slot u ^ ((r >> 2) & 3) (round 5).  The 80-byte padded rows of
  // rounds 1-4 were conflict-free for the fragment READS but not for the staging WRITES: a ds_write_b128 is serviced in eight
  // groups of 8 contiguous lanes over a 128-byte bank row, two 80-byte rows overlap there, and every write took twice its LDS-array
  // cycles (rocprofv3: SQ_LDS_BANK_CONFLICT / SQ_ACTIVE_INST_LDS 0.90-0.94 on the 1x1 launches, zero on the 3x3 kernels).  With
  // unpadded rows a write group covers exactly one 128-byte bank row (any permutation of the units inside a row keeps that), and
  // the XOR makes the sixteen rows of a ds_read_b128 lane group ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}: four rows per
  // residue mod 4, with four different (r >> 2) & 3) land on sixteen different 16-byte slots of the 256-byte read row.
  uint4* As = reinterpret_cast<uint4*>(smem);   // [2][BM][UPR]
  uint4* Bs = As + 2 * BM * UPR;                // [2][BN][UPR]
  float* stage = reinterpret_cast<float*>(smem);
  constexpr int PITCH = UPR;
  static_assert(UPR == 4, "swizzle assumes 64-byte tile rows");

  const ConvDesc& d = L.d;
  const int lin = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tn = lin % tiles_n, tm = lin / tiles_n;

  const int tid = threadIdx.x;
  const int lrow = tid / UPR, ku = tid % UPR;
  const int Cin = d.C0 + d.C1;
  const int Hl = d.ups ? 2 * d.Hin : d.Hin, Wl = d.ups ? 2 * d.Win : d.Win;
  const int HWo = d.Hout * d.Wout;

  int a_iy0[AP], a_ix0[AP];
  int64_t a_base[AP];
  bool a_ok[AP];
  const T* a_p0[AP];                          // ONE: address of channel ku * VEC of this thread's pixel in src0 / src1
  const T* a_p1[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int m = tm * BM + lrow + i * RPP;
    a_ok[i] = m < M;
    const int mm = a_ok[i] ? m : 0;
    if constexpr (ONE) {
      a_p0[i] = L.src0 + (int64_t)mm * d.C0 + ku * VEC;
      a_p1[i] = d.C1 ? L.src1 + (int64_t)mm * d.C1 + ku * VEC - d.C0 : a_p0[i];
    } else {
      const int bb = mm / HWo, rem = mm - bb * HWo;
      const int oy = rem / d.Wout, ox = rem - oy * d.Wout;
      a_iy0[i] = oy * d.stride - d.pad;
      a_ix0[i] = ox * d.stride - d.pad;
      a_base[i] = (int64_t)bb * d.Hin * d.Win;
    }
  }

  // TWO register stages (round 4): the loads of iteration it + 2 are issued while iteration it computes, so a load has two
  // iterations (two barriers, 16 MFMAs per wave) to land instead of one — with one stage the 8 MFMAs of an iteration covered
  // a fraction of the L2 / HBM latency and the 1x1 convs ran at 0.3-0.4 PFLOP/s
  // (native 16-byte vectors: arrays of the Vec16 / uint4 STRUCTS are split into 16-bit pieces or kept in scratch by hipcc 7.2)
  typedef __attribute__((ext_vector_type(4))) unsigned int stg_t;
  auto ldg = [](const T* p) { return *reinterpret_cast<const stg_t*>(p); };
  stg_t ra0[AP], rb0[BP], ra1[AP], rb1[BP];
  unsigned ok0 = 0, ok1 = 0;                               // bit i: unit i of the stage is inside the tensor
  const int niter = d.KH * d.KW * d.kchunks;
  auto gload = [&](stg_t(&ra)[AP], stg_t(&rb)[BP], unsigned& okm, int tap, int kc) {
    okm = 0;
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    const int c = kc * BK + ku * VEC;
    if constexpr (ONE) {
#pragma unroll
      for (int i = 0; i < AP; ++i) {
        // branch-free (an always-mapped stand-in address; the unit is zeroed by its mask when it is staged): with loads under a
        // branch hipcc's s_waitcnt placement falls back to vmcnt(0) and the second register stage would buy nothing
        const bool ok = a_ok[i] && c < Cin;
        const T* p = (c < d.C0 ? a_p0[i] : a_p1[i]) + kc * BK;
        ra[i] = ldg(ok ? p : L.src0);
        okm |= (ok ? 1u : 0u) << i;
      }
    } else
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      int iy = a_iy0[i] + kh, ix = a_ix0[i] + kw;
      const bool ok = a_ok[i] && (unsigned)iy < (unsigned)Hl && (unsigned)ix < (unsigned)Wl && c < Cin;
      if (d.ups) { iy >>= 1; ix >>= 1; }
      const int64_t pix = ok ? a_base[i] + (int64_t)iy * d.Win + ix : 0;
      const T* p = (c < d.C0) ? L.src0 + pix * d.C0 + c : L.src1 + pix * d.C1 + (c - d.C0);
      ra[i] = ldg(ok ? p : L.src0);                        // (branch-free, as above)
      okm |= (ok ? 1u : 0u) << i;
    }
    const T* wt = L.w + ((size_t)(tap * d.kchunks + kc) * d.CoutPad + (size_t)tn * BN) * BK;
#pragma unroll
    for (int j = 0; j < BP; ++j) rb[j] = ldg(wt + (size_t)(j * 256 + tid) * VEC);
  };

  const int wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WAVES_N, wn = wave % WAVES_N;
  const int l31 = lane & 31, hi = lane >> 5;
  const int ku_sw = ku ^ ((lrow >> 2) & 3);                  // staging slot of this thread's unit (rows lrow + 64 k: same key)
  const int sw_r = (l31 >> 2) & 3;
  static_assert(RPP % 16 == 0 && WM % 16 == 0, "swizzle key must not depend on the pass / wave tile");

  f32x16 acc[TM][2];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;

  Wide<T, TM> wacc;
  // coordinates of the NEXT load to issue; past the end they stay on the last chunk (harmless reloads that nobody stages): the
  // loop body then has no branch between a load and its use and the compiler's s_waitcnt vmcnt(N) counts are exact — with the
  // re-issue under `if (it + 2 < niter)` it waited for vmcnt(0) at every staging write
  int tap = 0, kc = 0, nxt = 0;
  auto advance = [&]() {
    const bool more = nxt + 1 < niter;
    nxt += more ? 1 : 0;
    const int k2 = kc + 1, wrap = k2 == d.kchunks;
    kc = more ? (wrap ? 0 : k2) : kc;
    tap = more ? tap + wrap : tap;
  };
  gload(ra0, rb0, ok0, tap, kc);
  advance();
  gload(ra1, rb1, ok1, tap, kc);
  advance();
  // one iteration: stage `it` (registers loaded two iterations ago) -> LDS buffer it & 1, barrier, re-issue the registers for
  // iteration it + 2, then the MFMAs
  auto step = [&](stg_t(&ra)[AP], stg_t(&rb)[BP], unsigned& okm, int it) {
    uint4* Ab = As + (it & 1) * BM * PITCH;
    uint4* Bb = Bs + (it & 1) * BN * PITCH;
#pragma unroll
    for (int i = 0; i < AP; ++i) {
      const unsigned m = 0u - ((okm >> i) & 1u);           // all ones / zero: padding, rows past M, channels past Cin
      *reinterpret_cast<stg_t*>(Ab + (lrow + i * RPP) * PITCH + ku_sw) = ra[i] & m;
    }
#pragma unroll
    for (int j = 0; j < BP; ++j) *reinterpret_cast<stg_t*>(Bb + (lrow + j * RPP) * PITCH + ku_sw) = rb[j];
    __syncthreads();
    gload(ra, rb, okm, tap, kc);
    advance();
    if constexpr (Wide<T>::on) clear_acc<TM>(acc);   // parity mode: 16-term partials summed in float64
#pragma unroll
    for (int call = 0; call < CALLS; ++call) {
      const int unit = Mma<T>::unit_of(call, hi) ^ sw_r;     // (rows wm * WM + i * 32 + l31: the swizzle key is (l31 >> 2) & 3)
      typename Mma<T>::Frag fa[TM], fb[2];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = Mma<T>::load(Ab + (wm * WM + i * 32 + l31) * PITCH + unit);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = Mma<T>::load(Bb + (wn * 64 + j * 32 + l31) * PITCH + unit);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) Mma<T>::mma(fa[i], fb[j], acc[i][j], hi);
    }
    wacc.add(acc);
  };
  for (int it = 0; it + 1 < niter; it += 2) {
    step(ra0, rb0, ok0, it);
    step(ra1, rb1, ok1, it + 1);
  }
  if (niter & 1) step(ra0, rb0, ok0, niter - 1);
  wacc.finish(acc);

  if (wide) {
    StatAcc<T> gs, gq;
    auto row_to_m = [&](int r) -> int64_t {
      const int m = tm * BM + wm * WM + r;
      return m < M ? (int64_t)m : (int64_t)-1;
    };
    epilogue_store<T, TM>(L, acc, stage + wave * 32 * 68, lane, tn * BN + wn * 64, row_to_m, gs, gq);
    if (fuse_stats) {
      const int nsplit = HWo / BM;
      const int bimg = (tm * BM) / HWo, slab = tm - bimg * nsplit;
      float* dst = L.gn_partials + ((size_t)bimg * nsplit + slab) * L.gn_groups * 2;
      epilogue_stats<WAVES_M, WAVES_N>(reinterpret_cast<StatAcc<T>*>(stage + 4 * 32 * 68), gs, gq, wave, lane, tn * BN, d.Cout,
                                       L.gn_groups, dst);
    }
  } else {
    // narrow fallback (Cout not a multiple of 8): C/D layout col = lane & 31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = tn * BN + wn * 64 + j * 32 + l31;
      if (col >= d.Cout) continue;
      const float bv = L.bias ? L.bias[col] : 0.0f;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = tm * BM + wm * WM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hi;
          if (row < M) {
            float v = acc[i][j][e] + bv;
            const size_t o = (size_t)row * d.Cout + col;
            if (L.residual) v += Elem<T>::load(L.residual[o]);
            L.out[o] = Elem<T>::store(v);
          }
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------------------------

// dynamic LDS of the generic kernels: their staging buffers, at least the shared epilogue's scratch
constexpr size_t staging_lds(size_t bytes) { return bytes < kEpilogueLds ? kEpilogueLds : bytes; }

// conv3x3_halo_kernel<T, TH, TW, BN>: the four tiles pick_halo (conv_choose.cpp) hands out
template <typename T>
static int launch_conv_halo(const ConvChoice& c, const ConvLaunch<T>& L, hipStream_t s) {
#define PRG_HALO(TH, TW, BN) \
  {conv_key(TH, TW, BN), &conv3x3_halo_kernel<T, TH, TW, BN>, 256, staging_lds((size_t)((TH + 2) * (TW + 2) * 8 + 2 * BN * 8) * 16), 0}
  static ConvKernel<ConvTileKernel<T>> tab[] = {PRG_HALO(8, 32, 64), PRG_HALO(4, 32, 128), PRG_HALO(8, 16, 128), PRG_HALO(8, 16, 64)};
#undef PRG_HALO
  return launch_conv_tiles(tab, conv_key(c.th, c.tw, c.bn), "halo conv", c, L, s);
}
// conv3x3_mx_kernel<TH, TW, BN>: MX-fp8 operands on the same tiles (PRG_MX_PURE)
static int launch_conv_mx_halo(const ConvChoice& c, const ConvLaunch<bf16_t>& L, hipStream_t s) {
#define PRG_MX(TH, TW, BN)                                                                                                              \
  {conv_key(TH, TW, BN), &conv3x3_mx_kernel<TH, TW, BN>, 256,                                                                           \
   staging_lds((size_t)(TH + 2) * (TW + 2) * 80 + (size_t)2 * BN * 80 + (((TH + 2) * (TW + 2) * 2 + 15) & ~15) + 2 * BN * 2 + 16), 0}
  static ConvKernel<ConvTileKernel<bf16_t>> tab[] = {PRG_MX(8, 32, 64), PRG_MX(4, 32, 128), PRG_MX(8, 16, 128), PRG_MX(8, 16, 64)};
#undef PRG_MX
  return launch_conv_tiles(tab, conv_key(c.th, c.tw, c.bn), "mx halo conv", c, L, s);
}

// conv_igemm_kernel<T, BM, BN, ONE>; mode = ONE (1x1, stride 1, no padding: the gather is a plain row read)
template <typename T>
static int launch_conv_igemm(const ConvChoice& c, const ConvLaunch<T>& L, hipStream_t s) {
  using Fn = void (*)(const ConvLaunch<T>, int, int, int, int, int);   // (L, M, tiles_m, tiles_n, fuse_stats, wide)
  constexpr int UPR = ConvTile<T>::BK / Elem<T>::kVec;
#define PRG_IGEMM(BM, BN)                                                                                                 \
  {conv_key(BM, BN, 1), &conv_igemm_kernel<T, BM, BN, true>, 256, staging_lds((size_t)2 * (BM + BN) * UPR * 16), 0},      \
  {conv_key(BM, BN, 0), &conv_igemm_kernel<T, BM, BN, false>, 256, staging_lds((size_t)2 * (BM + BN) * UPR * 16), 0}
  ConvKernel<Fn>* e = nullptr;
  int rc;
  if constexpr (std::is_same<T, bf16_t>::value) {            // (the 256 x 128 tile exists in bf16 only)
    static ConvKernel<Fn> tab[] = {PRG_IGEMM(256, 128), PRG_IGEMM(128, 128), PRG_IGEMM(256, 64), PRG_IGEMM(128, 64)};
    rc = conv_kernel_find(tab, conv_key(c.bm, c.bn, c.mode), "implicit-GEMM conv", &e);
  } else {
    static ConvKernel<Fn> tab[] = {PRG_IGEMM(128, 128), PRG_IGEMM(256, 64), PRG_IGEMM(128, 64)};
    rc = conv_kernel_find(tab, conv_key(c.bm, c.bn, c.mode), "implicit-GEMM conv", &e);
  }
#undef PRG_IGEMM
  if (rc) return rc;
  e->fn<<<dim3(c.grid), e->block, e->lds, s>>>(L, L.d.B * L.d.Hout * L.d.Wout, c.tiles_x, c.tiles_n, c.fuse_stats, L.d.Cout % 8 == 0);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

static int launch_family(const ConvChoice& c, const ConvLaunch<float>& L, hipStream_t s) {
  switch (c.family) {
    case kConvSplitW512: return launch_conv_split_w512(c, L, s);
    case kConvSplitHalo: case kConvSplitWs: case kConvSplitP64: case kConvSplitIgemm: return launch_conv_split(c, L, s);
    case kConvHalo: return launch_conv_halo(c, L, s);
    case kConvIgemm: return launch_conv_igemm(c, L, s);
    default: return fail(PRG_E_STATE, "conv: the selection named a family that has no float kernels");
  }
}

static int launch_family(const ConvChoice& c, const ConvLaunch<bf16_t>& L, hipStream_t s) {
  switch (c.family) {
    case kConvC64: return launch_conv_c64(c, L, s);
    case kConvWs: return launch_conv_ws(c, L, s);
    case kConvW256: case kConvW256Mx: return launch_conv_w256(c, L, s);
    case kConvMxHalo: return launch_conv_mx_halo(c, L, s);
    case kConvHalo: return launch_conv_halo(c, L, s);
    case kConvIgemm: return launch_conv_igemm(c, L, s);
    default: return fail(PRG_E_STATE, "conv: the selection named a family that has no bf16 kernels");
  }
}
// The one place that reads the selection's switches (each pins an alternative schedule that a test compares against the default).
const ConvSwitches& conv_switches() {
  static const ConvSwitches sw = [] {
    ConvSwitches v;
    v.conv_ws = env_int("PRG_CONV_WS", 1);
    v.conv_c64 = env_int("PRG_CONV_C64", 1);
    v.conv_w256 = env_int("PRG_CONV_W256", 1);
    v.conv_down_w256 = env_int("PRG_CONV_DOWN_W256", 1);
    v.conv_w256mx = env_int("PRG_CONV_W256MX", 1);
    v.w256_min_tiles = env_int("PRG_W256_MIN_TILES", 0);
    v.up2x2 = env_int("PRG_UP2X2", 1);
    v.h16 = env_int("PRG_H16", 1);
    v.mx_pure = env_int("PRG_MX_PURE", 0);
    v.split_up2x2 = env_int("PRG_SPLIT_UP2X2", 0);
    v.split_p64 = env_int("PRG_SPLIT_P64", 256);
    v.split_w512 = env_int("PRG_SPLIT_W512", 1);
    return v;
  }();
  return sw;
}

bool conv_h16_pair_ok(const ConvLaunch<bf16_t>& L1, const ConvLaunch<bf16_t>& L2) {
  return choose_h16_pair(conv_facts(L1), conv_facts(L2), device_cu_count(), conv_switches());
}

// validate, choose, fill the coefficient tables if the chosen kernel reads them, launch
template <typename T>
int launch_conv(const ConvLaunch<T>& Lin, hipStream_t s, int* gn_nsplit_out, int* acc_done, ConvChoice* chosen) {
  if (acc_done) *acc_done = 0;
  if (gn_nsplit_out) *gn_nsplit_out = 0;
  const ConvDesc& d = Lin.d;
  constexpr int VEC = Elem<T>::kVec;
  PRG_CHECK(Lin.src0 && Lin.w && Lin.out, "conv: null pointer");
  PRG_CHECK(d.C0 % VEC == 0 && d.C1 % VEC == 0, "conv: channel counts must be multiples of the 16-byte vector");
  PRG_CHECK(d.C1 == 0 || Lin.src1, "conv: second source missing");
  PRG_CHECK(!Lin.res_a || (Lin.residual && Lin.res_b && d.KH == 1 && d.KW == 1 && d.Cout % 8 == 0),
            "conv: the activated residual is a 1x1 (implicit-GEMM, wide epilogue) feature");
  PRG_CHECK(!Lin.res_fold.acc || (Lin.residual && d.KH == 1 && d.KW == 1 && d.Cout % 8 == 0 && Lin.res_fold.cpg % 8 == 0 &&
                                  Lin.res_fold.G * Lin.res_fold.cpg == d.Cout && Lin.res_fold.P && Lin.res_fold.Q),
            "conv: the folded activated residual needs a 1x1 conv whose 8-channel vectors lie inside one GroupNorm group");
  PRG_CHECK(d.CoutPad % 64 == 0 && d.CoutPad >= d.Cout, "conv: bad CoutPad");
  const int64_t M64 = (int64_t)d.B * d.Hout * d.Wout;
  PRG_CHECK(M64 > 0 && M64 < (int64_t)1 << 31, "conv: M out of range");

  const ConvChoice c = choose_conv(conv_facts(Lin), device_cu_count(), conv_switches());
  if (c.family == kConvNone) return fail(PRG_E_INVALID, c.why);

  ConvLaunch<T> L = Lin;
  if constexpr (std::is_same<T, bf16_t>::value) {
    if (c.fill_tables) {
      // Consumers without the in-kernel GroupNorm fold (common.h, GnFold): fill the pro_a / pro_b tables from the accumulators
      // with one small launch, then run on the tables as before.
      PRG_CHECK(L.pro_a && L.pro_b, "conv: pro_fold needs scratch coefficient tables in pro_a / pro_b");
      if (int rc = launch_gn_coeff_acc(L.pro_fold, const_cast<float*>(L.pro_a), const_cast<float*>(L.pro_b), d.B, d.C0, s)) return rc;
      L.pro_fold.acc = nullptr;
    }
  }
  if (int rc = launch_family(c, L, s)) return rc;
  if (gn_nsplit_out) *gn_nsplit_out = c.nsplit;
  if (acc_done) *acc_done = c.acc_done;
  if (chosen) *chosen = c;
  return PRG_OK;
}

template int launch_conv<float>(const ConvLaunch<float>&, hipStream_t, int*, int*, ConvChoice*);
template int launch_conv<bf16_t>(const ConvLaunch<bf16_t>&, hipStream_t, int*, int*, ConvChoice*);

// ---------------------------------------------------------------------------------------------
// stem: 7x7 pad 3 direct conv, float32 NCHW in (Cin 1 or 3) -> T NHWC out (sd:824 / dc:822)
// ---------------------------------------------------------------------------------------------
template <typename T, int CIN>
__global__ __launch_bounds__(256) void stem_conv_kernel(const float* __restrict__ x, const float* __restrict__ wk,
                                                        const float* __restrict__ bias, T* __restrict__ out, int H,
                                                        int W, int Cout) {
  constexpr int TS = 16, HALO = 3, TW = TS + 2 * HALO;  // 22
  __shared__ float tile[CIN * TW * TW];
  const int b = blockIdx.z, ty0 = blockIdx.y * TS, tx0 = blockIdx.x * TS;
  const int tid = threadIdx.x;
  for (int i = tid; i < CIN * TW * TW; i += 256) {
    int c = i / (TW * TW), rem = i - c * TW * TW;
    int yy = ty0 + rem / TW - HALO, xx = tx0 + rem % TW - HALO;
    tile[i] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? x[((size_t)b * CIN + c) * H * W + (size_t)yy * W + xx] : 0.0f;
  }
  __syncthreads();
  const int ly = tid / TS, lx = tid % TS;
  const int oy = ty0 + ly, ox = tx0 + lx;
  const bool ok = oy < H && ox < W;
  T* o = out + (((size_t)b * H + (ok ? oy : 0)) * W + (ok ? ox : 0)) * Cout;
  // the weight index is wave-uniform: the compiler reads it with scalar loads, so the inner loop is 1 LDS read per
  // 8 FMAs.  Accumulation order = (cin, kh, kw) ascending fmaf chain.
#pragma unroll 1
  for (int co = 0; co < Cout; co += 8) {
    float acc[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc[u] = 0.0f;
#pragma unroll 1
    for (int c = 0; c < CIN; ++c)
#pragma unroll
      for (int kh = 0; kh < 7; ++kh)
#pragma unroll
        for (int kw = 0; kw < 7; ++kw) {
          const float v = tile[c * TW * TW + (ly + kh) * TW + lx + kw];
          const float* wp = wk + ((kh * 7 + kw) * CIN + c) * Cout + co;
#pragma unroll
          for (int u = 0; u < 8; ++u) acc[u] = fmaf(v, wp[u], acc[u]);
        }
    if (ok) {
#pragma unroll
      for (int u = 0; u < 8; ++u) o[co + u] = Elem<T>::store(acc[u] + bias[co + u]);
    }
  }
}

template <typename T>
int launch_stem_conv(const float* x, const float* wk, const float* bias, T* out, int B, int Cin, int H, int W,
                     int Cout, hipStream_t s) {
  PRG_CHECK(Cin == 1 || Cin == 3, "stem conv: Cin must be 1 or 3");
  PRG_CHECK(Cout % 8 == 0, "stem conv: Cout must be a multiple of 8");
  dim3 grid(ceil_div(W, 16), ceil_div(H, 16), B);
  if (Cin == 1)
    stem_conv_kernel<T, 1><<<grid, 256, 0, s>>>(x, wk, bias, out, H, W, Cout);
  else
    stem_conv_kernel<T, 3><<<grid, 256, 0, s>>>(x, wk, bias, out, H, W, Cout);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}
template int launch_stem_conv<float>(const float*, const float*, const float*, float*, int, int, int, int, int,
                                     hipStream_t);
template int launch_stem_conv<bf16_t>(const float*, const float*, const float*, bf16_t*, int, int, int, int, int,
                                      hipStream_t);

// ---------------------------------------------------------------------------------------------
// stem on MFMA (bf16 path, Cin = 1, Cout = 64): the direct kernel above is VALU-bound (3136 FMA per pixel: 192 us at
// B = 64, 128 x 128); as a GEMM with K = 7 kernel rows x 8 columns (column 7 and row 7 are zero weights) it is
// HBM-bound on its 134 MB output.  x and the weights are split into bf16 hi + lo parts (x_hi W_hi + x_lo W_hi +
// x_hi W_lo: ~16 significant bits, the fp32 input is NOT rounded to bf16).  A block owns 32 x 8 pixels: the input
// window goes to LDS once, is expanded to P[row][px] = the 8 consecutive columns px-3 .. px+4 as one 16-byte
// fragment (hi and lo), and each wave runs 12 MFMAs per 32-pixel row against register-resident weight fragments.
// ---------------------------------------------------------------------------------------------

// CIN = 1: the denoiser's stem; CIN = 3 (round 5): MaskUnet's stem over the three DepthAugment planes (dc:822) — the same GEMM per
// input plane, one plane after the other through the same LDS images, the accumulators of the block's eight rows kept in registers
// (the direct kernel took 541 us per call with 3.9e7 LDS bank conflicts: VERDICT round 4, weak item 11).
// SPLIT (round 5, dtype f16x3): the same kernel on f16 hi + lo halves (22 significant bits, v_mfma_f32_32x32x16_f16) with a float32
// NHWC output — the f16x3 mode's stem ran on the direct fmaf kernel (194 us per evaluation at B = 64, 128 x 128: VALU-bound); the
// weights carry the split packer's per-output-channel power-of-two scale (conv_split.hip), undone on the float32 total (`wscale`).
template <int CIN, bool SPLIT>
__global__ __launch_bounds__(256) void stem_mfma_kernel(const float* __restrict__ x, const uint16_t* __restrict__ wf,
                                                        const float* __restrict__ bias, const float* __restrict__ wscale,
                                                        void* __restrict__ outv, int H, int W) {
  using E = typename std::conditional<SPLIT, _Float16, __bf16>::type;
  using EV = typename std::conditional<SPLIT, f16x8, bf16x8>::type;
  using OT = typename std::conditional<SPLIT, float, uint16_t>::type;
  constexpr int ROWS = 8, PR = ROWS + 7, RC = 40, LDS_ST = SPLIT ? 68 : 72;
  __shared__ float raw[(ROWS + 6) * RC];
  __shared__ __attribute__((aligned(16))) E Ph[PR * 32 * 8];
  __shared__ __attribute__((aligned(16))) E Pl[PR * 32 * 8];
  __shared__ __attribute__((aligned(16))) OT stage[64 * LDS_ST];
  OT* const out = reinterpret_cast<OT*>(outv);
  const int b = blockIdx.z, y0 = blockIdx.y * ROWS, x0 = blockIdx.x * 32, tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
  const int rt = wave & 1, prow = wave >> 1;     // 32-channel row tile; which row of the row pair
  f32x16 acc[ROWS / 2];
#pragma unroll
  for (int ti = 0; ti < ROWS / 2; ++ti)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[ti][e] = 0.0f;
#pragma unroll 1
  for (int c = 0; c < CIN; ++c) {
    if (c > 0) __syncthreads();                  // the previous plane's fragments are consumed
    for (int i = tid; i < (ROWS + 6) * RC; i += 256) {
      const int r = i / RC, cc = i - r * RC;
      const int yy = y0 - 3 + r, xx = x0 - 4 + cc;
      raw[i] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? x[(((size_t)b * CIN + c) * H + yy) * W + xx] : 0.0f;
    }
    __syncthreads();
    for (int e = tid; e < PR * 32; e += 256) {
      const int r = e >> 5, p = e & 31;
      EV vh, vl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = r < ROWS + 6 ? raw[r * RC + p + 1 + j] : 0.0f;      // row ROWS+6 only meets the zero weight row
        const E h16 = (E)v;
        vh[j] = h16;
        vl[j] = (E)(v - (float)h16);
      }
      *reinterpret_cast<EV*>(Ph + e * 8) = vh;
      *reinterpret_cast<EV*>(Pl + e * 8) = vl;
    }
    EV whi[4], wlo[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      whi[kk] = *reinterpret_cast<const EV*>(wf + (((((size_t)c * 2 + rt) * 2 + 0) * 4 + kk) * 64 + lane) * 8);
      wlo[kk] = *reinterpret_cast<const EV*>(wf + (((((size_t)c * 2 + rt) * 2 + 1) * 4 + kk) * 64 + lane) * 8);
    }
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < ROWS / 2; ++ti) {
      const int row = 2 * ti + prow;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int pr = row + 2 * kk + hi;           // kernel row 2 kk + hi of output row `row`
        const EV bh = *reinterpret_cast<const EV*>(Ph + (pr * 32 + l31) * 8);
        const EV bl = *reinterpret_cast<const EV*>(Pl + (pr * 32 + l31) * 8);
        if constexpr (SPLIT) {
          acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wlo[kk], bh, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi[kk], bl, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_f16(whi[kk], bh, acc[ti], 0, 0, 0);
        } else {
          acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo[kk], bh, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi[kk], bl, acc[ti], 0, 0, 0);
          acc[ti] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(whi[kk], bh, acc[ti], 0, 0, 0);
        }
      }
    }
  }
  float bv[16], sv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    bv[r] = bias[rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi];
    sv[r] = SPLIT ? wscale[rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi] : 1.0f;
  }
#pragma unroll
  for (int ti = 0; ti < ROWS / 2; ++ti) {
    // lane: pixel l31 of row 2 ti + prow, channels rt*32 + 8 g4 + 4 hi + {0..3}
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      if constexpr (SPLIT) {
        float4 w;
        w.x = acc[ti][4 * g4] * sv[4 * g4] + bv[4 * g4];
        w.y = acc[ti][4 * g4 + 1] * sv[4 * g4 + 1] + bv[4 * g4 + 1];
        w.z = acc[ti][4 * g4 + 2] * sv[4 * g4 + 2] + bv[4 * g4 + 2];
        w.w = acc[ti][4 * g4 + 3] * sv[4 * g4 + 3] + bv[4 * g4 + 3];
        *reinterpret_cast<float4*>(stage + (prow * 32 + l31) * LDS_ST + rt * 32 + 8 * g4 + 4 * hi) = w;
      } else {
        uint2 w;
        w.x = pack_bf16(acc[ti][4 * g4] + bv[4 * g4], acc[ti][4 * g4 + 1] + bv[4 * g4 + 1]);
        w.y = pack_bf16(acc[ti][4 * g4 + 2] + bv[4 * g4 + 2], acc[ti][4 * g4 + 3] + bv[4 * g4 + 3]);
        *reinterpret_cast<uint2*>(stage + (prow * 32 + l31) * LDS_ST + rt * 32 + 8 * g4 + 4 * hi) = w;
      }
    }
    __syncthreads();
    constexpr int EPV = SPLIT ? 4 : 8, UPP = 64 / EPV;   // elements per 16-byte vector; vectors per pixel
#pragma unroll
    for (int i = 0; i < 64 * UPP / 256; ++i) {
      const int v = tid + 256 * i;
      const int px = v / UPP, u = v % UPP;
      const int yy = y0 + 2 * ti + (px >> 5), xx = x0 + (px & 31);
      *reinterpret_cast<uint4*>(out + (((size_t)b * H + yy) * W + xx) * 64 + u * EPV) =
          *reinterpret_cast<const uint4*>(stage + px * LDS_ST + u * EPV);
    }
    __syncthreads();
  }
}

bool stem_conv_mfma_supported(int Cin, int Cout, int H, int W) { return (Cin == 1 || Cin == 3) && Cout == 64 && W % 32 == 0 && H % 8 == 0; }

// wf: [Cin][2 row tiles][hi | lo][4 k-steps][64 lanes][8] bf16 = the A fragments of W[co][c][kh][kw] (pack_stem_mfma_weights)
int launch_stem_conv_mfma(const float* x, const bf16_t* wf, const float* bias, bf16_t* out, int B, int Cin, int H, int W,
                          hipStream_t s) {
  PRG_CHECK(stem_conv_mfma_supported(Cin, 64, H, W) && x && wf && bias && out, "stem conv (MFMA): bad arguments");
  const uint16_t* w16 = reinterpret_cast<const uint16_t*>(wf);
  if (Cin == 1) stem_mfma_kernel<1, false><<<dim3(W / 32, H / 8, B), 256, 0, s>>>(x, w16, bias, nullptr, out, H, W);
  else stem_mfma_kernel<3, false><<<dim3(W / 32, H / 8, B), 256, 0, s>>>(x, w16, bias, nullptr, out, H, W);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

// f16x3: the same fragments as f16 hi / lo halves (pack_stem_mfma_weights_split), float32 output, wscale[64] undoes the packer's scale
int launch_stem_conv_mfma_split(const float* x, const uint16_t* wf, const float* bias, const float* wscale, float* out, int B, int Cin,
                                int H, int W, hipStream_t s) {
  PRG_CHECK(stem_conv_mfma_supported(Cin, 64, H, W) && x && wf && bias && wscale && out, "stem conv (split MFMA): bad arguments");
  if (Cin == 1) stem_mfma_kernel<1, true><<<dim3(W / 32, H / 8, B), 256, 0, s>>>(x, wf, bias, wscale, out, H, W);
  else stem_mfma_kernel<3, true><<<dim3(W / 32, H / 8, B), 256, 0, s>>>(x, wf, bias, wscale, out, H, W);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

// ---------------------------------------------------------------------------------------------
// head: 1x1 conv to one channel (+ sigmoid), T NHWC -> float32 (sd:918 / dc:868-869)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void head_conv_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                 float* __restrict__ out, int64_t M, int C, int sigmoid) {
  constexpr int VEC = Elem<T>::kVec;
  // LP lanes cooperate on one pixel: each takes a 16-byte vector, then a shuffle tree sums the partials
  const int LP = C / VEC >= 64 ? 64 : (C / VEC >= 32 ? 32 : (C / VEC >= 16 ? 16 : (C / VEC >= 8 ? 8 : (C / VEC >= 4 ? 4 : (C / VEC >= 2 ? 2 : 1)))));
  const int per_block = 256 / LP;
  const int sub = threadIdx.x % LP;
  for (int64_t m = (int64_t)blockIdx.x * per_block + threadIdx.x / LP; m < M; m += (int64_t)gridDim.x * per_block) {
    float acc = 0.0f;
    for (int c = sub * VEC; c < C; c += LP * VEC) {
      Vec16<T> v = vec_load(x + m * C + c);
#pragma unroll
      for (int u = 0; u < VEC; ++u) acc = fmaf(Elem<T>::load(v.e[u]), w[c + u], acc);
    }
    for (int o = LP >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (sub == 0) {
      float v = acc + bias[0];
      out[m] = sigmoid ? sigmoid_f(v) : v;
    }
  }
}

template <typename T>
int launch_head_conv(const T* x, const float* w, const float* bias, float* out, int64_t M, int C, int sigmoid,
                     hipStream_t s) {
  PRG_CHECK(C % Elem<T>::kVec == 0, "head conv: C must be a multiple of the vector width");
  int grid = (int)((M + 31) / 32);
  if (grid > 8192) grid = 8192;
  head_conv_kernel<T><<<grid, 256, 0, s>>>(x, w, bias, out, M, C, sigmoid);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}
template int launch_head_conv<float>(const float*, const float*, const float*, float*, int64_t, int, int, hipStream_t);
template int launch_head_conv<bf16_t>(const bf16_t*, const float*, const float*, float*, int64_t, int, int,
                                      hipStream_t);

}  // namespace prg
