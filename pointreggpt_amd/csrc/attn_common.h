// attn_common.h — what the matrix-pipe attention kernels (attn_fused.hip: bf16, attn_split.hip: f16x3) and the fused ResnetBlock
// tail (resblock_tail.hip) share: the tile constants, the slab rule of linear attention, the 32x32x16 MFMA's operand and
// accumulator layout as functions, the weight fragments a wave keeps in registers, the assignment of output tiles to waves and the
// dynamic-LDS opt-in.  A piece is shared only where the gfx950 listing of a per-tile kernel stays what it was with the piece
// written out (profiles/attn_refactor_ab.txt, which also lists what therefore stays written out).
// MFMA 32x32x16 (bf16 or f16): D[i][j] = sum_k A[i][k] B[k][j]; lane l supplies A[l&31][8(l>>5)..+7] and B[8(l>>5)..+7][l&31]
// and receives D[acc_row(r, l>>5)][l&31] in register r.
#pragma once
#include "blocks.h"
#include "wave_ops.h"

namespace prg {

constexpr int kTP = 64;                   // pixels per tile
constexpr int kTilesPerBlock = 8;
constexpr int kLdO = kHidden + 8;         // LDS row stride of the 128-wide attention-output rows (16-bit elements)
constexpr float kLnEps = 1e-5f;
constexpr float kQScale = 0.17677669529663687f;   // kDimHead^-1/2

// Linear attention: tiles per block as a function of the image size ONLY (a batch-independent slab structure keeps a
// scene's result identical for every batch size): 8 from 64 x 64 pixels up, fewer for the small levels, whose launches
// otherwise fill a quarter of the CUs with blocks that walk four tiles in series (16 x 16: 64 blocks -> 256).
// (measured round 3: 16 or 32 tiles per la_ctx block 73-75 against 72 us, 4 or 16 per la_out block 105-108 against 99 us)
// The slab structure of la_kmax / la_ctx's partials; la_out's pixels are independent (any partition) and use the same rule.
__host__ __device__ inline int tiles_per_block(int ntiles) {
  const int t = ntiles / 8;
  return t < 1 ? 1 : (t > kTilesPerBlock ? kTilesPerBlock : t);
}
inline int slabs(int N) { const int nt = ceil_div(N, kTP); return ceil_div(nt, tiles_per_block(nt)); }

__device__ inline f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.0f;
  return z;
}

// sum over the four lanes of a quad (quad_perm [1,0,3,2] then [2,3,0,1]), every lane gets the total
__device__ inline float quad_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  return v;
}

// row of the 32 x 32 accumulator tile that register r of a lane in half hi holds
__device__ inline int acc_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// The k-slot order: position of row d (of 32) in an operand whose contraction index is fed STRAIGHT FROM ACCUMULATOR REGISTERS.
// k-slot s of half hi in k-step i is d = 16 i + 8 (s >> 2) + 4 hi + (s & 3): exactly the d of accumulator register 8 i + s of a
// lane in half hi (acc_row), so the accumulators feed the next MFMA without any shuffle.  The contract between the pass that
// writes ctx^T (la_fin) / V^T (the bottleneck core's staging) and the MFMA that reads them against q / P registers.
__host__ __device__ inline int kslot(int d) { return (d >> 4) * 16 + ((d >> 2) & 1) * 8 + ((d >> 3) & 1) * 4 + (d & 3); }

// operand fragment of k-step kk: row l31 of 32 rows with stride ld, elements 16 kk + 8 hi .. + 7
__device__ inline bf16x8 frag(const __bf16* rows, int ld, int l31, int hi, int kk) {
  return *reinterpret_cast<const bf16x8*>(rows + l31 * ld + kk * 16 + hi * 8);
}
__device__ inline f16x8 frag(const _Float16* rows, int ld, int l31, int hi, int kk) {
  return *reinterpret_cast<const f16x8*>(rows + l31 * ld + kk * 16 + hi * 8);
}

// k-step fragments of 32 rows [r0, r0 + 32) of a row-major [.][COLS] matrix of 16-bit elements, straight from global memory into
// registers (each wave keeps its own rows for the whole block: no LDS copy, so several blocks fit on a CU)
template <int COLS, typename V, typename E>
__device__ inline void load_wfrags(V (&w)[COLS / 16], const E* mat, int r0, int l31, int hi) {
#pragma unroll
  for (int kk = 0; kk < COLS / 16; ++kk)
    w[kk] = *reinterpret_cast<const V*>(mat + (size_t)(r0 + l31) * COLS + kk * 16 + hi * 8);
}

// An output of RT row tiles of 32 channels x 2 pixel tiles of 32 over the four waves: accumulator a (of RT / 2) of a wave.
// RT = 2: one accumulator per wave; RT = 4: a wave's row tile with both pixel tiles; RT = 8: two row tiles, each with both.
template <int RT>
__device__ inline int y_row_tile(int wave, int a) { return RT == 2 ? (wave & 1) : (RT <= 4 ? wave : wave * (RT / 4) + (a >> 1)); }
template <int RT>
__device__ inline int y_pix_tile(int wave, int a) { return RT == 2 ? (wave >> 1) : (RT <= 4 ? a : (a & 1)); }

// opt-in to more than 64 KB of dynamic LDS (callers do it once per device: DeviceOnce)
template <typename K>
int set_lds(K kernel, size_t bytes) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return fail(PRG_E_HIP, std::string("hipFuncSetAttribute(dynamic LDS): ") + hipGetErrorString(e));
  return PRG_OK;
}

}  // namespace prg
