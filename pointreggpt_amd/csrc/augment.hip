// augment.hip — the registration loaders' per-item augmentation of a batch of ragged float64 clouds on the device
// (include/prg.h "Geometry", prg_augment_ragged_f64): cut each cloud to a point limit by a keyed random permutation, move it by
// its rigid transform, add uniform per-point noise.  postprocess.augment_cloud states the definition in numpy; every output
// bit is that function's.
//
// One thread per input row, workgroups dealt per cloud on blockIdx.y (cloudmove.h), so the matrix, the seed and whether the
// cloud is cut are workgroup-uniform.  One Philox4x32-10 call per row, counter {row, draw, "augm", 0}, key = the cloud's seed:
// word 0 is the row's sort key, words 1..3 its noise on x, y, z — so a row's noise does not depend on what the cut keeps.
//
// A cloud that is not cut (m == n) streams: 24 B in, 24 B + 4 B out per row, rows in input order, no LDS, no barrier.
// A cloud that is cut ranks its rows by counting: rank(i) = #{u : (key_u, u) < (key_i, i)}, the keys of all n rows swept
// through LDS in tiles of 256 (the counting rank of neighbors.hip / patches.hip, on 32-bit keys).  The keys of a tile are
// regenerated, not stored: one Philox call per key and workgroup against the 256 comparisons the workgroup then spends on it.
// Row i goes to slot rank(i) if that is below m.  No atomics: every slot has exactly one writer, ranks being a permutation.
#include "cloudmove.h"
#include "philox.h"

namespace prg {

constexpr uint32_t PHILOX_DOMAIN_AUGMENT = 0x6175676Du;      // third counter word: "augm"

__device__ __forceinline__ void augment_words(uint64_t seed, uint32_t draw, uint32_t row, uint32_t (&w)[4]) {
  w[0] = row; w[1] = draw; w[2] = PHILOX_DOMAIN_AUGMENT; w[3] = 0u;
  philox4x32_10(w, seed);
}

// (ku, u) < (ki, i) as 0 / 1, without a branch
__device__ __forceinline__ uint32_t key_before(uint32_t ku, uint32_t u, uint32_t ki, uint32_t i) {
  return (uint32_t)(ku < ki) | ((uint32_t)(ku == ki) & (uint32_t)(u < i));
}

// (u - 0.5) * noise with u = (w + 0.5) * 2^-32: u and u - 0.5 are exact in float64, the product is the only rounding
__device__ __forceinline__ double augment_jitter(uint32_t w, double noise) {
  return (((double)w + 0.5) * 2.3283064365386962890625e-10 - 0.5) * noise;
}

__global__ __launch_bounds__(256) void augment_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offsets,
                                                      int64_t total, const double* __restrict__ T,
                                                      const uint8_t* __restrict__ has_T, const uint64_t* __restrict__ seeds,
                                                      uint32_t draw, const uint32_t* __restrict__ keys, int64_t limit, double noise,
                                                      const int64_t* __restrict__ out_offsets, int64_t out_total,
                                                      double* __restrict__ out, int32_t* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[kCfRows];
  const int c = blockIdx.y;
  // everything the workgroup needs from memory before its first row is asked for at once, not one answer after the other: the
  // four offsets, the seed, the flag and the matrix (fetched beside its flag, not behind it)
  const int64_t o0 = offsets[c], o1 = offsets[c + 1], p0 = out_offsets[c], p1 = out_offsets[c + 1];
  const uint64_t seed = seeds[c];
  const bool moved = T != nullptr && (has_T == nullptr || has_T[c] != 0);
  double mat[12] = {};
  if (T != nullptr) {                                   // one branch around twelve loads, not twelve selects
#pragma unroll
    for (int k = 0; k < 12; ++k) mat[k] = T[(size_t)c * 16 + k];
  }
  const int64_t beg = min(max(o0, (int64_t)0), total);
  const int64_t end = min(max(o1, beg), total);
  // rows are counted in uint32: total < 2^31, so an index plus a tile or a grid stride cannot wrap
  const uint32_t n = (uint32_t)(end - beg);
  // the grid covers a cloud four times the average (cloudmove.h): in a batch of even clouds three workgroups in four have no row
  if (blockIdx.x * kCfRows >= n) return;
  const int64_t obeg = min(max(p0, (int64_t)0), out_total);
  const int64_t oend = min(max(p1, obeg), out_total);
  const uint32_t m = (uint32_t)min(min((int64_t)n, limit > 0 ? limit : (int64_t)n), oend - obeg);
  if (m == 0) return;
  const bool cut = m < n;
  const bool jitter = noise != 0.0;
  const uint32_t* ckeys = keys ? keys + beg : nullptr;

  // base is workgroup-uniform: every thread reaches the barriers of the sweep
  for (uint32_t base = blockIdx.x * kCfRows; base < n; base += gridDim.x * kCfRows) {
    const uint32_t i = base + threadIdx.x;
    const bool live = i < n;
    // the row is fetched first, so that it is in flight under the Philox rounds; a cloud that is cut reads the rows it drops too
    // (24 B per row against the n key comparisons the row costs anyway)
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) { x = pts[3 * (beg + i)]; y = pts[3 * (beg + i) + 1]; z = pts[3 * (beg + i) + 2]; }
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (live && (jitter || (cut && !ckeys))) augment_words(seed, draw, i, w);
    uint32_t slot = i;
    if (cut) {
      const uint32_t ki = !live ? 0u : ckeys ? ckeys[i] : w[0];
      uint32_t rank = 0;
      for (uint32_t t0 = 0; t0 < n; t0 += kCfRows) {
        const uint32_t u = t0 + threadIdx.x;
        // a slot past the cloud holds the largest key at an index above every row: it is before nothing
        uint32_t ku = 0xFFFFFFFFu;
        if (u < n) {
          if (ckeys) {
            ku = ckeys[u];
          } else {
            uint32_t wu[4];
            augment_words(seed, draw, u, wu);
            ku = wu[0];
          }
        }
        __syncthreads();                                            // the previous tile has been read by every wave
        tile[threadIdx.x] = ku;
        __syncthreads();
        const uint32_t nt = min((uint32_t)kCfRows, n - t0);         // nt rounded up to 4 stays inside the tile
        // tiles and workgroups both start at multiples of 256 rows: a tile is this workgroup's own rows or lies wholly on one
        // side of them, and there the index half of (key, index) is decided for the whole tile — one comparison per key
        if (t0 < base) {                                            // every u < i: before iff ku <= ki
          for (uint32_t j = 0; j < nt; j += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(&tile[j]);
            rank += (uint32_t)(k4.x <= ki) + (uint32_t)(k4.y <= ki) + (uint32_t)(k4.z <= ki) + (uint32_t)(k4.w <= ki);
          }
        } else if (t0 > base) {                                     // every u > i: before iff ku < ki
          for (uint32_t j = 0; j < nt; j += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(&tile[j]);
            rank += (uint32_t)(k4.x < ki) + (uint32_t)(k4.y < ki) + (uint32_t)(k4.z < ki) + (uint32_t)(k4.w < ki);
          }
        } else {
          for (uint32_t j = 0; j < nt; j += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4*>(&tile[j]);
            rank += key_before(k4.x, t0 + j, ki, i) + key_before(k4.y, t0 + j + 1, ki, i) +
                    key_before(k4.z, t0 + j + 2, ki, i) + key_before(k4.w, t0 + j + 3, ki, i);
          }
        }
      }
      slot = rank;
    }
    if (live && slot < m) {
      if (moved) { const Row3 r = rigid_move_row(mat, x, y, z); x = r.x; y = r.y; z = r.z; }
      if (jitter) {
        x = x + augment_jitter(w[1], noise);
        y = y + augment_jitter(w[2], noise);
        z = z + augment_jitter(w[3], noise);
      }
      const int64_t o = obeg + slot;
      out[3 * o] = x; out[3 * o + 1] = y; out[3 * o + 2] = z;
      rows[o] = (int32_t)i;
    }
  }
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_augment_ragged_f64(const double* pts, const int64_t* offsets, int C, int64_t total, const double* T,
                           const uint8_t* has_T, const uint64_t* seeds, uint32_t draw, const uint32_t* keys, int64_t limit,
                           double noise, const int64_t* out_offsets, int64_t out_total, double* out, int32_t* rows,
                           void* stream) {
  PRG_CHECK(offsets && out_offsets && seeds, "prg_augment_ragged_f64: null pointer");
  PRG_CHECK(C > 0 && C <= kCfMaxSegments, "prg_augment_ragged_f64: C out of range");
  PRG_CHECK(total >= 0 && total < ((int64_t)1 << 31) && out_total >= 0 && out_total < ((int64_t)1 << 31),
            "prg_augment_ragged_f64: bad shape");
  PRG_CHECK(limit >= 0, "prg_augment_ragged_f64: limit must be >= 0 (0 = no limit)");
  PRG_CHECK(noise >= 0 && noise <= 1.79769313486231570815e308, "prg_augment_ragged_f64: noise must be finite and >= 0");
  PRG_CHECK(T != nullptr || has_T == nullptr, "prg_augment_ragged_f64: has_T without T");
  PRG_CHECK(out == nullptr || out != pts, "prg_augment_ragged_f64: out must not be pts (rows are permuted)");
  PRG_CHECK(total == 0 || pts != nullptr, "prg_augment_ragged_f64: null pointer");
  PRG_CHECK(out_total == 0 || (out != nullptr && rows != nullptr), "prg_augment_ragged_f64: null pointer");
  if (total == 0 || out_total == 0) return PRG_OK;
  const dim3 grid((unsigned)cf_grid_x(total, C), (unsigned)C, 1);
  augment_kernel<<<grid, kCfRows, 0, (hipStream_t)stream>>>(pts, offsets, total, T, has_T, seeds, draw, keys, limit, noise,
                                                            out_offsets, out_total, out, rows);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
