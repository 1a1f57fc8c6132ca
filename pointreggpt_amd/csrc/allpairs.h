// allpairs.h — what the ragged float64 search kernels share (geometry.hip: overlap counts and nearest; radiuspairs.hip,
// neighbors.hip, patches.hip, finelabels.hip).  Every result of these kernels is promised bit for bit against the numpy
// specifications in postprocess.py, and the promise rests on all of them deciding every pair of points alike: the pieces that
// make the decision are here, once.
#pragma once
#include <type_traits>

#include "common.h"

namespace prg {

constexpr int AP_TILE = 256;     // rows of the candidate cloud per LDS tile = threads per workgroup of a sweep

// THE squared distance.  b - a, the three products written out and summed left to right in float64; the library is built with
// -ffp-contract=off, so there is no fma and the value is numpy's `dx * dx + dy * dy + dz * dz`.  Every caller compares it with
// a strict < (against r * r, or against the best so far): a NaN coordinate on either side gives NaN and a difference that
// overflows gives +inf, and neither is below anything.
__device__ __forceinline__ double dist2(double bx, double by, double bz, double ax, double ay, double az) {
  const double dx = bx - ax, dy = by - ay, dz = bz - az;
  return dx * dx + dy * dy + dz * dz;
}

// THE strict total order on (squared distance, index): (du, ju) < (dt, jt) as 0 / 1, without a branch
__device__ __forceinline__ int32_t before(double du, int32_t ju, double dt, int32_t jt) {
  return (int32_t)(du < dt) | ((int32_t)(du == dt) & (int32_t)(ju < jt));
}

// The pair layout of prg_overlap_counts: offs (2 * n_pairs + 1), pair p = segments 2p and 2p+1 of one buffer.  dir 0 queries
// segment 2p (rows [a0, a1)) against segment 2p+1 (rows [b0, b1)); dir 1 the other way round.
struct PairSegments { int64_t a0, a1, b0, b1; };
__device__ __forceinline__ PairSegments pair_segments(const int64_t* __restrict__ offs, int pair, int dir = 0) {
  return PairSegments{offs[2 * pair + dir], offs[2 * pair + dir + 1], dir == 0 ? offs[2 * pair + 1] : offs[2 * pair],
                      dir == 0 ? offs[2 * pair + 2] : offs[2 * pair + 1]};
}

// The indexed pair layout of prg_overlap_counts_indexed: offs (n_clouds + 1) are the segments of a SET of clouds and pair p is
// the clouds (s, t) = pair_index[2p], pair_index[2p + 1] — any cloud in any number of pairs, in either position, s == t
// included.  dir 0 queries cloud s against cloud t; dir 1 the other way round.  The two entries are read and compared with
// [0, n_clouds) before any address is formed from them: a pair with an entry outside returns false and g is left alone.
__device__ __forceinline__ bool indexed_pair_segments(const int64_t* __restrict__ offs, int n_clouds,
                                                      const int32_t* __restrict__ pair_index, int pair, int dir,
                                                      PairSegments& g) {
  const int32_t s = pair_index[2 * pair], t = pair_index[2 * pair + 1];
  if (s < 0 || s >= n_clouds || t < 0 || t >= n_clouds) return false;
  const int32_t a = dir == 0 ? s : t, b = dir == 0 ? t : s;
  g = PairSegments{offs[a], offs[a + 1], offs[b], offs[b + 1]};
  return true;
}

// The all-pairs sweep: calls visit(k, j_local, d2) for every query k < Q of this thread — row slab + k * AP_TILE + threadIdx.x,
// a query if it is below a1 — and every candidate row j of [b0, b1), j ascending, d2 = dist2(candidate, query).  The candidates
// stream through `tile` (3 * AP_TILE doubles of LDS, structure of arrays, one row per thread to stage); the next tile is
// fetched into registers before the arithmetic on the current one starts.  A dead query lane holds NaN coordinates: its d2 is
// NaN, which passes no strict <, so it neither counts nor writes.  Every thread of the workgroup must call it (barriers).
// The two radius passes (radiuspairs.hip) run on it; nearest_ragged_kernel (geometry.hip) has the same loop written out, for
// the reason given there.
template <int Q, typename Visit>
__device__ __forceinline__ void sweep(const double* __restrict__ pts, int64_t a1, int64_t slab, int64_t b0, int64_t b1,
                                      double* tile, Visit visit) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  double qx[Q], qy[Q], qz[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int64_t q = slab + k * AP_TILE + threadIdx.x;
    qx[k] = qy[k] = qz[k] = nan;
    if (q < a1) { qx[k] = pts[3 * q]; qy[k] = pts[3 * q + 1]; qz[k] = pts[3 * q + 2]; }
  }
  double nx = 0, ny = 0, nz = 0;                                // this thread's row of the next tile
  if (b0 + threadIdx.x < b1) { nx = pts[3 * (b0 + threadIdx.x)]; ny = pts[3 * (b0 + threadIdx.x) + 1]; nz = pts[3 * (b0 + threadIdx.x) + 2]; }
  for (int64_t t0 = b0; t0 < b1; t0 += AP_TILE) {
    const int n = (int)min((int64_t)AP_TILE, b1 - t0);          // rows of this tile that belong to the candidate cloud
    __syncthreads();                                            // the previous tile has been read by every wave
    tile[threadIdx.x] = nx;
    tile[AP_TILE + threadIdx.x] = ny;
    tile[2 * AP_TILE + threadIdx.x] = nz;
    __syncthreads();
    const int64_t r = t0 + AP_TILE + threadIdx.x;
    if (r < b1) { nx = pts[3 * r]; ny = pts[3 * r + 1]; nz = pts[3 * r + 2]; }
    const int32_t base = (int32_t)(t0 - b0);
    for (int j = 0; j < n; ++j) {
      const double bx = tile[j], by = tile[AP_TILE + j], bz = tile[2 * AP_TILE + j];
#pragma unroll
      for (int k = 0; k < Q; ++k) visit(k, base + j, dist2(bx, by, bz, qx[k], qy[k], qz[k]));
    }
  }
}

// Between a wave's writes to its PRIVATE piece of LDS and its own reads of it (and between those reads and the next writes).
// Within a wave the LDS returns in order and these waves never wait for each other, so no s_barrier is needed: the fence pins
// the compiler's order of the accesses and the wave barrier keeps it from moving code across the point.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// One slot of a patch table: entry e is row first + e of pts if it lies in [0, n), anything else is a pad.  Returns whether
// the slot holds a point; (x, y, z) are its coordinates, or NaN for a pad — a pad matches nothing.
__device__ __forceinline__ bool load_patch_slot(const double* __restrict__ pts, int64_t first, int64_t n, int32_t e, double& x,
                                                double& y, double& z) {
  const bool ok = e >= 0 && e < n;
  x = y = z = __longlong_as_double(0x7ff8000000000000LL);
  if (ok) { x = pts[3 * (first + e)]; y = pts[3 * (first + e) + 1]; z = pts[3 * (first + e) + 2]; }
  return ok;
}

// Host side: a patch of `limit` slots is NCH = ceil(limit / 64) chunks of one slot per lane, a template parameter of the patch
// kernels (1..4: limit <= 256).  f(std::integral_constant<int, NCH>) launches the instance.
template <typename F>
inline void dispatch_chunks(int limit, F&& f) {
  switch ((limit + 63) / 64) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

}  // namespace prg
