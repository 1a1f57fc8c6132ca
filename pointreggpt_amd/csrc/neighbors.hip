// neighbors.hip — from the ragged list of all pairs within a radius (radiuspairs.hip) to a neighbour TABLE: per query row its
// `limit` nearest candidates, nearest first, equal distances by ascending j, the remaining slots padded — the table a KPConv
// network's collate step builds per item with a KD-tree (neighbours, sub-sampling and up-sampling of every pyramid level).
//
// Input is count / fill's complete output on the buffer they ran on: row_start (total + 1) and corr (list_rows, 2).  The
// matches of query row q are corr rows [row_start[q], row_start[q + 1]), contiguous, in ascending j.  What is missing is the
// selection: order a row's m matches by (squared distance, j) and keep the first `limit`.
//
// Rank by counting — no sort, no atomics.  (d2, j) is a strict total order on a row's matches (j is unique within a row), so
//   rank(t) = #{ u : (d2_u, j_u) < (d2_t, j_t) }
// is a permutation of 0 .. m-1: match t goes to slot rank(t) if that is below `limit`, slots min(m, limit) .. limit-1 take the
// pad, and every slot of the row has exactly one writer.  d2 is recomputed from pts with allpairs.h's dist2, the expression that
// produced the list, and compared with its `before`, so the order is the one postprocess.radius_neighbors states in numpy, bit
// for bit; the list does not carry distances, and three gathered rows per match are cheaper than 8 more bytes per list row
// written by fill and read again here.
//
// Launch shape: one wave per query row, NB_ROWS = 4 rows per 256-thread workgroup, grid (ceil(max_cloud / 4), n_pairs).  A wave
// owns NB_CHUNK (d2, j) slots of LDS (structure of arrays, 12 bytes per match, 24 KB per workgroup: six workgroups per CU) and
// never waits for another wave: there is no __syncthreads, the waves of a workgroup have different m; a staged chunk needs
// allpairs.h's wave_lds_fence before it is read, and no more.
//   for every 64 matches t (one per lane: the targets)        -- iterates, m is unbounded
//     for every chunk of NB_CHUNK matches u                   -- iterates, m is unbounded
//       stage the chunk (lane-strided: j from corr, the row from pts, d2) unless it is the row's only chunk and already there
//       every lane walks the chunk four matches at a time (the chunk is filled up to a multiple of four with d2 = +inf, which is
//       below no match): broadcast ds_read_b128 of (d2_u, j_u), rank += (d2_u, j_u) < (d2_t, j_t), no branch
// A row with m <= NB_CHUNK, i.e. nearly every row (m is ~20-40 at loader radii, hundreds at a coarse level with a doubled
// radius), stages once.  Cost per wave: m * ceil(m / 64) compares, each 12 bytes of LDS broadcast against ~6 VALU ops (two
// float64 compares, one int32 compare, and / or, add) — against the O(cloud) sweep per row that produced the list it is small
// for m in the tens and overtakes it only past m ~ cloud / 8.
// Measured: 250 clouds of ~4.6 k rows against themselves, 1.14 M query rows, limit 38: 0.75 ms at 20 matches
// per row next to count 1.98 ms and fill 2.31 ms; 1.95 ms at 70 matches per row (two passes) next to 1.96 and 2.77.
//
// Memory safety does not lean on the list being well-formed: [row_start[q], row_start[q + 1]) is clipped to [0, list_rows), so
// corr is never read at or beyond list_rows, and a j outside the candidate cloud is clamped into it before pts is read.  On
// count / fill's output neither clamp changes anything.
// hipcc (gfx950, -O3): ns_select_kernel 56 VGPRs, 60 SGPRs, 24576 bytes LDS, 6 waves per SIMD, no scratch, no fma.
#include "allpairs.h"

namespace prg {

constexpr int NB_ROWS = 4;       // query rows (waves) per workgroup
constexpr int NB_CHUNK = 512;    // matches staged in LDS per wave

__global__ __launch_bounds__(64 * NB_ROWS) void ns_select_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offs,
                                                                 const int64_t* __restrict__ row_start,
                                                                 const int32_t* __restrict__ corr, int64_t list_rows, int limit,
                                                                 const int64_t* __restrict__ table_offsets,
                                                                 const int32_t* __restrict__ index_base,
                                                                 const int32_t* __restrict__ pad, int32_t* __restrict__ table) {
  __shared__ __attribute__((aligned(16))) double s_d2[NB_ROWS][NB_CHUNK];
  __shared__ __attribute__((aligned(16))) int32_t s_j[NB_ROWS][NB_CHUNK];
  const int pair = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const PairSegments g = pair_segments(offs, pair);
  const int64_t b0 = g.b0;
  const int64_t i = (int64_t)blockIdx.x * NB_ROWS + wave;       // query row, local; the same in every lane of the wave
  const int64_t q = g.a0 + i;
  if (q >= g.a1) return;                                        // beyond this query cloud (wave-uniform: no barrier below)
  const int32_t nb = (int32_t)(g.b1 - b0);
  const int32_t base = index_base ? index_base[pair] : 0;
  const int32_t padv = pad ? pad[pair] : nb;
  int32_t* __restrict__ out = table + (table_offsets[pair] + i) * (int64_t)limit;

  int64_t e = min(row_start[q + 1], list_rows), s = max(row_start[q], (int64_t)0);
  if (s > e) s = e;
  const int64_t mv = nb > 0 ? e - s : 0;                        // matches of this row: the same in every lane, and the compiler
  const int64_t m = ((int64_t)__builtin_amdgcn_readfirstlane((int32_t)(mv >> 32)) << 32) |       // is told so (scalar loops)
                    (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)mv);
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double ax = pts[3 * q], ay = pts[3 * q + 1], az = pts[3 * q + 2];
  double* sd = s_d2[wave];
  int32_t* sj = s_j[wave];

  // (d2, j) of list row s + t
  auto match = [&](int64_t t, double& d2, int32_t& j) {
    j = corr[2 * (s + t) + 1];
    const int64_t r = b0 + min(max(j, 0), nb - 1);
    d2 = dist2(pts[3 * r], pts[3 * r + 1], pts[3 * r + 2], ax, ay, az);
  };

  for (int64_t t0 = 0; t0 < m; t0 += 64) {
    const bool live = t0 + lane < m;
    double dt = 0.0;
    int32_t jt = 0;
    if (live) match(t0 + lane, dt, jt);
    int32_t rank = 0;
    for (int64_t c0 = 0; c0 < m; c0 += NB_CHUNK) {
      const int n = (int)min((int64_t)NB_CHUNK, m - c0);
      const int n4 = (n + 3) & ~3;                              // the walk below takes four at a time
      if (t0 == 0 || m > NB_CHUNK) {                            // a row of one chunk stages it once
        wave_lds_fence();                                       // the previous chunk has been read by every lane
        for (int u = lane; u < n4; u += 64) {
          double d2 = inf;                                      // filler up to a multiple of four: below no match, equal to none
          int32_t j = 0;
          if (u < n) match(c0 + u, d2, j);
          sd[u] = d2;
          sj[u] = j;
        }
        wave_lds_fence();                                       // ... and this one written before any lane reads it
      }
      for (int u = 0; u < n4; u += 4) {                         // every lane reads the same address: LDS broadcasts
        const double2 d01 = *reinterpret_cast<const double2*>(sd + u), d23 = *reinterpret_cast<const double2*>(sd + u + 2);
        const int4 j4 = *reinterpret_cast<const int4*>(sj + u);
        rank += before(d01.x, j4.x, dt, jt) + before(d01.y, j4.y, dt, jt) + before(d23.x, j4.z, dt, jt) +
                before(d23.y, j4.w, dt, jt);
      }
    }
    if (live && rank < limit) out[rank] = base + jt;
  }
  const int filled = (int)min(m, (int64_t)limit);
  for (int k = filled + lane; k < limit; k += 64) out[k] = padv;
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_radius_select_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t max_cloud,
                                 const int64_t* row_start, const int32_t* corr, int64_t list_rows, int limit,
                                 const int64_t* table_offsets, const int32_t* index_base, const int32_t* pad, int32_t* table,
                                 void* stream) {
  PRG_CHECK(pts && offsets && row_start && table_offsets && table && (corr || list_rows == 0),
            "prg_radius_select_ragged_f64: null pointer");
  PRG_CHECK_PAIRS("prg_radius_select_ragged_f64", n_pairs);
  PRG_CHECK(max_cloud > 0 && max_cloud < ((int64_t)1 << 31) && list_rows >= 0, "prg_radius_select_ragged_f64: bad sizes");
  PRG_CHECK(limit >= 1 && limit <= 1024, "prg_radius_select_ragged_f64: limit out of range (1..1024)");
  const dim3 grid((unsigned)((max_cloud + NB_ROWS - 1) / NB_ROWS), (unsigned)n_pairs, 1);
  ns_select_kernel<<<grid, 64 * NB_ROWS, 0, (hipStream_t)stream>>>(pts, offsets, row_start, corr, list_rows, limit, table_offsets,
                                                                  index_base, pad, table);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
