// radiuspairs.hip — every (row of A, row of B) of a cloud pair within a radius, as a ragged list: the ground-truth
// correspondences a registration loader looks up with a KD-tree per item (get_correspondences of the example loaders), produced
// next to the finished clouds while they are still on the device.
//
// The layout is prg_overlap_counts': pts (total,3) float64, offsets (2*n_pairs+1), pair p = query cloud A (segment 2p) against
// candidate cloud B (segment 2p+1).  The squared distance and the segment decode are allpairs.h's, shared with
// overlap_count_kernel and nearest_ragged_kernel (geometry.hip), and so is the sweep over B: both passes below hand it a lambda
// that compares d2 < r * r, so count and fill decide every (i, j) alike and the three kernels agree on every row.  Exact
// all-pairs search; no grid, no tree.
//
// Two passes, because the size of the list is data-dependent and the ABI neither reads device data on the host nor allocates:
//   1. rp_count_kernel: per query row the number of matches -> row_start[row] (rows that are no query row stay 0), then a
//      two-level exclusive scan over all buffer rows in place (rp_block_sums / scan.h's scan_blocks / rp_scan_rows, in int64: a
//      list may pass 2^31 rows even though no cloud does).
//   2. rp_fill_kernel: the thread that owns a query row owns its output range [row_start[r], row_start[r+1]) and writes it
//      in ascending j while the tiles stream past in ascending row order.  That IS the order (pair, i, j): no sort, and no
//      atomic whose arrival order would have to be undone.  An atomic cursor would save the second sweep over B but give a
//      list whose order changes from run to run, and the sort that repairs it costs more than the sweep (K is several times
//      the cloud size at loader radii).
//
// Launch shape — nearest_ragged_kernel's: grid (slabs, n_pairs), 256 threads, RP_Q = 2 query rows per thread, so a slab is 512
// rows of A.  Reasoning, from the figures in the comment above that kernel (float64 VALU op = 4 cycles per wave, ds_read_b64
// broadcast = 2 LDS cycles), NOT from a measurement of these two kernels:
//   count: per (candidate, query) 3 subtractions, 3 products, 2 sums, a compare and a conditional increment, ~40 cycles of VALU
//     per wave against 3 ds_read_b64 = 6 LDS cycles per candidate.  With one query per thread the four SIMDs ask the LDS for
//     24 cycles per 40, which 8-byte reads only deliver with ~4 waves per SIMD in flight; two queries per read halve that, and
//     the loop is VALU-bound like the sibling's.  There is no running minimum and no argument to carry (the sibling keeps
//     best + arg: 6 registers per query; here one 32-bit count), so registers are no limit at RP_Q = 2 and would not be at 4 —
//     but a third and fourth query buy nothing once the VALU is the bound, and thin out the workgroups: a batch of 16 pairs of
//     5 k rows is 160 workgroups at RP_Q = 2 for 256 CUs.
//   fill: the same loop with a store behind the compare.  A query row matches a handful of the thousands of candidates it
//     visits (2.2 / 3.9 per row of A at a 2.5 cm voxel and 3.75 / 5 cm, measured), so the store block is skipped by nearly every wave on
//     nearly every candidate: its price is the branch around it, not the store, and the 8 bytes per match are noise against
//     24 flops per (i, j).  It carries a 64-bit write position per query (4 registers) in place of the count.  The same RP_Q
//     keeps the slab boundaries of the two passes identical.
// hipcc: count 77 VGPRs (candidate loop unrolled by four, two candidates per ds_read_b128), fill 44; no scratch, no fma.
// Measured: 250 pairs of ~4.5 k-row clouds, count 1.73 ms, fill 1.66 ms, 2.6-2.7e12 tests/s, 0.84 of the
// sibling's call (both directions) on the same buffer; the same time at both radii.
#include "allpairs.h"
#include "scan.h"

namespace prg {

constexpr int RP_Q = 2;          // query rows per thread
constexpr int RP_SCAN = 1024;    // rows per block of the scan

// pass 1: row_start[q] = number of rows of B within the radius of query row q (row_start was zeroed: every other row stays 0)
__global__ __launch_bounds__(AP_TILE) void rp_count_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offs,
                                                           double r2, int64_t* __restrict__ row_start) {
  __shared__ double tile[AP_TILE * 3];
  const PairSegments g = pair_segments(offs, blockIdx.y);
  const int64_t slab = g.a0 + (int64_t)blockIdx.x * (AP_TILE * RP_Q);
  if (slab >= g.a1) return;                                     // whole slab beyond this cloud (uniform exit)
  int32_t cnt[RP_Q];
#pragma unroll
  for (int k = 0; k < RP_Q; ++k) cnt[k] = 0;
  sweep<RP_Q>(pts, g.a1, slab, g.b0, g.b1, tile, [&](int k, int32_t, double d2) {
    if (d2 < r2) ++cnt[k];
  });
#pragma unroll
  for (int k = 0; k < RP_Q; ++k) {
    const int64_t q = slab + k * AP_TILE + threadIdx.x;
    if (q < g.a1) row_start[q] = cnt[k];
  }
}

// pass 2: query row q writes (i, j) to rows row_start[q], row_start[q] + 1, ... of corr; rows at or beyond `capacity` are skipped
__global__ __launch_bounds__(AP_TILE) void rp_fill_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offs,
                                                          double r2, const int64_t* __restrict__ row_start, int64_t capacity,
                                                          int32_t* __restrict__ corr) {
  __shared__ double tile[AP_TILE * 3];
  const PairSegments g = pair_segments(offs, blockIdx.y);
  const int64_t slab = g.a0 + (int64_t)blockIdx.x * (AP_TILE * RP_Q);
  if (slab >= g.a1) return;                                     // whole slab beyond this cloud (uniform exit)
  int64_t pos[RP_Q];
  int32_t row[RP_Q];
#pragma unroll
  for (int k = 0; k < RP_Q; ++k) {
    const int64_t q = slab + k * AP_TILE + threadIdx.x;
    pos[k] = q < g.a1 ? row_start[q] : capacity;                // a dead lane never matches; if it did it would not write
    row[k] = (int32_t)(q - g.a0);
  }
  sweep<RP_Q>(pts, g.a1, slab, g.b0, g.b1, tile, [&](int k, int32_t j, double d2) {
    if (d2 < r2) {
      if (pos[k] < capacity) { corr[2 * pos[k]] = row[k]; corr[2 * pos[k] + 1] = j; }
      ++pos[k];
    }
  });
}

// ---- exclusive scan of v[0..n) in place, int64, two levels: block sums, one workgroup over them (scan.h), then the rows --------
__global__ __launch_bounds__(RP_SCAN) void rp_block_sums(const int64_t* __restrict__ v, int64_t n, int64_t* __restrict__ sums) {
  __shared__ int64_t wtot[RP_SCAN / 64];
  const int64_t i = (int64_t)blockIdx.x * RP_SCAN + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t inc = wave_inclusive<int64_t>(i < n ? v[i] : 0, lane);
  if (lane == 63) wtot[w] = inc;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t all = 0;
    for (int k = 0; k < RP_SCAN / 64; ++k) all += wtot[k];
    sums[blockIdx.x] = all;
  }
}

__global__ __launch_bounds__(RP_SCAN) void rp_scan_rows(int64_t* __restrict__ v, int64_t n, const int64_t* __restrict__ sums) {
  __shared__ int64_t wtot[RP_SCAN / 64];
  const int64_t i = (int64_t)blockIdx.x * RP_SCAN + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t x = i < n ? v[i] : 0;
  const int64_t inc = wave_inclusive(x, lane);
  if (lane == 63) wtot[w] = inc;
  __syncthreads();
  int64_t woff = 0;
  for (int k = 0; k < w; ++k) woff += wtot[k];
  if (i < n) v[i] = sums[blockIdx.x] + woff + inc - x;
}

static inline int64_t rp_scan_blocks_of(int64_t total) { return (total + 1 + RP_SCAN - 1) / RP_SCAN; }
static inline size_t rp_workspace(int64_t total) {
  if (total < 0) total = 0;
  return (((size_t)rp_scan_blocks_of(total) * sizeof(int64_t)) + 255) & ~(size_t)255;
}

}  // namespace prg

using namespace prg;

extern "C" {

size_t prg_radius_pairs_workspace_bytes(int64_t total) { return rp_workspace(total); }

int prg_radius_count_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t total, int64_t max_cloud,
                                double radius, int64_t* row_start, void* workspace, size_t workspace_bytes, void* stream) {
  PRG_CHECK(pts && offsets && row_start && workspace, "prg_radius_count_ragged_f64: null pointer");
  PRG_CHECK_PAIRS("prg_radius_count_ragged_f64", n_pairs);
  PRG_CHECK(total >= 0 && total < ((int64_t)1 << 31) && max_cloud > 0 && max_cloud < ((int64_t)1 << 31),
            "prg_radius_count_ragged_f64: bad sizes");
  PRG_CHECK_RADIUS("prg_radius_count_ragged_f64", radius);
  PRG_CHECK(workspace_bytes >= rp_workspace(total),
            "prg_radius_count_ragged_f64: workspace smaller than prg_radius_pairs_workspace_bytes");
  PRG_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "prg_radius_count_ragged_f64: workspace not 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int64_t* sums = (int64_t*)workspace;
  const int64_t n = total + 1;
  const int n_blocks = (int)rp_scan_blocks_of(total);
  PRG_HIP(hipMemsetAsync(row_start, 0, sizeof(int64_t) * (size_t)n, s));
  const int64_t slab = AP_TILE * RP_Q;
  const dim3 grid((unsigned)((max_cloud + slab - 1) / slab), (unsigned)n_pairs, 1);
  rp_count_kernel<<<grid, AP_TILE, 0, s>>>(pts, offsets, radius * radius, row_start);
  PRG_LAUNCH_CHECK();
  rp_block_sums<<<n_blocks, RP_SCAN, 0, s>>>(row_start, n, sums);
  PRG_LAUNCH_CHECK();
  scan_blocks<int64_t, false><<<1, kScanThreads, 0, s>>>(sums, n_blocks);   // no total: sums has n_blocks entries
  PRG_LAUNCH_CHECK();
  rp_scan_rows<<<n_blocks, RP_SCAN, 0, s>>>(row_start, n, sums);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

int prg_radius_fill_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, int64_t max_cloud, double radius,
                               const int64_t* row_start, int64_t capacity, int32_t* corr, void* stream) {
  PRG_CHECK(pts && offsets && row_start && (corr || capacity == 0), "prg_radius_fill_ragged_f64: null pointer");
  PRG_CHECK_PAIRS("prg_radius_fill_ragged_f64", n_pairs);
  PRG_CHECK(max_cloud > 0 && max_cloud < ((int64_t)1 << 31) && capacity >= 0, "prg_radius_fill_ragged_f64: bad sizes");
  PRG_CHECK_RADIUS("prg_radius_fill_ragged_f64", radius);
  if (capacity == 0) return PRG_OK;                             // nothing may be written
  const int64_t slab = AP_TILE * RP_Q;
  const dim3 grid((unsigned)((max_cloud + slab - 1) / slab), (unsigned)n_pairs, 1);
  rp_fill_kernel<<<grid, AP_TILE, 0, (hipStream_t)stream>>>(pts, offsets, radius * radius, row_start, capacity, corr);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
