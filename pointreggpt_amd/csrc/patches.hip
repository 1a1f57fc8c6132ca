// patches.hip — the patch-level ground truth of a coarse-to-fine registration network, from clouds that are already on the
// device: every fine point belongs to its nearest coarse node, every node keeps its `limit` nearest own points as its patch, and
// a (source node, target node) pair is a ground-truth match when the two patches overlap, with the share of overlapping points.
// postprocess.node_patches / postprocess.patch_overlaps state both in numpy; everything here is bit for bit that.
//
// 1. prg_patch_tables_ragged inverts the assignment prg_nearest_ragged_f64 produced on the buffer [points_c | nodes_c] per
//    cloud (its d2 and idx, untouched) into per-node tables.  Rank by counting, as neighbors.hip does for a query row's matches:
//    within a node (d2, row) is a strict total order on its members, so
//      rank(i) = #{ u : assign[u] == assign[i] and (d2[u], u) < (d2[i], i) }
//    is a permutation of 0 .. members-1, member i goes to slot rank(i) if that is below `limit`, and the member of rank 0 writes
//    the node's size: every written slot has one writer — no sort, no atomics, the same bytes on every run.  The slots no member
//    reaches, and the sizes of nodes without members, come from pt_pad_kernel, launched first on the same stream.
//    Launch shape of pt_rank_kernel — that of allpairs.h's sweep, with its own loop because it streams (d2, assign) and not
//    points: one thread per point, the (d2, assign) of the thread's own cloud through LDS in 256-row tiles, the next tile fetched
//    into registers before the arithmetic on the current one starts; the order is allpairs.h's `before`.  Both loops iterate,
//    so a node may own any number of points (a whole cloud).  Per (i,
//    u): an int32 compare, two float64 compares, an int32 compare and two conditional increments against 12 bytes of LDS broadcast;
//    O(rows^2) per cloud like the nearest-node sweep that produced its input, with about a third of that sweep's arithmetic.
//
// 2. prg_patch_overlap_ragged_f64 tests patch against patch for every (source node, target node) of every item and writes the
//    two hit counts densely, (a, b) row-major: the Python layer's nonzero is then already ordered by (a, b), and no count / scan /
//    fill is needed.  The test is allpairs.h's dist2 < r * r, the one of radiuspairs.hip; a slot is read by its load_patch_slot.
//    One THREAD per node pair decides whether the pair needs the test at all; one WAVE then runs the test for each surviving
//    pair of its 64 (ballot, then a wave-uniform loop over the set bits).  The pre-filter — optional: `boxes` NULL switches it
//    off — compares the patches' bounding boxes, which po_box_kernel wrote to caller-provided scratch first: a pair is skipped
//    (zeros written) when fl(lo_b - hi_a) >= r or fl(lo_a - hi_b) >= r along an axis.  It is exact: for every point pair of the
//    two patches |dx| >= that gap in real numbers, rounding is monotonic, so fl(dx) >= r in magnitude and fl(dx*dx) >= fl(r*r);
//    the other two products are >= 0 or NaN, and neither makes the sum < r*r.  A NaN gap (infinite coordinates) compares false
//    and the pair is tested.  An empty patch has the box (+inf, -inf) and is always skipped.
//    The test of a surviving pair: the source patch in registers (one point per lane and 64-slot chunk: NCH = ceil(limit / 64)
//    chunks, a template parameter so the chunk loops unroll), the target patch staged in this wave's LDS (structure of arrays,
//    NCH * 1.5 KB per wave); one sweep over the target points, each broadcast to all lanes, gives both counts: a lane's sticky
//    "found" is hits_src after ballot + popcount, and a non-zero ballot of the test itself means target point j was hit.
//    Waves never wait for each other: no __syncthreads, allpairs.h's wave_lds_fence around the staging.
//
// Memory safety does not lean on device data being well-formed: an assign outside [0, nodes) counts as -1; a table entry outside
// [0, rows of its cloud) is a pad (its point never matches); a dense output position outside [0, total_node_pairs) is not
// written.
// hipcc (gfx950, -O3): pt_rank_kernel 40 VGPRs, 3 KB LDS; po_hits_kernel<1..4> 38 / 40 / 50 / 62 VGPRs, 6 / 12 / 18 / 24 KB LDS;
// pt_pad_kernel 24 and po_box_kernel 32 VGPRs; no scratch, no fma.
// Measured: 250 items of two ~4.6 k-row clouds with ~400 nodes each, limit 64: tables 1.95 ms next to the nearest
// sweep's 1.26 ms; overlap 0.70 ms for 4.1e7 node pairs with the pre-filter, 11.9 ms without it.
#include "allpairs.h"

namespace prg {

constexpr int PT_TILE = 256;     // rows per LDS tile = threads per workgroup of pt_rank_kernel
constexpr int PT_ROWS = 4;       // table rows (waves) per workgroup of the pad and box kernels
constexpr int PO_THREADS = 256;  // node pairs per workgroup of po_hits_kernel

// every slot of every node of every cloud = pad, every size = 0
__global__ __launch_bounds__(64 * PT_ROWS) void pt_pad_kernel(const int64_t* __restrict__ offs, int limit,
                                                              const int64_t* __restrict__ table_offsets,
                                                              const int32_t* __restrict__ pad, int32_t* __restrict__ table,
                                                              int32_t* __restrict__ sizes) {
  const int pair = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t p0 = offs[2 * pair], p1 = offs[2 * pair + 1], n1 = offs[2 * pair + 2];
  const int64_t k = (int64_t)blockIdx.x * PT_ROWS + wave;
  if (k >= n1 - p1) return;                                     // beyond this cloud's nodes (wave-uniform)
  const int32_t padv = pad ? pad[pair] : (int32_t)(p1 - p0);
  const int64_t row = table_offsets[pair] + k;
  for (int s = lane; s < limit; s += 64) table[row * limit + s] = padv;
  if (lane == 0) sizes[row] = 0;
}

__global__ __launch_bounds__(PT_TILE) void pt_rank_kernel(const double* __restrict__ d2, const int32_t* __restrict__ assign,
                                                          const int64_t* __restrict__ offs, int limit,
                                                          const int64_t* __restrict__ table_offsets,
                                                          const int32_t* __restrict__ index_base, int32_t* __restrict__ table,
                                                          int32_t* __restrict__ sizes) {
  __shared__ double s_d[PT_TILE];
  __shared__ int32_t s_a[PT_TILE];
  const int pair = blockIdx.y;
  const int64_t p0 = offs[2 * pair], p1 = offs[2 * pair + 1], n1 = offs[2 * pair + 2];
  const int64_t slab = p0 + (int64_t)blockIdx.x * PT_TILE;
  if (slab >= p1) return;                                       // whole slab beyond this cloud (uniform exit)
  const int64_t m = n1 - p1;                                    // nodes of this cloud
  const int64_t q = slab + threadIdx.x;
  const int32_t li = (int32_t)(q - p0);                         // this thread's point, local row
  int32_t ai = -1;                                              // a dead lane and an unassigned point own no slot
  double di = 0.0;
  if (q < p1) {
    ai = assign[q];
    di = d2[q];
    if (ai < 0 || ai >= m) ai = -1;
  }
  int32_t rank = 0, cnt = 0;
  double nd = 0.0;                                              // this thread's row of the next tile
  int32_t na = -1;
  if (p0 + threadIdx.x < p1) { nd = d2[p0 + threadIdx.x]; na = assign[p0 + threadIdx.x]; }
  for (int64_t t0 = p0; t0 < p1; t0 += PT_TILE) {
    const int n = (int)min((int64_t)PT_TILE, p1 - t0);
    __syncthreads();                                            // the previous tile has been read by every wave
    s_d[threadIdx.x] = nd;
    s_a[threadIdx.x] = na;
    __syncthreads();
    const int64_t r = t0 + PT_TILE + threadIdx.x;
    if (r < p1) { nd = d2[r]; na = assign[r]; }
    const int32_t base = (int32_t)(t0 - p0);
    for (int j = 0; j < n; ++j) {
      const int32_t same = (int32_t)(s_a[j] == ai);
      cnt += same;
      rank += same & before(s_d[j], base + j, di, li);
    }
  }
  if (ai >= 0) {
    const int64_t row = table_offsets[pair] + ai;
    if (rank < limit) table[row * limit + rank] = (index_base ? index_base[pair] : 0) + li;
    if (rank == 0) sizes[row] = cnt;
  }
}

__device__ __forceinline__ double po_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double po_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// boxes[row] = (lo x y z, hi x y z) over the patch's points; NaN coordinates are left out (such a point never matches)
__global__ __launch_bounds__(64 * PT_ROWS) void po_box_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offs,
                                                              const int32_t* __restrict__ tables,
                                                              const int64_t* __restrict__ toffs, int limit,
                                                              double* __restrict__ boxes) {
  const int cloud = 2 * blockIdx.y + blockIdx.z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t k = (int64_t)blockIdx.x * PT_ROWS + wave;
  if (k >= toffs[cloud + 1] - toffs[cloud]) return;             // beyond this cloud's nodes (wave-uniform)
  const int64_t c0 = offs[cloud], nc = offs[cloud + 1] - c0;
  const int64_t row = toffs[cloud] + k;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double lx = inf, ly = inf, lz = inf, hx = -inf, hy = -inf, hz = -inf;
  for (int s = lane; s < limit; s += 64) {
    double x, y, z;
    if (load_patch_slot(pts, c0, nc, tables[row * limit + s], x, y, z)) {
      lx = fmin(lx, x); ly = fmin(ly, y); lz = fmin(lz, z);
      hx = fmax(hx, x); hy = fmax(hy, y); hz = fmax(hz, z);
    }
  }
  lx = po_wave_min(lx); ly = po_wave_min(ly); lz = po_wave_min(lz);
  hx = po_wave_max(hx); hy = po_wave_max(hy); hz = po_wave_max(hz);
  if (lane == 0) {
    double* o = boxes + 6 * row;
    o[0] = lx; o[1] = ly; o[2] = lz; o[3] = hx; o[4] = hy; o[5] = hz;
  }
}

template <int NCH>
__global__ __launch_bounds__(PO_THREADS) void po_hits_kernel(const double* __restrict__ pts, const int64_t* __restrict__ offs,
                                                             const int32_t* __restrict__ tables,
                                                             const int64_t* __restrict__ toffs, int limit, double r, double r2,
                                                             const int64_t* __restrict__ hit_offsets, int64_t total_pairs,
                                                             const double* __restrict__ boxes, int32_t* __restrict__ hits) {
  __shared__ double s_b[PO_THREADS / 64][3][64 * NCH];
  const int item = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t ts = toffs[2 * item], tt = toffs[2 * item + 1], te = toffs[2 * item + 2];
  const int64_t ms = tt - ts, mt = te - tt;                     // source and target nodes of this item
  const int64_t g = (int64_t)blockIdx.x * PO_THREADS + threadIdx.x;             // node pair of this thread: a * mt + b
  const int64_t out = hit_offsets[item] + g;
  bool live = ms > 0 && mt > 0 && mt <= 0x7fffffff && g <= 0x7fffffff && out >= 0 && out < total_pairs;
  int32_t a = 0, b = 0;
  if (live) {                                                   // g and mt fit 32 bits: one short division per thread
    a = (int32_t)((uint32_t)g / (uint32_t)mt);
    b = (int32_t)((uint32_t)g - (uint32_t)a * (uint32_t)mt);
    live = a < ms;
  }
  bool test = live;
  if (live && boxes) {
    const double* A = boxes + 6 * (ts + a);
    const double* B = boxes + 6 * (tt + b);
    const bool apart = (B[0] - A[3] >= r) | (A[0] - B[3] >= r) | (B[1] - A[4] >= r) | (A[1] - B[4] >= r) | (B[2] - A[5] >= r) |
                       (A[2] - B[5] >= r);
    test = !apart;
  }
  if (live && !test) { hits[2 * out] = 0; hits[2 * out + 1] = 0; }
  unsigned long long todo = __ballot(test);
  if (!todo) return;                                            // wave-uniform, and there is no barrier below
  const int64_t a0 = offs[2 * item], b0 = offs[2 * item + 1];
  const int64_t na = b0 - a0, nb = offs[2 * item + 2] - b0;
  double* sx = s_b[wave][0];
  double* sy = s_b[wave][1];
  double* sz = s_b[wave][2];
  while (todo) {
    const int l = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int32_t pa = __shfl(a, l, 64), pb = __shfl(b, l, 64);
    const int32_t po = __shfl((int32_t)g, l, 64);               // g of lane l, a tested lane: below 2^31
    const int32_t* ta = tables + (ts + pa) * (int64_t)limit;
    const int32_t* tb = tables + (tt + pb) * (int64_t)limit;
    double ax[NCH], ay[NCH], az[NCH];
    bool found[NCH];
    int kb = 0;                                                 // 1 + the last slot of the target patch that holds a point
    wave_lds_fence();                                           // the previous pair's patch has been read by every lane
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int s = c * 64 + lane;
      const bool in = s < limit;                                // a slot beyond the patch is a pad
      double x, y, z;
      load_patch_slot(pts, a0, na, in ? ta[s] : -1, ax[c], ay[c], az[c]);
      const unsigned long long has = __ballot(load_patch_slot(pts, b0, nb, in ? tb[s] : -1, x, y, z));
      found[c] = false;
      sx[s] = x; sy[s] = y; sz[s] = z;
      if (has) kb = c * 64 + 64 - __builtin_clzll(has);
    }
    wave_lds_fence();                                           // ... and this one written before any lane reads it
    int32_t hit_tgt = 0;
    for (int j = 0; j < kb; ++j) {                              // every lane reads the same address: LDS broadcasts
      const double bx = sx[j], by = sy[j], bz = sz[j];
      unsigned long long any = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const bool w = dist2(bx, by, bz, ax[c], ay[c], az[c]) < r2;
        found[c] |= w;
        any |= __ballot(w);
      }
      hit_tgt += any != 0;
    }
    int32_t hit_src = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) hit_src += (int32_t)__popcll(__ballot(found[c]));
    if (lane == 0) {
      const int64_t o = hit_offsets[item] + po;
      hits[2 * o] = hit_src;
      hits[2 * o + 1] = hit_tgt;
    }
  }
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_patch_tables_ragged(const double* d2, const int32_t* assign, const int64_t* offsets, int n_pairs, int64_t max_cloud,
                            int64_t max_nodes, int limit, const int64_t* table_offsets, const int32_t* index_base,
                            const int32_t* pad, int32_t* table, int32_t* sizes, void* stream) {
  PRG_CHECK(d2 && assign && offsets && table_offsets && table && sizes, "prg_patch_tables_ragged: null pointer");
  PRG_CHECK_PAIRS("prg_patch_tables_ragged", n_pairs);
  PRG_CHECK(max_cloud > 0 && max_cloud < ((int64_t)1 << 31) && max_nodes > 0 && max_nodes < ((int64_t)1 << 31),
            "prg_patch_tables_ragged: bad sizes");
  PRG_CHECK(limit >= 1 && limit <= 256, "prg_patch_tables_ragged: limit out of range (1..256)");
  hipStream_t s = (hipStream_t)stream;
  const dim3 pad_grid((unsigned)((max_nodes + PT_ROWS - 1) / PT_ROWS), (unsigned)n_pairs, 1);
  pt_pad_kernel<<<pad_grid, 64 * PT_ROWS, 0, s>>>(offsets, limit, table_offsets, pad, table, sizes);
  PRG_LAUNCH_CHECK();
  const dim3 grid((unsigned)((max_cloud + PT_TILE - 1) / PT_TILE), (unsigned)n_pairs, 1);
  pt_rank_kernel<<<grid, PT_TILE, 0, s>>>(d2, assign, offsets, limit, table_offsets, index_base, table, sizes);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

int prg_patch_overlap_ragged_f64(const double* pts, const int64_t* offsets, int n_pairs, const int32_t* tables,
                                 const int64_t* table_offsets, int64_t max_nodes, int limit, double radius,
                                 const int64_t* hit_offsets, int64_t total_node_pairs, int64_t max_item_pairs, double* boxes,
                                 int32_t* hits, void* stream) {
  PRG_CHECK(pts && offsets && tables && table_offsets && hit_offsets && hits, "prg_patch_overlap_ragged_f64: null pointer");
  PRG_CHECK_PAIRS("prg_patch_overlap_ragged_f64", n_pairs);
  PRG_CHECK(max_nodes > 0 && max_nodes < ((int64_t)1 << 31), "prg_patch_overlap_ragged_f64: bad sizes");
  PRG_CHECK(total_node_pairs > 0 && total_node_pairs <= ((int64_t)1 << 28) && max_item_pairs > 0 &&
                max_item_pairs <= total_node_pairs,
            "prg_patch_overlap_ragged_f64: node pairs out of range (1..2^28)");
  PRG_CHECK(limit >= 1 && limit <= 256, "prg_patch_overlap_ragged_f64: limit out of range (1..256)");
  PRG_CHECK_RADIUS("prg_patch_overlap_ragged_f64", radius);
  hipStream_t s = (hipStream_t)stream;
  if (boxes) {
    const dim3 box_grid((unsigned)((max_nodes + PT_ROWS - 1) / PT_ROWS), (unsigned)n_pairs, 2);
    po_box_kernel<<<box_grid, 64 * PT_ROWS, 0, s>>>(pts, offsets, tables, table_offsets, limit, boxes);
    PRG_LAUNCH_CHECK();
  }
  const dim3 grid((unsigned)((max_item_pairs + PO_THREADS - 1) / PO_THREADS), (unsigned)n_pairs, 1);
  const double r2 = radius * radius;
  dispatch_chunks(limit, [&](auto nch) {
    po_hits_kernel<decltype(nch)::value><<<grid, PO_THREADS, 0, s>>>(pts, offsets, tables, table_offsets, limit, radius, r2,
                                                                     hit_offsets, total_node_pairs, boxes, hits);
  });
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
