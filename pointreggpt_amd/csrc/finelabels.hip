// finelabels.hip — the fine-level ground truth of a coarse-to-fine registration network: for every selected (source node, target
// node) pair the (limit+1) x (limit+1) label matrix "point u of patch a and point v of patch b lie within the matching radius",
// with a slack row and a slack column for the patch points without a partner — the target of the consumers' optimal-transport
// loss.  postprocess.patch_corr_labels states it in numpy; everything here is bit for bit that.
//
// The test is allpairs.h's dist2 < r * r on slots read by its load_patch_slot, as in po_hits_kernel (patches.hip) — so a patch
// pair that prg_patch_overlap_ragged_f64 lists as overlapping has a match in its matrix, and one it does not list has none.
//
// fl_labels_kernel is po_hits_kernel's idiom turned by 90 degrees: ONE WAVE per selected pair, four waves per workgroup that never
// wait for each other (no __syncthreads; allpairs.h's wave_lds_fence behind the staging).  The SOURCE patch is
// staged in this wave's LDS (structure of arrays, NCH * 1.5 KB per wave; NCH = ceil(limit / 64) chunks, a template parameter so the
// chunk loops unroll), the TARGET patch sits in registers, one point per lane and chunk: the lanes run along v, so one store
// instruction writes 64 consecutive bytes of a label row.  One sweep over u, the source point broadcast from LDS to all lanes:
//   labels[u][v]     = the test, one byte per lane and chunk
//   labels[u][limit] = slot u valid and the ballot of the test over all chunks is empty          (lane 0, after the row)
//   labels[limit][v] = slot v valid and the lane's sticky "found" still false                    (after the sweep)
//   labels[limit][limit] = 0
// A pad slot holds NaN coordinates and therefore matches nothing; validity itself is by index only (a valid slot that points at a
// NaN row has its slack label set).  Every byte of a matrix has exactly one writer and is written once: no atomics, no second pass,
// the same bytes on every run.  Rows are limit + 1 bytes, so they are not dword-aligned: the stores are plain byte stores.
//
// Memory safety does not lean on device data being well-formed: a pair row outside [0, nodes) gives an all-zero matrix and reads
// nothing of `table`; a table entry outside [0, rows) is a pad and reads nothing of `pts`.
// hipcc (gfx950, -O3): register and LDS use are listed in DESIGN.md §4.11 (tools/kernel_regs.sh); no scratch, no fma.
#include "allpairs.h"

namespace prg {

constexpr int FL_WAVES = 4;      // selected pairs (waves) per workgroup

template <int NCH>
__global__ __launch_bounds__(64 * FL_WAVES) void fl_labels_kernel(const double* __restrict__ pts, int64_t rows,
                                                                  const int32_t* __restrict__ table, int64_t nodes, int limit,
                                                                  const int32_t* __restrict__ pairs, int64_t n_sel, double r2,
                                                                  uint8_t* __restrict__ labels) {
  __shared__ double s_a[FL_WAVES][3][64 * NCH];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * FL_WAVES + wave;
  if (s >= n_sel) return;                                       // wave-uniform, and there is no barrier below
  const int stride = limit + 1;
  uint8_t* out = labels + s * (int64_t)(stride * stride);
  const int32_t pa = pairs[2 * s], pb = pairs[2 * s + 1];
  if (pa < 0 || pa >= nodes || pb < 0 || pb >= nodes) {         // two empty patches (wave-uniform)
    for (int o = lane; o < stride * stride; o += 64) out[o] = 0;
    return;
  }
  const int32_t* ta = table + (int64_t)pa * limit;
  const int32_t* tb = table + (int64_t)pb * limit;
  double* sx = s_a[wave][0];
  double* sy = s_a[wave][1];
  double* sz = s_a[wave][2];
  double bx[NCH], by[NCH], bz[NCH];
  bool ok_b[NCH], found[NCH];
  unsigned long long ok_a[NCH];                                 // the valid slots of the source patch, one bit per slot
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int slot = c * 64 + lane;
    const bool in = slot < limit;                               // a slot beyond the patch is a pad
    double x, y, z;
    ok_a[c] = __ballot(load_patch_slot(pts, 0, rows, in ? ta[slot] : -1, x, y, z));
    ok_b[c] = load_patch_slot(pts, 0, rows, in ? tb[slot] : -1, bx[c], by[c], bz[c]);
    found[c] = false;
    sx[slot] = x; sy[slot] = y; sz[slot] = z;
  }
  wave_lds_fence();                                             // the source patch is written before any lane reads it
#pragma unroll
  for (int cu = 0; cu < NCH; ++cu) {
    const int nu = min(64, limit - cu * 64);
    for (int uu = 0; uu < nu; ++uu) {                           // every lane reads the same address: LDS broadcasts
      const int u = cu * 64 + uu;
      const double ax = sx[u], ay = sy[u], az = sz[u];
      uint8_t* row = out + u * stride;
      unsigned long long any = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int v = c * 64 + lane;
        const bool w = dist2(bx[c], by[c], bz[c], ax, ay, az) < r2;
        found[c] |= w;
        any |= __ballot(w);
        if (v < limit) row[v] = (uint8_t)w;
      }
      if (lane == 0) row[limit] = (uint8_t)(((ok_a[cu] >> uu) & 1ull) != 0 && any == 0);
    }
  }
  uint8_t* last = out + limit * stride;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int v = c * 64 + lane;
    if (v < limit) last[v] = (uint8_t)(ok_b[c] && !found[c]);
  }
  if (lane == 0) last[limit] = 0;
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_patch_corr_labels_f64(const double* pts, int64_t rows, const int32_t* table, int64_t nodes, int limit,
                              const int32_t* pairs, int64_t n_sel, double radius, uint8_t* labels, void* stream) {
  PRG_CHECK(table && pairs && labels, "prg_patch_corr_labels_f64: null pointer");
  PRG_CHECK(rows >= 0 && rows < ((int64_t)1 << 31) && (pts || rows == 0), "prg_patch_corr_labels_f64: bad rows / null points");
  PRG_CHECK(nodes >= 1 && nodes < ((int64_t)1 << 31), "prg_patch_corr_labels_f64: nodes out of range");
  PRG_CHECK(limit >= 1 && limit <= 256, "prg_patch_corr_labels_f64: limit out of range (1..256)");
  PRG_CHECK(n_sel >= 1 && n_sel <= ((int64_t)1 << 24), "prg_patch_corr_labels_f64: n_sel out of range (1..2^24)");
  PRG_CHECK_RADIUS("prg_patch_corr_labels_f64", radius);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((n_sel + FL_WAVES - 1) / FL_WAVES), 1, 1);
  const double r2 = radius * radius;
  dispatch_chunks(limit, [&](auto nch) {
    fl_labels_kernel<decltype(nch)::value><<<grid, 64 * FL_WAVES, 0, s>>>(pts, rows, table, nodes, limit, pairs, n_sel, r2, labels);
  });
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
