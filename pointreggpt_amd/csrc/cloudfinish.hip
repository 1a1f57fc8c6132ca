// cloudfinish.hip — the rigid move and the bounding-box crop of a batch of ragged float64 clouds on the device (include/prg.h
// "Geometry"): what hostpool.cpp's transform() and crop_aabb() do to one cloud before and after its voxel grid, so that a cloud
// can be finished (pre-transform -> crop -> prg_voxel_grid_ragged -> post-transform) without leaving the GPU.
//
// Same bits as the host: x' = x*T[0] + y*T[1] + z*T[2] + T[3] summed left to right in float64 (-ffp-contract=off: no FMA); a
// segment without a transform is copied, not multiplied by an identity (-0.0 * 1 + 0 * 0 + 0 * 0 + 0 = +0.0 would lose the sign);
// the crop keeps lo <= p' <= hi (inclusive) and is a flag, not a compaction: the voxel grid that follows skips unflagged rows.
//
// Memory-bound: 24 B in, 24 B + 1 B out per row.  A thread owns a row and reads its three doubles itself: the lanes of a wave
// are then 24 B apart in each of the three loads, but the three together cover the same 1536 consecutive bytes, so every fetched
// line is used completely.  Measured against a version that moves tiles of 256 rows through LDS with unit-stride lanes
// (tools/micro/rows3_access.hip, 20 M rows): 5.5 TB/s for this one, 5.1-5.4 TB/s for the staged one — the simpler kernel stays.
// Workgroups are dealt per segment (blockIdx.y, the way project_points_kernel and the voxel-grid kernels do), so a row's
// segment — its matrix — is known without a search.
#include "cloudmove.h"

namespace prg {

struct CfBox {
  double lo[3], hi[3];
};

// pts / out and valid / valid_out may alias: no __restrict__ on them.  A thread reads its row completely before it writes it, and no
// other thread touches that row.
template <bool kCrop>
__global__ __launch_bounds__(256) void rigid_crop_kernel(const double* pts, const uint8_t* valid,
                                                         const int64_t* __restrict__ offsets, int64_t total,
                                                         const double* __restrict__ T, const uint8_t* __restrict__ has_T,
                                                         CfBox box, double* out, uint8_t* valid_out) {
  const int b = blockIdx.y;
  const int64_t beg = min(max(offsets[b], (int64_t)0), total);
  const int64_t end = min(max(offsets[b + 1], beg), total);
  const bool moved = T != nullptr && (has_T == nullptr || has_T[b] != 0);
  if (!moved && !kCrop && out == pts && (valid_out == nullptr || valid_out == valid)) return;   // nothing would change
  double m[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) m[k] = moved ? T[(size_t)b * 16 + k] : 0.0;
  for (int64_t i = beg + (int64_t)blockIdx.x * kCfRows + threadIdx.x; i < end; i += (int64_t)gridDim.x * kCfRows) {
    double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    bool keep = valid == nullptr || valid[i] != 0;
    if (moved) { const Row3 r = rigid_move_row(m, x, y, z); x = r.x; y = r.y; z = r.z; }
    if (kCrop)        // every comparison with NaN is false: a masked row of garbage stays masked and nothing else happens to it
      keep = keep && x >= box.lo[0] && x <= box.hi[0] && y >= box.lo[1] && y <= box.hi[1] && z >= box.lo[2] && z <= box.hi[2];
    if (moved || out != pts) { out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z; }
    if (valid_out) valid_out[i] = keep ? 1 : 0;
  }
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_rigid_crop_ragged_f64(const double* pts, const uint8_t* valid, const int64_t* offsets, int B, int64_t total,
                              const double* T, const uint8_t* has_T, const double* lo, const double* hi, double* out,
                              uint8_t* valid_out, void* stream) {
  PRG_CHECK(offsets, "prg_rigid_crop_ragged_f64: null pointer");
  PRG_CHECK(B > 0 && B <= kCfMaxSegments && total >= 0 && total < ((int64_t)1 << 31), "prg_rigid_crop_ragged_f64: bad shape");
  PRG_CHECK((lo == nullptr) == (hi == nullptr), "prg_rigid_crop_ragged_f64: lo and hi go together");
  PRG_CHECK(T != nullptr || has_T == nullptr, "prg_rigid_crop_ragged_f64: has_T without T");
  const bool crop = lo != nullptr;
  PRG_CHECK(valid_out != nullptr || !crop, "prg_rigid_crop_ragged_f64: a crop needs valid_out");
  if (total == 0) return PRG_OK;
  PRG_CHECK(pts && out, "prg_rigid_crop_ragged_f64: null pointer");
  CfBox box = {};
  if (crop)
    for (int k = 0; k < 3; ++k) { box.lo[k] = lo[k]; box.hi[k] = hi[k]; }
  const dim3 grid((unsigned)cf_grid_x(total, B), (unsigned)B, 1);
  hipStream_t s = (hipStream_t)stream;
  if (crop)
    rigid_crop_kernel<true><<<grid, kCfRows, 0, s>>>(pts, valid, offsets, total, T, has_T, box, out, valid_out);
  else
    rigid_crop_kernel<false><<<grid, kCfRows, 0, s>>>(pts, valid, offsets, total, T, has_T, box, out, valid_out);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
