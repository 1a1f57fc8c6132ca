// cloudmove.h — what the per-row kernels over ragged float64 clouds share (cloudfinish.hip, augment.hip): THE rigid move, and
// the launch shape with workgroups dealt per segment on blockIdx.y.
#pragma once
#include "common.h"

namespace prg {

constexpr int kCfRows = 256;                 // threads per workgroup, one row each per pass
constexpr int kCfMaxSegments = 65535;        // gridDim.y

// THE rigid move: m = the first 12 doubles of a row-major 4x4.  x' = x*m[0] + y*m[1] + z*m[2] + m[3], summed left to right in
// float64; the library is built with -ffp-contract=off, so no product is fused into a sum and the value is hostpool.cpp's
// transform() and numpy's `x * T[r,0] + y * T[r,1] + z * T[r,2] + T[r,3]` (postprocess.rigid_move) bit for bit.
// By value in, by value out: written so, rigid_crop_kernel compiles to the instructions it had with the expression in place.
struct Row3 { double x, y, z; };
__device__ __forceinline__ Row3 rigid_move_row(const double (&m)[12], double px, double py, double pz) {
  return Row3{px * m[0] + py * m[1] + pz * m[2] + m[3], px * m[4] + py * m[5] + pz * m[6] + m[7],
              px * m[8] + py * m[9] + pz * m[10] + m[11]};
}

inline int cf_grid_x(int64_t total, int B) {
  // enough workgroups for a segment four times the average, one row per thread; longer segments loop (grid-stride)
  const int64_t avg = (total + B - 1) / B;
  const int64_t gx = (4 * avg + kCfRows - 1) / kCfRows;
  return (int)(gx < 1 ? 1 : gx > 4096 ? 4096 : gx);
}

}  // namespace prg
