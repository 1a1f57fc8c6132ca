// normals.hip — from a neighbour table (neighbors.hip) to oriented surface normals: per row the eigenvector of the smallest
// eigenvalue of its neighbourhood's scatter matrix, turned towards the camera that saw the cloud, and the surface variation
// lambda_min / (lambda_0 + lambda_1 + lambda_2).  What open3d's estimate_normals(KDTreeSearchParamHybrid(radius, max_nn)) +
// orient_normals_towards_camera_location do on the host per item, for a ragged stack of clouds in one launch.
//
// postprocess.estimate_normals is the definition and this kernel restates it operation for operation, in float64 without fma
// (-ffp-contract=off), with IEEE / and sqrt: the results are promised bit for bit.  Per row, k = min(count, limit) slots:
//   sums     every sum over the slots is NM_LANES = 8 partial sums — slot s goes to partial s mod 8, each partial starts at +0.0
//            and takes its slots in ascending order — combined by the tree ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7))
//   pass 1   mean = (sum x, sum y, sum z) / (double)k
//   pass 2   d = p - mean; S = sums of dx*dx, dx*dy, dx*dz, dy*dy, dy*dz, dz*dz (not divided by k)
//   Jacobi   NM_SWEEPS = 6 cyclic sweeps over (p, q) = (0,1), (0,2), (1,2), a rotation iff S_pq != 0 (jacobi_rotate below)
//   normal   the column of V under the smallest diagonal entry (ties: the lowest index), not renormalised
//   sign     negated iff (nx*(vx-px) + ny*(vy-py)) + nz*(vz-pz) < 0
//   k < min_neighbors or a non-finite row: (0, 0, 1) and variation 0, not oriented
//
// Launch shape: NM_LANES = 8 lanes per row, 32 rows per 256-thread workgroup, a 1-D grid over the Q table rows; the row's cloud
// is found by bisection of table_offsets (C + 1 <= 65536: 16 steps, the same addresses in all 8 lanes).  Lane l of a group reads
// slots l, l + 8, ...: the 8 lanes read 32 contiguous bytes of the table row per step, then gather the three coordinates; the
// second pass gathers again (the rows are in L2: a row's neighbours are its neighbours' neighbours' too) instead of keeping up
// to 1024 points per row anywhere.  The partial sums live in registers and the tree is three xor-shuffles within the group
// (float64 + is commutative bit for bit, so every lane of the group ends with the same bits): no LDS, no atomics, no workspace.
// The 3x3 eigenproblem is then computed by all 8 lanes alike — the lanes would idle otherwise — and lane 0 writes the row's
// outputs, each element exactly once.  No lane leaves before the shuffles; a group without a row runs with k = 0.
//
// Memory safety does not lean on the table being well-formed: a slot's index is clamped into the row's own cloud before pts
// is read, the point row of table row t must lie inside its cloud or the row is skipped, and table rows outside
// [table_offsets[0], table_offsets[C]) are neither read nor written.  On select's output no clamp changes anything.
#include "common.h"

namespace prg {

constexpr int NM_LANES = 8;      // lanes, and partial sums, per row
constexpr int NM_ROWS = 32;      // rows per 256-thread workgroup
constexpr int NM_SWEEPS = 6;     // cyclic Jacobi sweeps (tests/test_normals_spec.py: a seventh changes no bit)

// the fixed tree over the 8 partial sums of a group
__device__ __forceinline__ double nm_tree(double v) {
  v += __shfl_xor(v, 1, NM_LANES);
  v += __shfl_xor(v, 2, NM_LANES);
  v += __shfl_xor(v, 4, NM_LANES);
  return v;
}

// One Jacobi rotation in the (p, q) plane; r is the third index.  Done iff apq != 0.  theta = (aqq - app) / (2 apq),
// t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) with sgn(0) = +1 (an infinite theta, or an overflowing theta^2, gives t = 0),
// c = 1 / sqrt(t^2 + 1), s = t c.  v?p / v?q: the two columns of V.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& apr, double& aqr, double& v0p,
                                              double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq != 0.0) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    const double pr = c * apr - s * aqr, qr = s * apr + c * aqr;
    apr = pr;
    aqr = qr;
    apq = 0.0;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
  }
}

__device__ __forceinline__ bool nm_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }

__global__ __launch_bounds__(NM_LANES * NM_ROWS) void normals_kernel(const double* __restrict__ pts,
                                                                     const int64_t* __restrict__ offs, int C,
                                                                     const int32_t* __restrict__ table,
                                                                     const int64_t* __restrict__ table_offsets,
                                                                     const int32_t* __restrict__ count, int64_t Q, int limit,
                                                                     const double* __restrict__ viewpoints, int min_neighbors,
                                                                     double* __restrict__ normals, double* __restrict__ variation,
                                                                     double* __restrict__ scatter) {
  const int lane = threadIdx.x & (NM_LANES - 1);
  const int64_t t = (int64_t)blockIdx.x * NM_ROWS + (threadIdx.x / NM_LANES);   // table row: the same in the group's 8 lanes
  bool live = t < Q && t >= table_offsets[0] && t < table_offsets[C];
  int c = 0;
  int64_t first = 0, rows = 0, q = 0;
  if (live) {
    int lo = 0, hi = C;                                 // the last c in [0, C) with table_offsets[c] <= t
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (table_offsets[mid] <= t) lo = mid; else hi = mid;
    }
    c = lo;
    first = offs[c];
    rows = offs[c + 1] - first;
    q = first + (t - table_offsets[c]);
    live = q < first + rows;
  }
  double px = 0.0, py = 0.0, pz = 0.0;
  int k = 0;
  if (live) {
    px = pts[3 * q]; py = pts[3 * q + 1]; pz = pts[3 * q + 2];
    k = min(max(count[t], 0), limit);
  }
  const bool degenerate = k < min_neighbors || !(nm_finite(px) && nm_finite(py) && nm_finite(pz));
  if (degenerate) k = 0;
  const int32_t* __restrict__ slots = table + t * (int64_t)limit;
  const int64_t last = rows - 1;

  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int s = lane; s < k; s += NM_LANES) {
    const int64_t r = first + min(max((int64_t)slots[s] - first, (int64_t)0), last);
    sx = sx + pts[3 * r]; sy = sy + pts[3 * r + 1]; sz = sz + pts[3 * r + 2];
  }
  sx = nm_tree(sx); sy = nm_tree(sy); sz = nm_tree(sz);
  const double kf = (double)k;
  const double mx = sx / kf, my = sy / kf, mz = sz / kf;          // k = 0: NaN, and no slot uses it

  double sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  for (int s = lane; s < k; s += NM_LANES) {
    const int64_t r = first + min(max((int64_t)slots[s] - first, (int64_t)0), last);
    const double dx = pts[3 * r] - mx, dy = pts[3 * r + 1] - my, dz = pts[3 * r + 2] - mz;
    sxx = sxx + dx * dx; sxy = sxy + dx * dy; sxz = sxz + dx * dz;
    syy = syy + dy * dy; syz = syz + dy * dz; szz = szz + dz * dz;
  }
  sxx = nm_tree(sxx); sxy = nm_tree(sxy); sxz = nm_tree(sxz);
  syy = nm_tree(syy); syz = nm_tree(syz); szz = nm_tree(szz);
  if (!live || lane != 0) return;                                 // the group's 8 lanes hold the same S: lane 0 finishes the row

  double nx = 0.0, ny = 0.0, nz = 1.0, var = 0.0;
  if (!degenerate) {
    double a00 = sxx, a01 = sxy, a02 = sxz, a11 = syy, a12 = syz, a22 = szz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < NM_SWEEPS; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);     // (0, 1), r = 2
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);     // (0, 2), r = 1
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);     // (1, 2), r = 0
    }
    const bool s1 = a11 < a00;                          // selects, written out: an indexed column of V would live in scratch
    const double l1 = s1 ? a11 : a00;
    const bool s2 = a22 < l1;
    const double lmin = s2 ? a22 : l1;
    nx = s2 ? v02 : (s1 ? v01 : v00);
    ny = s2 ? v12 : (s1 ? v11 : v10);
    nz = s2 ? v22 : (s1 ? v21 : v20);
    const double sum = (a00 + a11) + a22;
    var = sum == 0.0 ? 0.0 : lmin / sum;
    const double vx = viewpoints[3 * c], vy = viewpoints[3 * c + 1], vz = viewpoints[3 * c + 2];
    const double d = (nx * (vx - px) + ny * (vy - py)) + nz * (vz - pz);
    if (d < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  }
  normals[3 * t] = nx; normals[3 * t + 1] = ny; normals[3 * t + 2] = nz;
  if (variation) variation[t] = var;
  if (scatter) {
    double* o = scatter + 6 * t;
    o[0] = sxx; o[1] = sxy; o[2] = sxz; o[3] = syy; o[4] = syz; o[5] = szz;
  }
}

}  // namespace prg

using namespace prg;

extern "C" {

int prg_normals_ragged_f64(const double* pts, const int64_t* offsets, int C, const int32_t* table, const int64_t* table_offsets,
                           const int32_t* pad, const int32_t* count, int64_t Q, int limit, const double* viewpoints,
                           int min_neighbors, double* normals, double* variation, double* scatter, void* stream) {
  (void)pad;                                            // the valid slots of a row are its first min(count, limit): see prg.h
  PRG_CHECK(Q >= 0 && Q < ((int64_t)1 << 31), "prg_normals_ragged_f64: Q out of range");
  PRG_CHECK(C > 0 && C <= 65535, "prg_normals_ragged_f64: C out of range (1..65535)");
  PRG_CHECK(limit >= 1 && limit <= 1024, "prg_normals_ragged_f64: limit out of range (1..1024)");
  PRG_CHECK(min_neighbors >= 3, "prg_normals_ragged_f64: min_neighbors must be >= 3");
  if (Q == 0) return PRG_OK;
  PRG_CHECK(pts && offsets && table && table_offsets && count && viewpoints && normals, "prg_normals_ragged_f64: null pointer");
  PRG_CHECK((const void*)normals != (const void*)pts && (const void*)variation != (const void*)pts &&
                (const void*)scatter != (const void*)pts,
            "prg_normals_ragged_f64: an output aliases pts");
  const unsigned grid = (unsigned)((Q + NM_ROWS - 1) / NM_ROWS);
  normals_kernel<<<grid, NM_LANES * NM_ROWS, 0, (hipStream_t)stream>>>(pts, offsets, C, table, table_offsets, count, Q, limit,
                                                                      viewpoints, min_neighbors, normals, variation, scatter);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
