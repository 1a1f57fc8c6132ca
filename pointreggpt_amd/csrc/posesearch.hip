// posesearch.hip — score candidate camera poses before a diffusion chain is spent on one of them.
//
// For every (scene b, candidate c) the rows of scene b's ragged float32 cloud are moved by poses[b, c] and projected into the
// scene's camera with camera.h's arithmetic — geometry.hip's, so a candidate's z-buffer here is prg_project_points_zbuffer's for
// that pose, bit for bit — and three integers come back: the rows the z-buffer takes (in_frame), the rows the target camera SEES
// (seen: within z_tol of their pixel's nearest depth, and inside the crop box in the target frame) and the pixels that received a
// row (covered).  seen / rows predicts the overlap of the pair that pose would generate: DDNM keeps every reprojected pixel, so
// the source points the target camera sees end up in the target cloud.
//
// Two passes over per-candidate z-buffers in the caller's workspace, a chunk of candidates at a time:
//   scatter  atomicMin of the depth's bit pattern per (candidate, pixel).  The atomic that finds the sentinel is the pixel's
//            first: exactly one per covered pixel, whatever the order, which is what `covered` counts.
//   count    the same projection again; a row is seen when z <= zmin(pixel) + z_tol (float32) and lo <= q <= hi.
// A thread loads its row once per chunk and applies the chunk's poses to it; pose, camera and box are uniform over the block
// (blockIdx and the loop counter), so they live in scalar registers.  A candidate's flags are reduced per wave by ballot, per
// block in LDS, and leave the block as ONE atomicAdd per (candidate, counter).  Integer atomics on 32-bit words: the counts do
// not depend on the order of the waves or on the chunking.
#include "camera.h"

namespace prg {

constexpr int PS_THREADS = 256;
constexpr int PS_BLOCKS = 64;        // row slabs per scene in flight; a block strides over the rest
constexpr int PS_MAX_CHUNK = 256;    // candidates per launch at most: the block's LDS counters
constexpr size_t PS_WORKSPACE_CAP = (size_t)256 << 20;

struct PoseBox {
  float lo[3], hi[3];
  int on;
};

// counter k of candidate c of scene b
__device__ __forceinline__ int32_t* ps_count(int32_t* counts, int b, int N, int c, int k) {
  return counts + ((size_t)b * N + c) * 3 + k;
}

// pass 1.  grid (PS_BLOCKS, B); zbuf: (B, nc, H*W) words, all kEmpty; candidates [c0, c0 + nc) of every scene.
__global__ __launch_bounds__(PS_THREADS) void pose_scatter_kernel(const float* __restrict__ pts, const int64_t* __restrict__ offsets,
                                                                  const float* __restrict__ poses, const float* __restrict__ K,
                                                                  uint32_t* __restrict__ zbuf, int32_t* __restrict__ counts, int N,
                                                                  int c0, int nc, int H, int W) {
  __shared__ int32_t first[PS_MAX_CHUNK];
  const int b = blockIdx.y;
  const int64_t beg = offsets[b], end = offsets[b + 1];
  const int64_t stride = (int64_t)gridDim.x * PS_THREADS;
  if (beg + (int64_t)blockIdx.x * PS_THREADS >= end) return;        // no slab for this block (uniform exit)
  for (int k = threadIdx.x; k < nc; k += PS_THREADS) first[k] = 0;
  __syncthreads();
  const Cam cam = load_cam(K, b);
  const int HW = H * W;
  const bool lead = (threadIdx.x & 63) == 0;
  for (int64_t base = beg + (int64_t)blockIdx.x * PS_THREADS; base < end; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < end;
    float x = 0.0f, y = 0.0f, z = 0.0f;                             // a dead lane's row fails z > 0
    if (live) { x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2]; }
    for (int k = 0; k < nc; ++k) {
      const float* P = poses + ((size_t)b * N + c0 + k) * 16;
      float qx, qy, qz;
      se3_apply(P, x, y, z, qx, qy, qz);
      size_t pix;
      bool won = false;
      if (live && splat_pixel(cam, qx, qy, qz, H, W, pix))
        won = atomicMin(zbuf + ((size_t)b * nc + k) * HW + pix, __float_as_uint(qz)) == kEmpty;
      const unsigned long long w = __ballot(won);
      if (lead && w) atomicAdd(first + k, (int32_t)__popcll(w));
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nc; k += PS_THREADS)
    if (first[k]) atomicAdd(ps_count(counts, b, N, c0 + k, 2), first[k]);
}

// pass 2.  The same grid over the finished z-buffers.
__global__ __launch_bounds__(PS_THREADS) void pose_count_kernel(const float* __restrict__ pts, const int64_t* __restrict__ offsets,
                                                                const float* __restrict__ poses, const float* __restrict__ K,
                                                                const uint32_t* __restrict__ zbuf, int32_t* __restrict__ counts, int N,
                                                                int c0, int nc, int H, int W, PoseBox box, float z_tol) {
  __shared__ int32_t acc[PS_MAX_CHUNK * 2];                         // (in_frame, seen) per candidate of the chunk
  const int b = blockIdx.y;
  const int64_t beg = offsets[b], end = offsets[b + 1];
  const int64_t stride = (int64_t)gridDim.x * PS_THREADS;
  if (beg + (int64_t)blockIdx.x * PS_THREADS >= end) return;        // no slab for this block (uniform exit)
  for (int k = threadIdx.x; k < 2 * nc; k += PS_THREADS) acc[k] = 0;
  __syncthreads();
  const Cam cam = load_cam(K, b);
  const int HW = H * W;
  const bool lead = (threadIdx.x & 63) == 0;
  for (int64_t base = beg + (int64_t)blockIdx.x * PS_THREADS; base < end; base += stride) {
    const int64_t i = base + threadIdx.x;
    const bool live = i < end;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (live) { x = pts[i * 3]; y = pts[i * 3 + 1]; z = pts[i * 3 + 2]; }
    for (int k = 0; k < nc; ++k) {
      const float* P = poses + ((size_t)b * N + c0 + k) * 16;
      float qx, qy, qz;
      se3_apply(P, x, y, z, qx, qy, qz);
      size_t pix;
      bool in = false, seen = false;
      if (live && splat_pixel(cam, qx, qy, qz, H, W, pix)) {
        in = true;
        const float zmin = __uint_as_float(zbuf[((size_t)b * nc + k) * HW + pix]);   // set by pass 1: this row at the least
        seen = qz <= zmin + z_tol;
        if (box.on)
          seen = seen && qx >= box.lo[0] && qx <= box.hi[0] && qy >= box.lo[1] && qy <= box.hi[1] && qz >= box.lo[2] &&
                 qz <= box.hi[2];
      }
      const unsigned long long wi = __ballot(in), ws = __ballot(seen);
      if (lead && wi) {
        atomicAdd(acc + 2 * k, (int32_t)__popcll(wi));
        if (ws) atomicAdd(acc + 2 * k + 1, (int32_t)__popcll(ws));
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 2 * nc; k += PS_THREADS)
    if (acc[k]) atomicAdd(ps_count(counts, b, N, c0 + (k >> 1), k & 1), acc[k]);
}

}  // namespace prg

using namespace prg;

extern "C" {

size_t prg_pose_candidate_workspace_bytes(int B, int N, int H, int W) {
  if (B < 1 || N < 1 || H < 1 || W < 1) return 0;
  const size_t one = (size_t)B * (size_t)H * (size_t)W * sizeof(uint32_t);       // one candidate per scene
  const size_t cap_n = PS_WORKSPACE_CAP / one;                                    // candidates that fit under the cap
  if (cap_n < 1) return one;
  return one * ((size_t)N < cap_n ? (size_t)N : cap_n);
}

int prg_pose_candidate_counts(const float* points, const int64_t* offsets, const float* poses, const float* K, int B, int N, int H,
                              int W, const float* box, float z_tol, int32_t* counts, void* workspace, size_t workspace_bytes,
                              void* stream) {
  PRG_CHECK(points && offsets && poses && K && counts && workspace, "prg_pose_candidate_counts: null pointer");
  PRG_CHECK(B >= 1 && B <= 65535 && N >= 1 && N <= 65535, "prg_pose_candidate_counts: B and N must be in 1..65535");
  PRG_CHECK(H >= 1 && W >= 1 && (int64_t)H * W <= 0x7FFFFFFF, "prg_pose_candidate_counts: bad image size");
  PRG_CHECK(z_tol >= 0.0f && z_tol <= 3.40282346638528859812e38f, "prg_pose_candidate_counts: z_tol must be finite and >= 0");
  PRG_CHECK((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "prg_pose_candidate_counts: workspace must be 4-byte aligned");
  const size_t one = (size_t)B * (size_t)H * (size_t)W * sizeof(uint32_t);
  PRG_CHECK(workspace_bytes >= one, "prg_pose_candidate_counts: the workspace holds less than one candidate per scene");
  size_t chunk = workspace_bytes / one;
  if (chunk > (size_t)N) chunk = (size_t)N;
  if (chunk > (size_t)PS_MAX_CHUNK) chunk = PS_MAX_CHUNK;
  PoseBox pb{};
  if (box) {
    for (int k = 0; k < 3; ++k) { pb.lo[k] = box[k]; pb.hi[k] = box[3 + k]; }
    pb.on = 1;
  }
  hipStream_t s = (hipStream_t)stream;
  PRG_HIP(hipMemsetAsync(counts, 0, sizeof(int32_t) * 3 * (size_t)B * N, s));
  const dim3 grid(PS_BLOCKS, (unsigned)B, 1);
  for (int c0 = 0; c0 < N; c0 += (int)chunk) {
    const int nc = N - c0 < (int)chunk ? N - c0 : (int)chunk;
    PRG_HIP(hipMemsetAsync(workspace, 0xFF, one * (size_t)nc, s));
    pose_scatter_kernel<<<grid, PS_THREADS, 0, s>>>(points, offsets, poses, K, (uint32_t*)workspace, counts, N, c0, nc, H, W);
    PRG_LAUNCH_CHECK();
    pose_count_kernel<<<grid, PS_THREADS, 0, s>>>(points, offsets, poses, K, (const uint32_t*)workspace, counts, N, c0, nc, H, W, pb,
                                                  z_tol);
    PRG_LAUNCH_CHECK();
  }
  return PRG_OK;
}

}  // extern "C"
