// voxelgrid.hip — PointCloud.voxel_down_sample for a batch of ragged clouds on the device (include/prg.h "Geometry"), and the
// merge kernel that builds its input for a scene-memory update.
//
// Per segment the result is hostpool.cpp's voxel_down_sample bit for bit: min over the valid rows, org = min - voxel/2,
// index = floor((p - org) / voxel) in float64, key = (ix*dy + iy)*dz + iz, voxels in ascending key order, the rows of a voxel
// summed one after the other in input order starting from the first, then divided by the count (-ffp-contract=off: no FMA).
//
// Stages (all on `stream`, nothing read back):
//   1. vg_min_kernel      per-segment minimum + non-finite flag: block reduction, then ONE integer atomic per block and axis
//                         on an order-preserving 64-bit encoding of the double (a minimum is exact in any order).
//   2. vg_dims_kernel     per-segment dx,dy,dz = max index + 1 by integer atomic max.
//   3. vg_keys_kernel     sort key (segment << 46 | voxel key) per valid row, all-ones for the rest; per-segment status.
//   4. rocprim::radix_sort_pairs (key, row) — stable, so equal keys stay in input order.  The only library primitive.
//   5. vg_count_heads / scan.h's scan_blocks / vg_reduce_runs: head flags where the key changes, a two-level exclusive scan gives
//      every voxel its output slot, and the thread that owns a run's head walks the run and sums it in order.  No float atomics:
//      the output is a pure function of the input whatever the launch geometry and whatever else is in the call.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "scan.h"

namespace prg {

static constexpr int kKeyBits = 46;                  // voxel keys < 2^46 per segment (a 40 m cube at 1 mm); segment id above
static constexpr int kMaxSegments = 65535;           // gridDim.y, and 16 segment bits: 46 + 16 < 64
static constexpr unsigned long long kNoKey = ~0ull;  // rows that take no part (invalid, outside every segment, failed segment)
static constexpr int kTile = 1024;                   // sorted rows per workgroup in stage 5 (4 slabs of 256)

struct VgSeg {                      // per-segment state, zero-initialised; every field only ever grows (atomic max / or)
  unsigned long long mn_inv[3];     // ~enc(min): enc() orders doubles as unsigned integers
  unsigned long long dim[3];        // max index + 1
  unsigned int bad;                 // a valid row is NaN / Inf
  unsigned int pad;
};

__device__ __forceinline__ unsigned long long vg_enc(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}
__device__ __forceinline__ double vg_dec(unsigned long long e) {
  return __longlong_as_double((long long)((e >> 63) ? (e ^ (1ull << 63)) : ~e));
}
__device__ __forceinline__ unsigned long long vg_index(double p, double org, double voxel) {
  const double q = floor((p - org) / voxel);
  return q < 4.0e18 ? (unsigned long long)(long long)q : 4000000000000000000ull;   // beyond int64: "too large" later on
}
__device__ __forceinline__ void vg_segment(const int64_t* offsets, int b, int64_t total, int64_t& beg, int64_t& end) {
  beg = min(max(offsets[b], (int64_t)0), total);
  end = min(max(offsets[b + 1], beg), total);
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// ---- 1. minimum and non-finite flag ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vg_min_kernel(const double* __restrict__ pts, const uint8_t* __restrict__ valid,
                                                     const int64_t* __restrict__ offsets, int64_t total,
                                                     VgSeg* __restrict__ seg) {
  __shared__ unsigned long long red[4][3];
  __shared__ unsigned int red_bad[4];
  const int b = blockIdx.y;
  int64_t beg, end;
  vg_segment(offsets, b, total, beg, end);
  if (beg + (int64_t)blockIdx.x * 256 >= end) return;
  unsigned long long e[3] = {kNoKey, kNoKey, kNoKey};
  unsigned int bad = 0;
  for (int64_t i = beg + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    if (valid && !valid[i]) continue;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) { bad = 1; continue; }
    const unsigned long long ex = vg_enc(x), ey = vg_enc(y), ez = vg_enc(z);
    e[0] = ex < e[0] ? ex : e[0]; e[1] = ey < e[1] ? ey : e[1]; e[2] = ez < e[2] ? ez : e[2];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) e[c] = wave_min_u64(e[c]);
  const unsigned int any_bad = __ballot(bad != 0) != 0ull;
  if (lane == 0) { red[w][0] = e[0]; red[w][1] = e[1]; red[w][2] = e[2]; red_bad[w] = any_bad; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long m = red[0][threadIdx.x];
    for (int k = 1; k < 4; ++k) m = red[k][threadIdx.x] < m ? red[k][threadIdx.x] : m;
    if (m != kNoKey) atomicMax(&seg[b].mn_inv[threadIdx.x], ~m);
  }
  if (threadIdx.x == 3 && (red_bad[0] | red_bad[1] | red_bad[2] | red_bad[3])) atomicOr(&seg[b].bad, 1u);
}

// ---- 2. grid dimensions ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vg_dims_kernel(const double* __restrict__ pts, const uint8_t* __restrict__ valid,
                                                      const int64_t* __restrict__ offsets, int64_t total, double voxel,
                                                      VgSeg* __restrict__ seg) {
  __shared__ unsigned long long red[4][3];
  const int b = blockIdx.y;
  int64_t beg, end;
  vg_segment(offsets, b, total, beg, end);
  if (beg + (int64_t)blockIdx.x * 256 >= end) return;
  if (seg[b].bad) return;                                    // status 1: no rows come out, and NaN has no index
  const double half = voxel * 0.5;
  const double ox = vg_dec(~seg[b].mn_inv[0]) - half, oy = vg_dec(~seg[b].mn_inv[1]) - half, oz = vg_dec(~seg[b].mn_inv[2]) - half;
  unsigned long long d[3] = {0, 0, 0};
  for (int64_t i = beg + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    if (valid && !valid[i]) continue;
    const unsigned long long ix = vg_index(pts[3 * i], ox, voxel) + 1, iy = vg_index(pts[3 * i + 1], oy, voxel) + 1,
                             iz = vg_index(pts[3 * i + 2], oz, voxel) + 1;
    d[0] = ix > d[0] ? ix : d[0]; d[1] = iy > d[1] ? iy : d[1]; d[2] = iz > d[2] ? iz : d[2];
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = wave_max_u64(d[c]);
  if (lane == 0) { red[w][0] = d[0]; red[w][1] = d[1]; red[w][2] = d[2]; }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long m = red[0][threadIdx.x];
    for (int k = 1; k < 4; ++k) m = red[k][threadIdx.x] > m ? red[k][threadIdx.x] : m;
    if (m) atomicMax(&seg[b].dim[threadIdx.x], m);
  }
}

// ---- 3. sort keys and status -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vg_keys_kernel(const double* __restrict__ pts, const uint8_t* __restrict__ valid,
                                                      const int64_t* __restrict__ offsets, int64_t total, double voxel,
                                                      const VgSeg* __restrict__ seg, unsigned long long* __restrict__ keys,
                                                      uint32_t* __restrict__ rows, int32_t* __restrict__ status) {
  const int b = blockIdx.y;
  int64_t beg, end;
  vg_segment(offsets, b, total, beg, end);
  const unsigned long long dy = seg[b].dim[1], dz = seg[b].dim[2];
  const double cells = (double)seg[b].dim[0] * (double)dy * (double)dz;
  const int st = seg[b].bad ? 1 : (cells >= (double)(1ull << kKeyBits) ? 2 : 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) status[b] = st;
  if (beg + (int64_t)blockIdx.x * 256 >= end) return;
  const double half = voxel * 0.5;
  const double ox = vg_dec(~seg[b].mn_inv[0]) - half, oy = vg_dec(~seg[b].mn_inv[1]) - half, oz = vg_dec(~seg[b].mn_inv[2]) - half;
  for (int64_t i = beg + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    unsigned long long key = kNoKey;
    if (st == 0 && !(valid && !valid[i])) {
      const unsigned long long ix = vg_index(pts[3 * i], ox, voxel), iy = vg_index(pts[3 * i + 1], oy, voxel),
                               iz = vg_index(pts[3 * i + 2], oz, voxel);
      key = ((unsigned long long)b << kKeyBits) | ((ix * dy + iy) * dz + iz);
    }
    keys[i] = key;
    rows[i] = (uint32_t)i;
  }
}

// ---- 5. runs of equal keys -> voxel means ------------------------------------------------------------------------------
__device__ __forceinline__ bool vg_is_head(const unsigned long long* __restrict__ keys, int64_t i, int64_t total) {
  if (i >= total) return false;
  const unsigned long long k = keys[i];
  return k != kNoKey && (i == 0 || keys[i - 1] != k);
}

__global__ __launch_bounds__(256) void vg_count_heads(const unsigned long long* __restrict__ keys, int64_t total,
                                                      uint32_t* __restrict__ block_heads) {
  __shared__ unsigned int wsum[4];
  const int64_t base = (int64_t)blockIdx.x * kTile;
  unsigned int n = 0;
#pragma unroll
  for (int k = 0; k < kTile / 256; ++k) n += (unsigned int)__popcll(__ballot(vg_is_head(keys, base + k * 256 + threadIdx.x, total)));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;   // n is wave-uniform
  __syncthreads();
  if (threadIdx.x == 0) block_heads[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void vg_reduce_runs(const double* __restrict__ pts, const unsigned long long* __restrict__ keys,
                                                      const uint32_t* __restrict__ rows, int64_t total, int B,
                                                      const uint32_t* __restrict__ block_heads, int n_blocks,
                                                      double* __restrict__ out, int64_t* __restrict__ out_offsets) {
  __shared__ unsigned int wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t slot0 = block_heads[blockIdx.x];                   // voxels before this tile
  const int64_t n_voxels = block_heads[n_blocks];
  for (int k = 0; k < kTile / 256; ++k) {
    const int64_t i = (int64_t)blockIdx.x * kTile + k * 256 + threadIdx.x;
    const bool head = vg_is_head(keys, i, total);
    const unsigned long long bal = __ballot(head);
    if (lane == 0) wsum[w] = (unsigned int)__popcll(bal);
    __syncthreads();
    uint32_t woff = 0, all = 0;
    for (int j = 0; j < 4; ++j) {
      if (j < w) woff += wsum[j];
      all += wsum[j];
    }
    __syncthreads();
    const unsigned long long key = i < total ? keys[i] : kNoKey;
    if (i == 0 && key == kNoKey)                               // no row of the call takes part
      for (int b = 0; b <= B; ++b) out_offsets[b] = 0;
    if (key != kNoKey) {
      const int s = (int)(key >> kKeyBits);
      if (head) {
        const int64_t slot = (int64_t)slot0 + woff + __popcll(bal & ((1ull << lane) - 1ull));
        const int prev = i == 0 ? -1 : (int)(keys[i - 1] >> kKeyBits);
        for (int b = prev + 1; b <= s; ++b) out_offsets[b] = slot;        // segment s starts here; those before it are empty
        // np.add.reduceat: the first row, then += the rest in input order (the sort is stable)
        const uint32_t r0 = rows[i];
        double sx = pts[3 * (size_t)r0], sy = pts[3 * (size_t)r0 + 1], sz = pts[3 * (size_t)r0 + 2];
        int64_t j = i + 1;
        for (; j < total && keys[j] == key; ++j) {
          const uint32_t r = rows[j];
          sx += pts[3 * (size_t)r]; sy += pts[3 * (size_t)r + 1]; sz += pts[3 * (size_t)r + 2];
        }
        const double c = (double)(j - i);
        out[3 * slot] = sx / c; out[3 * slot + 1] = sy / c; out[3 * slot + 2] = sz / c;
      }
      if (i == total - 1 || keys[i + 1] == kNoKey)              // the last row that takes part closes every later segment
        for (int b = s + 1; b <= B; ++b) out_offsets[b] = n_voxels;
    }
    slot0 += all;
  }
}

// ---- memory update input: [memory_b widened to float64, valid = 1 | the HW rows of xyz[b] with valid[b]] ---------------------
__global__ __launch_bounds__(256) void vg_merge_kernel(const float* __restrict__ mem, const int64_t* __restrict__ mem_offsets,
                                                       int64_t mem_rows, const double* __restrict__ xyz,
                                                       const uint8_t* __restrict__ valid, int HW, double* __restrict__ merged,
                                                       uint8_t* __restrict__ merged_valid, int64_t* __restrict__ merged_offsets,
                                                       int B) {
  const int b = blockIdx.y;
  int64_t beg, end;
  vg_segment(mem_offsets, b, mem_rows, beg, end);
  const int64_t n_mem = end - beg, dst = beg + (int64_t)b * HW;     // rows of the segments before: their memory + b views
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    merged_offsets[b] = dst;
    if (b == B - 1) merged_offsets[B] = dst + n_mem + HW;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_mem + HW; i += (int64_t)gridDim.x * 256) {
    double x, y, z;
    uint8_t v = 1;
    if (i < n_mem) {
      const float* p = mem + 3 * (beg + i);
      x = (double)p[0]; y = (double)p[1]; z = (double)p[2];
    } else {
      const size_t r = (size_t)b * HW + (size_t)(i - n_mem);
      x = xyz[3 * r]; y = xyz[3 * r + 1]; z = xyz[3 * r + 2];
      v = valid[r] ? 1 : 0;
    }
    double* q = merged + 3 * (dst + i);
    q[0] = x; q[1] = y; q[2] = z;
    merged_valid[dst + i] = v;
  }
}

// ---- workspace layout (host arithmetic only) ---------------------------------------------------------------------------
struct VgLayout {
  size_t seg, keys0, keys1, rows0, rows1, heads, sort, sort_bytes, bytes;
  int n_blocks;
};

static inline size_t vg_align(size_t x) { return (x + 255) & ~(size_t)255; }

static VgLayout vg_layout(int64_t total, int B) {
  VgLayout L;
  const size_t n = (size_t)(total > 0 ? total : 0), nb = (size_t)(B > 0 ? B : 0);
  L.n_blocks = (int)((n + kTile - 1) / kTile);
  size_t at = 0;
  L.seg = at;   at += vg_align(nb * sizeof(VgSeg));
  L.keys0 = at; at += vg_align(n * 8);
  L.keys1 = at; at += vg_align(n * 8);
  L.rows0 = at; at += vg_align(n * 4);
  L.rows1 = at; at += vg_align(n * 4);
  L.heads = at; at += vg_align(((size_t)L.n_blocks + 1) * 4);
  // rocPRIM's radix sort on caller-provided double buffers keeps digit histograms and one look-back word per (digit, block of
  // >= 1024 rows) besides: 1 MiB + 4 bytes per row covers it with a wide margin; the call checks what the library asks for
  L.sort = at;  L.sort_bytes = vg_align(((size_t)1 << 20) + n * 4); at += L.sort_bytes;
  L.bytes = at;
  return L;
}

static inline int vg_grid_x(int64_t total, int B) {
  // slabs of 1024 rows for a segment four times the average; longer ones loop (grid-stride)
  const int64_t avg = (total + B - 1) / B;
  int64_t gx = (4 * avg + 1023) / 1024;
  return (int)(gx < 1 ? 1 : gx > 1024 ? 1024 : gx);
}

}  // namespace prg

using namespace prg;

extern "C" {

size_t prg_voxel_grid_workspace_bytes(int64_t total, int B) { return vg_layout(total, B).bytes; }

int prg_voxel_grid_ragged(const double* pts, const uint8_t* valid, const int64_t* offsets, int B, int64_t total, double voxel,
                          double* out, int64_t* out_offsets, int32_t* status, void* workspace, size_t workspace_bytes,
                          void* stream) {
  PRG_CHECK(offsets && out_offsets && status, "prg_voxel_grid_ragged: null pointer");
  PRG_CHECK(B > 0 && B <= kMaxSegments && total >= 0 && total < ((int64_t)1 << 31), "prg_voxel_grid_ragged: bad shape");
  PRG_CHECK(voxel > 0, "prg_voxel_grid_ragged: voxel_size <= 0");
  hipStream_t s = (hipStream_t)stream;
  if (total == 0) {
    PRG_HIP(hipMemsetAsync(out_offsets, 0, sizeof(int64_t) * ((size_t)B + 1), s));
    PRG_HIP(hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)B, s));
    return PRG_OK;
  }
  PRG_CHECK(pts && out && workspace, "prg_voxel_grid_ragged: null pointer");
  const VgLayout L = vg_layout(total, B);
  PRG_CHECK(workspace_bytes >= L.bytes, "prg_voxel_grid_ragged: workspace smaller than prg_voxel_grid_workspace_bytes");
  PRG_CHECK((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "prg_voxel_grid_ragged: workspace not 8-byte aligned");
  char* ws = (char*)workspace;
  VgSeg* seg = (VgSeg*)(ws + L.seg);
  unsigned long long *keys0 = (unsigned long long*)(ws + L.keys0), *keys1 = (unsigned long long*)(ws + L.keys1);
  uint32_t *rows0 = (uint32_t*)(ws + L.rows0), *rows1 = (uint32_t*)(ws + L.rows1), *heads = (uint32_t*)(ws + L.heads);

  PRG_HIP(hipMemsetAsync(seg, 0, sizeof(VgSeg) * (size_t)B, s));
  PRG_HIP(hipMemsetAsync(keys0, 0xFF, sizeof(unsigned long long) * (size_t)total, s));   // rows outside every segment: no key
  const dim3 grid((unsigned)vg_grid_x(total, B), (unsigned)B, 1);
  vg_min_kernel<<<grid, 256, 0, s>>>(pts, valid, offsets, total, seg);
  PRG_LAUNCH_CHECK();
  vg_dims_kernel<<<grid, 256, 0, s>>>(pts, valid, offsets, total, voxel, seg);
  PRG_LAUNCH_CHECK();
  vg_keys_kernel<<<grid, 256, 0, s>>>(pts, valid, offsets, total, voxel, seg, keys0, rows0, status);
  PRG_LAUNCH_CHECK();

  int seg_bits = 0;
  while ((B >> seg_bits) != 0) ++seg_bits;             // the all-ones key sorts behind segment B - 1
  rocprim::double_buffer<unsigned long long> dk(keys0, keys1);
  rocprim::double_buffer<uint32_t> dv(rows0, rows1);
  size_t need = 0;
  PRG_HIP(rocprim::radix_sort_pairs(nullptr, need, dk, dv, (unsigned int)total, 0u, (unsigned)(kKeyBits + seg_bits), s));
  PRG_CHECK(need <= L.sort_bytes, "prg_voxel_grid_ragged: the sort asks for more temporary storage than the workspace reserves");
  need = L.sort_bytes;
  PRG_HIP(rocprim::radix_sort_pairs(ws + L.sort, need, dk, dv, (unsigned int)total, 0u, (unsigned)(kKeyBits + seg_bits), s));

  vg_count_heads<<<L.n_blocks, 256, 0, s>>>(dk.current(), total, heads);
  PRG_LAUNCH_CHECK();
  scan_blocks<uint32_t, true><<<1, kScanThreads, 0, s>>>(heads, L.n_blocks);   // heads[n_blocks] = voxels of the whole call
  PRG_LAUNCH_CHECK();
  vg_reduce_runs<<<L.n_blocks, 256, 0, s>>>(pts, dk.current(), dv.current(), total, B, heads, L.n_blocks, out, out_offsets);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

int prg_merge_memory_f64(const float* memory, const int64_t* memory_offsets, int64_t memory_rows, const double* xyz,
                         const uint8_t* valid, int B, int HW, double* merged, uint8_t* merged_valid, int64_t* merged_offsets,
                         void* stream) {
  PRG_CHECK(memory_offsets && xyz && valid && merged && merged_valid && merged_offsets, "prg_merge_memory_f64: null pointer");
  PRG_CHECK((memory || memory_rows == 0) && memory_rows >= 0, "prg_merge_memory_f64: null memory cloud");
  PRG_CHECK(B > 0 && B <= kMaxSegments && HW > 0, "prg_merge_memory_f64: bad shape");
  const dim3 grid((unsigned)vg_grid_x(memory_rows + (int64_t)B * HW, B), (unsigned)B, 1);
  vg_merge_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(memory, memory_offsets, memory_rows, xyz, valid, HW, merged,
                                                        merged_valid, merged_offsets, B);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // extern "C"
