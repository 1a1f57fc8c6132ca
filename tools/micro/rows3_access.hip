// A/B of access patterns for a 3-double-row streaming kernel: LDS-staged unit-stride lanes vs a thread reading its own row.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
#include <algorithm>
struct Box { double lo[3], hi[3]; };
__device__ __forceinline__ void work(const double* m, const Box& box, double& x, double& y, double& z, bool& keep) {
  const double px = x, py = y, pz = z;
  x = px * m[0] + py * m[1] + pz * m[2] + m[3];
  y = px * m[4] + py * m[5] + pz * m[6] + m[7];
  z = px * m[8] + py * m[9] + pz * m[10] + m[11];
  keep = x >= box.lo[0] && x <= box.hi[0] && y >= box.lo[1] && y <= box.hi[1] && z >= box.lo[2] && z <= box.hi[2];
}
template <int ROWS>   // ROWS rows per tile, 256 threads
__global__ __launch_bounds__(256) void staged(const double* pts, int64_t per, const double* T, Box box, double* out, uint8_t* vout) {
  __shared__ double tile[3 * ROWS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int64_t beg = (int64_t)b * per, end = beg + per;
  double m[12];
  for (int k = 0; k < 12; ++k) m[k] = T[b * 16 + k];
  for (int64_t t0 = beg + (int64_t)blockIdx.x * ROWS; t0 < end; t0 += (int64_t)gridDim.x * ROWS) {
    const int n = (int)min((int64_t)ROWS, end - t0);
    const double* src = pts + 3 * t0; double* dst = out + 3 * t0;
#pragma unroll
    for (int k = 0; k < 3 * ROWS / 256; ++k) { const int j = k * 256 + tid; if (j < 3 * n) tile[j] = src[j]; }
    __syncthreads();
#pragma unroll
    for (int r = tid; r < ROWS; r += 256) if (r < n) {
      double x = tile[3 * r], y = tile[3 * r + 1], z = tile[3 * r + 2]; bool keep;
      work(m, box, x, y, z, keep);
      tile[3 * r] = x; tile[3 * r + 1] = y; tile[3 * r + 2] = z; vout[t0 + r] = keep;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3 * ROWS / 256; ++k) { const int j = k * 256 + tid; if (j < 3 * n) dst[j] = tile[j]; }
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void direct(const double* pts, int64_t per, const double* T, Box box, double* out, uint8_t* vout) {
  const int b = blockIdx.y;
  const int64_t beg = (int64_t)b * per, end = beg + per;
  double m[12];
  for (int k = 0; k < 12; ++k) m[k] = T[b * 16 + k];
  for (int64_t i = beg + (int64_t)blockIdx.x * 256 + threadIdx.x; i < end; i += (int64_t)gridDim.x * 256) {
    double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2]; bool keep;
    work(m, box, x, y, z, keep);
    out[3 * i] = x; out[3 * i + 1] = y; out[3 * i + 2] = z; vout[i] = keep;
  }
}
#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(_e), __LINE__); return 1; } } while (0)
int main() {
  const int B = 64;
  for (int64_t total : {2000000LL, 20000000LL}) {
    const int64_t per = total / B;
    double *pts, *out, *T; uint8_t* v;
    CK(hipMalloc(&pts, total * 24)); CK(hipMalloc(&out, total * 24)); CK(hipMalloc(&v, total)); CK(hipMalloc(&T, B * 128));
    std::vector<double> h(total * 3); for (size_t i = 0; i < h.size(); ++i) h[i] = (double)((i * 2654435761u) % 4000) / 1000.0 - 1.5;
    std::vector<double> hT(B * 16, 0.0); for (int b = 0; b < B; ++b) { hT[b*16] = 0.98; hT[b*16+1] = -0.19; hT[b*16+4] = 0.19; hT[b*16+5] = 0.98; hT[b*16+10] = 1; hT[b*16+3] = 0.1; hT[b*16+15] = 1; }
    CK(hipMemcpy(pts, h.data(), total * 24, hipMemcpyHostToDevice)); CK(hipMemcpy(T, hT.data(), B * 128, hipMemcpyHostToDevice));
    Box box = {{-1.5, -1.5, 0.5}, {1.5, 1.5, 3.5}};
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int64_t avg = per;
    for (int variant = 0; variant < 6; ++variant) {
      std::vector<float> ms;
      for (int it = 0; it < 25; ++it) {
        CK(hipEventRecord(e0));
        int gx256 = (int)std::min<int64_t>(4096, (4 * avg + 255) / 256), gx512 = (int)std::min<int64_t>(4096, (4 * avg + 511) / 512);
        int gx1 = (int)std::min<int64_t>(4096, (avg + 255) / 256);
        switch (variant) {
          case 0: staged<256><<<dim3(gx256, B), 256>>>(pts, per, T, box, out, v); break;
          case 1: staged<256><<<dim3(gx1, B), 256>>>(pts, per, T, box, out, v); break;
          case 2: staged<512><<<dim3(gx512, B), 256>>>(pts, per, T, box, out, v); break;
          case 3: staged<1024><<<dim3((gx512 + 1) / 2, B), 256>>>(pts, per, T, box, out, v); break;
          case 4: direct<<<dim3(gx256, B), 256>>>(pts, per, T, box, out, v); break;
          case 5: direct<<<dim3(gx1, B), 256>>>(pts, per, T, box, out, v); break;
        }
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float t; CK(hipEventElapsedTime(&t, e0, e1)); if (it >= 5) ms.push_back(t);
      }
      CK(hipGetLastError());
      std::sort(ms.begin(), ms.end());
      const char* names[] = {"staged256 grid4x", "staged256 grid1x(capped 4096)", "staged512", "staged1024", "direct grid4x", "direct grid1x"};
      printf("rows %lld  %-32s median %.4f ms  %.0f GB/s\n", (long long)total, names[variant], ms[ms.size() / 2], 49.0 * total / (ms[ms.size() / 2] * 1e-3) / 1e9);
    }
    CK(hipFree(pts)); CK(hipFree(out)); CK(hipFree(v)); CK(hipFree(T));
  }
  return 0;
}
