// validate.hip — checkpoint validation on the device: the forward process q(x_t | x_0), the training loss of one network output
// (GaussianDiffusion.q_sample / p_losses, sd:1448-1497) and the sums behind MaskTrainer.compute_metrics (dc:1229-1250).
// Three streaming kernels (16-byte loads where the rows allow them) and two small second passes; no atomics, no host
// synchronisation, everything on the caller's stream.  Built with -ffp-contract=off: every float32 step below is one rounded
// operation, as torch computes it; the contract is stated at the entries in include/prg.h.
//
// Summation order (depends on HW alone; pointreggpt_amd/validate.py states it in numpy as `ordered_sum`):
//   block k of sample b owns pixels [4096 k, 4096 (k + 1)); thread j of 256 takes the quads j, j + 256, j + 512, j + 768 of the
//   block in that order and adds their terms, widened to float64, one by one in pixel order to an accumulator that starts at
//   +0 (pixels past HW add nothing: acc + 0 is acc); the 64 lanes of a wave are folded by six xor exchanges, lane bit 0 first
//   (a balanced tree over neighbouring lanes; IEEE addition commutes, so both partners hold the same bits); thread 0 adds the
//   four wave totals in wave order; the second pass adds the ceil(HW / 4096) block partials of a sample in index order.
//   (The packed counts travel through the same 8-byte slots; a double load or store moves their bits unchanged.)
#include "common.h"
#include "philox.h"
#include "sampler.h"
#include "wave_ops.h"

namespace prg {

constexpr int kValThreads = 256, kValIters = 4;
constexpr int kValBlockPixels = kValThreads * 4 * kValIters;   // 4096
constexpr int kValSlots = 3;                                     // 8-byte workspace slots per (sample, block): the mask metrics' need

static inline int val_blocks(int HW) { return ceil_div(HW, kValBlockPixels); }

// ---- 64-bit lane exchange: a double (or the packed counts) goes as its two 32-bit halves through wave_ops.h's lane_xor ----
template <int BIT>
__device__ inline uint64_t lane_xor_u64(uint64_t v) {
  const float lo = lane_xor<BIT>(__uint_as_float((uint32_t)v));
  const float hi = lane_xor<BIT>(__uint_as_float((uint32_t)(v >> 32)));
  return (uint64_t)__float_as_uint(lo) | ((uint64_t)__float_as_uint(hi) << 32);
}
template <int BIT>
__device__ inline double lane_xor_f64(double v) {
  return __longlong_as_double((long long)lane_xor_u64<BIT>((uint64_t)__double_as_longlong(v)));
}
__device__ inline double wave_sum_f64(double v) {
  v = v + lane_xor_f64<0>(v);
  v = v + lane_xor_f64<1>(v);
  v = v + lane_xor_f64<2>(v);
  v = v + lane_xor_f64<3>(v);
  v = v + lane_xor_f64<4>(v);
  v = v + lane_xor_f64<5>(v);
  return v;
}
__device__ inline uint64_t wave_sum_u64(uint64_t v) {
  v += lane_xor_u64<0>(v);
  v += lane_xor_u64<1>(v);
  v += lane_xor_u64<2>(v);
  v += lane_xor_u64<3>(v);
  v += lane_xor_u64<4>(v);
  v += lane_xor_u64<5>(v);
  return v;
}

// ---- one quad (4 consecutive pixels of a sample's row) as 16 bytes, or pixel by pixel where the row is not 16-byte aligned ----
template <bool VEC>
__device__ inline void load_quad(float (&v)[4], const float* __restrict__ row, int q, int HW) {
  if constexpr (VEC) {
    const float4 t = *reinterpret_cast<const float4*>(row + (size_t)q * 4);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = q * 4 + e < HW ? row[(size_t)q * 4 + e] : 0.0f;
  }
}
template <bool VEC>
__device__ inline void store_quad(float* __restrict__ row, int q, int HW, const float (&v)[4]) {
  if constexpr (VEC) {
    *reinterpret_cast<float4*>(row + (size_t)q * 4) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (q * 4 + e < HW) row[(size_t)q * 4 + e] = v[e];
  }
}
// the noise of quad q of sample b: the stored row, or Philox draw `draw` of seeds[b] under the validation tag
template <bool VEC>
__device__ inline void noise_quad(float (&n)[4], const float* __restrict__ noise_row, uint64_t key, uint32_t draw, int q, int HW) {
  if (noise_row) {
    load_quad<VEC>(n, noise_row, q, HW);
  } else {
    const float4 t = philox_normal4(key, draw, (uint32_t)q, PHILOX_DOMAIN_VALIDATE);
    n[0] = t.x; n[1] = t.y; n[2] = t.z; n[3] = t.w;
  }
}

// ---- prg_q_sample: x_t = fl(fl(a x0) + fl(s n)) ----
template <bool VEC>
__global__ __launch_bounds__(kValThreads) void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ a,
                                                               const float* __restrict__ s, const float* __restrict__ noise,
                                                               const uint64_t* __restrict__ seeds, uint32_t draw, int HW,
                                                               float* __restrict__ x_t, float* __restrict__ noise_out) {
  const int b = blockIdx.y;
  const size_t row = (size_t)b * HW;
  const float ab = a[b], sb = s[b];
  const uint64_t key = noise ? 0 : seeds[b];
  const int q0 = blockIdx.x * (kValThreads * kValIters) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < kValIters; ++it) {
    const int q = q0 + it * kValThreads;
    if ((size_t)q * 4 >= (size_t)HW) break;
    float x[4], n[4], r[4];
    load_quad<VEC>(x, x0 + row, q, HW);
    noise_quad<VEC>(n, noise ? noise + row : nullptr, key, draw, q, HW);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p0 = ab * x[e], p1 = sb * n[e];
      r[e] = p0 + p1;
    }
    store_quad<VEC>(x_t + row, q, HW, r);
    if (noise_out) store_quad<VEC>(noise_out + row, q, HW, n);
  }
}

// ---- block partial: the four wave totals through LDS, added by thread 0 in wave order ----
__device__ inline double block_sum_f64(double acc, double* lds) {
  const double w = wave_sum_f64(acc);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = w;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) t = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  __syncthreads();
  return t;   // valid in thread 0
}

// ---- prg_diffusion_loss, first pass ----
template <bool VEC>
__global__ __launch_bounds__(kValThreads) void diffusion_loss_kernel(const float* __restrict__ u, const float* __restrict__ x0,
                                                                     const float* __restrict__ noise, const uint64_t* __restrict__ seeds,
                                                                     uint32_t draw, const float* __restrict__ a, const float* __restrict__ s,
                                                                     int objective, int loss_type, int HW, double* __restrict__ ws) {
  __shared__ double lds[4];
  const int b = blockIdx.y;
  const size_t row = (size_t)b * HW;
  const float ab = a[b], sb = s[b];
  const uint64_t key = noise ? 0 : seeds[b];
  const int q0 = blockIdx.x * (kValThreads * kValIters) + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int it = 0; it < kValIters; ++it) {
    const int q = q0 + it * kValThreads;
    if ((size_t)q * 4 < (size_t)HW) {
      float uu[4], x[4], n[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      load_quad<VEC>(uu, u + row, q, HW);
      load_quad<VEC>(x, x0 + row, q, HW);
      if (objective != 0) noise_quad<VEC>(n, noise ? noise + row : nullptr, key, draw, q, HW);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float target;
        if (objective == 0) target = x[e];
        else if (objective == 1) target = n[e];
        else { const float p0 = ab * n[e], p1 = sb * x[e]; target = p0 - p1; }
        const float d = uu[e] - target;
        const float term = loss_type == 0 ? fabsf(d) : d * d;
        if (q * 4 + e < HW) acc = acc + (double)term;
      }
    }
  }
  const double t = block_sum_f64(acc, lds);
  if (threadIdx.x == 0) ws[(size_t)b * gridDim.x + blockIdx.x] = t;
}

// second pass, one workgroup per sample: the partials come in through LDS, kFinishChunk at a time with every thread loading, and
// thread 0 adds them in index order (a lone thread reading global memory would wait out one load latency per few partials: 4096 of
// them at 16 Mpx); mean = sum / HW, loss = mean * (double)w[b]
constexpr int kFinishChunk = 1024;
__global__ __launch_bounds__(kValThreads) void diffusion_loss_finish_kernel(const double* __restrict__ ws, const float* __restrict__ w,
                                                                            int HW, int nblk, double* __restrict__ out) {
  __shared__ double buf[kFinishChunk];
  const int b = blockIdx.x;
  double sum = 0.0;
  for (int base = 0; base < nblk; base += kFinishChunk) {
    const int n = min(kFinishChunk, nblk - base);
    for (int i = threadIdx.x; i < n; i += kValThreads) buf[i] = ws[(size_t)b * nblk + base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) sum = sum + buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double mean = sum / (double)HW;
    out[2 * b] = mean;
    out[2 * b + 1] = mean * (double)w[b];
  }
}

// ---- prg_mask_metrics, first pass: |d| and d^2 sums, and the four counts packed as 16-bit fields (a block has 4096 pixels) ----
template <bool VEC>
__global__ __launch_bounds__(kValThreads) void mask_metrics_kernel(const float* __restrict__ prob, const float* __restrict__ input,
                                                                   const float* __restrict__ label, const float* __restrict__ mask,
                                                                   float thr, float tol, int HW, double* __restrict__ ws) {
  __shared__ double lds[4];
  __shared__ unsigned long long cnt_lds[4];
  const int b = blockIdx.y;
  const size_t row = (size_t)b * HW;
  const int q0 = blockIdx.x * (kValThreads * kValIters) + threadIdx.x;
  double acc_abs = 0.0, acc_sq = 0.0;
  uint64_t cnt = 0;
#pragma unroll
  for (int it = 0; it < kValIters; ++it) {
    const int q = q0 + it * kValThreads;
    if ((size_t)q * 4 < (size_t)HW) {
      float p[4], in[4], lb[4], mk[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      load_quad<VEC>(p, prob + row, q, HW);
      load_quad<VEC>(in, input + row, q, HW);
      load_quad<VEC>(lb, label + row, q, HW);
      if (mask) load_quad<VEC>(mk, mask + row, q, HW);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float mv = mask ? mk[e] : (fabsf(lb[e] - in[e]) < tol ? 1.0f : 0.0f);   // PairedDepthDataset's label mask (dc:941)
        const bool o = p[e] > thr, m = mv > thr;                                      // NaN compares false
        const float out = o ? in[e] : 0.0f, lab = m ? lb[e] : 0.0f;
        const float d = lab - out;
        const float sq = d * d;
        if (q * 4 + e < HW) {
          acc_abs = acc_abs + (double)fabsf(d);
          acc_sq = acc_sq + (double)sq;
          cnt += (uint64_t)1 << (16 * (2 * (int)m + (int)o));
        }
      }
    }
  }
  // (a wave holds at most 1024 pixels, a block 4096: no field reaches 2^16)
  const uint64_t wc = wave_sum_u64(cnt);
  if ((threadIdx.x & 63) == 0) cnt_lds[threadIdx.x >> 6] = wc;
  const double t_abs = block_sum_f64(acc_abs, lds);
  const double t_sq = block_sum_f64(acc_sq, lds);
  if (threadIdx.x == 0) {
    double* slot = ws + ((size_t)b * gridDim.x + blockIdx.x) * kValSlots;
    slot[0] = t_abs;
    slot[1] = t_sq;
    reinterpret_cast<unsigned long long*>(slot)[2] = cnt_lds[0] + cnt_lds[1] + cnt_lds[2] + cnt_lds[3];
  }
}

__global__ __launch_bounds__(kValThreads) void mask_metrics_finish_kernel(const double* __restrict__ ws, int nblk,
                                                                          long long* __restrict__ counts, double* __restrict__ sums) {
  __shared__ double buf[kFinishChunk * kValSlots];
  const int b = blockIdx.x;
  double s_abs = 0.0, s_sq = 0.0;
  long long c[4] = {0, 0, 0, 0};
  for (int base = 0; base < nblk; base += kFinishChunk) {
    const int n = min(kFinishChunk, nblk - base);
    for (int i = threadIdx.x; i < n * kValSlots; i += kValThreads) buf[i] = ws[((size_t)b * nblk + base) * kValSlots + i];
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < n; ++i) {
        s_abs = s_abs + buf[i * kValSlots];
        s_sq = s_sq + buf[i * kValSlots + 1];
        const unsigned long long pk = (unsigned long long)__double_as_longlong(buf[i * kValSlots + 2]);
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] += (long long)((pk >> (16 * j)) & 0xFFFFull);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) counts[4 * b + j] = c[j];
    sums[2 * b] = s_abs;
    sums[2 * b + 1] = s_sq;
  }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace prg

using namespace prg;

// the bounds every entry shares: gridDim.y = B, and B * HW floats addressed with pixel indices that fit an int
#define PRG_CHECK_VAL_SHAPE(fn) \
  PRG_CHECK(B >= 1 && B <= 65535 && HW >= 1 && HW <= (1 << 30), fn ": B in [1, 65535], HW in [1, 2^30]")
#define PRG_CHECK_VAL_NOISE(fn)                                                                            \
  PRG_CHECK((noise != nullptr) != (seeds != nullptr), fn ": exactly one of noise and seeds");             \
  PRG_CHECK(noise || HW % 4 == 0, fn ": H*W must be a multiple of 4 with Philox noise")

extern "C" size_t prg_validate_workspace_bytes(int B, int HW) {
  if (B < 1 || B > 65535 || HW < 1 || HW > (1 << 30)) return 0;
  return (size_t)B * (size_t)val_blocks(HW) * kValSlots * sizeof(double);
}

extern "C" int prg_q_sample(const float* x0, const float* a, const float* s, const float* noise, const uint64_t* seeds,
                            uint32_t draw, int B, int HW, float* x_t, float* noise_out, void* stream) {
  PRG_CHECK(x0 && a && s && x_t, "prg_q_sample: null pointer");
  PRG_CHECK_VAL_SHAPE("prg_q_sample");
  PRG_CHECK_VAL_NOISE("prg_q_sample");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(val_blocks(HW), B, 1);
  const bool vec = HW % 4 == 0 && aligned16(x0) && aligned16(x_t) && aligned16(noise) && aligned16(noise_out);
  if (vec) q_sample_kernel<true><<<grid, kValThreads, 0, st>>>(x0, a, s, noise, seeds, draw, HW, x_t, noise_out);
  else q_sample_kernel<false><<<grid, kValThreads, 0, st>>>(x0, a, s, noise, seeds, draw, HW, x_t, noise_out);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

extern "C" int prg_diffusion_loss(const float* u, const float* x0, const float* noise, const uint64_t* seeds, uint32_t draw,
                                  const float* a, const float* s, const float* w, int objective, int loss_type, int B, int HW,
                                  void* workspace, size_t workspace_bytes, double* out, void* stream) {
  PRG_CHECK(u && x0 && a && s && w && workspace && out, "prg_diffusion_loss: null pointer");
  PRG_CHECK_VAL_SHAPE("prg_diffusion_loss");
  PRG_CHECK_VAL_NOISE("prg_diffusion_loss");
  PRG_CHECK(objective >= 0 && objective <= 2, "prg_diffusion_loss: unknown objective");
  PRG_CHECK(loss_type == 0 || loss_type == 1, "prg_diffusion_loss: unknown loss type");
  PRG_CHECK(workspace_bytes >= prg_validate_workspace_bytes(B, HW) && aligned16(workspace), "prg_diffusion_loss: workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = val_blocks(HW);
  const dim3 grid(nblk, B, 1);
  double* ws = static_cast<double*>(workspace);
  const bool vec = HW % 4 == 0 && aligned16(u) && aligned16(x0) && aligned16(noise);
  if (vec) diffusion_loss_kernel<true><<<grid, kValThreads, 0, st>>>(u, x0, noise, seeds, draw, a, s, objective, loss_type, HW, ws);
  else diffusion_loss_kernel<false><<<grid, kValThreads, 0, st>>>(u, x0, noise, seeds, draw, a, s, objective, loss_type, HW, ws);
  PRG_LAUNCH_CHECK();
  diffusion_loss_finish_kernel<<<B, kValThreads, 0, st>>>(ws, w, HW, nblk, out);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

extern "C" int prg_mask_metrics(const float* prob, const float* input, const float* label, const float* mask, float threshold,
                                float tol, int B, int HW, void* workspace, size_t workspace_bytes, int64_t* counts, double* sums,
                                void* stream) {
  PRG_CHECK(prob && input && label && workspace && counts && sums, "prg_mask_metrics: null pointer");
  PRG_CHECK_VAL_SHAPE("prg_mask_metrics");
  PRG_CHECK(workspace_bytes >= prg_validate_workspace_bytes(B, HW) && aligned16(workspace), "prg_mask_metrics: workspace too small or misaligned");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = val_blocks(HW);
  const dim3 grid(nblk, B, 1);
  double* ws = static_cast<double*>(workspace);
  const bool vec = HW % 4 == 0 && aligned16(prob) && aligned16(input) && aligned16(label) && aligned16(mask);
  if (vec) mask_metrics_kernel<true><<<grid, kValThreads, 0, st>>>(prob, input, label, mask, threshold, tol, HW, ws);
  else mask_metrics_kernel<false><<<grid, kValThreads, 0, st>>>(prob, input, label, mask, threshold, tol, HW, ws);
  PRG_LAUNCH_CHECK();
  mask_metrics_finish_kernel<<<B, kValThreads, 0, st>>>(ws, nblk, reinterpret_cast<long long*>(counts), sums);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}
