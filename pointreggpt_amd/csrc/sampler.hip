// sampler.hip — one fused elementwise kernel per denoising transition (HBM-bound: 20-24 B/pixel/step):
// x0 from the network output, DDNM known-pixel replacement, clamp, posterior / DDIM combination, noise.
// Built with -ffp-contract=off: the float ops are in the reference's order (sd:1158-1162, 1173-1180, 1210-1218,
// 1250-1251, 1280, 1369-1373) so that, given identical network outputs and noise, the state is bit-identical.
#include "sampler.h"
#include "philox.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace prg {

// ---- noise from Philox4x32-10 (philox.h): key = per-scene seed, counter = (pixel quad, draw index, stream tag) ----
// the normals are philox_normal4 (philox.h) under the sampler's own tag, PHILOX_DOMAIN_NORMAL

// four uniforms in [0,1) on the 2^-24 grid (torch's float32 uniform_ grid, 0 included) for the DDNM keep mask of (scene key,
// draw index, pixel quad): word i >> 8, exactly representable, serves pixel 4 * quad + i.  The third counter word separates
// this stream from the normals' of the same (key, draw, quad).
__device__ inline float4 philox_keep4(uint64_t key, uint32_t draw, uint32_t quad) {
  uint32_t c[4] = {quad, draw, PHILOX_DOMAIN_KEEP, 0u};
  philox4x32_10(c, key);
  const float k = 5.9604644775390625e-08f;  // 2^-24
  return make_float4((float)(c[0] >> 8) * k, (float)(c[1] >> 8) * k, (float)(c[2] >> 8) * k, (float)(c[3] >> 8) * k);
}

// torch.clamp: NaN stays NaN (fminf / fmaxf would return the bound and hide a non-finite network output as depth 0)
__device__ inline float clamp1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// x0 before any clamp, from the network output u.  OBJ = 0: u itself; otherwise p * x - q * u with -ffp-contract=off: two rounded
// products, one subtraction, like torch's three ops (sd:1153-1156, 1169-1171).  (A function named at every use, not a local
// variable: with OBJ = 0 each use is then the plain us[e] it was, and hipcc emits the instruction stream it emitted before.)
template <int OBJ>
__device__ __forceinline__ float x0_raw(float p, float q, float x, float u) {
  if constexpr (OBJ == 0) return u;
  else return p * x - q * u;
}

// One transition on image b.  DROP (stochastic DDNM, sd:1213-1216 / 1223-1225): a known pixel is replaced iff its uniform > keep_p
// (float32 comparison, like torch's of a float32 tensor with a 0-dim float64 one).  DROP = false is the kernel as it was before the
// keep mask existed: same instructions, same data.  OBJ (prg_sampler_set_objective): what the network predicts.  0 = x0 itself, and
// again the kernel as it was: obj_p / obj_q are dead there, no table is read and no branch is taken per pixel.  1 (pred_noise,
// sd:1194-1197) and 2 (pred_v, sd:1204-1208): x0 before the clamp is x0_raw above; with OBJ = 1 the noise estimate is u itself,
// never re-derived from the clamped x0 (sd:1195).
template <bool DROP, int OBJ>
__device__ inline void sampler_step_image(const SamplerStepCore& a, const prg_step& st, int k, int b, bool last, float keep_p,
                                          float obj_p, float obj_q, int q0, int q_stride) {
  const size_t img = (size_t)b * a.HW;
  for (int q = q0; q * 4 < a.HW; q += q_stride) {
    const size_t o = img + (size_t)q * 4;
    const float4 xv = *reinterpret_cast<const float4*>(a.x + o);
    const float4 uv = *reinterpret_cast<const float4*>(a.u + o);
    float4 cd = make_float4(0, 0, 0, 0), cm = make_float4(-1, -1, -1, -1), nz = make_float4(0, 0, 0, 0);
    if (a.cond) {
      cd = *reinterpret_cast<const float4*>(a.cond + (size_t)b * 2 * a.HW + (size_t)q * 4);
      cm = *reinterpret_cast<const float4*>(a.cond + (size_t)b * 2 * a.HW + a.HW + (size_t)q * 4);
    }
    if (st.sigma != 0.0f) {
      if (a.noise)
        nz = *reinterpret_cast<const float4*>(a.noise + ((size_t)(k + 1) * a.B + b) * a.HW + (size_t)q * 4);
      else
        nz = philox_normal4(a.seeds[b], (uint32_t)(k + 1), (uint32_t)q, PHILOX_DOMAIN_NORMAL);
    }
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, us[4] = {uv.x, uv.y, uv.z, uv.w};
    const float cds[4] = {cd.x, cd.y, cd.z, cd.w}, cms[4] = {cm.x, cm.y, cm.z, cm.w};
    const float nzs[4] = {nz.x, nz.y, nz.z, nz.w};
    bool kept[4] = {true, true, true, true};
    if (DROP) {
      float4 ku;
      if (a.keep_u)
        ku = *reinterpret_cast<const float4*>(a.keep_u + ((size_t)k * a.B + b) * a.HW + (size_t)q * 4);
      else
        ku = philox_keep4(a.seeds[b], (uint32_t)(k + 1), (uint32_t)q);
      kept[0] = ku.x > keep_p; kept[1] = ku.y > keep_p; kept[2] = ku.z > keep_p; kept[3] = ku.w > keep_p;
    }
    float r[4], f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float x0p = (st.clip_pred & 1) ? clamp1(x0_raw<OBJ>(obj_p, obj_q, xs[e], us[e])) : x0_raw<OBJ>(obj_p, obj_q, xs[e], us[e]);
      const bool known = a.cond && ((cms[e] + 1.0f) * 0.5f > 0.5f);  // get_mask_from_img_cond (sd:507-508)
      float x0 = (DROP ? known && kept[e] : known) ? cds[e] : x0p;   // keep_mask & mask_rpj (sd:1216): a dropped pixel stays in-painted
      if (st.clip_pred & 2) x0 = clamp1(x0);   // p_mean_variance clip_denoised (sd:1250); ddim_sample has no such clamp
      float v = st.c_x0 * x0;
      if (st.clip_pred & 4) {
        // refine row (has_refine_step, sd:1307-1314 / 1374-1388): evaluation without the replacement; only the KNOWN
        // pixels take the clamped x0 of the network output (posterior mean at t = 0 is exactly x0: coef1 = 1, coef2 = 0)
        r[e] = known ? clamp1(x0_raw<OBJ>(obj_p, obj_q, xs[e], us[e])) : xs[e];
        f[e] = (r[e] + 1.0f) * 0.5f;
        continue;
      }
      if (st.c_x != 0.0f) v = v + st.c_x * xs[e];
      if (st.c_eps != 0.0f) {
        const float eps = OBJ == 1 ? us[e] : (st.sqrt_recip * xs[e] - x0p) / st.sqrt_recipm1;
        v = v + st.c_eps * eps;
      }
      if (st.sigma != 0.0f) v = v + st.sigma * nzs[e];
      r[e] = v;
      f[e] = (v + 1.0f) * 0.5f;
    }
    *reinterpret_cast<float4*>(a.x + o) = make_float4(r[0], r[1], r[2], r[3]);
    if (last) *reinterpret_cast<float4*>(a.final_out + o) = make_float4(f[0], f[1], f[2], f[3]);
  }
}

// OBJ = 0 takes the core of the arguments alone (sampler.h): same kernel arguments, same instructions as before the objectives existed
template <int OBJ>
using StepKernelArgs = std::conditional_t<OBJ == 0, SamplerStepCore, SamplerStepArgs>;

// grid (chunks, B); each thread handles 4 consecutive pixels.  KEEP = false (no keep table: the host chooses it, launch_sampler_step) is
// the kernel as it was before the keep mask existed; KEEP = true reads the row's threshold.  OBJ != 0 reads the row's (p, q) the
// same way: once per launch, uniform.
template <bool KEEP, int OBJ>
__global__ __launch_bounds__(256) void sampler_step_kernel(StepKernelArgs<OBJ> a) {
  const int k = *a.step_idx;
  const prg_step st = a.steps[k];
  const int b = blockIdx.y;
  const bool last = k == a.n_steps - 1;
  // The row decides whether a keep mask is drawn, so the branch is uniform across the launch.  No table, a negative threshold,
  // no condition, or the refine row (which ignores the table): every known pixel is replaced and nothing is drawn.
  const float keep_p = KEEP ? a.keep_p[k] : -1.0f;
  float obj_p = 0.0f, obj_q = 0.0f;
  if constexpr (OBJ != 0) { obj_p = a.obj_p[k]; obj_q = a.obj_q[k]; }
  // (the grid-stride bounds are taken here: read in the kernel itself, blockDim folds to the launch bound's uniform group size;
  // read inside a device function it is the generic form, one more dependent load at the head of every launch)
  const int q0 = blockIdx.x * blockDim.x + threadIdx.x, q_stride = gridDim.x * blockDim.x;
  if (KEEP && keep_p >= 0.0f && a.cond && !(st.clip_pred & 4))
    sampler_step_image<true, OBJ>(a, st, k, b, last, keep_p, obj_p, obj_q, q0, q_stride);
  else
    sampler_step_image<false, OBJ>(a, st, k, b, last, keep_p, obj_p, obj_q, q0, q_stride);
  // Every workgroup read the step counter at its first instruction; the last one to arrive here advances it for the
  // next launch and re-arms the ticket (kernel boundaries order this against the neighbouring launches).
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nwg = gridDim.x * gridDim.y;
    if (atomicAdd(a.ticket, 1) == nwg - 1) {
      *a.ticket = 0;
      *a.step_idx = k + 1;
    }
  }
}

__global__ void sampler_init_kernel(float* __restrict__ x, const float* __restrict__ noise,
                                    const uint64_t* __restrict__ seeds, int HW) {
  const int b = blockIdx.y;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q * 4 < HW; q += gridDim.x * blockDim.x) {
    const size_t o = (size_t)b * HW + (size_t)q * 4;
    float4 v;
    if (noise)
      v = *reinterpret_cast<const float4*>(noise + o);
    else
      v = philox_normal4(seeds[b], 0u, (uint32_t)q, PHILOX_DOMAIN_NORMAL);
    *reinterpret_cast<float4*>(x + o) = v;
  }
}

static inline dim3 step_grid(int HW, int B) {
  // about one workgroup per CU: the last-arriver ticket of sampler_step_kernel is one atomic per workgroup on a single
  // address (~12 ns each, serialised): 1024 workgroups cost more than the launch the ticket saves
  int gx = ceil_div(HW / 4, 256);
  const int cap = 256 / B > 1 ? 256 / B : 1;
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  return dim3(gx, B, 1);
}

template <int OBJ>
static void launch_step_objective(const SamplerStepArgs& a, hipStream_t s) {
  if (a.keep_p)
    sampler_step_kernel<true, OBJ><<<step_grid(a.HW, a.B), 256, 0, s>>>(a);
  else
    sampler_step_kernel<false, OBJ><<<step_grid(a.HW, a.B), 256, 0, s>>>(a);
}

int launch_sampler_step(const SamplerStepArgs& a, hipStream_t s) {
  PRG_CHECK(a.HW % 4 == 0, "sampler: H*W must be a multiple of 4");
  PRG_CHECK(a.objective >= 0 && a.objective <= 2, "sampler: unknown objective");
  PRG_CHECK(a.objective == 0 || (a.obj_p && a.obj_q), "sampler: this objective needs its (p, q) table");
  // the instantiation is the host's choice: one objective per launch, nothing for the kernel to branch on
  if (a.objective == 1) launch_step_objective<1>(a, s);
  else if (a.objective == 2) launch_step_objective<2>(a, s);
  else launch_step_objective<0>(a, s);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}
int launch_sampler_init(float* x, const float* noise, const uint64_t* seeds, int B, int HW, hipStream_t s) {
  PRG_CHECK(HW % 4 == 0, "sampler: H*W must be a multiple of 4");
  sampler_init_kernel<<<step_grid(HW, B), 256, 0, s>>>(x, noise, seeds, HW);
  PRG_LAUNCH_CHECK();
  return PRG_OK;
}

}  // namespace prg

using namespace prg;

// has_keep: the launches also get a table of `reps` + 1 copies of keep_p (and keep_u); without it the table pointer is null.
// objective != 0: and tables of as many copies of (obj_p, obj_q).
static int debug_sampler_step(float* x, const float* u, const float* img_cond, const uint64_t* seeds, const prg_step* step, bool has_keep,
                              float keep_p, const float* keep_u, int objective, float obj_p, float obj_q, int B, int HW, int reps,
                              float* avg_us, void* stream) {
  PRG_CHECK(x && u && seeds && step && B > 0 && HW > 0 && HW % 4 == 0 && reps > 0, "prg_debug_sampler_step: bad argument");
  PRG_CHECK(objective >= 0 && objective <= 2, "prg_debug_sampler_step: unknown objective");
  hipStream_t s = (hipStream_t)stream;
  // a table of `reps` copies of the transition (+1 row so that no launch is the chain's last), the device step counter and the ticket
  std::vector<prg_step> rows((size_t)reps + 1, *step);
  std::vector<float> keep(has_keep ? rows.size() : 0, keep_p);
  std::vector<float> obj(objective ? 2 * rows.size() : 0, obj_p);   // [p copies | q copies], behind the keep table
  std::fill(obj.begin() + obj.size() / 2, obj.end(), obj_q);
  char* scratch = nullptr;
  const size_t tab = sizeof(prg_step) * rows.size();
  const size_t obj_off = tab + 2 * sizeof(int) + sizeof(float) * keep.size();
  PRG_HIP(hipMalloc(&scratch, obj_off + sizeof(float) * obj.size()));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = PRG_OK;
  auto fail = [&](hipError_t e) { if (e != hipSuccess && rc == PRG_OK) { set_error(std::string("prg_debug_sampler_step: ") + hipGetErrorString(e)); rc = PRG_E_HIP; } };
  fail(hipMemcpyAsync(scratch, rows.data(), tab, hipMemcpyHostToDevice, s));
  fail(hipMemsetAsync(scratch + tab, 0, 2 * sizeof(int), s));
  if (has_keep) fail(hipMemcpyAsync(scratch + tab + 2 * sizeof(int), keep.data(), sizeof(float) * keep.size(), hipMemcpyHostToDevice, s));
  if (objective) fail(hipMemcpyAsync(scratch + obj_off, obj.data(), sizeof(float) * obj.size(), hipMemcpyHostToDevice, s));
  fail(hipEventCreate(&e0));
  fail(hipEventCreate(&e1));
  if (rc == PRG_OK) {
    SamplerStepArgs a{};
    a.x = x; a.u = u; a.cond = img_cond; a.noise = nullptr; a.steps = reinterpret_cast<const prg_step*>(scratch);
    a.step_idx = reinterpret_cast<int*>(scratch + tab); a.ticket = a.step_idx + 1; a.seeds = seeds; a.final_out = x;
    a.B = B; a.HW = HW; a.n_steps = reps + 1;
    if (has_keep) { a.keep_p = reinterpret_cast<const float*>(scratch + tab + 2 * sizeof(int)); a.keep_u = keep_u; }
    if (objective) {
      a.objective = objective;
      a.obj_p = reinterpret_cast<const float*>(scratch + obj_off);
      a.obj_q = a.obj_p + rows.size();
    }
    fail(hipEventRecord(e0, s));
    for (int i = 0; i < reps && rc == PRG_OK; ++i) rc = launch_sampler_step(a, s);
    fail(hipEventRecord(e1, s));
    fail(hipStreamSynchronize(s));
    float ms = 0.0f;
    if (rc == PRG_OK) fail(hipEventElapsedTime(&ms, e0, e1));
    if (avg_us) *avg_us = ms * 1e3f / (float)reps;
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(scratch);
  return rc;
}

extern "C" int prg_debug_sampler_step(float* x, const float* u, const float* img_cond, const uint64_t* seeds, const prg_step* step, int B,
                                      int HW, int reps, float* avg_us, void* stream) {
  return debug_sampler_step(x, u, img_cond, seeds, step, false, -1.0f, nullptr, 0, 0.0f, 0.0f, B, HW, reps, avg_us, stream);
}

extern "C" int prg_debug_sampler_step_keep(float* x, const float* u, const float* img_cond, const uint64_t* seeds, const prg_step* step,
                                           float keep_p, const float* keep_u, int B, int HW, int reps, float* avg_us, void* stream) {
  return debug_sampler_step(x, u, img_cond, seeds, step, true, keep_p, keep_u, 0, 0.0f, 0.0f, B, HW, reps, avg_us, stream);
}

extern "C" int prg_debug_sampler_step_objective(float* x, const float* u, const float* img_cond, const uint64_t* seeds, const prg_step* step,
                                                int objective, float p, float q, float keep_p, const float* keep_u, int B, int HW,
                                                int reps, float* avg_us, void* stream) {
  return debug_sampler_step(x, u, img_cond, seeds, step, true, keep_p, keep_u, objective, p, q, B, HW, reps, avg_us, stream);
}
