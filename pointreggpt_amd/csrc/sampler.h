// sampler.h — the per-transition elementwise update of the DDNM / DDIM samplers and the on-device noise.
#pragma once
#include "common.h"

namespace prg {

// third Philox counter word: the normals use 0x70726721, the keep-mask uniforms "keep", the noise of the validation path's
// forward process (validate.hip) "vald": a validation run with a generation run's seeds shares no draw with its chains
constexpr uint32_t PHILOX_DOMAIN_NORMAL = 0x70726721u;
constexpr uint32_t PHILOX_DOMAIN_KEEP = 0x6B656570u;
constexpr uint32_t PHILOX_DOMAIN_VALIDATE = 0x76616C64u;

// What every instantiation of sampler_step_kernel receives.  The objective-0 instantiations receive this part ALONE: their kernel
// arguments, and with them their code, are what they were before the objectives existed.
struct SamplerStepCore {
  float* x;                 // state (B, HW), updated in place
  const float* u;           // U-Net output (B, HW)
  const float* cond;        // (B, 2, HW) in [-1,1] or null
  const float* noise;       // stored draws (n_steps + 1, B, HW) or null -> Philox
  const prg_step* steps;    // device copy of the transition table
  int* step_idx;            // device step counter: read by every workgroup, advanced by the last one to finish
  int* ticket;              // arrival counter of the workgroups of one launch (self-resetting)
  const uint64_t* seeds;    // device (B,) Philox keys (used when noise == null)
  float* final_out;         // (B, HW): written on the last transition as (x + 1) / 2
  const float* keep_p;      // device (n_steps,) DDNM keep thresholds or null: row k with keep_p[k] >= 0 replaces a known pixel
                            // iff its uniform > keep_p[k]; < 0 (and null): every known pixel, nothing drawn
  const float* keep_u;      // stored uniforms (n_steps, B, HW), slab k feeds transition k, or null -> Philox (DOMAIN_KEEP)
  int B, HW, n_steps;
};

// The launch arguments: the core and what the network's output means.
struct SamplerStepArgs : SamplerStepCore {
  int objective;            // what u is: 0 = x0 (pred_x0), 1 = the noise (pred_noise), 2 = v (pred_v); prg_sampler_set_objective
  const float* obj_p;       // device (n_steps,) coefficients of x0r = obj_p[k] * x - obj_q[k] * u; read iff objective != 0
  const float* obj_q;
};

int launch_sampler_step(const SamplerStepArgs& a, hipStream_t s);
// x = start image: noise slab 0, or Philox draw 0
int launch_sampler_init(float* x, const float* noise, const uint64_t* seeds, int B, int HW, hipStream_t s);

}  // namespace prg
