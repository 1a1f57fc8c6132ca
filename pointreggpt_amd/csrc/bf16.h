// bf16.h — the bf16 storage type and its conversions, for device code (through common.h) and for the host-only weight
// preparation (weights_host.h), which is compiled as plain C++ without the HIP runtime.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PRG_HOST_DEVICE __host__ __device__
#else
#define PRG_HOST_DEVICE
#endif

namespace prg {

// ---------------------------------------------------------------------------------------------
// bf16 storage type (raw 16 bits; conversions round-to-nearest-even, NaN preserved)
// ---------------------------------------------------------------------------------------------
struct bf16_t {
  uint16_t v;
};

PRG_HOST_DEVICE inline float bf16_to_f32(bf16_t b) {
  union {
    uint32_t u;
    float f;
  } x;
  x.u = ((uint32_t)b.v) << 16;
  return x.f;
}

PRG_HOST_DEVICE inline bf16_t f32_to_bf16(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  // gfx950 has a native round-to-nearest-even conversion (v_cvt_pk_bf16_f32)
  bf16_t r;
  r.v = __builtin_bit_cast(uint16_t, (__bf16)f);
  return r;
#else
  union {
    uint32_t u;
    float f;
  } x;
  x.f = f;
  bf16_t r;
  if ((x.u & 0x7fffffffu) > 0x7f800000u) {  // NaN
    r.v = (uint16_t)((x.u >> 16) | 0x40);
    return r;
  }
  uint32_t lsb = (x.u >> 16) & 1u;
  x.u += 0x7fffu + lsb;
  r.v = (uint16_t)(x.u >> 16);
  return r;
#endif
}

}  // namespace prg
