// philox.h — Philox4x32-10 on the device (Salmon, Moraes, Dror, Shaw, SC'11): the counter-based generator behind the sampler's
// noise and keep masks (sampler.hip), the validation path's forward process (validate.hip) and the cloud augmentation (augment.hip).  One call turns a 4-word counter and a 64-bit
// key (k0 = low word, k1 = high word) into four 32-bit words; what the words become is the caller's contract (include/prg.h).
// The streams of one key are kept apart by the third counter word, a tag of four ASCII bytes.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace prg {

__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}
__device__ inline void philox4x32_10(uint32_t (&c)[4], uint64_t key) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// Four standard normals for (key, draw index, pixel quad) of the stream `tag` (the third counter word): two Box-Muller pairs.
// The sampler's noise (sampler.hip, tag PHILOX_DOMAIN_NORMAL) and the forward process of the validation path (validate.hip,
// PHILOX_DOMAIN_VALIDATE): the same arithmetic, streams kept apart by the tag alone.
__device__ inline float4 philox_normal4(uint64_t key, uint32_t draw, uint32_t quad, uint32_t tag) {
  uint32_t c[4] = {quad, draw, tag, 0u};
  philox4x32_10(c, key);
  const float k = 2.3283064365386963e-10f;  // 2^-32
  const float u0 = ((float)c[0] + 0.5f) * k, u1 = ((float)c[1] + 0.5f) * k;
  const float u2 = ((float)c[2] + 0.5f) * k, u3 = ((float)c[3] + 0.5f) * k;
  const float r0 = sqrtf(-2.0f * logf(fminf(fmaxf(u0, 1e-12f), 1.0f)));
  const float r1 = sqrtf(-2.0f * logf(fminf(fmaxf(u2, 1e-12f), 1.0f)));
  float s0, c0, s1, c1;
  sincosf(6.283185307179586f * u1, &s0, &c0);
  sincosf(6.283185307179586f * u3, &s1, &c1);
  return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

}  // namespace prg
