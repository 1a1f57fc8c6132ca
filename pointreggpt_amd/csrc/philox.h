// philox.h — Philox4x32-10 on the device (Salmon, Moraes, Dror, Shaw, SC'11): the counter-based generator behind the sampler's
// noise and keep masks (sampler.hip) and the cloud augmentation (augment.hip).  One call turns a 4-word counter and a 64-bit
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

}  // namespace prg
