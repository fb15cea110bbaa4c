// Counter-based Gaussian noise shared by the kernels that draw on the device (sampler.hip,
// bayes.hip): Philox4x32-10 keyed by `seed`; counter = (q_lo, q_hi, step, draw) with
// q = global_element / 4; 4 normals per counter via Box-Muller.  One definition, so every
// kernel that names the same (seed, step, draw, element) reads the same bits
// (bpk_philox_normal_f32 writes them out).  FMA contraction is off inside these functions
// whatever the including file chooses.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bpk {

__device__ inline uint4 philox4x32_10(uint4 ctr, uint2 key) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  constexpr uint32_t W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += W0;
    key.y += W1;
  }
  return ctr;
}

__device__ inline float u01(uint32_t r) {  // (0, 1]
#pragma clang fp contract(off)
  return ((float)(r >> 8) + 1.0f) * (1.0f / 16777216.0f);
}

// the 4 normals of Philox block q (global elements 4 q .. 4 q + 3)
__device__ inline void normal4(uint64_t q, int step, int draw, uint64_t seed, float out[4]) {
#pragma clang fp contract(off)
  const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)step,
                                           (uint32_t)draw),
                                make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const float two_pi = 6.283185307179586f;
  const float r0 = sqrtf(-2.0f * logf(u01(r.x)));
  const float r1 = sqrtf(-2.0f * logf(u01(r.z)));
  float s0, c0, s1, c1;
  sincosf(two_pi * u01(r.y), &s0, &c0);
  sincosf(two_pi * u01(r.w), &s1, &c1);
  out[0] = r0 * c0;
  out[1] = r0 * s0;
  out[2] = r1 * c1;
  out[3] = r1 * s1;
}

}  // namespace bpk
