// ppo_noise.h -- the action noise of the actor-critic collection kernel (cs_rollout_actor_critic,
// copterstep_rollout_ac.hip): one Philox2x32-10 call per (env, nonce, step, pair of action components) and the
// Box-Muller transform of its two words, in float32.  Plain C++ with no dependence on the device headers, so that a host
// program compiles the very same code (tests/host/ppo_noise_host.cpp prints draws; tests/ppo_ref.py restates them in
// NumPy).  DESIGN.md section 17.
//
// What is reproducible where: the two uniforms u1, u2 are integer arithmetic and two float32 operations each -- NumPy
// gives the same bits.  epsilon itself goes through logf, sqrtf, cosf and sinf, which are the math library's of whoever
// compiles this header: the device library's in the kernel, the host's libm in the host program.  Both are accurate to
// a few float32 ulp, neither is correctly rounded, so epsilon is reproducible only to that accuracy (measured: DESIGN.md
// section 17).  A true Gaussian, not the Irwin-Hall sum of mppi_noise.h / es_noise.h: the learner's score function
// assumes one, and a draw of bounded support biases it.
#pragma once

#include <math.h>

#include "mppi_noise.h"

namespace cs {

// The fifth Philox key of a seed: key_force and key_action are the halves of h = splitmix64(seed) (cs_seed), the MPPI
// noise key is the low half of splitmix64(h), the ES key that of splitmix64(splitmix64(h)); the policy-noise key is the
// low half of splitmix64(splitmix64(splitmix64(h))).
CS_MPPI_FN uint32_t ppo_noise_key(uint64_t seed) {
  return (uint32_t)mppi_splitmix64(mppi_splitmix64(mppi_splitmix64(mppi_splitmix64(seed))));
}

constexpr float kPpoTwoPi = 0x1.921fb6p+2f;  // fl32(2 pi)

// The two uniforms of (global env id g, nonce, step k = 1.., pair = c >> 1 of the action component c): counter =
// (g, nonce), key = key_pi + 2 k + pair (mod 2^32) -- a pure function of its arguments and the seed, the same whatever
// the batch size, the sharding, the number of steps of a call or the launch history; g and the nonce are full 32-bit
// numbers, keys are distinct for pair <= 1 (A <= 4) and k < 2^31.  With m1, m2 the top 24 bits of the two output words:
//     u1 = fl32( fl32((float)m1 + 0.5f) * 2^-24 )   in (0, 1]   (m1 + 0.5 is rounded to 24 bits for m1 >= 2^23: to even)
//     u2 = (float)m2 * 2^-24                        in [0, 1)   (exact)
CS_MPPI_FN void ppo_noise_uniforms(uint32_t key_pi, uint32_t g, uint32_t nonce, uint32_t k, uint32_t pair, float& u1,
                                   float& u2) {
#pragma clang fp contract(off)
  uint32_t r0, r1;
  mppi_philox2x32_10(g, nonce, key_pi + 2u * k + pair, r0, r1);
  const float m1 = (float)(r0 >> 8) + 0.5f;
  u1 = m1 * 0x1p-24f;
  u2 = (float)(r1 >> 8) * 0x1p-24f;
}

// Box-Muller in float32: R = sqrtf(-2 logf(u1)), t = fl32(2 pi) u2, eps_even = R cosf(t), eps_odd = R sinf(t): the two
// standard normals of the components 2 pair and 2 pair + 1.  |eps| <= sqrt(2 ln 2^25) = 5.89.
CS_MPPI_FN void ppo_noise_pair(uint32_t key_pi, uint32_t g, uint32_t nonce, uint32_t k, uint32_t pair, float& e_even,
                               float& e_odd) {
#pragma clang fp contract(off)
  float u1, u2;
  ppo_noise_uniforms(key_pi, g, nonce, k, pair, u1, u2);
  const float l = logf(u1);
  const float r = sqrtf(-2.0f * l);
  const float t = kPpoTwoPi * u2;
  e_even = r * cosf(t);
  e_odd = r * sinf(t);
}

}  // namespace cs
