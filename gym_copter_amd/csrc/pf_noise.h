// pf_noise.h -- the draws of the bootstrap particle filter (cs_rollout_pf, copterstep_rollout_pf.hip): one
// Philox2x32-10 call per (env, nonce, step, particle, state component), the Irwin-Hall sum of its four 16-bit halves
// (mppi_noise.h's draw, so that NumPy reproduces every particle bit for bit), the lower-triangular colouring in float64,
// and the step's resampling word.  Plain C++ with no dependence on the device headers, so that a host program compiles
// the very same code (tests/host/pf_noise_host.cpp prints draws; tests/pf_ref.py restates them in NumPy: integer
// arithmetic, ONE float32 multiply, and float64 multiplies and adds that are never fused).  DESIGN.md section 21.
#pragma once

#include "mppi_noise.h"

namespace cs {

constexpr int kPfParticleBits = 10;  // particle indices take 10 bits of the key (CS_PF_MAX_PARTICLES = 1 024)
constexpr int kPfSlotBits = 4;       // 16 slots per (step, particle): 0 .. 11 the state components, 12 the resampling word
constexpr uint32_t kPfResampleSlot = 12u;

// The sixth Philox key of a seed: key_force and key_action are the halves of h = splitmix64(seed) (cs_seed), the MPPI
// key is the low half of splitmix64(h), the ES key that of the third splitmix64 of the seed, the policy-noise key that
// of the fourth; the particle filter's is the low half of the fifth.
CS_MPPI_FN uint32_t pf_noise_key(uint64_t seed) {
  return (uint32_t)mppi_splitmix64(mppi_splitmix64(mppi_splitmix64(mppi_splitmix64(mppi_splitmix64(seed)))));
}

// The two Philox words of (global env id g, nonce, step k, particle p, slot j): counter = (g, nonce),
// key = key_pf + ((k * 1024 + p) * 16 + j) (mod 2^32) -- a pure function of its arguments and the seed, the same whatever
// the number of particles, the batch size, the sharding or the chunking.  k = 0 is the Gaussian start, k >= 1 the global
// index of a step; keys are distinct for k < 2^18.
CS_MPPI_FN void pf_words(uint32_t key_pf, uint32_t g, uint32_t nonce, uint32_t k, uint32_t p, uint32_t j, uint32_t& r0,
                         uint32_t& r1) {
  mppi_philox2x32_10(g, nonce, key_pf + ((((k << kPfParticleBits) + p) << kPfSlotBits) + j), r0, r1);
}

// epsilon of state component j = 0 .. 11: mppi_noise's Irwin-Hall draw of order 4 (mppi_irwin_hall: mean 0, variance
// 1 - 2^-32, support +-3.46).
CS_MPPI_FN float pf_noise(uint32_t key_pf, uint32_t g, uint32_t nonce, uint32_t k, uint32_t p, uint32_t j) {
  uint32_t r0, r1;
  pf_words(key_pf, g, nonce, k, p, j, r0, r1);
  return mppi_irwin_hall(r0, r1);
}

// u of step k >= 1: the top 16 bits of the first word of slot 12 at particle 0 -- the offset of the systematic
// resampling comb, in units of 2^-16 of a tooth.
CS_MPPI_FN uint32_t pf_resample_u(uint32_t key_pf, uint32_t g, uint32_t nonce, uint32_t k) {
  uint32_t r0, r1;
  pf_words(key_pf, g, nonce, k, 0u, kPfResampleSlot, r0, r1);
  return r0 >> 16;
}

// Row i of w = L eps with L [12,12] lower triangular (row-major at stride `stride` between consecutive entries):
// sum_{j <= i} L[i][j] (double)eps[j], j ascending, one multiply and one add per term, never fused; the first term starts
// the sum.
CS_MPPI_FN double pf_colour(const double* L, int stride, int i, const float (&eps)[12]) {
#pragma clang fp contract(off)
  double acc = L[(i * 12) * stride] * (double)eps[0];
  for (int j = 1; j <= i; ++j) {
    const double t = L[(i * 12 + j) * stride] * (double)eps[j];
    acc = acc + t;
  }
  return acc;
}

}  // namespace cs
