// mppi_noise.h -- the perturbation draw of the MPPI kernels (cs_rollout_mppi_costs / cs_rollout_mppi_update,
// copterstep_rollout_mppi.hip): one Philox2x32-10 call per (env, nonce, step, sample, action component) and the
// Irwin-Hall sum of its four 16-bit halves.  Plain C++ with no dependence on the device headers, so that a host program
// compiles the very same code (tests/host/mppi_noise_host.cpp prints draws; tests/mppi_ref.py restates them in NumPy,
// bit for bit: integer arithmetic and ONE float32 multiply).  DESIGN.md section 14.  Below it, the smooth noise of
// section 15: two knot draws blended per step (tests/host/mppi_smooth_host.cpp; tests/mppi_smooth_ref.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define CS_MPPI_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define CS_MPPI_FN inline
#endif

namespace cs {

// fl32(sqrt(3) 2^-16): a sum of four independent 16-bit uniforms has the variance (2^32 - 1) / 3
constexpr float kMppiNoiseScale = 0x1.bb67aep-16f;
// sample indices take 16 bits of the key (cs_rollout_mppi_io.num_samples <= CS_MPPI_MAX_SAMPLES = 65 535: the grid's y)
constexpr int kMppiSampleBits = 16;

CS_MPPI_FN uint64_t mppi_splitmix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ULL;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// The third Philox key of a seed: key_force and key_action are the halves of h = splitmix64(seed) (cs_seed); the noise
// key is the low half of splitmix64(h).
CS_MPPI_FN uint32_t mppi_noise_key(uint64_t seed) { return (uint32_t)mppi_splitmix64(mppi_splitmix64(seed)); }

// Philox2x32-10 (Salmon et al., SC'11), as dev_codec.h's
CS_MPPI_FN void mppi_philox2x32_10(uint32_t c0, uint32_t c1, uint32_t key, uint32_t& o0, uint32_t& o1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p = (unsigned long long)0xD256D193U * c0;
    c0 = (uint32_t)(p >> 32) ^ key ^ c1;
    c1 = (uint32_t)p;
    key += 0x9E3779B9U;
  }
  o0 = c0;
  o1 = c1;
}

// The Irwin-Hall draw of order 4 from the two words of one Philox call (also es_noise.h's and pf_noise.h's):
// T = the sum of the four 16-bit halves of the 64 bits minus 131 070 (an exact integer, |T| <= 131 070);
// epsilon = (float)T x kMppiNoiseScale: mean 0, variance 1 - 2^-32, support +-3.46.
CS_MPPI_FN float mppi_irwin_hall(uint32_t r0, uint32_t r1) {
  const int32_t t = (int32_t)((r0 >> 16) + (r0 & 0xFFFFu) + (r1 >> 16) + (r1 & 0xFFFFu)) - 131070;
  return (float)t * kMppiNoiseScale;
}

// epsilon of (global env id, nonce `stream`, step k = 1.., sample p, action component j): counter = (env id, stream),
// key = key_noise + (((k - 1) << 16) + p) * 4 + j (mod 2^32) -- a pure function of its arguments and the seed, the same
// whatever the batch size, the sharding, the number of samples or the launch history; distinct keys for k <= 16 384.
CS_MPPI_FN float mppi_noise(uint32_t key_noise, uint32_t env_id, uint32_t stream, uint32_t k, uint32_t p, uint32_t j) {
  uint32_t r0, r1;
  mppi_philox2x32_10(env_id, stream, key_noise + ((((k - 1u) << kMppiSampleBits) + p) * 4u + j), r0, r1);
  return mppi_irwin_hall(r0, r1);
}

// Smooth noise (cs_rollout_mppi_costs_ex / cs_rollout_mppi_update_ex, copterstep_rollout_mppi_smooth.hip; DESIGN.md
// section 15): step k reads the draws of two neighbouring knots, eps(p, knot, j) and eps(p, knot + 1, j) -- mppi_noise
// with the knot number in its step slot -- and blends them with the caller's two float32 weights of that step:
//     eps~ = fl32( fl32(w0 * e0) + fl32(w1 * e1) )
// two multiplies and one add, never fused; the second term is left out altogether when w1 == 0, so that knot = k with
// w = (1, 0) is mppi_noise(k) bit for bit (1 * e is exact).  The caller guarantees knot >= 1 and knot + 1 <= 16 384.
CS_MPPI_FN float mppi_knot_blend(float w0, float e0, float w1, float e1) {
#pragma clang fp contract(off)
  const float a = w0 * e0;
  if (w1 == 0.0f) return a;
  const float b = w1 * e1;
  return a + b;
}

CS_MPPI_FN float mppi_noise_smooth(uint32_t key_noise, uint32_t env_id, uint32_t stream, uint32_t knot, float w0,
                                   float w1, uint32_t p, uint32_t j) {
  const float e0 = mppi_noise(key_noise, env_id, stream, knot, p, j);
  if (w1 == 0.0f) return mppi_knot_blend(w0, e0, 0.0f, 0.0f);
  return mppi_knot_blend(w0, e0, w1, mppi_noise(key_noise, env_id, stream, knot + 1u, p, j));
}

}  // namespace cs
