// es_noise.h -- the perturbation draw of the evolution-strategies entry points (cs_es_perturb / cs_es_gradient,
// copterstep_rollout_es.hip): one Philox2x32-10 call per (pair, nonce, parameter) and the Irwin-Hall sum of its four
// 16-bit halves, mppi_noise.h's construction under a key of its own.  Plain C++ with no dependence on the device
// headers, so that a host program compiles the very same code (tests/host/es_noise_host.cpp prints draws;
// tests/es_ref.py restates them in NumPy, bit for bit: integer arithmetic and ONE float32 multiply).  DESIGN.md
// section 16.
#pragma once

#include "mppi_noise.h"

namespace cs {

// The fourth Philox key of a seed: key_force and key_action are the halves of h = splitmix64(seed) (cs_seed), the MPPI
// noise key is the low half of splitmix64(h); the ES key is the low half of splitmix64(splitmix64(h)).
CS_MPPI_FN uint32_t es_noise_key(uint64_t seed) {
  return (uint32_t)mppi_splitmix64(mppi_splitmix64(mppi_splitmix64(seed)));
}

// epsilon of (global pair index, nonce `stream`, parameter index p): counter = (pair, stream), key = key_es + p (mod
// 2^32) -- a pure function of its arguments and the seed, the same whatever the population size, the number of
// parameters, the split of the population over calls (pair_base) or the launch history.  The pair index and the nonce
// are full 32-bit numbers (the index wraps at 2^32); keys are distinct for p < 2^32.  The value is mppi_noise's
// (mppi_irwin_hall): Irwin-Hall of order 4, mean 0, variance 1 - 2^-32, support +-3.46.
CS_MPPI_FN float es_noise(uint32_t key_es, uint32_t pair, uint32_t stream, uint32_t p) {
  uint32_t r0, r1;
  mppi_philox2x32_10(pair, stream, key_es + p, r0, r1);
  return mppi_irwin_hall(r0, r1);
}

}  // namespace cs
