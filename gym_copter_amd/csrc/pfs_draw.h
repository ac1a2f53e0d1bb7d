// pfs_draw.h -- the draws and the whitening of the backward-simulation particle smoother (cs_pf_smooth,
// copterstep_pf_smooth.hip): a path's uniform from slot 13 of the particle filter's Philox keys (pf_noise.h: slots 0 .. 11
// are the state components, 12 the resampling word), the inverse-CDF rule on integer weights in exact 64-bit integer
// arithmetic, and the product with the inverse noise factor in pf_colour's order.  Plain C++ with no dependence on the
// device headers, so that a host program compiles the very same code (tests/host/pfs_draw_host.cpp prints draws;
// tests/pf_smooth_ref.py restates them in NumPy).  DESIGN.md section 27.
#pragma once

#include "pf_noise.h"

namespace cs {

constexpr uint32_t kPfsDrawSlot = 13u;  // the slot of a path's backward draw: the key's particle field holds the path
constexpr int kPfsDrawBits = 24;        // u is the top 24 bits of the first word: the resolution of the integer weights
static_assert(kPfsDrawSlot < (1u << kPfSlotBits) && kPfsDrawSlot != kPfResampleSlot, "a free slot of the filter's keys");

// u of (global env id g, nonce, global row kg, path m): a pure function of its arguments and the seed -- the same
// whatever the number of paths or particles, the batch size, the sharding or the chunking.  m < 1 024 (the key's particle
// field).
CS_MPPI_FN unsigned long long pfs_draw_u(uint32_t key_pf, uint32_t g, uint32_t nonce, uint32_t kg, uint32_t m) {
  uint32_t r0, r1;
  pf_words(key_pf, g, nonce, kg, m, kPfsDrawSlot, r0, r1);
  return (unsigned long long)(r0 >> (32 - kPfsDrawBits));
}

// The test of the inverse-CDF rule: with C the inclusive cumulative sum of the integer weights and S1 = C[P-1], the drawn
// index is the smallest p with pfs_draw_passes(C[p], u, S1).  Weights are <= 2^24 and P <= 1 024, so S1 <= 2^34 and both
// sides are below 2^58.  C[P-1] passes for every u < 2^24 as long as S1 > 0.
CS_MPPI_FN bool pfs_draw_passes(unsigned long long c, unsigned long long u, unsigned long long s1) {
  return (c << kPfsDrawBits) > u * s1;
}

// The rule itself, one weight at a time (the kernel makes the same search over a wavefront's scan): P - 1 if no index
// passes (every weight 0).
CS_MPPI_FN int pfs_draw_index(const uint32_t* w, int P, unsigned long long u) {
  unsigned long long s1 = 0;
  for (int p = 0; p < P; ++p) s1 += w[p];
  unsigned long long c = 0;
  for (int p = 0; p < P; ++p) {
    c += w[p];
    if (pfs_draw_passes(c, u, s1)) return p;
  }
  return P - 1;
}

// Row r of y = Linv x with Linv [12,12] lower triangular (row-major at stride `stride` between consecutive entries):
// sum_{j <= r} Linv[r][j] x[j], j ascending, one multiply and one add per term, never fused; the first term starts the
// sum (pf_colour's order).
CS_MPPI_FN double pfs_whiten(const double* Linv, int stride, int r, const double (&x)[12]) {
#pragma clang fp contract(off)
  double acc = Linv[(r * 12) * stride] * x[0];
  for (int j = 1; j <= r; ++j) {
    const double t = Linv[(r * 12 + j) * stride] * x[j];
    acc = acc + t;
  }
  return acc;
}

}  // namespace cs
