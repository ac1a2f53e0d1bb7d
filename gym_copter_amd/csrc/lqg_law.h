// lqg_law.h -- the two small formulas of the output-feedback rollout (cs_rollout_lqg, copterstep_rollout_lqg.hip) that
// are neither the truth's step nor the filter's: the affine feedback law at the filter's estimate, and the formation of
// the measurement from the true state and the caller's noise.  Plain C++ with no dependence on the device headers, so
// that a host program can compile the very same code (tests/host/lqg_law_host.cpp).  The arithmetic is fixed -- terms in
// index order, one operation at a time; the including translation unit forbids floating-point contraction -- and
// tests/lqg_ref.py restates it.  DESIGN.md section 22.
#pragma once

#if defined(__HIPCC__)
#define CS_LQG_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define CS_LQG_FN inline
#endif

namespace cs {

// The deviation the law acts on: dx[j] = xhat[j] - xbar[j], element j of xhat at [j * xhat_stride] (the device keeps the
// estimate in a lane-private LDS column, a host program contiguously) and of xbar at [j * xbar_stride].
CS_LQG_FN void lqg_deviation(const double* xhat, int xhat_stride, const double* xbar, int xbar_stride, double (&dx)[12]) {
#pragma unroll
  for (int j = 0; j < 12; ++j) dx[j] = xhat[j * xhat_stride] - xbar[j * xbar_stride];
}

// One motor's law: fl32(abar + sum_j gain[j] dx[j]), from (double) abar, j ascending, one multiply and one add per term,
// one rounding to float32 (cs_rollout_feedback_states' arithmetic without its alpha d term).
CS_LQG_FN float lqg_law(float abar, const double* gain, int gain_stride, const double (&dx)[12]) {
  double t = (double)abar;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    const double p = gain[j * gain_stride] * dx[j];
    t = t + p;
  }
  return (float)t;
}

// One measurement: z = sum_j h[j] x[j] + e, the first product starting the sum, j ascending, one multiply and one add
// per term, then the noise.  A NaN e ("no measurement") gives a NaN z.
CS_LQG_FN double lqg_measure(const double* h, const double* x, int x_stride, double e) {
  double acc = h[0] * x[0];
#pragma unroll
  for (int j = 1; j < 12; ++j) {
    const double p = h[j] * x[j * x_stride];
    acc = acc + p;
  }
  return acc + e;
}

}  // namespace cs
