// lqr_solve.h -- the A x A solve of the iLQR backward pass (cs_rollout_lqr, copterstep_rollout_lqr.hip): an unrolled
// Cholesky factorisation and its two triangular solves, all in registers (A = the task's action width: 1, 2 or 4).
// Plain C++ with no dependence on the device headers, so that a host program can compile the very same code
// (tests/host/lqr_chol_host.cpp: the not-positive-definite path is tested there, not by feeding the kernel an invalid R).
// The arithmetic is fixed -- subtractions in index order, one division per element, IEEE sqrt; the including translation
// unit forbids floating-point contraction -- and tests/lqr_ref.py restates it operation for operation.  DESIGN.md
// section 13.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define CS_LQR_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define CS_LQR_FN inline
#endif

namespace cs {

// m (row-major, its LOWER triangle read) -> its Cholesky factor L in the lower triangle, in place: m = L L^T.  Returns
// false if a pivot was <= 0 or not finite (NaN included); the factorisation is carried through regardless, so the
// caller's results are then whatever the arithmetic gives (NaN after the sqrt of a negative pivot).
template <int A>
CS_LQR_FN bool lqr_cholesky(double (&m)[A * A]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < A; ++j) {
    double p = m[j * A + j];
#pragma unroll
    for (int k = 0; k < j; ++k) p -= m[j * A + k] * m[j * A + k];
    ok = ok && p > 0.0 && p <= 1.7976931348623157e308;
    const double l = sqrt(p);
    m[j * A + j] = l;
#pragma unroll
    for (int i = j + 1; i < A; ++i) {
      double t = m[i * A + j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= m[i * A + k] * m[j * A + k];
      m[i * A + j] = t / l;
    }
  }
  return ok;
}

// b <- (L L^T)^-1 b: the forward substitution, then the backward one
template <int A>
CS_LQR_FN void lqr_solve(const double (&l)[A * A], double (&b)[A]) {
#pragma unroll
  for (int i = 0; i < A; ++i) {
    double t = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= l[i * A + k] * b[k];
    b[i] = t / l[i * A + i];
  }
#pragma unroll
  for (int i = A - 1; i >= 0; --i) {
    double t = b[i];
#pragma unroll
    for (int k = i + 1; k < A; ++k) t -= l[k * A + i] * b[k];
    b[i] = t / l[i * A + i];
  }
}

}  // namespace cs
