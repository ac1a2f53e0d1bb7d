// ekf_update.h -- the measurement update of the extended Kalman filter (cs_rollout_ekf, copterstep_rollout_ekf.hip): one
// scalar measurement z = h^T x + e, e ~ N(0, r), applied to a 12-state mean and the packed upper triangle of its
// covariance.  Plain C++ with no dependence on the device headers, so that a host program can compile the very same code
// (tests/host/ekf_update_host.cpp: the s <= 0, NaN-z and M = 12 paths are tested there).  The arithmetic is fixed -- sums
// in index order from their first term, one division per gain entry; the including translation unit forbids
// floating-point contraction -- and tests/ekf_ref.py restates it.  DESIGN.md section 19.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define CS_EKF_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define CS_EKF_FN inline
#endif

namespace cs {

// the packed upper triangle, column-major: (i, j) = (j, i), i <= j, at j (j + 1) / 2 + i (78 entries for 12 states)
constexpr int kEkfSym = 78;
CS_EKF_FN int ekf_sym_at(int i, int j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }

// What a filter accumulates over its updates.
struct EkfStats {
  double nis;     // the sum of nu^2 / s over the updates of a step
  double loglik;  // the sum of -1/2 (nu^2 / s + ln(2 pi s))
  bool ok;        // every s so far was finite and > 0
};

// One scalar update: x [12] and P [78] with element k at [k * stride] (the device keeps them in lane-private LDS columns,
// a host program contiguously), h [12] contiguous.  A NaN z is "no measurement": nothing changes.  With p = P h,
// s = h^T p + r, nu = z - h^T x, g = p / s:  x <- x + g nu,  P <- P - g p^T (upper triangle).  A non-finite or non-positive
// s clears st.ok; the update is carried through regardless.
CS_EKF_FN void ekf_scalar_update(double* x, double* P, int stride, const double* h, double r, double z, EkfStats& st) {
  if (z != z) return;
  double hv[12], p[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) hv[j] = h[j];
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    double acc = P[ekf_sym_at(a, 0) * stride] * hv[0];
#pragma unroll
    for (int b = 1; b < 12; ++b) acc += P[ekf_sym_at(a, b) * stride] * hv[b];
    p[a] = acc;
  }
  double hp = hv[0] * p[0], hx = hv[0] * x[0];
#pragma unroll
  for (int a = 1; a < 12; ++a) {
    hp += hv[a] * p[a];
    hx += hv[a] * x[a * stride];
  }
  const double s = hp + r;
  const double nu = z - hx;
  st.ok = st.ok && s > 0.0 && s <= 1.7976931348623157e308;
  double g[12];
#pragma unroll
  for (int a = 0; a < 12; ++a) g[a] = p[a] / s;
#pragma unroll
  for (int a = 0; a < 12; ++a) x[a * stride] += g[a] * nu;
#pragma unroll
  for (int j = 0; j < 12; ++j) {
#pragma unroll
    for (int i = 0; i <= j; ++i) P[(j * (j + 1) / 2 + i) * stride] -= g[i] * p[j];
  }
  const double e = (nu * nu) / s;
  st.nis += e;
  st.loglik -= 0.5 * (e + log(6.283185307179586 * s));
}

}  // namespace cs
