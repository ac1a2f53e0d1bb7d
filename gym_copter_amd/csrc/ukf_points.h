// ukf_points.h -- the sigma points and the weighted moments of the unscented Kalman filter (cs_rollout_ukf,
// copterstep_rollout_ukf.hip): the 2 * 12 + 1 = 25 points of a mean and the Cholesky factor of its covariance, and the
// mean and covariance of the 25 propagated points.  Plain C++ with no dependence on the device headers, so that a host
// program can compile the very same code (tests/host/ukf_points_host.cpp: the positive definite path and a non-positive
// pivot are tested there).  Every operand the filter keeps is addressed through a stride: element k of an array at
// [k * stride] (the device keeps them in lane-private LDS columns, stride 64; a host program contiguously, stride 1).
// Symmetric matrices are ekf_update.h's packed upper triangle; the factor is rts_solve.h's rts_cholesky.  DESIGN.md
// section 23.
//
// The arithmetic is fixed -- the including translation unit forbids floating-point contraction -- and tests/ukf_ref.py
// restates it:
//   factor   P = L L^T with L = U^T, U rts_cholesky's (its diagonal slots hold inv[j] = 1 / sqrt(pivot j)): for a > j
//            L[a][j] = U[j][a]; L[j][j] = 1 / inv[j] (one division); L[a][j] = 0 for a < j.
//   points   point 0 = x; for j = 0 .. 11 and a >= j: point (1 + j)[a] = x[a] + gamma * L[a][j] and
//            point (13 + j)[a] = x[a] - gamma * L[a][j] (one multiply, then one add or one subtract); for a < j both
//            are x[a] itself.  The column order and the lower factor are part of the filter: another root, another filter.
//   moments  one pass about y0, the propagated point 0, over the propagated points y1 .. y24 in this order:
//            sy[a] = (..((0 + y1[a]) + y2[a]) + ..) + y24[a];  d_i[a] = y_i[a] - y0[a];
//            S[a][c] = (..((0 + d_1[a] * d_1[c]) + d_2[a] * d_2[c]) + ..) + d_24[a] * d_24[c] for a <= c.  Then
//            x-[a] = wm0 * y0[a] + wi * sy[a];   m[a] = x-[a] - y0[a];   c2 = 2 - (wc0 + 24 * wi);
//            P-[a][c] = (wi * S[a][c] - c2 * (m[a] * m[c])) + Q[a][c] for a <= c: Q last, with one add per entry.
//            For weights whose mean set sums to one (wm0 + 24 wi = 1) this is, in exact arithmetic,
//            wc0 d0 d0^T + wi sum_i di di^T + Q with di = y_i - x-: it needs neither stored points nor a second pass.
//   landed   no points: P- [a][c] = P[a][c] + Q[a][c], one add per entry; the mean is kept.
#pragma once

#include <cmath>

#include "ekf_update.h"
#include "rts_solve.h"

namespace cs {

constexpr int kUkfPoints = 25;  // 2 * 12 + 1

// What the caller's (alpha, beta, kappa) come to: the points' spread and the three distinct weights.
struct UkfWeights {
  double gamma;  // sqrt(12 + lambda)
  double wm0;    // the centre point's weight in the mean
  double wc0;    // ... and in the covariance
  double wi;     // every other point's weight, in both
};

// Point p of the 25 -> out [12] contiguous, from the mean x [12] (strided) and U [78] = rts_cholesky's factor of its
// covariance (strided).
CS_EKF_FN void ukf_point(int p, const double* x, const double* U, int stride, double gamma, double* out) {
  const int j = p == 0 ? 12 : (p - 1) % 12;  // (p = 0: no column, every a < j)
  const bool minus = p > 12;
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    const double xa = x[a * stride];
    if (a < j) {
      out[a] = xa;
    } else {
      const double u = U[(a * (a + 1) / 2 + j) * stride];
      const double t = gamma * (a == j ? 1.0 / u : u);
      out[a] = minus ? xa - t : xa + t;
    }
  }
}

// The moments' start: y0 [12] contiguous, the propagated point 0, is kept (Y0 [12], strided) and the sums cleared
// (sy [12] contiguous, S [78] strided).
CS_EKF_FN void ukf_moments_begin(const double* y0, double* Y0, double* sy, double* S, int stride) {
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    Y0[a * stride] = y0[a];
    sy[a] = 0.0;
  }
#pragma clang loop unroll(disable)
  for (int e = 0; e < kEkfSym; ++e) S[e * stride] = 0.0;
}

// One propagated point y [12] contiguous (points 1 .. 24 in order) into the sums.
CS_EKF_FN void ukf_moments_add(const double* y, const double* Y0, double* sy, double* S, int stride) {
  double d[12];
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    d[a] = y[a] - Y0[a * stride];
    sy[a] += y[a];
  }
#pragma unroll
  for (int c = 0; c < 12; ++c) {
#pragma unroll
    for (int a = 0; a <= c; ++a) S[(c * (c + 1) / 2 + a) * stride] += d[a] * d[c];
  }
}

// The prior: x [12] (strided) <- x-, T [78] (strided) <- P-, from the sums; Q [12][12] row-major contiguous (its upper
// triangle is read).
CS_EKF_FN void ukf_moments_finish(const UkfWeights& w, const double* Y0, const double* sy, const double* S,
                                  const double* Q, double* x, double* T, int stride) {
  double m[12];
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    const double y0 = Y0[a * stride];
    const double xm = w.wm0 * y0 + w.wi * sy[a];
    x[a * stride] = xm;
    m[a] = xm - y0;
  }
  const double c2 = 2.0 - (w.wc0 + 24.0 * w.wi);
#pragma unroll
  for (int c = 0; c < 12; ++c) {
#pragma unroll
    for (int a = 0; a <= c; ++a) {
      const int e = c * (c + 1) / 2 + a;
      T[e * stride] = (w.wi * S[e * stride] - c2 * (m[a] * m[c])) + Q[a * 12 + c];
    }
  }
}

// A LANDED mean's prior covariance, in place: T [78] (strided) <- P + Q.
CS_EKF_FN void ukf_landed(double* T, const double* Q, int stride) {
#pragma unroll
  for (int c = 0; c < 12; ++c) {
#pragma unroll
    for (int a = 0; a <= c; ++a) T[(c * (c + 1) / 2 + a) * stride] += Q[a * 12 + c];
  }
}

}  // namespace cs
