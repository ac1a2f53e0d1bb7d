// urts_cross.h -- the cross-covariance of the unscented Rauch-Tung-Striebel smoother (cs_urts_smooth,
// copterstep_urts.hip): what the smoother adds to the sigma points and moments of ukf_points.h and the solve of
// rts_solve.h.  From the 24 propagated points y1 .. y24 of a step and the factor of the covariance the points were made
// from, W = C^T = (wi * gamma) dY L^T with dY[:, c] = y(1 + c) - y(13 + c): in exact arithmetic the textbook
// C = sum_i wc_i (chi_i - xhat)(y_i - x-)^T, because chi_(1 + c) - xhat = gamma L[:, c] = -(chi_(13 + c) - xhat), point 0
// contributes nothing and x- cancels in each +- pair.  W takes the place of rts_solve.h's W = A P_f.  Plain C++ with no
// dependence on the device headers, so that a host program can compile the very same code
// (tests/host/urts_cross_host.cpp).  Every operand is addressed through a stride: element k of an array at [k * stride]
// (the device keeps them in lane-private LDS columns, stride 64; a host program contiguously, stride 1).  W [12][12] is
// rts_solve.h's: W[i][c] at [(i * 12 + c) * stride], i the component after the step, c the one before it.  DESIGN.md
// section 25.
//
// The arithmetic is fixed -- the including translation unit forbids floating-point contraction -- and tests/urts_ref.py
// restates it:
//   pairs    point 1 + c, c = 0 .. 11, stores dY[a][c] = y[a]; point 13 + c subtracts: dY[a][c] = dY[a][c] - y[a].
//   diag     L[c][c] = 1 / inv[c], one division each (ukf_point's own expression), with inv[c] rts_cholesky's diagonal.
//   scale    s = wi * gamma, one multiply.
//   row      for every row i and c = 0 .. 11:  acc = dY[i][0] * L[c][0];  acc += dY[i][j] * L[c][j] for j = 1 .. c in
//            order;  W[i][c] = s * acc.  L[c][j] = U[j][c] for j < c.  A row of W is a function of the same row of dY
//            and of the factor: the transform runs in place.
//   landed   no points were made: W[i][c] = P[i][c], the symmetric matrix itself (the step is the identity).
#pragma once

#include "ekf_update.h"
#include "ukf_points.h"

namespace cs {

// Propagated point p = 1 .. 24 (y [12] contiguous) into dY, kept in W's rows.
CS_EKF_FN void urts_cross_add(int p, const double* y, double* W, int stride) {
  const int c = (p - 1) % 12;
  const bool minus = p > 12;
#pragma unroll
  for (int a = 0; a < 12; ++a) {
    double* const e = W + (a * 12 + c) * stride;
    *e = minus ? *e - y[a] : y[a];
  }
}

// The diagonal of L, diag [12] contiguous, from U [78] = rts_cholesky's factor (strided).
CS_EKF_FN void urts_cross_diag(const double* U, int stride, double* diag) {
#pragma unroll
  for (int c = 0; c < 12; ++c) diag[c] = 1.0 / U[(c * (c + 1) / 2 + c) * stride];
}

// The scale of the transform.
CS_EKF_FN double urts_cross_scale(const UkfWeights& w) { return w.wi * w.gamma; }

// Row i of dY -> row i of W, in place: row points at W[i][0].
CS_EKF_FN void urts_cross_row(double* row, const double* U, const double* diag, double s, int stride) {
  double d[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) d[j] = row[j * stride];
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    double acc = d[0] * (c == 0 ? diag[0] : U[(c * (c + 1) / 2) * stride]);
#pragma unroll
    for (int j = 1; j <= c; ++j) acc += d[j] * (j == c ? diag[c] : U[(c * (c + 1) / 2 + j) * stride]);
    row[c * stride] = s * acc;
  }
}

// A LANDED row: W <- P [78] packed (strided), the full symmetric matrix.
CS_EKF_FN void urts_cross_landed(const double* P, double* W, int stride) {
#pragma clang loop unroll(disable)
  for (int i = 0; i < 12; ++i) {
#pragma unroll
    for (int c = 0; c < 12; ++c) W[(i * 12 + c) * stride] = P[ekf_sym_at(i, c) * stride];
  }
}

}  // namespace cs
