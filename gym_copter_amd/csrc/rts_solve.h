// rts_solve.h -- the dense algebra of the Rauch-Tung-Striebel smoother (cs_rollout_rts, copterstep_rollout_rts.hip): the
// Cholesky factorisation of a 12 x 12 prior covariance, the two substitutions that give a column of G = P-^-1 W, the
// smoothed mean and one column of the smoothed covariance.  Plain C++ with no dependence on the device headers, so that
// a host program can compile the very same code (tests/host/rts_solve_host.cpp: the positive definite path, a
// non-positive pivot and a non-finite pivot are tested there).  Every operand is addressed through a stride: element k
// of an array at [k * stride] (the device keeps them in lane-private LDS columns, stride 64; a host program
// contiguously, stride 1).  Symmetric matrices are ekf_update.h's packed upper triangle.  DESIGN.md section 20.
//
// The arithmetic is fixed -- the including translation unit forbids floating-point contraction -- and tests/rts_ref.py
// restates it:
//   factor   P- = U^T U, U upper triangular (U^T is the L of P- = L L^T), in place, column j = 0 .. 11 of the packed
//            triangle in order.  For i = 0 .. j-1:  s = P[i][j];  s -= U[k][i] * U[k][j] for k = 0 .. i-1 in order;
//            U[i][j] = s * inv[i].  Then the pivot d = P[j][j];  d -= U[k][j] * U[k][j] for k = 0 .. j-1 in order;
//            inv[j] = 1 / sqrt(d), kept in the diagonal's slot (the substitutions multiply by it; U[j][j] itself is
//            needed nowhere else).  A pivot that is <= 0 or not finite (NaN included) clears ok; the arithmetic is
//            carried through regardless (lqr_cholesky's rule), so the results are then whatever it gives.
//   solve    a column w of W, in place:  forward  y[i] = (w[i] - sum_{k<i} U[k][i] * y[k]) * inv[i] for i = 0 .. 11,
//            backward  g[i] = (y[i] - sum_{k>i} U[i][k] * g[k]) * inv[i] for i = 11 .. 0; each sum is subtracted term by
//            term in increasing k from the left-hand value.
//   mean     xs[i] = xf[i] + sum_r G[r][i] * dx[r]; the sum in increasing r from its first term, then one add.
//   column   t[r] = sum_k D[r][k] * G[k][c] for r = 0 .. 11, then for i = 0 .. c
//            Ps[i][c] = Pf[i][c] + sum_r G[r][i] * t[r]; both sums in increasing index from their first term.
#pragma once

#include <cmath>

#include "ekf_update.h"

namespace cs {

// P- [78] packed -> U with the reciprocal pivots on the diagonal, in place.  Returns false if a pivot was <= 0 or not
// finite.
CS_EKF_FN bool rts_cholesky(double* P, int stride) {
  bool ok = true;
#pragma clang loop unroll(disable)
  for (int j = 0; j < 12; ++j) {
    double* const col = P + (j * (j + 1) / 2) * stride;
#pragma clang loop unroll(disable)
    for (int i = 0; i < j; ++i) {
      const double* const ci = P + (i * (i + 1) / 2) * stride;
      double s = col[i * stride];
#pragma clang loop unroll(disable)
      for (int k = 0; k < i; ++k) s -= ci[k * stride] * col[k * stride];
      col[i * stride] = s * ci[i * stride];
    }
    double d = col[j * stride];
#pragma clang loop unroll(disable)
    for (int k = 0; k < j; ++k) d -= col[k * stride] * col[k * stride];
    ok = ok && d > 0.0 && d <= 1.7976931348623157e308;
    col[j * stride] = 1.0 / sqrt(d);
  }
  return ok;
}

// Column c of W [12][12] (W[i][c] at [(i * 12 + c) * stride]) -> that column of G = P-^-1 W, in place; U is
// rts_cholesky's.
CS_EKF_FN void rts_solve_column(const double* U, double* W, int c, int stride) {
  double y[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    double s = W[(i * 12 + c) * stride];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= U[(i * (i + 1) / 2 + k) * stride] * y[k];
    y[i] = s * U[(i * (i + 1) / 2 + i) * stride];
  }
#pragma unroll
  for (int i = 11; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 12; ++k) s -= U[(k * (k + 1) / 2 + i) * stride] * y[k];
    y[i] = s * U[(i * (i + 1) / 2 + i) * stride];
    W[(i * 12 + c) * stride] = y[i];
  }
}

// The smoothed mean: xs [12] (strided) = xf + G^T dx, with xf and dx [12] contiguous.
CS_EKF_FN void rts_mean(const double* G, int stride, const double* xf, const double* dx, double* xs) {
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    double acc = G[i * stride] * dx[0];
#pragma unroll
    for (int r = 1; r < 12; ++r) acc += G[(r * 12 + i) * stride] * dx[r];
    xs[i * stride] = xf[i] + acc;
  }
}

// Column c of the smoothed covariance above its diagonal: Ps[i][c] = Pf[i][c] + (G^T D G)[i][c] for i <= c, into the
// packed triangle Ps (strided).  D [78] packed and G [12][12] are strided; pf_col points at Pf[0][c] of a row-major
// 12 x 12 matrix in the caller's memory (Pf[i][c] at pf_col[i * 12]; the whole column is read).
CS_EKF_FN void rts_ps_column(const double* D, const double* G, int c, int stride, const double* pf_col, double* Ps) {
  double g[12], t[12], pf[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) pf[k] = pf_col[k * 12];  // (all twelve at once: they come from the caller's memory)
#pragma unroll
  for (int k = 0; k < 12; ++k) g[k] = G[(k * 12 + c) * stride];
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    double acc = D[ekf_sym_at(r, 0) * stride] * g[0];
#pragma unroll
    for (int k = 1; k < 12; ++k) acc += D[ekf_sym_at(r, k) * stride] * g[k];
    t[r] = acc;
  }
  double* const col = Ps + (c * (c + 1) / 2) * stride;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    if (i <= c) {
      double acc = G[i * stride] * t[0];
#pragma unroll
      for (int r = 1; r < 12; ++r) acc += G[(r * 12 + i) * stride] * t[r];
      col[i * stride] = pf[i] + acc;
    }
  }
}

}  // namespace cs
