// urts_cross_host.cpp -- one backward step of cs_urts_smooth (gym_copter_amd/csrc/urts_cross.h, with the points and the
// moments of ukf_points.h and the algebra of rts_solve.h) on the host, in the kernel's order:
//   urts_cross_host  gamma wm0 wc0 wi  landed  xf0 .. xf11  xpred0 .. xpred11  xs0 .. xs11  then three row-major 12 x 12
//                    matrices of 144 values each: Pf (the upper triangle is factored; whole columns enter Ps), Q and the
//                    smoothed covariance of the row above (the upper triangle is read), then 25 x 12 values y: the
//                    propagated points, whatever map made them (ignored with landed = 1)
// factors Pf, takes the moments of y and W = (wi gamma) dY L^T (landed: W = Pf, P- = Pf + Q), then D = Ps' - P-, the
// factor of P-, G = P-^-1 W, xs = xf + G^T (xs' - xpred), Ps = Pf + G^T D G; prints "ok <0|1> <0|1>" (the two
// factorisations), then the 144 values of W row-major, the 78 of P- packed (column-major: (i, j), i <= j, at
// j (j + 1) / 2 + i), the 144 of G, the 12 of xs and the 78 of Ps packed, as hexadecimal floats (exact).
// tests/test_urts_cpu.py runs it: tests/urts_ref.py must reproduce every value bit for bit, and the kernel's non-positive
// pivot paths are this code.
#include <cstdio>
#include <cstdlib>

#include "urts_cross.h"

int main(int argc, char** argv) {
  if (argc != 1 + 4 + 1 + 36 + 3 * 144 + cs::kUkfPoints * 12) {
    fprintf(stderr, "usage: urts_cross_host gamma wm0 wc0 wi landed <12 xf> <12 xpred> <12 xs'> <144 Pf> <144 Q> <144 Ps'> <300 y>\n");
    return 2;
  }
  char** v = argv + 1;
  const cs::UkfWeights w{strtod(v[0], nullptr), strtod(v[1], nullptr), strtod(v[2], nullptr), strtod(v[3], nullptr)};
  const bool landed = atoi(v[4]) != 0;
  v += 5;
  double xf[12], dx[12], xs[12], U[cs::kEkfSym], S[cs::kEkfSym], D[cs::kEkfSym], Pf[144], Q[144], W[144], Y0[12], sy[12];
  for (int j = 0; j < 12; ++j) xf[j] = strtod(v[j], nullptr);
  for (int j = 0; j < 12; ++j) dx[j] = strtod(v[24 + j], nullptr) - strtod(v[12 + j], nullptr);
  v += 36;
  for (int j = 0; j < 144; ++j) {
    Pf[j] = strtod(v[j], nullptr);
    Q[j] = strtod(v[144 + j], nullptr);
  }
  for (int j = 0; j < 12; ++j)
    for (int i = 0; i <= j; ++i) {
      U[j * (j + 1) / 2 + i] = Pf[i * 12 + j];
      D[j * (j + 1) / 2 + i] = strtod(v[288 + i * 12 + j], nullptr);
    }
  v += 432;
  bool ok_f = true;
  if (landed) {
    cs::urts_cross_landed(U, W, 1);
    for (int e = 0; e < cs::kEkfSym; ++e) S[e] = U[e];
    cs::ukf_landed(S, Q, 1);
  } else {
    ok_f = cs::rts_cholesky(U, 1);
    for (int p = 0; p < cs::kUkfPoints; ++p) {
      double y[12];
      for (int j = 0; j < 12; ++j) y[j] = strtod(v[p * 12 + j], nullptr);
      if (p == 0) {
        cs::ukf_moments_begin(y, Y0, sy, S, 1);
      } else {
        cs::ukf_moments_add(y, Y0, sy, S, 1);
        cs::urts_cross_add(p, y, W, 1);
      }
    }
    cs::ukf_moments_finish(w, Y0, sy, S, Q, Y0, S, 1);
    double diag[12];
    cs::urts_cross_diag(U, 1, diag);
    const double s = cs::urts_cross_scale(w);
    for (int a = 0; a < 12; ++a) cs::urts_cross_row(W + a * 12, U, diag, s, 1);
  }
  printf("ok %d", ok_f ? 1 : 0);
  double Wout[144], Pm[cs::kEkfSym];
  for (int j = 0; j < 144; ++j) Wout[j] = W[j];
  for (int e = 0; e < cs::kEkfSym; ++e) Pm[e] = S[e];
  for (int e = 0; e < cs::kEkfSym; ++e) D[e] -= S[e];
  const bool ok_s = cs::rts_cholesky(S, 1);
  printf(" %d\n", ok_s ? 1 : 0);
  for (int c = 0; c < 12; ++c) cs::rts_solve_column(S, W, c, 1);
  cs::rts_mean(W, 1, xf, dx, xs);
  for (int c = 0; c < 12; ++c) cs::rts_ps_column(D, W, c, 1, Pf + c, S);
  for (int j = 0; j < 144; ++j) printf("%a\n", Wout[j]);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", Pm[j]);
  for (int j = 0; j < 144; ++j) printf("%a\n", W[j]);
  for (int j = 0; j < 12; ++j) printf("%a\n", xs[j]);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", S[j]);
  return 0;
}
