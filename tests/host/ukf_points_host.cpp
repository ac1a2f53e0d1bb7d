// ukf_points_host.cpp -- the sigma points and the weighted moments of cs_rollout_ukf (gym_copter_amd/csrc/ukf_points.h,
// with the factorisation of rts_solve.h) on the host:
//   ukf_points_host  gamma wm0 wc0 wi  x0 .. x11  then two row-major 12 x 12 matrices of 144 values each: P (the upper
//                    triangle is read) and Q, then 25 x 12 values y: the propagated points, whatever map made them
// factors P, forms the 25 points, takes the moments of y, and the LANDED prior P + Q; prints "ok <0|1>", then the 78
// values of the factor (packed upper triangle, column-major; the diagonal holds the reciprocal pivots' roots), the
// 25 x 12 of the points, the 12 of x-, the 78 of P- packed and the 78 of P + Q packed, as hexadecimal floats (exact).
// tests/test_rollout_ukf_cpu.py runs it: tests/ukf_ref.py must reproduce every value bit for bit, and the kernel's
// non-positive pivot path is this code.
#include <cstdio>
#include <cstdlib>

#include "ukf_points.h"

int main(int argc, char** argv) {
  if (argc != 1 + 4 + 12 + 2 * 144 + cs::kUkfPoints * 12) {
    fprintf(stderr, "usage: ukf_points_host gamma wm0 wc0 wi <12 x> <144 P> <144 Q> <300 y>\n");
    return 2;
  }
  char** v = argv + 1;
  const cs::UkfWeights w{strtod(v[0], nullptr), strtod(v[1], nullptr), strtod(v[2], nullptr), strtod(v[3], nullptr)};
  v += 4;
  double x[12], P[cs::kEkfSym], U[cs::kEkfSym], S[cs::kEkfSym], Q[144], Y0[12], sy[12], xm[12];
  for (int j = 0; j < 12; ++j) x[j] = strtod(v[j], nullptr);
  v += 12;
  for (int j = 0; j < 12; ++j)
    for (int i = 0; i <= j; ++i) P[j * (j + 1) / 2 + i] = U[j * (j + 1) / 2 + i] = strtod(v[i * 12 + j], nullptr);
  for (int j = 0; j < 144; ++j) Q[j] = strtod(v[144 + j], nullptr);
  v += 288;
  const bool ok = cs::rts_cholesky(U, 1);
  printf("ok %d\n", ok ? 1 : 0);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", U[j]);
  for (int p = 0; p < cs::kUkfPoints; ++p) {
    double pt[12];
    cs::ukf_point(p, x, U, 1, w.gamma, pt);
    for (int j = 0; j < 12; ++j) printf("%a\n", pt[j]);
  }
  for (int p = 0; p < cs::kUkfPoints; ++p) {
    double y[12];
    for (int j = 0; j < 12; ++j) y[j] = strtod(v[p * 12 + j], nullptr);
    if (p == 0)
      cs::ukf_moments_begin(y, Y0, sy, S, 1);
    else
      cs::ukf_moments_add(y, Y0, sy, S, 1);
  }
  for (int j = 0; j < 12; ++j) xm[j] = x[j];
  double T[cs::kEkfSym];
  cs::ukf_moments_finish(w, Y0, sy, S, Q, xm, T, 1);
  for (int j = 0; j < 12; ++j) printf("%a\n", xm[j]);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", T[j]);
  cs::ukf_landed(P, Q, 1);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", P[j]);
  return 0;
}
