// rts_solve_host.cpp -- the dense algebra of cs_rollout_rts (gym_copter_amd/csrc/rts_solve.h) on the host:
//   rts_solve_host  xf0 .. xf11  dx0 .. dx11  then four row-major 12 x 12 matrices of 144 values each:
//                   P- (the upper triangle is read), W, D (the upper triangle is read), Pf
// runs one backward step -- factor P-, G = P-^-1 W, xs = xf + G^T dx, Ps = Pf + G^T D G -- and prints "ok <0|1>", then the
// 78 values of the factor (packed upper triangle, column-major: (i, j), i <= j, at j (j + 1) / 2 + i; the diagonal holds
// the reciprocal pivots' roots), the 144 of G row-major, the 12 of xs and the 78 of Ps packed, as hexadecimal floats
// (exact).  tests/test_rollout_rts_cpu.py runs it: the kernel's non-positive and non-finite pivot paths are this code.
#include <cstdio>
#include <cstdlib>

#include "rts_solve.h"

int main(int argc, char** argv) {
  if (argc != 1 + 24 + 4 * 144) {
    fprintf(stderr, "usage: rts_solve_host <12 xf> <12 dx> <144 P-> <144 W> <144 D> <144 Pf>\n");
    return 2;
  }
  char** v = argv + 1;
  double xf[12], dx[12], xs[12], U[cs::kEkfSym], D[cs::kEkfSym], Ps[cs::kEkfSym], W[144], Pf[144];
  for (int j = 0; j < 12; ++j) xf[j] = strtod(v[j], nullptr);
  for (int j = 0; j < 12; ++j) dx[j] = strtod(v[12 + j], nullptr);
  v += 24;
  for (int j = 0; j < 12; ++j)
    for (int i = 0; i <= j; ++i) {
      U[j * (j + 1) / 2 + i] = strtod(v[i * 12 + j], nullptr);
      D[j * (j + 1) / 2 + i] = strtod(v[288 + i * 12 + j], nullptr);
    }
  for (int j = 0; j < 144; ++j) {
    W[j] = strtod(v[144 + j], nullptr);
    Pf[j] = strtod(v[432 + j], nullptr);
  }
  const bool ok = cs::rts_cholesky(U, 1);
  for (int c = 0; c < 12; ++c) cs::rts_solve_column(U, W, c, 1);
  cs::rts_mean(W, 1, xf, dx, xs);
  for (int c = 0; c < 12; ++c) cs::rts_ps_column(D, W, c, 1, Pf + c, Ps);
  printf("ok %d\n", ok ? 1 : 0);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", U[j]);
  for (int j = 0; j < 144; ++j) printf("%a\n", W[j]);
  for (int j = 0; j < 12; ++j) printf("%a\n", xs[j]);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", Ps[j]);
  return 0;
}
