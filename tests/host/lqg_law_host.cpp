// lqg_law_host.cpp -- the feedback law and the measurement formation of cs_rollout_lqg (gym_copter_amd/csrc/lqg_law.h)
// on the host:
//   lqg_law_host A M  xhat0 .. xhat11  xbar0 .. xbar11  x0 .. x11
//                     then A times: abar g0 .. g11        (one motor's nominal action and gain row)
//                     then M times: h0 .. h11 e           (e = nan: no measurement)
// prints the A actions (float32) and the M measurements (float64) as hexadecimal floats (exact), one per line.
// tests/test_rollout_lqg_cpu.py runs it: tests/lqg_ref.py must reproduce every value bit for bit.
#include <cstdio>
#include <cstdlib>

#include "lqg_law.h"

int main(int argc, char** argv) {
  const int a = argc > 1 ? atoi(argv[1]) : 0;
  const int m = argc > 2 ? atoi(argv[2]) : 0;
  if (a < 1 || a > 4 || m < 1 || m > 12 || argc != 3 + 36 + a * 13 + m * 13) {
    fprintf(stderr, "usage: lqg_law_host A M <12 xhat> <12 xbar> <12 x> A x <abar, 12 gains> M x <12 h values, e>\n");
    return 2;
  }
  char** v = argv + 3;
  double xhat[12], xbar[12], x[12];
  for (int j = 0; j < 12; ++j) xhat[j] = strtod(v[j], nullptr);
  for (int j = 0; j < 12; ++j) xbar[j] = strtod(v[12 + j], nullptr);
  for (int j = 0; j < 12; ++j) x[j] = strtod(v[24 + j], nullptr);
  v += 36;
  double dx[12];
  cs::lqg_deviation(xhat, 1, xbar, 1, dx);
  for (int c = 0; c < a; ++c, v += 13) {
    double g[12];
    for (int j = 0; j < 12; ++j) g[j] = strtod(v[1 + j], nullptr);
    printf("%a\n", (double)cs::lqg_law(strtof(v[0], nullptr), g, 1, dx));
  }
  for (int i = 0; i < m; ++i, v += 13) {
    double h[12];
    for (int j = 0; j < 12; ++j) h[j] = strtod(v[j], nullptr);
    printf("%a\n", cs::lqg_measure(h, x, 1, strtod(v[12], nullptr)));
  }
  return 0;
}
