// ekf_update_host.cpp -- the scalar measurement update of cs_rollout_ekf (gym_copter_amd/csrc/ekf_update.h) on the host:
//   ekf_update_host M x0 .. x11 P00 P01 .. (144 row-major values, the upper triangle is read)
//                   then M times: h0 .. h11 r z        (z = nan: no measurement)
// prints "ok <0|1>", then nis, loglik, the 12 values of the mean and the 78 of the packed upper triangle (column-major:
// (i, j), i <= j, at j (j + 1) / 2 + i) as hexadecimal floats (exact).  tests/test_rollout_ekf_cpu.py runs it: the kernel's
// s <= 0 and skipped-measurement paths are this code.
#include <cstdio>
#include <cstdlib>

#include "ekf_update.h"

int main(int argc, char** argv) {
  const int m = argc > 1 ? atoi(argv[1]) : 0;
  if (m < 1 || m > 12 || argc != 2 + 12 + 144 + m * 14) {
    fprintf(stderr, "usage: ekf_update_host M <12 mean values> <144 covariance values> M x <12 h values, r, z>\n");
    return 2;
  }
  char** v = argv + 2;
  double x[12], P[cs::kEkfSym];
  for (int j = 0; j < 12; ++j) x[j] = strtod(v[j], nullptr);
  v += 12;
  for (int j = 0; j < 12; ++j)
    for (int i = 0; i <= j; ++i) P[j * (j + 1) / 2 + i] = strtod(v[i * 12 + j], nullptr);
  v += 144;
  cs::EkfStats st{0.0, 0.0, true};
  for (int k = 0; k < m; ++k, v += 14) {
    double h[12];
    for (int j = 0; j < 12; ++j) h[j] = strtod(v[j], nullptr);
    cs::ekf_scalar_update(x, P, 1, h, strtod(v[12], nullptr), strtod(v[13], nullptr), st);
  }
  printf("ok %d\n", st.ok ? 1 : 0);
  printf("%a\n%a\n", st.nis, st.loglik);
  for (int j = 0; j < 12; ++j) printf("%a\n", x[j]);
  for (int j = 0; j < cs::kEkfSym; ++j) printf("%a\n", P[j]);
  return 0;
}
