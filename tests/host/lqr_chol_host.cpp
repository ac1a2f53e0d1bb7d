// lqr_chol_host.cpp -- the A x A Cholesky and solve of cs_rollout_lqr (gym_copter_amd/csrc/lqr_solve.h) on the host:
//   lqr_chol_host A m00 m01 ... (A*A row-major values) b0 ... (A values)
// prints "ok <0|1>", then the factor's A*A values and the solution's A values as hexadecimal floats (exact).
// tests/test_gpu_rollout_lqr.py runs it on crafted matrices: the kernel's not-positive-definite path is this code.
#include <cstdio>
#include <cstdlib>

#include "lqr_solve.h"

template <int A>
static int run(char** v) {
  double m[A * A], b[A];
  for (int j = 0; j < A * A; ++j) m[j] = strtod(v[j], nullptr);
  for (int j = 0; j < A; ++j) b[j] = strtod(v[A * A + j], nullptr);
  const bool ok = cs::lqr_cholesky<A>(m);
  cs::lqr_solve<A>(m, b);
  printf("ok %d\n", ok ? 1 : 0);
  for (int j = 0; j < A * A; ++j) printf("%a\n", m[j]);
  for (int j = 0; j < A; ++j) printf("%a\n", b[j]);
  return 0;
}

int main(int argc, char** argv) {
  const int a = argc > 1 ? atoi(argv[1]) : 0;
  if ((a != 1 && a != 2 && a != 4) || argc != 2 + a * a + a) {
    fprintf(stderr, "usage: lqr_chol_host A <A*A matrix values> <A right-hand side values>\n");
    return 2;
  }
  return a == 1 ? run<1>(argv + 2) : a == 2 ? run<2>(argv + 2) : run<4>(argv + 2);
}
