// boxqp_host.cpp -- the box-constrained QP of cs_ilqr_box_backward (gym_copter_amd/csrc/boxqp_solve.h) on the host:
//   boxqp_host [file]      (no file: standard input)
// Each input line is one problem, values separated by blanks and read by strtod (decimal, hexadecimal, inf, nan):
//   A  H (A*A, row-major, symmetric)  g (A)  l (A)  u (A)  k (A: a right-hand side for boxqp_gain)  max_iters
// and each output line its answer: "pd ok iters lower upper", then x (A), the masked factor (A*A) and the gain column
// (A) as hexadecimal floats (exact).  pd is lqr_cholesky's verdict on H itself.  tests/test_ilqr_box_cpu.py holds
// tests/boxqp_ref.py to these bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "boxqp_solve.h"

template <int A>
static bool run(char* p) {
  double v[A * A + 4 * A + 1];
  for (int j = 0; j < A * A + 4 * A + 1; ++j) {
    char* end;
    v[j] = strtod(p, &end);
    if (end == p) return false;
    p = end;
  }
  double h[A * A], fach[A * A], g[A], l[A], u[A], k[A];
  for (int j = 0; j < A * A; ++j) fach[j] = h[j] = v[j];
  for (int j = 0; j < A; ++j) {
    g[j] = v[A * A + j];
    l[j] = v[A * A + A + j];
    u[j] = v[A * A + 2 * A + j];
    k[j] = v[A * A + 3 * A + j];
  }
  const bool pd = cs::lqr_cholesky<A>(fach);
  cs::BoxQp<A> q;
  cs::boxqp_solve<A>(h, fach, g, l, u, (int)v[A * A + 4 * A], q);
  cs::boxqp_gain<A>(q, k);
  printf("%d %d %d %u %u", pd ? 1 : 0, q.ok ? 1 : 0, q.iters, q.lower, q.upper);
  for (int j = 0; j < A; ++j) printf(" %a", q.x[j]);
  for (int j = 0; j < A * A; ++j) printf(" %a", q.fac[j]);
  for (int j = 0; j < A; ++j) printf(" %a", k[j]);
  printf("\n");
  return true;
}

int main(int argc, char** argv) {
  FILE* in = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (in == nullptr) {
    fprintf(stderr, "boxqp_host: cannot open %s\n", argv[1]);
    return 2;
  }
  static char line[4096];
  while (fgets(line, sizeof line, in) != nullptr) {
    if (strspn(line, " \t\r\n") == strlen(line)) continue;
    char* end;
    const long a = strtol(line, &end, 10);
    const bool ok = a == 1 ? run<1>(end) : a == 2 ? run<2>(end) : a == 4 ? run<4>(end) : false;
    if (!ok) {
      fprintf(stderr, "boxqp_host: bad line (A in {1, 2, 4}, then A*A + 4 A + 1 values): %s", line);
      return 2;
    }
  }
  if (in != stdin) fclose(in);
  return 0;
}
