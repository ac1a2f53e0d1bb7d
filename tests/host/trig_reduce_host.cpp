// trig_reduce_host.cpp -- the device sin / cos (gym_copter_amd/csrc/trig_reduce.h: reduction, polynomial kernel, quadrant)
// compiled for the host, with the library's own constants, fma / rint sequence and contraction off:
//   trig_reduce_host [ARGS_PER_SIGN = 1000000] [IDENTITY_ARGS = 10000000]
// 1. bit-identity below 8e5: sincos_reduced against a verbatim copy of the reduction it replaced (old_sincos below), sin
//    and cos, FULL and short, on IDENTITY_ARGS random arguments (uniform and log-uniform, either sign) plus +-0, the
//    denormals' ends, every k pi/2 + pi/4 for |k| <= 2000 with +-50 ulps around it, and 0.785, pi/4 and 8e5 with their
//    neighbours.  Prints "identity <arguments> <mismatches>".
// 2. accuracy by magnitude: max(|sin - sinl|, |cos - cosl|) over ARGS_PER_SIGN arguments of either sign per magnitude M:
//    x in M [1/2, 1) for M <= 7.9e5, the ARGS_PER_SIGN doubles around 8e5 itself (half below the fold's threshold, half
//    at or above it), x in M [1, 5/4) above.  Prints "acc <M> <FULL> <short> <FULL of the old code> <short of the old
//    code>" per required magnitude and "beyond ..." for the magnitudes past the requirement (where accuracy ends).
// 3. prints "inrange <FULL> <short>": the largest figures of the rows below 8e5, and "bar 4".
// Exit status 1 when a bit differs or a required row exceeds 4 x the in-range figure of its column.
// tests/test_trig_reduce_cpu.py runs it and asserts on what it prints.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "trig_reduce.h"

namespace {

// --- the reduction as it was before trig_reduce.h (dev_math.h: sincos_f64), verbatim but for the constants' source ---
template <bool FULL>
void old_sincos(const double* t, double x, double& s, double& c) {
  if (__builtin_expect(fabs(x) >= 8.0e5, 0)) {
    const double n1 = rint(x * (1.0 / (6.283185307179586476925 * 131072.0)));
    // 2pi * 2^17 in the same three pieces as pi/2 below (power-of-two scalings are exact)
    x = fma(-n1, 1.57079632673412561417e+00 * 524288.0, x);
    x = fma(-n1, 6.07710050630396597660e-11 * 524288.0, x);
    x = fma(-n1, 2.02226624879595063154e-21 * 524288.0, x);
  }
  const double fn = rint(x * t[0]);
  double y = fma(-fn, t[1], x);
  y = fma(-fn, t[2], y);
  y = fma(-fn, t[3], y);
  const int q = (int)fn;
  double sy, cy;
  cs::sincos_kernel<FULL>(t, y, sy, cy);
  const double s0 = (q & 1) ? cy : sy;
  const double c0 = (q & 1) ? sy : cy;
  s = (q & 2) ? -s0 : s0;
  c = ((q + 1) & 2) ? -c0 : c0;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
double next_unit() { return (double)(next_u64() >> 11) * 0x1.0p-53; }  // [0, 1)

uint64_t bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
double step_ulps(double v, int k) {  // v moved by k units in the last place (v > 0 and far from 0)
  const uint64_t b = bits(v) + (uint64_t)(int64_t)k;
  double r;
  memcpy(&r, &b, 8);
  return r;
}

double T[cs::kTrigConstants];
uint64_t n_identity = 0, n_mismatch = 0;

void identity_one(double x) {
  for (int sign = 0; sign < 2; ++sign, x = -x) {
    double s0, c0, s1, c1;
    old_sincos<true>(T, x, s0, c0);
    cs::sincos_reduced<true>(T, x, s1, c1);
    bool same = bits(s0) == bits(s1) && bits(c0) == bits(c1);
    old_sincos<false>(T, x, s0, c0);
    cs::sincos_reduced<false>(T, x, s1, c1);
    same = same && bits(s0) == bits(s1) && bits(c0) == bits(c1);
    ++n_identity;
    if (!same && n_mismatch++ < 5) printf("mismatch at %a\n", x);
  }
}

struct Err {
  long double full = 0, shrt = 0, old_full = 0, old_shrt = 0;
};
void accuracy_one(double x, Err& e) {
  long double rs, rc;
  sincosl((long double)x, &rs, &rc);
  double s, c;
  cs::sincos_reduced<true>(T, x, s, c);
  e.full = fmaxl(e.full, fmaxl(fabsl(s - rs), fabsl(c - rc)));
  cs::sincos_reduced<false>(T, x, s, c);
  e.shrt = fmaxl(e.shrt, fmaxl(fabsl(s - rs), fabsl(c - rc)));
  old_sincos<true>(T, x, s, c);
  e.old_full = fmaxl(e.old_full, fmaxl(fabsl(s - rs), fabsl(c - rc)));
  old_sincos<false>(T, x, s, c);
  e.old_shrt = fmaxl(e.old_shrt, fmaxl(fabsl(s - rs), fabsl(c - rc)));
}

}  // namespace

int main(int argc, char** argv) {
  const long per_sign = argc > 1 ? atol(argv[1]) : 1000000;
  const long n_ident = argc > 2 ? atol(argv[2]) : 10000000;
  if (per_sign < 1 || n_ident < 1) {
    fprintf(stderr, "usage: trig_reduce_host [ARGS_PER_SIGN] [IDENTITY_ARGS]\n");
    return 2;
  }
  cs::trig_constants(T);

  // ---- 1. bit-identity below 8e5 ----
  const double specials[] = {0.0, 4.9406564584124654e-324, 1e-320, 2.2250738585072009e-308, 2.2250738585072014e-308,
                             1e-300, 1e-160, 1e-20, 1.0, 7.9e5, 799999.0};
  for (double v : specials) identity_one(v);
  const double pio4 = 0.78539816339744830962, edges[] = {0.785, pio4, 0.78, 0.8, 1.5707963267948966, 3.141592653589793};
  for (double v : edges)
    for (int k = -50; k <= 50; ++k) identity_one(step_ulps(v, k));
  for (int k = -50; k < 0; ++k) identity_one(step_ulps(8.0e5, k));  // the last arguments that are not folded
  for (int k = 0; k <= 2000; ++k) {
    const double v = (double)((long double)k * 1.57079632679489661923132169163975144L + 0.78539816339744830961566084581987572L);
    for (int j = -50; j <= 50; ++j) identity_one(step_ulps(v, j));  // (identity_one takes both signs: k and -k - 1)
  }
  for (long i = 0; i < n_ident; i += 4) {  // two arguments of either sign per turn
    identity_one(8.0e5 * next_unit());                         // uniform: mostly thousands of quadrants out
    identity_one(exp(log(1e-320) + next_unit() * (log(8.0e5) - log(1e-320))));  // log-uniform: every binade, denormals too
  }
  printf("identity %llu %llu\n", (unsigned long long)n_identity, (unsigned long long)n_mismatch);

  // ---- 2. accuracy by magnitude ----
  const double required[] = {0.78, 3.0, 300.0, 3e4, 7.9e5, 8e5, 8.1e5, 1e8, 1e11, 7e11};
  const double beyond[] = {1e15, 1e17, 1e18, 1e20};  // (a quarter of the arguments each)
  Err in_range, rows[16];
  int nrows = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const double* mags = pass ? beyond : required;
    const int n = pass ? (int)(sizeof beyond / sizeof *beyond) : (int)(sizeof required / sizeof *required);
    for (int m = 0; m < n; ++m) {
      const double M = mags[m];
      Err e;
      for (long i = 0; i < (pass ? (per_sign + 3) / 4 : per_sign); ++i) {
        double x;
        if (M == 8e5) {
          const long k = i - per_sign / 2;  // ... 8e5 - 1 ulp, 8e5 itself, 8e5 + 1 ulp ...
          x = step_ulps(M, (int)(k > 2000000000L ? 2000000000L : k < -2000000000L ? -2000000000L : k));
        } else {
          x = M < 8e5 ? M * (0.5 + 0.5 * next_unit()) : M * (1.0 + 0.25 * next_unit());
        }
        accuracy_one(x, e);
        accuracy_one(-x, e);
      }
      printf("%s %.3g %.3Le %.3Le %.3Le %.3Le\n", pass ? "beyond" : "acc", M, e.full, e.shrt, e.old_full, e.old_shrt);
      if (!pass) {
        rows[nrows++] = e;
        if (M < 8e5) {
          in_range.full = fmaxl(in_range.full, e.full);
          in_range.shrt = fmaxl(in_range.shrt, e.shrt);
        }
      }
    }
  }
  printf("inrange %.3Le %.3Le\nbar 4\n", in_range.full, in_range.shrt);
  bool ok = n_mismatch == 0;
  for (int m = 0; m < nrows; ++m) ok = ok && rows[m].full <= 4 * in_range.full && rows[m].shrt <= 4 * in_range.shrt;
  // NaN and the infinities give NaN, never a number
  const double bad[] = {NAN, INFINITY, -INFINITY};
  for (double v : bad) {
    double s, c;
    cs::sincos_reduced<true>(T, v, s, c);
    ok = ok && s != s && c != c;
    cs::sincos_reduced<false>(T, v, s, c);
    ok = ok && s != s && c != c;
  }
  printf("%s\n", ok ? "trig_reduce_host: OK" : "trig_reduce_host: FAILED");
  return ok ? 0 : 1;
}
