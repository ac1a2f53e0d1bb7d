// boxqp_solve.h -- the box-constrained A x A quadratic programme of the control-limited iLQR backward pass
// (cs_ilqr_box_backward, copterstep_ilqr_box.hip): minimise f(x) = 1/2 x^T H x + g^T x over l <= x <= u by projected
// Newton steps (Tassa, Mansard, Todorov: "Control-limited differential dynamic programming", ICRA 2014), all in
// registers, on the Cholesky of lqr_solve.h.  Plain C++ with no dependence on the device headers, so that a host
// program compiles the very same code (tests/host/boxqp_host.cpp).  The arithmetic is fixed -- sums in index order from
// 0.0, one multiply and one add per term; the including translation unit forbids floating-point contraction -- and
// tests/boxqp_ref.py restates it operation for operation.  DESIGN.md section 24.
//
//   clamp(v)   v < l ? l : (v > u ? u : v)                                   (a NaN stays a NaN)
//   (Hx)_a     sum_b H_ab x_b,   f(x) = sum_a x_a (0.5 (Hx)_a + g_a)
//   start      x = clamp(-(H^-1 g)): the caller's factor of H, lqr_solve on g, the sign flipped
//   iteration, at most kBoxQpIters of them (none when max_iters = 0):
//     gr = g + Hx
//     control a is CLAMPED if (x_a <= l_a and gr_a > 0) or (x_a >= u_a and gr_a < 0), else FREE
//     none free: stop
//     M_ab = H_ab where a and b are free, else delta_ab;  lqr_cholesky(M) (a bad pivot: ok = false, carried through)
//     rhs_a = -(g_a + sum_{b clamped} H_ab x_b) on free rows (the sum starts from g_a), 0 on clamped;  lqr_solve
//     s_a = rhs_a - x_a on free rows, 0 on clamped
//     max|s| <= 1e-14 max(1, max|x|): stop   (the maxima by `if (v > m) m = v` from 0 and 1: a NaN never raises them)
//     Armijo: t = 1; x_c = clamp(x + t s); accept when f(x_c) - f(x) <= (0.1 t) (gr^T s), else t <- 0.6 t; at most
//     kBoxQpTrials trials.  No trial accepted: the iteration could only repeat itself, which exhausts the cap; stop.
//   The cap exhausted (the 16th iteration still moved x, or no trial was accepted): ok = false.
// With l = -inf, u = +inf nothing is ever clamped, M is H, rhs is -g and s is 0 exactly: x is the unconstrained
// -(H^-1 g) bit for bit after one iteration.
#pragma once

#include "lqr_solve.h"

namespace cs {

constexpr int kBoxQpIters = 16;
constexpr int kBoxQpTrials = 30;

template <int A>
struct BoxQp {
  double x[A];        // the minimiser
  double fac[A * A];  // the factor of the last iteration's masked matrix (the identity where none was formed)
  unsigned lower;     // bit a: control a held at its lower bound (last iteration's set; with no iteration: where the
  unsigned upper;     //        start's clamp raised x_a), and at its upper bound
  int iters;          // iterations used
  bool ok;            // false: a bad pivot of a masked factor, or the cap exhausted
};

CS_LQR_FN double boxqp_clamp(double v, double l, double u) { return v < l ? l : (v > u ? u : v); }

template <int A>
CS_LQR_FN void boxqp_times(const double (&h)[A * A], const double (&x)[A], double (&hx)[A]) {
#pragma unroll
  for (int a = 0; a < A; ++a) {
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < A; ++b) acc += h[a * A + b] * x[b];
    hx[a] = acc;
  }
}

template <int A>
CS_LQR_FN double boxqp_value(const double (&hx)[A], const double (&g)[A], const double (&x)[A]) {
  double f = 0.0;
#pragma unroll
  for (int a = 0; a < A; ++a) f += x[a] * (0.5 * hx[a] + g[a]);
  return f;
}

// h: H, full and symmetric; fach: its factor (lqr_cholesky); g, l, u as above; max_iters <= kBoxQpIters
template <int A>
CS_LQR_FN void boxqp_solve(const double (&h)[A * A], const double (&fach)[A * A], const double (&g)[A],
                           const double (&l)[A], const double (&u)[A], int max_iters, BoxQp<A>& q) {
  constexpr unsigned kAll = (1u << A) - 1u;
  q.lower = q.upper = 0u;
#pragma unroll
  for (int a = 0; a < A; ++a) q.x[a] = g[a];
  lqr_solve<A>(fach, q.x);
#pragma unroll
  for (int a = 0; a < A; ++a) {
    const double v = -q.x[a];
    q.x[a] = boxqp_clamp(v, l[a], u[a]);
    if (v < l[a]) q.lower |= 1u << a;
    else if (v > u[a]) q.upper |= 1u << a;
  }
#pragma unroll
  for (int j = 0; j < A * A; ++j) q.fac[j] = (j % (A + 1)) == 0 ? 1.0 : 0.0;
  q.iters = 0;
  q.ok = true;
  bool done = max_iters <= 0;
#pragma clang loop unroll(disable)
  for (int it = 0; it < kBoxQpIters; ++it) {
    if (done || it >= max_iters) break;
    q.iters = it + 1;
    double hx[A], gr[A];
    boxqp_times<A>(h, q.x, hx);
    unsigned lo = 0u, up = 0u;
#pragma unroll
    for (int a = 0; a < A; ++a) {
      gr[a] = g[a] + hx[a];
      if (q.x[a] <= l[a] && gr[a] > 0.0) lo |= 1u << a;
      else if (q.x[a] >= u[a] && gr[a] < 0.0) up |= 1u << a;
    }
    q.lower = lo;
    q.upper = up;
    const unsigned cl = lo | up;
#pragma unroll
    for (int j = 0; j < A * A; ++j) q.fac[j] = (j % (A + 1)) == 0 ? 1.0 : 0.0;
    if (cl == kAll) {
      done = true;
      break;
    }
#pragma unroll
    for (int a = 0; a < A; ++a) {
#pragma unroll
      for (int b = 0; b < A; ++b) {
        if (!((cl >> a) & 1u) && !((cl >> b) & 1u)) q.fac[a * A + b] = h[a * A + b];
      }
    }
    const bool pd = lqr_cholesky<A>(q.fac);
    q.ok = q.ok && pd;
    double s[A];
#pragma unroll
    for (int a = 0; a < A; ++a) {
      double t = g[a];
#pragma unroll
      for (int b = 0; b < A; ++b) {
        if ((cl >> b) & 1u) t += h[a * A + b] * q.x[b];
      }
      s[a] = ((cl >> a) & 1u) ? 0.0 : -t;
    }
    lqr_solve<A>(q.fac, s);
    double ms = 0.0, mx = 1.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
      s[a] = ((cl >> a) & 1u) ? 0.0 : s[a] - q.x[a];
      const double vs = fabs(s[a]), vx = fabs(q.x[a]);
      if (vs > ms) ms = vs;
      if (vx > mx) mx = vx;
    }
    if (ms <= 1e-14 * mx) {
      done = true;
      break;
    }
    double gs = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) gs += gr[a] * s[a];
    const double f0 = boxqp_value<A>(hx, g, q.x);
    double t = 1.0;
    bool accepted = false;
    double xc[A];
#pragma clang loop unroll(disable)
    for (int trial = 0; trial < kBoxQpTrials; ++trial) {
      double hc[A];
#pragma unroll
      for (int a = 0; a < A; ++a) xc[a] = boxqp_clamp(q.x[a] + t * s[a], l[a], u[a]);
      boxqp_times<A>(h, xc, hc);
      const double df = boxqp_value<A>(hc, g, xc) - f0;
      if (df <= 0.1 * t * gs) {
        accepted = true;
        break;
      }
      t = 0.6 * t;
    }
    if (!accepted) break;
#pragma unroll
    for (int a = 0; a < A; ++a) q.x[a] = xc[a];
  }
  q.ok = q.ok && done;
}

// kk <- the free rows of -(H_ff)^-1 kk_f by the factor boxqp_solve left, 0.0 on the clamped rows: a column of the gains
template <int A>
CS_LQR_FN void boxqp_gain(const BoxQp<A>& q, double (&kk)[A]) {
  const unsigned cl = q.lower | q.upper;
#pragma unroll
  for (int a = 0; a < A; ++a) kk[a] = ((cl >> a) & 1u) ? 0.0 : kk[a];
  lqr_solve<A>(q.fac, kk);
#pragma unroll
  for (int a = 0; a < A; ++a) kk[a] = ((cl >> a) & 1u) ? 0.0 : -kk[a];
}

}  // namespace cs
