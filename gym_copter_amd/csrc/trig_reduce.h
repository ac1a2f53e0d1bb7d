// trig_reduce.h -- the argument reduction and the polynomial kernels of the device sin / cos (dev_math.h: sincos_f64).
// Plain C++ with no dependence on the device headers, so that a host program compiles the very same code
// (tests/host/trig_reduce_host.cpp compares it with sinl / cosl and, below 8e5, bit for bit with the reduction it
// replaced).  Every multiply-add is written out; the including translation unit forbids floating-point contraction.
// DESIGN.md section 3.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define CS_TRIG_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define CS_TRIG_FN inline
#endif

namespace cs {

// sin/cos constants: [0] 2/pi, [1..3] pi/2 in three pieces (33+33+53 bits, fdlibm
// pio2_1, pio2_2, pio2_2t), [4..9] S1..S6, [10..15] C1..C6 (fdlibm k_sin / k_cos),
// [16..19] / [20..24] the shorter minimax polynomials of the float32 state modes
constexpr int kTrigConstants = 25;
inline void trig_constants(double (&t)[kTrigConstants]) {
  const double v[kTrigConstants] = {6.36619772367581382433e-01,  1.57079632673412561417e+00,
                                    6.07710050630396597660e-11,  2.02226624879595063154e-21,
                                    -1.66666666666666324348e-01, 8.33333333332248946124e-03,
                                    -1.98412698298579493134e-04, 2.75573137070700676789e-06,
                                    -2.50507602534068634195e-08, 1.58969099521155010221e-10,
                                    4.16666666666666019037e-02,  -1.38888888888741095749e-03,
                                    2.48015872894767294178e-05,  -2.75573143513906633035e-07,
                                    2.08757232129817482790e-09,  -1.13596475577881948265e-11,
                                    // sin(y) = y + y^3 * (s0 + s1 z + s2 z^2 + s3 z^3), z = y^2, |y| <= pi/4: 1.4e-11
                                    -0x1.555555545e43fp-3, 0x1.11110def9bd00p-7, -0x1.a013a80b71025p-13,
                                    0x1.6dbe28b3498d4p-19,
                                    // cos(y) = 1 + z * (c0 + c1 z + c2 z^2 + c3 z^3 + c4 z^4): 2.3e-13
                                    -0x1.fffffffffe699p-2, 0x1.5555555150044p-5, -0x1.6c16bae67d7a6p-10,
                                    0x1.a012993437ed5p-16, -0x1.2474f436b27edp-22};
  for (int i = 0; i < kTrigConstants; ++i) t[i] = v[i];
}

// sin and cos of |y| <= pi/4: the fdlibm k_sin / k_cos minimax polynomials (FULL) or the two shorter ones.
template <bool FULL>
CS_TRIG_FN void sincos_kernel(const double* t, double y, double& sy, double& cy) {
  const double z = y * y;
  if constexpr (FULL) {
    double ps = fma(z, t[9], t[8]);
    ps = fma(z, ps, t[7]);
    ps = fma(z, ps, t[6]);
    ps = fma(z, ps, t[5]);
    ps = fma(z, ps, t[4]);
    sy = fma(y * z, ps, y);
    double pc = fma(z, t[15], t[14]);
    pc = fma(z, pc, t[13]);
    pc = fma(z, pc, t[12]);
    pc = fma(z, pc, t[11]);
    pc = fma(z, pc, t[10]);
    cy = 1.0 - fma(0.5, z, -(z * z) * pc);
  } else {
    double ps = fma(z, t[19], t[18]);
    ps = fma(z, ps, t[17]);
    ps = fma(z, ps, t[16]);
    sy = fma(y * z, ps, y);
    double pc = fma(z, t[24], t[23]);
    pc = fma(z, pc, t[22]);
    pc = fma(z, pc, t[21]);
    pc = fma(z, pc, t[20]);
    cy = fma(z, pc, 1.0);
  }
}

// x = fn * pi/2 + y with |y| <= pi/4 (up to the rounding of fn's choice); returns y, q = fn as an integer.
// Cody-Waite by pi/2 in three pieces: each fma subtracts fn times a piece whose product with fn is exact or far below
// the running value's last bit -- which holds only while the running value is SMALL.  So an angle of 8e5 rad or more
// (2^19 * pi/2; not reached by a physical trajectory) is first folded by n1 multiples of 2^17 * 2pi, in the same three
// pieces scaled by 2^19 (exact), with the pieces of the two reductions interleaved by size: the leading piece of the
// fold alone first (exact: both operands are multiples of its last bit), fn chosen from a copy that has the second piece
// too, then pi/2's leading piece (exact again), and only then, on a value below pi/4 + 2^-15 n1, the small pieces in
// descending order.  Subtracting all three pieces of the fold first, as this code did before, rounds n1 * 6e-11 * 2^19
// into a running value of up to 4e5, at that value's last bit: 2^-34 = 5.8e-11 absolute.  Measured against sinl / cosl
// (tests/host/trig_reduce_host.cpp, the table in DESIGN.md section 3): the error below 8e5 at every magnitude up to
// 1e15; the in-range path (no fold) is operation for operation what it was.
CS_TRIG_FN double trig_reduce(const double* t, double x, int& q) {
  double fn, y;
  if (__builtin_expect(fabs(x) >= 8.0e5, 0)) {
    const double n1 = rint(x * (1.0 / (6.283185307179586476925 * 131072.0)));
    const double r = fma(-n1, 1.57079632673412561417e+00 * 524288.0, x);
    fn = rint(fma(-n1, 6.07710050630396597660e-11 * 524288.0, r) * t[0]);
    y = fma(-fn, t[1], r);
    y = fma(-n1, 6.07710050630396597660e-11 * 524288.0, y);
    y = fma(-fn, t[2], y);
    y = fma(-n1, 2.02226624879595063154e-21 * 524288.0, y);
    y = fma(-fn, t[3], y);
  } else {
    fn = rint(x * t[0]);
    y = fma(-fn, t[1], x);
    y = fma(-fn, t[2], y);
    y = fma(-fn, t[3], y);
  }
  q = (int)fn;
  return y;
}

// sin and cos of any x: the reduction, the kernel, the quadrant.  NaN and +-inf give NaN, NaN.
template <bool FULL>
CS_TRIG_FN void sincos_reduced(const double* t, double x, double& s, double& c) {
  int q;
  const double y = trig_reduce(t, x, q);
  double sy, cy;
  sincos_kernel<FULL>(t, y, sy, cy);
  const double s0 = (q & 1) ? cy : sy;
  const double c0 = (q & 1) ? sy : cy;
  s = (q & 2) ? -s0 : s0;
  c = ((q + 1) & 2) ? -c0 : c0;
}

}  // namespace cs
