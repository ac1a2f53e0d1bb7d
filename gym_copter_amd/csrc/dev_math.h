// dev_math.h -- float64 sin / cos / sqrt sized for these kernels.
// Device code of copterstep_kernels.hip (included there, inside its floating-point-contraction pragma);
// not a stand-alone header.
#pragma once

#include "trig_reduce.h"

namespace cs {
namespace {

// ---------------------------------------------------------------------------------
// float64 sin/cos and sqrt, sized for this kernel (no library slow paths, no scratch)
// ---------------------------------------------------------------------------------
// Cody-Waite reduction by pi/2 in three pieces (33+33+53 bits) + a polynomial kernel on
// |y| <= pi/4: the fdlibm k_sin / k_cos minimax polynomials (<= ~1 ulp) where the state is kept in
// float64 words (FULL), and two shorter ones (sin 1.4e-11, cos 2.3e-13 absolute) where it is
// rounded to 29 or 24 significant bits anyway.  Larger angles than 2^19*pi/2 (not reached by a
// physical trajectory: 8e5 rad) are first folded by multiples of 2^17 * 2pi.  The reduction and the kernels are
// trig_reduce.h, which a host program compiles too; its table (tests/host/trig_reduce_host.cpp against sinl / cosl,
// max abs error of sin and cos, 2 M arguments of either sign per magnitude):
//   |x|              FULL       short      (FULL / short of the fold as it was: all three of its pieces first)
//   <= 7.9e5         1.8e-16    1.36e-11   (no fold: unchanged, bit for bit)
//   8e5 +- 5e5 ulps  8.1e-17    6.5e-13    6.1e-13 / 6.5e-13
//   8.1e5 - 1.0e6    2.1e-16    1.36e-11   3.0e-12 / 1.6e-11
//   1e8              2.1e-16    1.36e-11   2.9e-11 / 3.4e-11
//   1e11 - 1e17      2.1e-16    1.38e-11   5.8e-11 / 5.8e-11  (2^-34: the last bit of a folded value of 4e5)
//   1e18             3.7e-9     3.7e-9
//   1e20             4.8e-7     4.8e-7
// Accuracy ends between 1e17 and 1e18: from 2^36 folds on (5.6e16 rad) the fold's second piece times their number no
// longer fits below the leading remainder's last bit, and the error grows with the angle.
// (experiment build -DCS_EXP_FULLTRIG: the fdlibm-length polynomials in the float32 storage modes as well -- what the
// short ones save in time against what they cost in parity)
#ifdef CS_EXP_FULLTRIG
constexpr bool kFullTrigInEveryMode = true;
#else
constexpr bool kFullTrigInEveryMode = false;
#endif
// The three kernels above in LOCK-STEP: one Horner step of all six chains, then the next -- the same operations on the
// same values as three sincos_kernel calls (bit-identical), in an order the compiler may not undo: an empty asm
// statement that names the six accumulators after every step (each next step depends on its outputs; asm volatile
// statements keep their order).  Left to itself the compiler emits each chain as back-to-back dependent float64 FMAs
// (8 cycles apiece for a lone wavefront, profiles/r02_issue_cost_ubench.txt) although the six chains are independent;
// six-way interleaved an instruction costs 4.5-5.  (__builtin_amdgcn_sched_barrier does not do it: the optimiser moves
// the arithmetic across the intrinsic before the machine scheduler ever sees it -- tried, round 6.)
#define CS_PIN6(a, b, c, d, e, f) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f))
#define CS_PIN3(a, b, c) asm volatile("" : "+v"(a), "+v"(b), "+v"(c))
template <bool FULL>
__device__ __forceinline__ void sincos3_lockstep(const double* t, double a, double b, double g, double& sa,
                                                 double& ca, double& sb, double& cb, double& sg, double& cg) {
  double za = a * a, zb = b * b, zg = g * g;
  CS_PIN3(za, zb, zg);
  constexpr int S0 = FULL ? 9 : 19, NS = FULL ? 5 : 3;   // sine: t[S0] .. t[S0 - NS], NS Horner steps
  constexpr int C0 = FULL ? 15 : 24, NC = FULL ? 5 : 4;  // cosine: t[C0] .. t[C0 - NC]
  double pa = fma(za, t[S0], t[S0 - 1]), pb = fma(zb, t[S0], t[S0 - 1]), pg = fma(zg, t[S0], t[S0 - 1]);
  double qa = fma(za, t[C0], t[C0 - 1]), qb = fma(zb, t[C0], t[C0 - 1]), qg = fma(zg, t[C0], t[C0 - 1]);
  CS_PIN6(pa, pb, pg, qa, qb, qg);
#pragma unroll
  for (int k = 2; k <= NS; ++k) {
    pa = fma(za, pa, t[S0 - k]);
    pb = fma(zb, pb, t[S0 - k]);
    pg = fma(zg, pg, t[S0 - k]);
    qa = fma(za, qa, t[C0 - k]);
    qb = fma(zb, qb, t[C0 - k]);
    qg = fma(zg, qg, t[C0 - k]);
    CS_PIN6(pa, pb, pg, qa, qb, qg);
  }
  double ya = a * za, yb = b * zb, yg = g * zg;
  if constexpr (FULL) {
    double wa = -(za * za) * qa, wb = -(zb * zb) * qb, wg = -(zg * zg) * qg;
    CS_PIN6(ya, yb, yg, wa, wb, wg);
    sa = fma(ya, pa, a);
    sb = fma(yb, pb, b);
    sg = fma(yg, pg, g);
    double ua = fma(0.5, za, wa), ub = fma(0.5, zb, wb), ug = fma(0.5, zg, wg);
    CS_PIN6(sa, sb, sg, ua, ub, ug);
    ca = 1.0 - ua;
    cb = 1.0 - ub;
    cg = 1.0 - ug;
  } else {
    static_assert(FULL || NC == NS + 1, "short form: the cosine chains are one step longer");
    qa = fma(za, qa, t[C0 - NC]);  // the cosine's last Horner step shares a slot with the sine's y * z
    qb = fma(zb, qb, t[C0 - NC]);
    qg = fma(zg, qg, t[C0 - NC]);
    CS_PIN6(ya, yb, yg, qa, qb, qg);
    sa = fma(ya, pa, a);
    sb = fma(yb, pb, b);
    sg = fma(yg, pg, g);
    ca = fma(za, qa, 1.0);
    cb = fma(zb, qb, 1.0);
    cg = fma(zg, qg, 1.0);
  }
}

// the constants come from the kernel-argument block (DevConst::trig, filled by
// trig_constants()): wide scalar loads instead of literal moves per wavefront
template <bool FULL>
__device__ __forceinline__ void sincos_f64(const DevConst& k, double x, double& s, double& c) {
  sincos_reduced<FULL>(k.trig, x, s, c);
}

// sin and cos of the three Euler angles.  Roll and pitch of a live env are inside +-pi/4 (the task
// ends the episode beyond, task.py:116): when that holds for the whole wavefront the reduction is the
// identity (fn = 0, y = x exactly) and is skipped -- bit-identical to the general path.  Yaw is
// unbounded, but the yaw torque of this airframe is weak (D << B): it usually qualifies too.
struct Trig {
  double sph, cph, sth, cth, sps, cps;
};
// __all() without its detour through an integer: HIP's __all(p) turns p into 0 / 1 in a vector register and compares that
// again (v_cndmask + v_cmp per call); a ballot of the NEGATED predicate against zero is scalar work on the compare's own
// mask.  Same meaning: true iff p holds on every ACTIVE lane.  Used in the K-step loops (bound by their instruction
// count); the one-launch kernels keep __all: the ballot form measured +-0.1 % there (profiles/r06_ab_kstep_instruction_count.txt, D).
__device__ __forceinline__ bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0ull; }
// IN_LOOP: the call sits in a K-step loop, where laying the in-range path out as the fall-through pays
// (-3 % per step); in the one-step kernel the same layout measured +2.5 %, so it keeps the compiler's
template <bool FULL, bool IN_LOOP>
__device__ __forceinline__ void sincos_roll_pitch(const DevConst& c, double phi, double the, Trig& t) {
  const bool in_range = IN_LOOP ? wave_all(fabs(phi) < 0.785 && fabs(the) < 0.785)
                                : __all(fabs(phi) < 0.785 && fabs(the) < 0.785);
  if (IN_LOOP ? __builtin_expect(in_range, 1) : in_range) {
    sincos_kernel<FULL>(c.trig, phi, t.sph, t.cph);
    sincos_kernel<FULL>(c.trig, the, t.sth, t.cth);
  } else {
    sincos_f64<FULL>(c, phi, t.sph, t.cph);
    sincos_f64<FULL>(c, the, t.sth, t.cth);
  }
}
template <bool FULL, bool IN_LOOP>
__device__ __forceinline__ void sincos_yaw(const DevConst& c, double psi, Trig& t) {
  const bool in_range = IN_LOOP ? wave_all(fabs(psi) < 0.785) : __all(fabs(psi) < 0.785);
  if (IN_LOOP ? __builtin_expect(in_range, 1) : in_range) {
    sincos_kernel<FULL>(c.trig, psi, t.sps, t.cps);
  } else {
    sincos_f64<FULL>(c, psi, t.sps, t.cps);
  }
}

// sqrt for a >= 0: hardware v_rsq_f64 seed + Heron corrections; 0, +inf and NaN pass through.
// STEPS = 2: <= 1 ulp.  STEPS = 1 (~2^-40 relative): the shaping potential, whose only consumers are a
// float32 reward and a prev_shaping word of the state's precision.
template <int STEPS>
__device__ __forceinline__ double sqrt_f64(double a) {
  const double r = __builtin_amdgcn_rsq(a);
  double y = a * r;
  const double h = 0.5 * r;
#pragma unroll
  for (int k = 0; k < STEPS; ++k) y = fma(fma(-y, y, a), h, y);
  return __builtin_amdgcn_class(a, 0x260) ? a : y;  // +-0 (0x20 | 0x40) and +inf (0x200)
}

}  // namespace
}  // namespace cs
