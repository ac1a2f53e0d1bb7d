// rollout_adjoint.h -- reverse-mode (adjoint) rules of one _Task.step(): the transposes of jacobian_tangents.h's
// euler_tangent, wrench_tangent and the Lander shaping gradient, for the vector-Jacobian products of cs_rollout_vjp
// (dynamics/__init__.py:114-197, :249-302; envs/task.py:77-137; envs/lander.py:46-74).  Device code of
// copterstep_rollout_grad.hip (included there, inside its floating-point-contraction pragma, after jacobian_tangents.h);
// not a stand-alone header.  DESIGN.md section 10.
//
// Where forward mode carries 12 + A tangent directions through a step (the Jacobian: 12 x 16 numbers per env-step),
// reverse mode carries ONE covector: the adjoint lambda of the state (12 float64) and, within a step, the adjoint of the
// wrench (5).  Every rule below is the exact transpose of its tangent rule, so lambda' J == (J^T lambda')^T term by
// term.  Branch-free like the tangents: a call that does not integrate has dt = 0 (identity), LEVELING zeroes the
// adjoint of the phi, theta slots that the call overwrites.
#pragma once

namespace cs {
namespace {

// The lane's accumulators of the coefficient adjoints (PARAM builds): row j of Coef at acc[j * kBlock], in the LDS
// (copterstep_rollout_grad.hip: rollout_vjp_param_kernel); rows kAccPe .. kAccPe + 2 hold the perturbation's adjoint
constexpr int kAccPe = kCoefRows;
constexpr int kAccRows = kCoefRows + 3;

// The adjoint of one integrating Dynamics.setMotors() (forward Euler x' = x + dt f(x, w), euler_tangent): on entry `l`
// is the adjoint of the state AFTER the call, on exit that of the state BEFORE it (x, with t its sin / cos); the
// adjoint of the call's wrench is added to `mw`.  The perturbation's adjoint (dt times the velocity adjoints on entry) is
// taken by the caller, in the call where it enters.  PARAM (cs_rollout_vjp_ex): the adjoints of
// the per-call coefficients G, c_d*, g_* are added to the lane's LDS accumulators `acc` as well -- the transposes of
// where euler_rotation and thrust_ned multiply by them.
template <bool GYRO, bool PARAM = false>
__device__ __forceinline__ void euler_adjoint(const Coef& q, const Wrench& w, const Trig& t, const double (&x)[12],
                                              double dt, bool leveling, double (&l)[12], Wrench& mw,
                                              double* acc = nullptr) {
  const double sph = t.sph, cph = t.cph, sth = t.sth, cth = t.cth, sps = t.sps, cps = t.cps;
  const double Rx = cph * cps * sth + sph * sps;  // ax / bz
  const double Ry = cph * sps * sth - cps * sph;  // ay / bz
  const double Rz = cph * cth;                    // (netz - G) / bz
  // the call overwrites phi, theta when it levels the wings (:174-175): nothing of the old values survives
  const double l6 = leveling ? 0.0 : l[6], l8 = leveling ? 0.0 : l[8];
  const double p = x[7], th = x[9], ps = x[11];  // angular rates before the call
  const double e1 = dt * l[1], e3 = dt * l[3], e5 = dt * l[5];     // adjoints of the three accelerations
  const double f7 = dt * l[7], f9 = -(dt * l[9]), f11 = dt * l[11];  // ... of d7, d9s, d11
  mw.bz += (e1 * Rx + e3 * Ry) + e5 * Rz;
  mw.aphi += f7;
  mw.athe += f9;
  mw.apsi += f11;
  const double b1 = w.bz * e1, b3 = w.bz * e3, b5 = w.bz * e5;
  const double n6 = l6 + (b1 * (cph * sps - sph * cps * sth) + b3 * (-(sph * sps * sth) - cps * cph) + b5 * (-(sph * cth)));
  const double n8 = l8 + (b1 * (cph * cps * cth) + b3 * (cph * sps * cth) + b5 * (-(cph * sth)));
  const double n10 = l[10] + (b1 * (sph * cps - cph * sps * sth) + b3 * (cph * cps * sth + sps * sph));
  double n7 = l[7] + dt * l6 + (q.c_dthe * ps * f9 + q.c_dpsi * th * f11);
  double n9 = l[9] + dt * l8 + (q.c_dphi * ps * f7 + q.c_dpsi * p * f11);
  const double n11 = l[11] + dt * l[10] + (q.c_dphi * th * f7 + q.c_dthe * p * f9);
  if constexpr (GYRO) {  // d7 -= g_phi (dthe om), d9s += g_the (dphi om)
    n7 += q.g_the * w.om * f9;
    n9 -= q.g_phi * w.om * f7;
    mw.om += q.g_the * p * f9 - q.g_phi * th * f7;
  }
  if constexpr (PARAM) {  // netz = bz Rz + G; d7 = c_dphi ps th + ..., d9s = c_dthe ps p + ..., d11 = c_dpsi th p + ...
    acc[4 * kBlock] += e5;
    acc[5 * kBlock] += (ps * th) * f7;
    acc[6 * kBlock] += (ps * p) * f9;
    acc[7 * kBlock] += (th * p) * f11;
    if constexpr (GYRO) {
      acc[9 * kBlock] -= (th * w.om) * f7;
      acc[10 * kBlock] += (p * w.om) * f9;
    }
  }
  l[1] += dt * l[0];
  l[3] += dt * l[2];
  l[5] += dt * l[4];
  l[6] = n6;
  l[8] = n8;
  l[10] = n10;
  l[7] = n7;
  l[9] = n9;
  l[11] = n11;
}

// The adjoint of the float64 motor law (wrench_tangent) and of the clip: the wrench adjoint `mw` -> the adjoint of the
// four motor values, summed into the task's action columns (the fan-out of _get_motors, as step_jacobian_kernel sums
// them), zero where the action was clipped.
template <int A>
__device__ __forceinline__ void motor_adjoint(const Coef& q, const double (&m)[4], const double (&clipd)[4],
                                              const Wrench& mw, double (&ga)[4]) {
  const double sr[4] = {-1.0, 1.0, 1.0, -1.0};   // roll:  (m1^2 + m2^2) - (m0^2 + m3^2)
  const double sp[4] = {-1.0, 1.0, -1.0, 1.0};   // pitch: (m1^2 + m3^2) - (m0^2 + m2^2)
  const double sy[4] = {1.0, 1.0, -1.0, -1.0};   // yaw and om: (m0 + m1) - (m2 + m3)
#pragma unroll
  for (int c = 0; c < 4; ++c) ga[c] = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double sq = q.k_thrust * mw.bz + sr[j] * (q.k_roll * mw.aphi) + sp[j] * (q.k_pitch * mw.athe) +
                      sy[j] * (q.k_yaw * mw.apsi);
    const double gm = clipd[j] * (2.0 * m[j] * sq + sy[j] * mw.om);
    const int col = A == 4 ? j : A == 2 ? ((j == 1 || j == 2) ? 1 : 0) : 0;
    ga[col] += gm;
  }
}

}  // namespace
}  // namespace cs
