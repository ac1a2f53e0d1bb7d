// jacobian_tangents.h -- forward-mode tangents of one _Task.step(): the derivatives of Dynamics.setMotors x substeps
// (dynamics/__init__.py:114-197, :249-302) and of the Lander shaping potential (lander.py:46-74) with respect to the
// state and the action.  Device code of copterstep_jacobian.hip (included there, inside its floating-point-contraction
// pragma, after dev_physics.h / dev_task.h); not a stand-alone header.
//
// Register budget.  The whole tangent block [dx' / dx | dx' / da] is 12 x 16 float64 = 384 VGPRs per lane, out of one
// 512-entry VGPR + AGPR file (MI355X_MICROARCH, "VGPR"): carried whole it cannot even hold the primal beside it.
// Instead the directions go in blocks of kJacDirs (forward mode in direction blocks): one block carries 12 x kJacDirs
// tangents through the substeps next to the primal, and the primal -- ~120 float64 operations per substep, cheap next
// to the 12 x 16 x 8 bytes each env writes -- is run again for every block.  kJacDirs = 2 is the widest block that does
// not spill (make report, gfx950): 4 directions took 306 VGPRs + AGPRs with 24 spilled (one wavefront per SIMD); 2 take
// <= 256, two wavefronts per SIMD and no scratch.  The tangent update is branch-free like the primal (a call that does not
// integrate has dt = 0): a divergent if / else around it kept the old and the new tangents live together (+160 VGPRs).
#pragma once

namespace cs {
namespace {

constexpr int kJacDirs = 2;

// The wrench of the float64 motor law (dev_physics.h: thrust_model / torque_model) and its tangent in one direction:
// bz = k_thrust * sum(m^2), aphi = k_roll * ((m1^2 + m2^2) - (m0^2 + m3^2)), ..., om = (m0 + m1) - (m2 + m3)
__device__ __forceinline__ Wrench wrench_tangent(const Coef& q, const double (&m)[4], const double (&dm)[4]) {
  const double t0 = 2.0 * m[0] * dm[0], t1 = 2.0 * m[1] * dm[1], t2 = 2.0 * m[2] * dm[2], t3 = 2.0 * m[3] * dm[3];
  Wrench d;
  d.bz = q.k_thrust * (((t0 + t1) + t2) + t3);
  d.aphi = q.k_roll * ((t1 + t2) - (t0 + t3));
  d.athe = q.k_pitch * ((t1 + t3) - (t0 + t2));
  d.apsi = q.k_yaw * ((t0 + t1) - (t2 + t3));
  d.om = (dm[0] + dm[1]) - (dm[2] + dm[3]);
  return d;
}

// One integrating Dynamics.setMotors() applied to a tangent v (12 components) with wrench tangent dw, from the state x
// BEFORE the call (t = its sin / cos).  The derivative of forward Euler x' = x + dt f(x, w):  v' = v + dt (df/dx v +
// df/dw dw), with f the state derivative of :273-289 and the body-Z -> NED rotation of :292-302.  The perturbation is a
// constant of the call: it has no tangent.
template <bool GYRO>
__device__ __forceinline__ void euler_tangent(const Coef& q, const Wrench& w, const Wrench& dw, const Trig& t,
                                              const double (&x)[12], double dt, double* v) {
  const double sph = t.sph, cph = t.cph, sth = t.sth, cth = t.cth, sps = t.sps, cps = t.cps;
  const double Rx = cph * cps * sth + sph * sps;  // ax / bz
  const double Ry = cph * sps * sth - cps * sph;  // ay / bz
  const double Rz = cph * cth;                    // (netz - G) / bz
  const double dphi = v[6], dthe = v[8], dpsi = v[10];
  const double dRx = dphi * (cph * sps - sph * cps * sth) + dthe * (cph * cps * cth) + dpsi * (sph * cps - cph * sps * sth);
  const double dRy = dphi * (-(sph * sps * sth) - cps * cph) + dthe * (cph * sps * cth) + dpsi * (cph * cps * sth + sps * sph);
  const double dRz = dphi * (-(sph * cth)) + dthe * (-(cph * sth));
  const double p = x[7], th = x[9], ps = x[11];  // angular rates before the call
  const double vp = v[7], vt = v[9], vs = v[11];
  double d7 = q.c_dphi * (vs * th + ps * vt) + dw.aphi;
  double d9s = q.c_dthe * (vs * p + ps * vp) + dw.athe;
  if constexpr (GYRO) {
    d7 -= q.g_phi * (vt * w.om + th * dw.om);
    d9s += q.g_the * (vp * w.om + p * dw.om);
  }
  const double d11 = q.c_dpsi * (vt * p + th * vp) + dw.apsi;
  v[0] += dt * v[1];
  v[2] += dt * v[3];
  v[4] += dt * v[5];
  v[1] += dt * (dw.bz * Rx + w.bz * dRx);
  v[3] += dt * (dw.bz * Ry + w.bz * dRy);
  v[5] += dt * (dw.bz * Rz + w.bz * dRz);
  v[6] += dt * vp;
  v[8] += dt * vt;
  v[10] += dt * vs;
  v[7] += dt * d7;
  v[9] -= dt * d9s;
  v[11] += dt * d11;
}

// What the primal of one step needs besides the state: the evaluation point of one env.
struct JacPoint {
  double x[12];
  int fs;           // flight status before the step
  bool active;      // the physics runs: not LANDED at the start (task.py:86-87) and no NEXT_STEP reset pending
  double px, py, pz;  // the pending perturbation, doubled (2 F / M), -0.0 when none
};

// Branch bits (include/copterstep.h: CS_JAC_*)
enum {
  kJacIntegrated = 1, kJacLanded = 2, kJacContact = 4, kJacLeveling = 8, kJacCrashed = 16, kJacReset = 32,
  kJacClipped = 64
};

// The primal of `nsub` setMotors calls -- the arithmetic of physics_call() (dev_physics.h), call by call, with the
// perturbation in the first call only (physics_substeps) -- and kJacDirs tangents carried along.  Returns the branch
// bits of the calls; x ends as the state after the physics.
template <bool FULL, bool GYRO>
__device__ __forceinline__ uint32_t jacobian_block(const DevConst& c, const Coef& q, const Wrench& w,
                                                   const Wrench (&dw)[kJacDirs], const JacPoint& pt, double (&x)[12],
                                                   double (&v)[kJacDirs][12]) {
  uint32_t bits = 0u;
  int fs = pt.fs;
  double px = pt.px, py = pt.py, pz = pt.pz;
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = pt.x[k];
#pragma clang loop unroll(disable)
  for (int sub = 0; sub < c.nsub; ++sub) {
    Trig t;
    sincos_roll_pitch<FULL, false>(c, x[6], x[8], t);
    sincos_yaw<FULL, false>(c, x[10], t);
    double ax, ay, netz;
    thrust_ned(q, w.bz, t, ax, ay, netz);
    CallPlan p = plan_call(c, fs, netz, x[4], x[5], x[3], x[6]);
    if (!pt.active) p = CallPlan{false, false, false, fs};
    if (pt.active && fs == CS_STATUS_CRASHED) bits |= kJacCrashed;
    bits |= (p.integ ? kJacIntegrated : 0u) | (p.contact ? kJacContact : 0u) | (p.leveling ? kJacLeveling : 0u);
    const double dt = p.integ ? c.dt : 0.0;
    // tangents first: they read the state before the call.  Branch-free, as the primal: a call that does not
    // integrate has dt = 0 (identity rows), and leveling zeroes the phi, theta rows (:174-175)
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d) {
      euler_tangent<GYRO>(q, w, dw[d], t, x, dt, v[d]);
      v[d][6] = p.leveling ? 0.0 : v[d][6];
      v[d][8] = p.leveling ? 0.0 : v[d][8];
    }
    euler_translation(dt, ax, ay, netz, px, py, pz, x);
    euler_rotation<GYRO>(q, w, dt, p.leveling, x + 6);
    fs = p.fs_next;
    px = py = pz = -0.0;
  }
  return bits;
}

// Gradient of the Lander shaping potential (lander.py:48-57) at x: -xyz_pen * x_k / |x[0..5]| on the six
// translational slots, -yaw_pen * (psi, dpsi) / |(psi, dpsi)| on slots 10, 11; the derivative of sqrt at 0 is taken
// as 0, and the |dz| > dz_max penalty is a constant.
__device__ __forceinline__ void shaping_gradient(const DevConst& c, const double (&x)[12], double (&g)[12]) {
  double s6 = x[0] * x[0];
#pragma unroll
  for (int k = 1; k < 6; ++k) s6 = fma(x[k], x[k], s6);
  const double r6 = sqrt(s6), r2 = sqrt(fma(x[11], x[11], x[10] * x[10]));
  const double f6 = r6 > 0.0 ? -c.xyz_pen / r6 : 0.0;
  const double f2 = r2 > 0.0 ? -c.yaw_pen / r2 : 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) g[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) g[k] = f6 * x[k];
  g[10] = f2 * x[10];
  g[11] = f2 * x[11];
}

// One wavefront's [64 envs][12 rows][width] slab of the LDS, written to the env-major output `dst` ([N][12][ncols]
// elements, the slab's columns at c0 ..) with lane-consecutive elements: consecutive lanes write consecutive
// addresses within an env's row piece, so one store instruction covers 32 row pieces of 16 bytes (float64) that lie
// within 3 KiB, instead of 64 rows 1 KiB apart as per-lane stores would -- and the pieces of one env row, written by
// the blocks of one wavefront microseconds apart, meet in the L2 before it writes the line back.
template <class OUT, int WIDTH, int ROWS>
__device__ __forceinline__ void store_slab(OUT* dst, const double* slab, int lane, uint32_t env0, uint32_t n,
                                           int ncols, int c0) {
  constexpr int kPer = ROWS * WIDTH;
  constexpr int kTotal = kWave * kPer;
  // (not unrolled: unrolled, the compiler hoists every iteration's address arithmetic out of the block loop and spills)
#pragma clang loop unroll(disable)
  for (int k = 0; k < (kTotal + kWave - 1) / kWave; ++k) {
    const int v = k * kWave + lane;
    if (kTotal % kWave != 0 && v >= kTotal) break;
    const int e = v / kPer, rem = v - e * kPer, r = rem / WIDTH, cc = rem - r * WIDTH;
    if (env0 + (uint32_t)e < n)
      dst[(size_t)(env0 + (uint32_t)e) * (size_t)(ROWS * ncols) + (size_t)(r * ncols + c0 + cc)] =
          (OUT)slab[(e * ROWS + r) * kJacDirs + cc];
  }
}

}  // namespace
}  // namespace cs
