// rollout_tangent.h -- forward-mode (tangent) rules of a K-step rollout: the forward derivative of fold_vehicle's closed
// form (the transpose partner of unfold_vehicle_kernel, copterstep_rollout_grad.hip) and the tangent of one
// _Task.step(), whose transpose is rollout_step.h's step_adjoint term for term (dynamics/__init__.py:114-197, :249-302;
// envs/task.py:77-137; envs/lander.py:46-74).  Device code of copterstep_jvp.hip (included there, inside its
// floating-point-contraction pragma, after jacobian_tangents.h and rollout_step.h); not a stand-alone header.
// DESIGN.md section 26.
//
// The directions go in blocks of kJacDirs (jacobian_tangents.h: the widest block that does not spill), the primal of a
// step is recomputed from its start state for every block, call by call, as jacobian_block and step_adjoint recompute
// it.  PARAM builds (tangents of the vehicle and of the pending force) read the block's coefficient tangents from
// lane-private LDS columns -- row j of Coef for direction d at tc[(d * kCoefRows + j) * kBlock] -- where each term
// arises, as the adjoint keeps its accumulators (rollout_adjoint.h); the plain build carries none.
#pragma once

namespace cs {
namespace {

constexpr double kPiTan = 3.141592653589793238462643383279502884;

// The forward derivative of fold_vehicle (copterstep_api.hip; fold_vehicle_kernel) at the raw column r, in the raw
// direction t: the tangents of Coef's 11 rows.  Rows that do not enter the configuration contribute exactly 0: B under
// the lift law, rho and C_L under the B law, Jr without the rotor-gyro term.
__device__ __forceinline__ void fold_tangent(const double (&r)[12], const double (&t)[12], int lift, int gyro,
                                             double (&tc)[kCoefRows]) {
  const double B = r[0], D = r[1], M = r[2], L = r[3], Ix = r[4], Iy = r[5], Iz = r[6], Jr = r[7], maxrpm = r[8],
               rho = r[10], C_L = r[11];
  const double ws = maxrpm * kPiTan / 30.0;
  const double ws2 = ws * ws;
  const double t_ws = t[8] * (kPiTan / 30.0);
  const double t_ws2 = 2.0 * ws * t_ws;
  double kthrust, kroll, t_kthrust, t_kroll;
  if (lift) {  // kthrust = kroll = KL = 0.025 rho C_L L^3 ws2
    const double l2 = (L / 2.0) * (L / 2.0);
    const double base = 0.5 * (0.05 * L * 4.0) * l2;
    kthrust = kroll = base * rho * C_L * ws2;
    t_kthrust = t_kroll = ((base * C_L * ws2) * t[10] + (base * rho * ws2) * t[11]) +
                          ((0.075 * L * L * rho * C_L * ws2) * t[3] + (base * rho * C_L) * t_ws2);
  } else {  // kthrust = B ws2, kroll = L B ws2
    kthrust = B * ws2;
    kroll = L * B * ws2;
    t_kthrust = ws2 * t[0] + B * t_ws2;
    t_kroll = ((B * ws2) * t[3] + (L * ws2) * t[0]) + (L * B) * t_ws2;
  }
  tc[0] = -t_kthrust / M + (kthrust / (M * M)) * t[2];
  tc[1] = t_kroll / Ix - (kroll / (Ix * Ix)) * t[4];
  tc[2] = t_kroll / Iy - (kroll / (Iy * Iy)) * t[5];
  tc[3] = ((ws2 / Iz) * t[1] + (D / Iz) * t_ws2) - ((D * ws2) / (Iz * Iz)) * t[6];
  tc[4] = t[9];
  tc[5] = (t[5] - t[6]) / Ix - ((Iy - Iz) / (Ix * Ix)) * t[4];
  tc[6] = (t[6] - t[4]) / Iy - ((Iz - Ix) / (Iy * Iy)) * t[5];
  tc[7] = (t[4] - t[5]) / Iz - ((Ix - Iy) / (Iz * Iz)) * t[6];
  tc[8] = -(2.0 / (M * M)) * t[2];
  tc[9] = tc[10] = 0.0;
  if (gyro) {
    tc[9] = ((ws / Ix) * t[7] + (Jr / Ix) * t_ws) - ((Jr * ws) / (Ix * Ix)) * t[4];
    tc[10] = ((ws / Iy) * t[7] + (Jr / Iy) * t_ws) - ((Jr * ws) / (Iy * Iy)) * t[5];
  }
}

// The tangent of one step in kJacDirs directions.  On entry v[d] is the tangent of the step's start state in.x, on
// exit that of the state after the step (the storage rounding is straight-through); tr[d] = the tangent of its
// reward.  ta[d] = the tangent of the action row (the task's A columns; the clip's derivative and _get_motors' fan-out
// are applied here), tp[d] = the tangent of call 0's perturbation (px0, py0, pz0).  resetting, prev_diff, prev_none: as
// step_adjoint takes them.  PARAM: tc = the lane's coefficient tangents in the LDS (above).
template <int TASK, int MODE, bool GYRO, bool PARAM>
__device__ __forceinline__ void step_tangent(const DevConst& c, const Coef& q, const StepIn& in, double px0, double py0,
                                             double pz0, const double (&tp)[kJacDirs][3], bool resetting,
                                             bool prev_diff, bool prev_none, const double (&ta)[kJacDirs][4],
                                             const double* tc, double (&v)[kJacDirs][12], double (&tr)[kJacDirs]) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  const float araw[4] = {in.act.x, in.act.y, in.act.z, in.act.w};
  float mf[4];
  double m[4], clipd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mf[j] = clip01(araw[j]);
    m[j] = (double)mf[j];
    clipd[j] = (araw[j] >= 0.f && araw[j] <= 1.f) ? 1.0 : 0.0;
  }
  Wrench w;  // the wrench the step applied (its derivative below is the float64 law's, as in cs_step_jacobian)
  if (c.act_f32) {
    w = motor_model_f32(c, mf[0], mf[1], mf[2], mf[3]);
  } else {
    w.bz = thrust_model(q, mf[0], mf[1], mf[2], mf[3]);
    torque_model(q, mf[0], mf[1], mf[2], mf[3], w);
  }
  Wrench dw[kJacDirs];
#pragma unroll
  for (int d = 0; d < kJacDirs; ++d) {
    double dm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = A == 4 ? j : A == 2 ? ((j == 1 || j == 2) ? 1 : 0) : 0;
      dm[j] = clipd[j] * ta[d][col];
    }
    dw[d] = wrench_tangent(q, m, dm);
    if constexpr (PARAM) {  // bz = k_thrust sum(m^2), aphi = k_roll (...), ...: the gains' tangents times the signed sums
      const double q0 = m[0] * m[0], q1 = m[1] * m[1], q2 = m[2] * m[2], q3 = m[3] * m[3];
      const double* t = tc + d * kCoefRows * kBlock;
      dw[d].bz += t[0 * kBlock] * (((q0 + q1) + q2) + q3);
      dw[d].aphi += t[1 * kBlock] * ((q1 + q2) - (q0 + q3));
      dw[d].athe += t[2 * kBlock] * ((q1 + q3) - (q0 + q2));
      dw[d].apsi += t[3 * kBlock] * ((q0 + q1) - (q2 + q3));
    }
  }
  // reward = shaping(x') - shaping(start): the start's half of the telescoping term, taken before v moves on
  double pre[kJacDirs] = {};
  if constexpr (task_is_lander(TASK)) {
    if (prev_diff) {
      double gs[12];
      shaping_gradient(c, in.x, gs);
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) acc = fma(gs[k], v[d][k], acc);
        pre[d] = acc;
      }
    }
  }

  // ---- the calls: the primal of physics_call(), the tangents first (they read the state before the call) ----
  const bool active = !resetting && in.fs != CS_STATUS_LANDED;
  int fs = in.fs;
  double px = px0, py = py0, pz = pz0;
  double x[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = in.x[k];
#pragma clang loop unroll(disable)
  for (int sub = 0; sub < c.nsub; ++sub) {
    Trig t;
    sincos_roll_pitch<FULL, false>(c, x[6], x[8], t);
    sincos_yaw<FULL, false>(c, x[10], t);
    double ax, ay, netz;
    thrust_ned(q, w.bz, t, ax, ay, netz);
    CallPlan p = plan_call(c, fs, netz, x[4], x[5], x[3], x[6]);
    if (!active) p = CallPlan{false, false, false, fs};
    const double dt = p.integ ? c.dt : 0.0;
    const double dt0 = sub == 0 ? dt : 0.0;  // the perturbation enters the first call only
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d) {
      euler_tangent<GYRO>(q, w, dw[d], t, x, dt, v[d]);
      v[d][1] += dt0 * tp[d][0];
      v[d][3] += dt0 * tp[d][1];
      v[d][5] += dt0 * tp[d][2];
      if constexpr (PARAM) {  // netz = bz Rz + G; d7 = c_dphi ps th + ..., d9s = c_dthe ps p + ..., d11 = c_dpsi th p
        const double* tcd = tc + d * kCoefRows * kBlock;
        const double pr = x[7], th = x[9], ps = x[11];
        v[d][5] += dt * tcd[4 * kBlock];
        double e7 = (ps * th) * tcd[5 * kBlock];
        double e9 = (ps * pr) * tcd[6 * kBlock];
        if constexpr (GYRO) {
          e7 -= (th * w.om) * tcd[9 * kBlock];
          e9 += (pr * w.om) * tcd[10 * kBlock];
        }
        v[d][7] += dt * e7;
        v[d][9] -= dt * e9;
        v[d][11] += dt * ((th * pr) * tcd[7 * kBlock]);
      }
      v[d][6] = p.leveling ? 0.0 : v[d][6];
      v[d][8] = p.leveling ? 0.0 : v[d][8];
    }
    euler_translation(dt, ax, ay, netz, px, py, pz, x);
    euler_rotation<GYRO>(q, w, dt, p.leveling, x + 6);
    fs = p.fs_next;
    px = py = pz = -0.0;
  }

  // ---- reward: grad shaping(x') . v' - grad shaping(start) . v; none under a tilt (tested on the stored words), a
  //      None, a reset, or a Hover task ----
#pragma unroll
  for (int d = 0; d < kJacDirs; ++d) tr[d] = 0.0;
  if constexpr (task_is_lander(TASK)) {
    const bool tilt = !test_oob(c, round_stored<MODE>(x[0]), round_stored<MODE>(x[2])) &&
                      test_tilt(c, round_stored<MODE>(x[6]), round_stored<MODE>(x[8]));
    if (!resetting && !prev_none && !tilt) {
      double gs[12];
      shaping_gradient(c, x, gs);
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 12; ++k) acc = fma(gs[k], v[d][k], acc);
        tr[d] = acc - pre[d];
      }
    }
  }
  if (resetting) {  // the step replaces the state: nothing of the start survives it
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d)
#pragma unroll
      for (int k = 0; k < 12; ++k) v[d][k] = 0.0;
  }
}

// Row `row` of a [.., N, 12] tangent output in OUT (double, or float: the float64 values rounded): a whole wavefront's
// 64 rows through the LDS (xrow, 6 KiB) with 16 B per lane and store, as store_x_row; a partial one lane by lane.
template <class OUT>
__device__ __forceinline__ void store_t_row(double* xrow, OUT* dst, size_t row, const RowOut& r,
                                            const double (&x)[12]) {
  if (r.whole) {
#pragma unroll
    for (int j = 0; j < 12; j += 2)
      *reinterpret_cast<double2*>(xrow + r.lane * 12 + j) = make_double2(x[j], x[j + 1]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    OUT* base = dst + (row + r.env0) * 12;
    if constexpr (sizeof(OUT) == 8) {
      const double2* src = reinterpret_cast<const double2*>(xrow);
      double2* d2 = reinterpret_cast<double2*>(base);
#pragma unroll
      for (int v = 0; v < 6; ++v) d2[v * kWave + r.lane] = src[v * kWave + r.lane];
    } else {
      float4* d4 = reinterpret_cast<float4*>(base);
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        const double2* src = reinterpret_cast<const double2*>(xrow + (v * kWave + r.lane) * 4);
        const double2 a = src[0], b = src[1];
        d4[v * kWave + r.lane] = make_float4((float)a.x, (float)a.y, (float)b.x, (float)b.y);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else if (r.valid) {
    OUT* d = dst + (row + r.i) * 12;
#pragma unroll
    for (int j = 0; j < 12; ++j) d[j] = (OUT)x[j];
  }
}

}  // namespace
}  // namespace cs
