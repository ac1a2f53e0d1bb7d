// rollout_step.h -- the pieces the rollout kernels share.  For the five forwards whose states must be
// cs_rollout_states' bit for bit (rollout_forward in rollout_sweep.h, the closed-loop forward of
// copterstep_rollout_mlp.hip, the cost kernels of copterstep_rollout_mppi.hip and copterstep_rollout_mppi_smooth.hip,
// the population kernel of copterstep_rollout_es.hip): the explicit start point, the choice between it and the stored
// env (rollout_start), one _Task.step() with auto-reset disabled, and the perturbation of the step after it
// (next_perturbation).  For the backwards (rollout_vjp_sweep, copterstep_rollout_lqr.hip, which decode the start
// themselves): the tape loads and cotangents, and the adjoint of one step.  Device code of those translation units
// (included inside their floating-point-contraction pragma, after rollout_adjoint.h); not a stand-alone header.
// DESIGN.md sections 10, 12 and 14 to 16.
#pragma once

#ifdef CS_DEBUG_ROLLOUT  // debug build (make DEFS=-DCS_DEBUG_ROLLOUT exp NAME=debug): the recompute is checked
#include <cassert>
#endif

namespace cs {
namespace {

// The caller's explicit start point of env i (cs_rollout_io.start_*): x, status, pending force, prev_shaping.  Without a
// prev_shaping it is shaping(x0), rounded to a stored word as step() stores it (differentiated by the backward).
template <int TASK, int MODE>
__device__ __forceinline__ void explicit_start(const DevConst& c, const Coef& q, const cs_rollout_io& io, uint32_t i,
                                               uint32_t n, bool valid, double (&x)[12], int& fs, bool& pend,
                                               double& px, double& py, double& pz, double& prev_sh) {
  using T = typename ModeOf<MODE>::T;
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = valid ? io.start_x_dev[(size_t)k * n + i] : 0.0;
  fs = valid ? (int)io.start_status_dev[i] : CS_STATUS_AIRBORNE;
  pend = io.start_force_dev != nullptr;
  px = py = pz = -0.0;
  if (pend && valid) {
    px = io.start_force_dev[i] * q.two_inv_M;
    py = io.start_force_dev[(size_t)n + i] * q.two_inv_M;
    pz = io.start_force_dev[(size_t)2 * n + i] * q.two_inv_M;
  }
  if (io.start_prev_shaping_dev != nullptr) {
    prev_sh = valid ? io.start_prev_shaping_dev[i] : 0.0;
  } else if constexpr (task_is_lander(TASK)) {
    prev_sh = (double)(T)lander_shaping(c, x);
  } else {
    prev_sh = 0.0;
  }
}

// Where a forward rollout starts, after the caller's unpack_env / resolve_episode of the stored env: io's explicit start
// point (no reset is pending there), else the stored env with its pending perturbation.  The one definition of the five
// forward kernels, whose states the tests compare bit for bit.
template <int TASK, int MODE, class TILE>
__device__ __forceinline__ void rollout_start(const DevConst& c, const Coef& q, const cs_rollout_io& io,
                                              const TILE& tile, uint32_t i, uint32_t n, bool valid, Env<MODE>& e,
                                              double& px, double& py, double& pz) {
  if (io.start_x_dev != nullptr) {
    explicit_start<TASK, MODE>(c, q, io, i, n, valid, e.x, e.fs, e.pend, px, py, pz, e.prev_sh);
    e.reset_pending = false;
  } else {
    pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
  }
}

// One _Task.step() with auto-reset disabled, from the pieces advance() (dev_task.h) is built from, in its order: the
// clip and motor law, physics_substeps (the K-step form, IN_LOOP), the stored-word rounding, judge_step and the
// prev_shaping / step counter updates, and a NEXT_STEP reset already pending (only ever in the first step).  The
// perturbation is passed in (px, py, pz); e.pend says on return whether it is still pending.
template <int TASK, int MODE>
__device__ __forceinline__ void rollout_step(const DevConst& c, const Coef& q, Env<MODE>& e, const float4 act,
                                             double px, double py, double pz, double& reward, bool& term,
                                             bool& trunc) {
  using T = typename ModeOf<MODE>::T;
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  const bool resetting = e.reset_pending;
  const int status0 = e.fs;
  if (!resetting && status0 != CS_STATUS_LANDED) {
    const float a0 = clip01(act.x), a1 = clip01(act.y), a2 = clip01(act.z), a3 = clip01(act.w);
    Wrench w;
    if (c.act_f32) {
      w = motor_model_f32(c, a0, a1, a2, a3);
    } else {
      w.bz = thrust_model(q, a0, a1, a2, a3);
      torque_model(q, a0, a1, a2, a3, w);
    }
    if (c.gyro) {
      physics_substeps<FULL, true, false, true>(c, q, w, e.x, e.fs, e.pend, px, py, pz);
    } else {
      physics_substeps<FULL, false, false, true>(c, q, w, e.x, e.fs, e.pend, px, py, pz);
    }
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) e.x[k] = round_stored<MODE>(e.x[k]);
  reward = 0.0;
  term = trunc = false;
  if (!resetting) {
    double sh = 0.0;
    if constexpr (task_is_lander(TASK)) sh = lander_shaping(c, e.x);
    const Verdict v = judge_step<TASK>(c, c.tl_trunc != 0, status0, e.steps, sh, e.prev_sh,
                                       test_inside(c, e.x[0], e.x[2]), test_oob(c, e.x[0], e.x[2]),
                                       test_tilt(c, e.x[6], e.x[8]));
    if constexpr (task_is_lander(TASK)) e.prev_sh = (double)(T)sh;
    reward = v.reward;
    term = v.term;
    trunc = v.trunc;
    e.steps = min(e.steps + 1, (int)c.steps_mask);
  } else {  // the masked reset of advance(): fresh state, the next episode (its perturbation pending), steps = 1
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const T w0 = (k == 4) ? (T)c.z0 : (T)0;
      e.x[k] = (double)w0;
    }
    next_episode<MODE, true>(e);
    e.fs = c.status0;
    e.pend = true;
    e.expl = false;
    e.steps = 1;
    e.prev_sh = c.reset_shaping;
    e.reset_pending = false;
  }
}

// The perturbation of the step after a rollout_step: the new episode's where that step was the reset (`resetting`: the
// Philox draw step() would make), none once the pending one is consumed.  With rollout_start, the forward kernels' one
// definition.
template <int MODE, class TILE>
__device__ __forceinline__ void next_perturbation(const DevConst& c, const Coef& q, const TILE& tile, uint32_t i,
                                                  bool resetting, const Env<MODE>& e, double& px, double& py,
                                                  double& pz) {
  if (resetting) {
    pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
  } else if (!e.pend) {
    px = py = pz = -0.0;
  }
}

// What the backward recomputes one step from: its start state and status, and its action.
struct StepIn {
  double x[12];
  int fs;
  float4 act;
};

// lam += the cotangent of step k's x row; returns that of its reward
__device__ __forceinline__ double add_cotangents(const cs_rollout_io& io, size_t row, uint32_t i, double (&lam)[12]) {
  if (io.gx_dev != nullptr) {
    const double2* g = reinterpret_cast<const double2*>(io.gx_dev + (row + i) * 12);
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const double2 v = g[j];
      lam[2 * j] += v.x;
      lam[2 * j + 1] += v.y;
    }
  }
  return io.gr_dev != nullptr ? io.gr_dev[row + i] : 0.0;
}

// step k (0-based) >= 1: its start is the tape's row k - 1
template <int TASK>
__device__ __forceinline__ void load_tape_step(const cs_rollout_io& io, uint32_t n, uint32_t i, int k, StepIn& in) {
  const size_t prev = (size_t)(k - 1) * n;
  const double2* xr = reinterpret_cast<const double2*>(io.x_dev + (prev + i) * 12);
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const double2 v = xr[j];
    in.x[2 * j] = v.x;
    in.x[2 * j + 1] = v.y;
  }
  in.fs = (int)io.status_dev[prev + i];
  in.act = load_action_at<TASK>(io.actions_dev + ((size_t)k * n + i) * task_act_dim(TASK));
}

// The adjoint of one step.  On entry `lam` is the adjoint of the state after the step (the cotangent of its x row
// included), on exit that of its start state; ga = the gradient of its action row.  The step's primal is recomputed
// from its start with the arithmetic of physics_call() (as jacobian_block does), call by call:
//   resetting  a NEXT_STEP reset pending (first step of a stored start only): the step replaces the state, all zero
//   prev_diff  prev_shaping is shaping(start) and differentiated (every step but the first; the first of an explicit
//              start without a prev_shaping), prev_none = upstream's None (reward 0)
//   PARAM      (cs_rollout_vjp_ex) the step's coefficient adjoints are added to the lane's accumulators `acc`: the
//              per-call terms and the motor law's (mw . the sums of squared motor values); the adjoint of call 0's
//              perturbation (px, py, pz) is stored to its rows kAccPe ..
template <int TASK, int MODE, bool GYRO, bool PARAM = false>
__device__ __forceinline__ void step_adjoint(const DevConst& c, const Coef& q, const StepIn& in, double gr, double px0,
                                             double py0, double pz0, bool resetting, bool prev_diff, bool prev_none,
                                             const double* tape_next, double (&lam)[12], double (&ga)[4],
                                             double* acc = nullptr) {
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
  const bool active = !resetting && in.fs != CS_STATUS_LANDED;
  const int nsub = c.nsub;

  // the primal of `upto` calls from the step's start (the perturbation in the first), then the sin / cos and the plan
  // of call `upto` at the state reached: x = the start of that call
  auto primal_to = [&](int upto, double (&x)[12], Trig& t, CallPlan& p, double& ax, double& ay, double& netz) {
    int fs = in.fs;
    double px = px0, py = py0, pz = pz0;
#pragma unroll
    for (int k = 0; k < 12; ++k) x[k] = in.x[k];
#pragma clang loop unroll(disable)
    for (int sub = 0;; ++sub) {
      sincos_roll_pitch<FULL, false>(c, x[6], x[8], t);
      sincos_yaw<FULL, false>(c, x[10], t);
      thrust_ned(q, w.bz, t, ax, ay, netz);
      p = plan_call(c, fs, netz, x[4], x[5], x[3], x[6]);
      if (!active) p = CallPlan{false, false, false, fs};
      if (sub == upto) break;
      const double dt = p.integ ? c.dt : 0.0;
      euler_translation(dt, ax, ay, netz, px, py, pz, x);
      euler_rotation<GYRO>(q, w, dt, p.leveling, x + 6);
      fs = p.fs_next;
      px = py = pz = -0.0;
    }
  };

  // ---- the last call: its sin / cos, plan and angular rates (what its adjoint reads), then x' in place ----
  double x[12];
  Trig t;
  CallPlan p;
  double ax, ay, netz;
  primal_to(nsub - 1, x, t, p, ax, ay, netz);
  const double dtl = p.integ ? c.dt : 0.0;
  const bool levl = p.leveling;
  double rates[12];  // (only slots 7, 9, 11 are read)
  rates[7] = x[7];
  rates[9] = x[9];
  rates[11] = x[11];
  euler_translation(dtl, ax, ay, netz, nsub == 1 ? px0 : -0.0, nsub == 1 ? py0 : -0.0, nsub == 1 ? pz0 : -0.0, x);
  euler_rotation<GYRO>(q, w, dtl, levl, x + 6);
  double (&xn)[12] = x;
#ifdef CS_DEBUG_ROLLOUT
  if (tape_next != nullptr) {
    for (int k = 0; k < 12; ++k) assert(round_stored<MODE>(xn[k]) == tape_next[k] || xn[k] != xn[k]);
  }
#endif
  // ---- reward: grad shaping(x'), and -grad shaping(start) through prev_shaping; none under a tilt (reward =
  //      -penalty, tested on the stored words), a None, a reset, or a Hover task ----
  bool rew = false;
  if constexpr (task_is_lander(TASK)) {
    const bool tilt = !test_oob(c, round_stored<MODE>(xn[0]), round_stored<MODE>(xn[2])) &&
                      test_tilt(c, round_stored<MODE>(xn[6]), round_stored<MODE>(xn[8]));
    rew = !resetting && !prev_none && !tilt;
    if (rew) {
      double gs[12];
      shaping_gradient(c, xn, gs);
#pragma unroll
      for (int k = 0; k < 12; ++k) lam[k] = fma(gr, gs[k], lam[k]);
    }
  }

  // ---- the calls in reverse: call `sub` at its start state, recomputed from the step's start ----
  Wrench mw{0.0, 0.0, 0.0, 0.0, 0.0};
  if constexpr (PARAM) {
    if (nsub == 1) {  // x[1] += dt (ax + px), ...: the perturbation's adjoint is dt x the velocity adjoint after the call
      acc[(kAccPe + 0) * kBlock] = dtl * lam[1];
      acc[(kAccPe + 1) * kBlock] = dtl * lam[3];
      acc[(kAccPe + 2) * kBlock] = dtl * lam[5];
    }
  }
  euler_adjoint<GYRO, PARAM>(q, w, t, rates, dtl, levl, lam, mw, acc);
#pragma clang loop unroll(disable)
  for (int sub = nsub - 2; sub >= 0; --sub) {
    primal_to(sub, x, t, p, ax, ay, netz);
    const double dts = p.integ ? c.dt : 0.0;
    if constexpr (PARAM) {
      if (sub == 0) {
        acc[(kAccPe + 0) * kBlock] = dts * lam[1];
        acc[(kAccPe + 1) * kBlock] = dts * lam[3];
        acc[(kAccPe + 2) * kBlock] = dts * lam[5];
      }
    }
    euler_adjoint<GYRO, PARAM>(q, w, t, x, dts, p.leveling, lam, mw, acc);
  }
  if (rew && prev_diff) {  // reward = shaping(x') - shaping(start): the telescoping term
    double gs[12];
    shaping_gradient(c, in.x, gs);
#pragma unroll
    for (int k = 0; k < 12; ++k) lam[k] = fma(-gr, gs[k], lam[k]);
  }
  motor_adjoint<A>(q, m, clipd, mw, ga);
  if constexpr (PARAM) {  // bz = k_thrust sum(m^2), aphi = k_roll (...), ... (thrust_model, torque_model)
    const double q0 = m[0] * m[0], q1 = m[1] * m[1], q2 = m[2] * m[2], q3 = m[3] * m[3];
    acc[0 * kBlock] += mw.bz * (((q0 + q1) + q2) + q3);
    acc[1 * kBlock] += mw.aphi * ((q1 + q2) - (q0 + q3));
    acc[2 * kBlock] += mw.athe * ((q1 + q3) - (q0 + q2));
    acc[3 * kBlock] += mw.apsi * ((q0 + q1) - (q2 + q3));
  }
  if (resetting) {
#pragma unroll
    for (int k = 0; k < 12; ++k) lam[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) ga[k] = 0.0;
  }
}

template <class OUT, int A>
__device__ __forceinline__ void store_ga(void* dst, size_t row, uint32_t i, const double (&ga)[4]) {
  OUT* d = reinterpret_cast<OUT*>(dst) + (row + i) * A;
#pragma unroll
  for (int j = 0; j < A; ++j) d[j] = (OUT)ga[j];
}

}  // namespace
}  // namespace cs
