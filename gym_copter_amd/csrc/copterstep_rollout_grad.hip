// copterstep_rollout_grad.hip -- differentiable K-step rollouts on gfx950 (cs_rollout_states / cs_rollout_vjp,
// include/copterstep.h): the states, rewards and flags of K steps with auto-reset disabled, and the reverse-mode gradient
// of a loss on them with respect to the actions and the start state.  Nothing of the env state is written.
//
// Upstream lines differentiated (paths relative to the upstream checkout):
//   dynamics/__init__.py:114-197 (setMotors), :249-290 (state derivative), :292-302 (_bodyZToInertial),
//   envs/task.py:77-137 (step: the clip of :91, the LANDED skip of :86-87), envs/lander.py:46-74 (reward, whose
//   prev_shaping makes reward_k a function of x_{k-1} as well as of x_k).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  The forward kernel keeps the env in
// registers for K steps (the pieces of advance(): physics_substeps, the stored-word rounding, judge_step) and writes
// each step's state row through the LDS.  The backward kernel sweeps k = K .. 1 with the adjoint in registers; each
// step's primal is recomputed from the caller's tape (the forward's x and status rows), the substep start states from
// the step's start (O(substeps^2) calls).  The pieces the closed-loop rollouts share are in rollout_step.h.  DESIGN.md
// section 10.
#include <string>

#include "copterstep_jacobian.h"

// the primal must round as the step kernels do (copterstep_kernels.hip): the backward's recomputed primal is the tape
// bit for bit, or its branch decisions could differ from the forward's
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"

namespace cs {
namespace {

template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void rollout_states_kernel(const DevConst c, const DevState s,
                                                                const cs_rollout_io io) {
  constexpr int A = task_act_dim(TASK);
  __shared__ __attribute__((aligned(16))) double xrow[kBlock * 12];  // 6 KiB: the wavefront's state rows of a step
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const bool valid = i < n;
  const bool whole = env0 + (uint32_t)kWave <= n;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, valid ? i : 0u);
  // the stored env, decoded as step_many_kernel decodes it (its counters are the rollout's in both start forms)
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);
  Env<MODE> e;
  unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
  resolve_episode<MODE>(c, tile, e);
  double px, py, pz;
  if (io.start_x_dev != nullptr) {
    explicit_start<TASK, MODE>(c, q, io, i, n, valid, e.x, e.fs, e.pend, px, py, pz, e.prev_sh);
    e.reset_pending = false;
  } else {
    pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
  }

  const float* act_lane = io.actions_dev + (size_t)(valid ? i : 0u) * A;
  const size_t act_step = (size_t)n * A;
#pragma clang loop unroll(disable)
  for (int k = 0; k < io.num_steps; ++k) {
    const float4 act = load_action_at<TASK>(act_lane);
    act_lane += act_step;
    const bool resetting = e.reset_pending;
    double reward;
    bool term, trunc;
    rollout_step<TASK, MODE>(c, q, e, act, px, py, pz, reward, term, trunc);
    if (resetting) {  // the new episode's perturbation (the Philox draw step() would make)
      pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
    } else if (!e.pend) {
      px = py = pz = -0.0;
    }

    const size_t row = (size_t)k * n;  // 64-bit: K x N x 12 doubles pass 4 GiB at 1 M envs
    if (io.x_dev != nullptr) {
      if (whole) {  // 64 rows of 96 B through the LDS: six 1 KiB stores of 16 B per lane
#pragma unroll
        for (int j = 0; j < 12; j += 2)
          *reinterpret_cast<double2*>(xrow + lane * 12 + j) = make_double2(e.x[j], e.x[j + 1]);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const double2* src = reinterpret_cast<const double2*>(xrow);
        double2* dst = reinterpret_cast<double2*>(io.x_dev + (row + env0) * 12);
#pragma unroll
        for (int v = 0; v < 6; ++v) dst[v * kWave + lane] = src[v * kWave + lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      } else if (valid) {
        double* dst = io.x_dev + (row + i) * 12;
#pragma unroll
        for (int j = 0; j < 12; ++j) dst[j] = e.x[j];
      }
    }
    if (valid) {
      if (io.reward_dev != nullptr) io.reward_dev[row + i] = reward;
      if (io.terminated_dev != nullptr) io.terminated_dev[row + i] = term ? 1 : 0;
      if (io.truncated_dev != nullptr) io.truncated_dev[row + i] = trunc ? 1 : 0;
      if (io.status_dev != nullptr) io.status_dev[row + i] = (uint8_t)e.fs;
    }
  }
}

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_vjp_kernel(const DevConst c, const DevState s,
                                                             const cs_rollout_io io) {
  constexpr int A = task_act_dim(TASK);
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const bool valid = i < n;
  const uint32_t ii = valid ? i : 0u;  // (padding lanes recompute env 0's steps and store nothing)
  const int K = io.num_steps;
  const bool f32out = io.out_dtype == CS_JAC_F32;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double lam[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) lam[k] = 0.0;
  double ga[4];

  // ---- steps K-1 .. 2: starts from the tape, the next step's inputs fetched while this one computes ----
  StepIn cur;
  if (K > 1) load_tape_step<TASK>(io, n, ii, K - 1, cur);
#pragma clang loop unroll(disable)
  for (int k = K - 1; k >= 2; --k) {
    StepIn nxt;  // (the earlier step's tape row and action, in flight while this step computes)
    load_tape_step<TASK>(io, n, ii, k - 1, nxt);
    const double gr = add_cotangents(io, (size_t)k * n, ii, lam);
    const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
    tape_next = io.x_dev + ((size_t)k * n + ii) * 12;
#endif
    step_adjoint<TASK, MODE, GYRO>(c, q, cur, gr, -0.0, -0.0, -0.0, false, true, false, tape_next, lam, ga);
    if (valid && io.g_actions_dev != nullptr) {
      if (f32out)
        store_ga<float, A>(io.g_actions_dev, (size_t)k * n, i, ga);
      else
        store_ga<double, A>(io.g_actions_dev, (size_t)k * n, i, ga);
    }
    cur = nxt;
  }

  // ---- step 1 (peeled: the loop's steps have no perturbation) ----
  // A stored-start lane with a NEXT_STEP reset pending resets in step 0, and the new episode's perturbation (the draw
  // step() makes) enters the first call of step 1: its recompute needs it, or its x' is not the tape's.  Every other
  // perturbation is consumed in step 0 or only ever meets calls that do not integrate.
  if (K > 1) {
    double px = -0.0, py = -0.0, pz = -0.0;
    if (io.start_x_dev == nullptr) {
      using TILE = TileIO<MODE>;
      const TILE tile(s, tile_index, lane);
      Env<MODE> e;
      unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
      if (e.reset_pending) {  // (rollout_step's masked reset, then the forward's draw for the new episode)
        resolve_episode<MODE>(c, tile, e);
        next_episode<MODE, true>(e);
        pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, true, false, px, py, pz);
      }
    }
    const double gr = add_cotangents(io, (size_t)n, ii, lam);
    const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
    tape_next = io.x_dev + ((size_t)n + ii) * 12;
#endif
    step_adjoint<TASK, MODE, GYRO>(c, q, cur, gr, px, py, pz, false, true, false, tape_next, lam, ga);
    if (valid && io.g_actions_dev != nullptr) {
      if (f32out)
        store_ga<float, A>(io.g_actions_dev, (size_t)n, i, ga);
      else
        store_ga<double, A>(io.g_actions_dev, (size_t)n, i, ga);
    }
  }

  // ---- step 0: from the start point, decoded as the forward decoded it ----
  StepIn in;
  double px, py, pz;
  bool resetting = false, prev_diff = false, prev_none = false;
  if (io.start_x_dev != nullptr) {
    bool pend;
    double prev_sh;
    explicit_start<TASK, MODE>(c, q, io, i, n, valid, in.x, in.fs, pend, px, py, pz, prev_sh);
    prev_diff = io.start_prev_shaping_dev == nullptr;
    prev_none = prev_sh != prev_sh;
  } else {
    using TILE = TileIO<MODE>;
    const TILE tile(s, tile_index, lane);
    Env<MODE> e;
    unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
    resolve_episode<MODE>(c, tile, e);
    pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
#pragma unroll
    for (int k = 0; k < 12; ++k) in.x[k] = e.x[k];
    in.fs = e.fs;
    resetting = e.reset_pending;
    prev_none = e.prev_sh != e.prev_sh;
  }
  in.act = load_action_at<TASK>(io.actions_dev + (size_t)ii * A);
  const double gr0 = add_cotangents(io, 0, ii, lam);
  const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
  if (!resetting) tape_next = io.x_dev + (size_t)ii * 12;  // (a resetting step is not recomputed: its gradient is 0)
#endif
  step_adjoint<TASK, MODE, GYRO>(c, q, in, gr0, px, py, pz, resetting, prev_diff, prev_none, tape_next, lam, ga);
  if (valid) {
    if (io.g_actions_dev != nullptr) {
      if (f32out)
        store_ga<float, A>(io.g_actions_dev, 0, i, ga);
      else
        store_ga<double, A>(io.g_actions_dev, 0, i, ga);
    }
    if (io.g_x0_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        if (f32out)
          reinterpret_cast<float*>(io.g_x0_dev)[(size_t)k * n + i] = (float)lam[k];
        else
          reinterpret_cast<double*>(io.g_x0_dev)[(size_t)k * n + i] = lam[k];
      }
    }
  }
}

// Where the parameter-gradient backward writes (cs_rollout_vjp_ex): g_coef [kCoefRows, N] float64 (the adjoints of
// Coef's rows, for unfold_vehicle_kernel), g_force [3, N] (newtons; float32 when f32) or nullptr.
struct ParamGradOut {
  double* g_coef;
  void* g_force;
  uint32_t f32;
};

// pending_perturbation() with the force kept: f = the pending force in newtons (0 when none), (px, py, pz) = f two_inv_M
// with the same bits as pending_perturbation's (f x 1.0 is f, and -0.0 x 1.0 is -0.0)
template <int MODE, class TILE>
__device__ __forceinline__ void pending_force(const DevConst& c, const Coef& q, const TILE& tile, uint32_t i,
                                              uint32_t episode, uint32_t ep_far, bool pend, bool expl, double (&f)[3],
                                              double& px, double& py, double& pz) {
  Coef unit = q;
  unit.two_inv_M = 1.0;
  pending_perturbation<MODE, true>(c, unit, tile, i, episode, ep_far, pend, expl, f[0], f[1], f[2]);
  px = f[0] * q.two_inv_M;
  py = f[1] * q.two_inv_M;
  pz = f[2] * q.two_inv_M;
#pragma unroll
  for (int j = 0; j < 3; ++j) f[j] = pend ? f[j] : 0.0;
}

// rollout_vjp_kernel's sweep with the coefficient adjoints (acc = this lane's LDS columns, po = where the coefficient
// and force adjoints go); instantiated with PARAM = true only.  With PARAM = false it is that kernel's sweep, which
// keeps its own text because calling this function from it, though equivalent, changed its instruction schedule
// (profiles/rollout_param_grad_isa.txt).  The two copies must change together: ANY fix to the plain sweep in
// rollout_vjp_kernel must be mirrored here, and the other way round (the bit-identity of g_actions / g_x0 between the
// two, tests/test_gpu_rollout_param_grad.py, catches a copy that drifts).
template <int TASK, int MODE, bool GYRO, bool PARAM>
__device__ __forceinline__ void rollout_vjp_body(const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                                 const ParamGradOut& po, double* acc) {
  constexpr int A = task_act_dim(TASK);
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const bool valid = i < n;
  const uint32_t ii = valid ? i : 0u;  // (padding lanes recompute env 0's steps and store nothing)
  const int K = io.num_steps;
  const bool f32out = io.out_dtype == CS_JAC_F32;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double lam[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) lam[k] = 0.0;
  double ga[4];
  if constexpr (PARAM) {
#pragma unroll
    for (int j = 0; j < 2 * kAccRows; ++j) acc[j * kBlock] = 0.0;
  }

  // ---- steps K-1 .. 2: starts from the tape, the next step's inputs fetched while this one computes ----
  StepIn cur;
  if (K > 1) load_tape_step<TASK>(io, n, ii, K - 1, cur);
#pragma clang loop unroll(disable)
  for (int k = K - 1; k >= 2; --k) {
    StepIn nxt;  // (the earlier step's tape row and action, in flight while this step computes)
    load_tape_step<TASK>(io, n, ii, k - 1, nxt);
    const double gr = add_cotangents(io, (size_t)k * n, ii, lam);
    const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
    tape_next = io.x_dev + ((size_t)k * n + ii) * 12;
#endif
    step_adjoint<TASK, MODE, GYRO, PARAM>(c, q, cur, gr, -0.0, -0.0, -0.0, false, true, false, tape_next, lam, ga,
                                          acc);
    if (valid && io.g_actions_dev != nullptr) {
      if (f32out)
        store_ga<float, A>(io.g_actions_dev, (size_t)k * n, i, ga);
      else
        store_ga<double, A>(io.g_actions_dev, (size_t)k * n, i, ga);
    }
    cur = nxt;
  }

  // ---- step 1 (peeled: the loop's steps have no perturbation) ----
  // A stored-start lane with a NEXT_STEP reset pending resets in step 0, and the new episode's perturbation (the draw
  // step() makes) enters the first call of step 1: its recompute needs it, or its x' is not the tape's.  Every other
  // perturbation is consumed in step 0 or only ever meets calls that do not integrate.
  if (K > 1) {
    double px = -0.0, py = -0.0, pz = -0.0;
    double f1[3] = {0.0, 0.0, 0.0};  // (PARAM) that draw in newtons: px = f1[0] two_inv_M
    if (io.start_x_dev == nullptr) {
      using TILE = TileIO<MODE>;
      const TILE tile(s, tile_index, lane);
      Env<MODE> e;
      unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
      if (e.reset_pending) {  // (rollout_step's masked reset, then the forward's draw for the new episode)
        resolve_episode<MODE>(c, tile, e);
        next_episode<MODE, true>(e);
        if constexpr (PARAM) {
          pending_force<MODE>(c, q, tile, i, e.episode, e.ep_far, true, false, f1, px, py, pz);
        } else {
          pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, true, false, px, py, pz);
        }
      }
    }
    const double gr = add_cotangents(io, (size_t)n, ii, lam);
    const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
    tape_next = io.x_dev + ((size_t)n + ii) * 12;
#endif
    step_adjoint<TASK, MODE, GYRO, PARAM>(c, q, cur, gr, px, py, pz, false, true, false, tape_next, lam, ga, acc);
    if constexpr (PARAM) {  // the new episode's draw is a constant, 2 / M multiplies it: only two_inv_M's adjoint
      acc[8 * kBlock] += (acc[(kAccPe + 0) * kBlock] * f1[0] + acc[(kAccPe + 1) * kBlock] * f1[1]) +
                         acc[(kAccPe + 2) * kBlock] * f1[2];
    }
    if (valid && io.g_actions_dev != nullptr) {
      if (f32out)
        store_ga<float, A>(io.g_actions_dev, (size_t)n, i, ga);
      else
        store_ga<double, A>(io.g_actions_dev, (size_t)n, i, ga);
    }
  }

  // ---- step 0: from the start point, decoded as the forward decoded it ----
  StepIn in;
  double px, py, pz;
  double f0[3] = {0.0, 0.0, 0.0};  // (PARAM) the start's pending force in newtons: px = f0[0] two_inv_M
  bool fpend = false;              // (PARAM) a force is pending at the start: only then has it a gradient
  bool resetting = false, prev_diff = false, prev_none = false;
  if (io.start_x_dev != nullptr) {
    bool pend;
    double prev_sh;
    explicit_start<TASK, MODE>(c, q, io, i, n, valid, in.x, in.fs, pend, px, py, pz, prev_sh);
    prev_diff = io.start_prev_shaping_dev == nullptr;
    prev_none = prev_sh != prev_sh;
    if constexpr (PARAM) {
      fpend = pend && valid;
      if (fpend) {
#pragma unroll
        for (int j = 0; j < 3; ++j) f0[j] = io.start_force_dev[(size_t)j * n + i];
      }
    }
  } else {
    using TILE = TileIO<MODE>;
    const TILE tile(s, tile_index, lane);
    Env<MODE> e;
    unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
    resolve_episode<MODE>(c, tile, e);
    if constexpr (PARAM) {
      pending_force<MODE>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, f0, px, py, pz);
      fpend = e.pend;
    } else {
      pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, px, py, pz);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) in.x[k] = e.x[k];
    in.fs = e.fs;
    resetting = e.reset_pending;
    prev_none = e.prev_sh != e.prev_sh;
  }
  in.act = load_action_at<TASK>(io.actions_dev + (size_t)ii * A);
  const double gr0 = add_cotangents(io, 0, ii, lam);
  const double* tape_next = nullptr;
#ifdef CS_DEBUG_ROLLOUT
  if (!resetting) tape_next = io.x_dev + (size_t)ii * 12;  // (a resetting step is not recomputed: its gradient is 0)
#endif
  // (PARAM) step 0 accumulates into the second set of rows, added unless the step is a NEXT_STEP reset: that step
  // computes nothing (dt = 0), but its pre-reset state need not be finite
  step_adjoint<TASK, MODE, GYRO, PARAM>(c, q, in, gr0, px, py, pz, resetting, prev_diff, prev_none, tape_next, lam,
                                        ga, PARAM ? acc + kAccRows * kBlock : nullptr);
  if constexpr (PARAM) {
    double* acc0 = acc + kAccRows * kBlock;
    // the perturbation's adjoint, where there is a perturbation: none pending (consumed, or an explicit start without
    // start_force_dev) and a NEXT_STEP reset (its new draw is a constant) give a force gradient of exactly 0
    const bool live = fpend && !resetting;
    const double pe[3] = {live ? acc0[(kAccPe + 0) * kBlock] : 0.0, live ? acc0[(kAccPe + 1) * kBlock] : 0.0,
                          live ? acc0[(kAccPe + 2) * kBlock] : 0.0};
    acc[8 * kBlock] += (pe[0] * f0[0] + pe[1] * f0[1]) + pe[2] * f0[2];
    if (valid) {  // the coefficient adjoints [11, N] for the unfold kernel, the force's [3, N] in the caller's dtype
#pragma unroll
      for (int j = 0; j < kCoefRows; ++j)
        po.g_coef[(size_t)j * n + i] = resetting ? acc[j * kBlock] : acc[j * kBlock] + acc0[j * kBlock];
      if (po.g_force != nullptr) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double g = q.two_inv_M * pe[j];
          if (po.f32)
            reinterpret_cast<float*>(po.g_force)[(size_t)j * n + i] = (float)g;
          else
            reinterpret_cast<double*>(po.g_force)[(size_t)j * n + i] = g;
        }
      }
    }
  }
  if (valid) {
    if (io.g_actions_dev != nullptr) {
      if (f32out)
        store_ga<float, A>(io.g_actions_dev, 0, i, ga);
      else
        store_ga<double, A>(io.g_actions_dev, 0, i, ga);
    }
    if (io.g_x0_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        if (f32out)
          reinterpret_cast<float*>(io.g_x0_dev)[(size_t)k * n + i] = (float)lam[k];
        else
          reinterpret_cast<double*>(io.g_x0_dev)[(size_t)k * n + i] = lam[k];
      }
    }
  }
}

// The parameter-gradient backward (cs_rollout_vjp_ex): the plain sweep plus the coefficient adjoints, accumulated over
// the steps in lane-private LDS columns, read-modify-written where each term arises, not in registers: the plain sweep
// already holds 231-255 VGPRs (profiles/rollout_param_grad_resources.txt).  Two sets of kAccRows rows (step 0 has its
// own), 2 x 14 x 8 B x 64 lanes = 14 KiB per workgroup.  The sweep still needs 243-255 VGPRs + up to 44 AGPRs: 1
// wavefront per SIMD in 35 of 36 instantiations, where the plain kernel has 2.
template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_vjp_param_kernel(const DevConst c, const DevState s,
                                                                   const cs_rollout_io io, const ParamGradOut po) {
  __shared__ double acc[2 * kAccRows * kBlock];
  rollout_vjp_body<TASK, MODE, GYRO, true>(c, s, io, po, acc + threadIdx.x);
}

#define CS_RG_TASKS(M)                           \
  switch (task) {                                \
    case CS_TASK_LANDER3D: M(CS_TASK_LANDER3D); break; \
    case CS_TASK_HOVER3D: M(CS_TASK_HOVER3D); break;   \
    case CS_TASK_LANDER2D: M(CS_TASK_LANDER2D); break; \
    case CS_TASK_LANDER1D: M(CS_TASK_LANDER1D); break; \
    case CS_TASK_HOVER2D: M(CS_TASK_HOVER2D); break;   \
    case CS_TASK_HOVER1D: M(CS_TASK_HOVER1D); break;   \
    default: return hipErrorInvalidValue;        \
  }

hipError_t launch_rollout_states(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                 hipStream_t stream) {
  const dim3 grid((s.n + kBlock - 1) / kBlock), block(kBlock);
#define CS_RS_MODE(TASK)                                                                                          \
  do {                                                                                                            \
    if (mode == CS_STATE_F32G)                                                                                    \
      hipLaunchKernelGGL((rollout_states_kernel<TASK, CS_STATE_F32G>), grid, block, 0, stream, c, s, io);          \
    else if (mode == CS_STATE_F32_RN)                                                                             \
      hipLaunchKernelGGL((rollout_states_kernel<TASK, CS_STATE_F32_RN>), grid, block, 0, stream, c, s, io);        \
    else                                                                                                          \
      hipLaunchKernelGGL((rollout_states_kernel<TASK, CS_STATE_F64>), grid, block, 0, stream, c, s, io);           \
  } while (0)
  CS_RG_TASKS(CS_RS_MODE)
#undef CS_RS_MODE
  return hipGetLastError();
}

hipError_t launch_rollout_vjp(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              hipStream_t stream) {
  const dim3 grid((s.n + kBlock - 1) / kBlock), block(kBlock);
#define CS_RV_GYRO(TASK, MODE)                                                                                    \
  do {                                                                                                            \
    if (c.gyro)                                                                                                   \
      hipLaunchKernelGGL((rollout_vjp_kernel<TASK, MODE, true>), grid, block, 0, stream, c, s, io);               \
    else                                                                                                          \
      hipLaunchKernelGGL((rollout_vjp_kernel<TASK, MODE, false>), grid, block, 0, stream, c, s, io);              \
  } while (0)
#define CS_RV_MODE(TASK)                                                                                          \
  do {                                                                                                            \
    if (mode == CS_STATE_F32G)                                                                                    \
      CS_RV_GYRO(TASK, CS_STATE_F32G);                                                                            \
    else if (mode == CS_STATE_F32_RN)                                                                             \
      CS_RV_GYRO(TASK, CS_STATE_F32_RN);                                                                          \
    else                                                                                                          \
      CS_RV_GYRO(TASK, CS_STATE_F64);                                                                             \
  } while (0)
  CS_RG_TASKS(CS_RV_MODE)
#undef CS_RV_MODE
#undef CS_RV_GYRO
  return hipGetLastError();
}

hipError_t launch_rollout_vjp_param(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                    const ParamGradOut& po, hipStream_t stream) {
  const dim3 grid((s.n + kBlock - 1) / kBlock), block(kBlock);
#define CS_RP_GYRO(TASK, MODE)                                                                                    \
  do {                                                                                                            \
    if (c.gyro)                                                                                                   \
      hipLaunchKernelGGL((rollout_vjp_param_kernel<TASK, MODE, true>), grid, block, 0, stream, c, s, io, po);     \
    else                                                                                                          \
      hipLaunchKernelGGL((rollout_vjp_param_kernel<TASK, MODE, false>), grid, block, 0, stream, c, s, io, po);    \
  } while (0)
#define CS_RP_MODE(TASK)                                                                                          \
  do {                                                                                                            \
    if (mode == CS_STATE_F32G)                                                                                    \
      CS_RP_GYRO(TASK, CS_STATE_F32G);                                                                            \
    else if (mode == CS_STATE_F32_RN)                                                                             \
      CS_RP_GYRO(TASK, CS_STATE_F32_RN);                                                                          \
    else                                                                                                          \
      CS_RP_GYRO(TASK, CS_STATE_F64);                                                                             \
  } while (0)
  CS_RG_TASKS(CS_RP_MODE)
#undef CS_RP_MODE
#undef CS_RP_GYRO
  return hipGetLastError();
}
#undef CS_RG_TASKS

// ---------------------------------------------------------------------------------------------------------------------
// vehicle tables on the device
// ---------------------------------------------------------------------------------------------------------------------
constexpr double kPiDev = 3.141592653589793238462643383279502884;

// fold_vehicle (copterstep_api.hip) of env i's raw column, operation for operation (this file compiles without
// contraction, and float64 division is IEEE): the host's bits.  raw [12, n], coef [11, stride].
__global__ __launch_bounds__(256) void fold_vehicle_kernel(const double* __restrict__ raw, uint32_t n, int lift,
                                                           double* __restrict__ coef, uint32_t stride) {
  const uint32_t tile = blockIdx.x;  // (elementwise: 256 envs per workgroup, no state tiles touched)
  const uint32_t i = tile * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r[kVehicleRows];
#pragma unroll
  for (int j = 0; j < kVehicleRows; ++j) r[j] = raw[(size_t)j * n + i];
  const double B = r[0], D = r[1], M = r[2], L = r[3], Ix = r[4], Iy = r[5], Iz = r[6], Jr = r[7], maxrpm = r[8],
               G = r[9], rho = r[10], C_L = r[11];
  const double ws = maxrpm * kPiDev / 30.0;
  const double ws2 = ws * ws;
  double kthrust, kroll;
  if (lift) {
    const double S = 0.05 * L * 4.0;
    const double KL = 0.5 * rho * S * C_L * (L / 2.0) * (L / 2.0) * ws2;
    kthrust = KL;
    kroll = KL;
  } else {
    kthrust = B * ws2;
    kroll = L * B * ws2;
  }
  const double k[kCoefRows] = {-kthrust / M,       kroll / Ix,         kroll / Iy,         (D * ws2) / Iz,
                               G,                  (Iy - Iz) / Ix,     (Iz - Ix) / Iy,     (Ix - Iy) / Iz,
                               2.0 / M,            Jr / Ix * ws,       Jr / Iy * ws};
#pragma unroll
  for (int j = 0; j < kCoefRows; ++j) coef[(size_t)j * stride + i] = k[j];
}

struct VehicleRaw {
  double v[kVehicleRows];
};

// The chain rule through fold_vehicle: the adjoints of the 11 coefficients (gcoef [11, n]) -> those of the 12 raw rows
// (gveh [12, n], float32 when f32), at env i's raw column (raw [12, n], or the uniform vehicle when raw is nullptr).
// Rows that do not enter the configuration are exactly 0: B under the lift law, rho and C_L under the B law, Jr without
// the rotor-gyro term.
__global__ __launch_bounds__(256) void unfold_vehicle_kernel(const double* __restrict__ gcoef,
                                                             const double* __restrict__ raw, const VehicleRaw uni,
                                                             uint32_t n, int lift, int gyro, void* __restrict__ gveh,
                                                             uint32_t f32) {
  const uint32_t tile = blockIdx.x;  // (elementwise: 256 envs per workgroup, no state tiles touched)
  const uint32_t i = tile * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r[kVehicleRows], a[kCoefRows];
#pragma unroll
  for (int j = 0; j < kVehicleRows; ++j) r[j] = raw != nullptr ? raw[(size_t)j * n + i] : uni.v[j];
#pragma unroll
  for (int j = 0; j < kCoefRows; ++j) a[j] = gcoef[(size_t)j * n + i];
  const double B = r[0], D = r[1], M = r[2], L = r[3], Ix = r[4], Iy = r[5], Iz = r[6], Jr = r[7], maxrpm = r[8],
               rho = r[10], C_L = r[11];
  const double ws = maxrpm * kPiDev / 30.0;
  const double ws2 = ws * ws;
  // c0 = -kthrust / M, c1 = kroll / Ix, c2 = kroll / Iy, c3 = D ws2 / Iz, c4 = G, c5 = (Iy - Iz) / Ix,
  // c6 = (Iz - Ix) / Iy, c7 = (Ix - Iy) / Iz, c8 = 2 / M, c9 = Jr ws / Ix, c10 = Jr ws / Iy
  double kthrust, kroll, g_B = 0.0, g_L, g_rho = 0.0, g_CL = 0.0, g_ws2;
  const double g_kthrust = -a[0] / M;
  const double g_kroll = a[1] / Ix + a[2] / Iy;
  if (lift) {  // kthrust = kroll = KL = 0.5 rho (0.2 L) C_L (L / 2)^2 ws2 = 0.025 rho C_L L^3 ws2
    const double l2 = (L / 2.0) * (L / 2.0);
    const double base = 0.5 * (0.05 * L * 4.0) * l2;  // KL / (rho C_L ws2)
    const double KL = base * rho * C_L * ws2;
    kthrust = kroll = KL;
    const double g_KL = g_kthrust + g_kroll;
    g_rho = g_KL * (base * C_L * ws2);
    g_CL = g_KL * (base * rho * ws2);
    g_L = g_KL * (0.075 * L * L * rho * C_L * ws2);
    g_ws2 = g_KL * (base * rho * C_L);
  } else {  // kthrust = B ws2, kroll = L B ws2
    kthrust = B * ws2;
    kroll = L * B * ws2;
    g_B = (g_kthrust + g_kroll * L) * ws2;
    g_L = g_kroll * B * ws2;
    g_ws2 = g_kthrust * B + g_kroll * (L * B);
  }
  g_ws2 += a[3] * D / Iz;
  double g_ws = 2.0 * ws * g_ws2;
  double g_Jr = 0.0;
  if (gyro) {
    g_Jr = (a[9] / Ix + a[10] / Iy) * ws;
    g_ws += Jr * (a[9] / Ix + a[10] / Iy);
  }
  const double g[kVehicleRows] = {
      g_B,
      a[3] * ws2 / Iz,
      (a[0] * kthrust - 2.0 * a[8]) / (M * M),
      g_L,
      -(a[1] * kroll + a[5] * (Iy - Iz) + (gyro ? a[9] * Jr * ws : 0.0)) / (Ix * Ix) - a[6] / Iy + a[7] / Iz,
      -(a[2] * kroll + a[6] * (Iz - Ix) + (gyro ? a[10] * Jr * ws : 0.0)) / (Iy * Iy) + a[5] / Ix - a[7] / Iz,
      -(a[3] * D * ws2 + a[7] * (Ix - Iy)) / (Iz * Iz) - a[5] / Ix + a[6] / Iy,
      g_Jr,
      g_ws * (kPiDev / 30.0),
      a[4],
      g_rho,
      g_CL};
#pragma unroll
  for (int j = 0; j < kVehicleRows; ++j) {
    if (f32)
      reinterpret_cast<float*>(gveh)[(size_t)j * n + i] = (float)g[j];
    else
      reinterpret_cast<double*>(gveh)[(size_t)j * n + i] = g[j];
  }
}

// the parameter block of the _ex calls, checked before the context like io
int check_param_io(const cs_rollout_param_io* pio, const char* who) {
  const std::string w(who);
  if (pio->struct_size != sizeof(cs_rollout_param_io))
    return report_error(CS_ERR_ABI, (w + ": pio->struct_size " + std::to_string(pio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_param_io)) + " (sizeof(cs_rollout_param_io))")
                                        .c_str());
  if (pio->out_dtype != CS_JAC_F64 && pio->out_dtype != CS_JAC_F32)
    return report_error(CS_ERR_ARG, (w + ": unknown pio->out_dtype (CS_JAC_F64 or CS_JAC_F32)").c_str());
  return CS_OK;
}

// the DevState a call with pio launches on: the env's, or with pio->vehicle_dev the override folded into the scratch
int override_state(const ParamView& pv, const cs_rollout_param_io* pio, const DevState& s0, hipStream_t stream,
                   const char* who, DevState* out) {
  *out = s0;
  if (pio == nullptr || pio->vehicle_dev == nullptr) return CS_OK;
  hipLaunchKernelGGL(fold_vehicle_kernel, dim3((pv.n + 255) / 256), dim3(256), 0, stream, pio->vehicle_dev, pv.n,
                     pv.lift, pv.coef_dev, pv.stride);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return report_hip(e, (std::string(who) + ": fold kernel launch").c_str());
  out->veh = pv.coef_dev;
  out->veh_stride = pv.stride;
  return CS_OK;
}

}  // namespace

// the argument block, checked before the context (a caller's layout error is reported as such, without a device)
int check_rollout_io(const cs_rollout_io* io, const char* who, bool vjp) {
  const std::string w(who);
  if (io == nullptr) return report_error(CS_ERR_ARG, (w + ": null io").c_str());
  if (io->struct_size != sizeof(cs_rollout_io))
    return report_error(CS_ERR_ABI, (w + ": io->struct_size " + std::to_string(io->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_io)) + " (sizeof(cs_rollout_io))").c_str());
  if (io->num_steps < 1) return report_error(CS_ERR_ARG, (w + ": num_steps must be >= 1").c_str());
  if (io->actions_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": actions_dev is required").c_str());
  if (io->start_x_dev == nullptr &&
      (io->start_status_dev != nullptr || io->start_force_dev != nullptr || io->start_prev_shaping_dev != nullptr))
    return report_error(CS_ERR_ARG,
                        (w + ": start_status_dev / start_force_dev / start_prev_shaping_dev describe an explicit start: "
                             "start_x_dev is required").c_str());
  if (io->start_x_dev != nullptr && io->start_status_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": an explicit start needs start_status_dev").c_str());
  if (vjp) {
    if (io->out_dtype != CS_JAC_F64 && io->out_dtype != CS_JAC_F32)
      return report_error(CS_ERR_ARG, (w + ": unknown out_dtype (CS_JAC_F64 or CS_JAC_F32)").c_str());
    if (io->x_dev == nullptr || io->status_dev == nullptr)
      return report_error(CS_ERR_ARG, (w + ": the tape (x_dev and status_dev of cs_rollout_states) is required").c_str());
  }
  return CS_OK;
}

}  // namespace cs

extern "C" int cs_rollout_states_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_param_io* pio,
                                    void* stream) {
  if (pio == nullptr) return cs_rollout_states(ctx, io, stream);
  if (int rc_ = cs::check_rollout_io(io, "cs_rollout_states_ex", false)) return rc_;
  if (int rc_ = cs::check_param_io(pio, "cs_rollout_states_ex")) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_states_ex", stream, &v)) return rc_;
  cs::ParamView pv;
  if (int rc_ = cs::param_view(ctx, "cs_rollout_states_ex", pio->vehicle_dev != nullptr, false, &pv)) return rc_;
  cs::DevState s;
  if (int rc_ = cs::override_state(pv, pio, *v.s, (hipStream_t)stream, "cs_rollout_states_ex", &s)) return rc_;
  const hipError_t e = cs::launch_rollout_states(v.task, v.mode, *v.c, s, *io, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_states_ex: kernel launch");
  return CS_OK;
}

extern "C" int cs_rollout_vjp_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_param_io* pio, void* stream) {
  if (pio == nullptr) return cs_rollout_vjp(ctx, io, stream);
  if (int rc_ = cs::check_rollout_io(io, "cs_rollout_vjp_ex", true)) return rc_;
  if (int rc_ = cs::check_param_io(pio, "cs_rollout_vjp_ex")) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_vjp_ex", stream, &v)) return rc_;
  const bool grad = pio->g_vehicle_dev != nullptr || pio->g_force_dev != nullptr;
  cs::ParamView pv;
  if (int rc_ = cs::param_view(ctx, "cs_rollout_vjp_ex", pio->vehicle_dev != nullptr, grad, &pv)) return rc_;
  cs::DevState s;
  if (int rc_ = cs::override_state(pv, pio, *v.s, (hipStream_t)stream, "cs_rollout_vjp_ex", &s)) return rc_;
  const hipStream_t st = (hipStream_t)stream;
  if (!grad) {
    const hipError_t e = cs::launch_rollout_vjp(v.task, v.mode, *v.c, s, *io, st);
    if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_vjp_ex: kernel launch");
    return CS_OK;
  }
  const cs::ParamGradOut po{pv.gcoef_dev, pio->g_force_dev, pio->out_dtype == CS_JAC_F32 ? 1u : 0u};
  hipError_t e = cs::launch_rollout_vjp_param(v.task, v.mode, *v.c, s, *io, po, st);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_vjp_ex: kernel launch");
  if (pio->g_vehicle_dev != nullptr) {
    cs::VehicleRaw uni;
    for (int j = 0; j < cs::kVehicleRows; ++j) uni.v[j] = pv.uniform_raw[j];
    const double* raw = pio->vehicle_dev != nullptr ? pio->vehicle_dev : pv.raw_dev;
    hipLaunchKernelGGL(cs::unfold_vehicle_kernel, dim3((pv.n + 255) / 256), dim3(256), 0, st, pv.gcoef_dev, raw, uni,
                       pv.n, pv.lift, pv.gyro, pio->g_vehicle_dev, po.f32);
    e = hipGetLastError();
    if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_vjp_ex: unfold kernel launch");
  }
  return CS_OK;
}

extern "C" int cs_rollout_states(cs_ctx* ctx, const cs_rollout_io* io, void* stream) {
  if (int rc_ = cs::check_rollout_io(io, "cs_rollout_states", false)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_states", stream, &v)) return rc_;
  const hipError_t e = cs::launch_rollout_states(v.task, v.mode, *v.c, *v.s, *io, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_states: kernel launch");
  return CS_OK;
}

extern "C" int cs_rollout_vjp(cs_ctx* ctx, const cs_rollout_io* io, void* stream) {
  if (int rc_ = cs::check_rollout_io(io, "cs_rollout_vjp", true)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_vjp", stream, &v)) return rc_;
  const hipError_t e = cs::launch_rollout_vjp(v.task, v.mode, *v.c, *v.s, *io, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_vjp: kernel launch");
  return CS_OK;
}
