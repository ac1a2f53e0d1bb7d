// copterstep_jvp.hip -- forward-mode tangents of K-step rollouts on gfx950 (cs_jvp_rollout, include/copterstep.h): D
// input directions on the actions, the start state, the vehicle rows and the start's pending force, pushed forward
// through the K steps of a rollout whose tape cs_rollout_states wrote.  The linear map is the one whose transpose
// cs_rollout_vjp / cs_rollout_vjp_ex apply.  Nothing of the env state is written.
//
// Upstream lines differentiated (paths relative to the upstream checkout):
//   dynamics/__init__.py:114-197 (setMotors), :249-290 (state derivative), :292-302 (_bodyZToInertial),
//   envs/task.py:77-137 (step: the clip of :91, the LANDED skip of :86-87), envs/lander.py:46-74 (reward, whose
//   prev_shaping makes reward_k a function of x_{k-1} as well as of x_k).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  The directions go in blocks of
// kJacDirs, a loop inside the kernel; for every block the lane sweeps k = 1 .. K with the block's tangents in
// registers, each step's primal recomputed from the tape row before it (rollout_tangent.h).  PARAM builds fold the
// block's raw vehicle tangents to coefficient tangents first (fold_tangent) and keep them in lane-private LDS columns.
// DESIGN.md section 26.
#include <string>

#include "copterstep_jacobian.h"

// the primal must round as the step kernels do (copterstep_kernels.hip): the recomputed primal is the tape bit for bit,
// or its branch decisions could differ from the forward's
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "rollout_adjoint.h"
#include "rollout_step.h"
#include "rollout_sweep.h"
#include "rollout_tangent.h"
#include "dev_launch.h"

namespace cs {
namespace {

struct VehicleBase {
  double v[kVehicleRows];
};

// what the sweep reads and writes beyond cs_rollout_io (cs_jvp_io, with the fold tangent's base point)
struct JvpArgs {
  const double* t_actions;  // [D,K,N,A] or nullptr
  const double* t_x0;       // [D,12,N] or nullptr
  const double* t_vehicle;  // [D,12,N] or nullptr
  const double* t_force;    // [D,3,N] or nullptr
  const double* raw;        // [12,N] the fold tangent's base point, nullptr = uni
  void* t_x;                // [D,K,N,12] or nullptr
  void* t_reward;           // [D,K,N] or nullptr
  uint32_t dirs, f32;
  int lift, gyro;
  VehicleBase uni;
};

template <int TASK, int MODE, bool GYRO, bool PARAM>
__global__ __launch_bounds__(kBlock) void rollout_jvp_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                             const JvpArgs ja) {
  constexpr int A = task_act_dim(TASK);
  __shared__ __attribute__((aligned(16))) double xrow[kBlock * 12];         // 6 KiB: the wavefront's tangent rows
  __shared__ double tcs[PARAM ? kJacDirs * kCoefRows * kBlock : 1];         // 11 KiB: the block's coefficient tangents
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut r{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const bool valid = r.valid;
  const uint32_t ii = valid ? i : 0u;  // (padding lanes recompute env 0's steps and store nothing)
  const int K = io.num_steps;
  const uint32_t D = ja.dirs;
  double* tc = tcs + lane;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);

#pragma clang loop unroll(disable)
  for (uint32_t d0 = 0; d0 < D; d0 += kJacDirs) {
    // the block's directions d0 .. d0 + kJacDirs - 1; one past the last is a zero direction that stores nothing
    bool live[kJacDirs];
    uint32_t dd[kJacDirs];
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d) {
      live[d] = d0 + (uint32_t)d < D;
      dd[d] = live[d] ? d0 + (uint32_t)d : d0;
    }
    if constexpr (PARAM) {
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) {
        double tcd[kCoefRows];
#pragma unroll
        for (int j = 0; j < kCoefRows; ++j) tcd[j] = 0.0;
        if (ja.t_vehicle != nullptr && live[d]) {
          double raw[kVehicleRows], t[kVehicleRows];
#pragma unroll
          for (int j = 0; j < kVehicleRows; ++j) {
            raw[j] = ja.raw != nullptr ? ja.raw[(size_t)j * n + ii] : ja.uni.v[j];
            t[j] = ja.t_vehicle[((size_t)dd[d] * kVehicleRows + j) * n + ii];
          }
          fold_tangent(raw, t, ja.lift, ja.gyro, tcd);
        }
#pragma unroll
        for (int j = 0; j < kCoefRows; ++j) tc[(d * kCoefRows + j) * kBlock] = tcd[j];
      }
    }
    double v[kJacDirs][12];
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d)
#pragma unroll
      for (int k = 0; k < 12; ++k)
        v[d][k] = (ja.t_x0 != nullptr && live[d]) ? ja.t_x0[((size_t)dd[d] * 12 + k) * n + ii] : 0.0;

#pragma clang loop unroll(disable)
    for (int k = 0; k < K; ++k) {
      StepIn in;
      double px = -0.0, py = -0.0, pz = -0.0;
      double tp[kJacDirs][3] = {};
      bool resetting = false, prev_diff = true, prev_none = false;
      if (k == 0) {  // from the start point, decoded as the forward decoded it
        double f0[3] = {0.0, 0.0, 0.0};  // (PARAM) the start's pending force in newtons: px = f0[0] two_inv_M
        bool fpend = false;              // (PARAM) a force is pending at the start: only then has it a tangent
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
          for (int j = 0; j < 12; ++j) in.x[j] = e.x[j];
          in.fs = e.fs;
          resetting = e.reset_pending;
          prev_diff = false;
          prev_none = e.prev_sh != e.prev_sh;
        }
        in.act = load_action_at<TASK>(io.actions_dev + (size_t)ii * A);
        if constexpr (PARAM) {  // p = f two_inv_M: none pending and a NEXT_STEP reset give a tangent of exactly 0
          if (fpend && !resetting) {
#pragma unroll
            for (int d = 0; d < kJacDirs; ++d)
#pragma unroll
              for (int j = 0; j < 3; ++j) {
                const double tf = (ja.t_force != nullptr && live[d]) ? ja.t_force[((size_t)dd[d] * 3 + j) * n + ii]
                                                                     : 0.0;
                tp[d][j] = q.two_inv_M * tf + f0[j] * tc[(d * kCoefRows + 8) * kBlock];
              }
          }
        }
      } else {
        load_tape_step<TASK>(io, n, ii, k, in);
        // A stored-start lane with a NEXT_STEP reset pending resets in step 0, and the new episode's perturbation
        // enters the first call of step 1 (rollout_vjp_sweep): a constant draw that 2 / M multiplies
        if (k == 1 && io.start_x_dev == nullptr) {
          using TILE = TileIO<MODE>;
          const TILE tile(s, tile_index, lane);
          Env<MODE> e;
          unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
          if (e.reset_pending) {
            resolve_episode<MODE>(c, tile, e);
            next_episode<MODE, true>(e);
            if constexpr (PARAM) {
              double f1[3] = {0.0, 0.0, 0.0};
              pending_force<MODE>(c, q, tile, i, e.episode, e.ep_far, true, false, f1, px, py, pz);
#pragma unroll
              for (int d = 0; d < kJacDirs; ++d)
#pragma unroll
                for (int j = 0; j < 3; ++j) tp[d][j] = f1[j] * tc[(d * kCoefRows + 8) * kBlock];
            } else {
              pending_perturbation<MODE, true>(c, q, tile, i, e.episode, e.ep_far, true, false, px, py, pz);
            }
          }
        }
      }
      double ta[kJacDirs][4] = {};
      if (ja.t_actions != nullptr) {
#pragma unroll
        for (int d = 0; d < kJacDirs; ++d) {
          if (live[d]) {
            const double* p = ja.t_actions + (((size_t)dd[d] * K + k) * n + ii) * A;
#pragma unroll
            for (int j = 0; j < A; ++j) ta[d][j] = p[j];
          }
        }
      }
      double tr[kJacDirs];
      step_tangent<TASK, MODE, GYRO, PARAM>(c, q, in, px, py, pz, tp, resetting, prev_diff, prev_none, ta,
                                            PARAM ? tc : nullptr, v, tr);
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) {
        if (!live[d]) continue;  // (wavefront-uniform)
        const size_t row = ((size_t)dd[d] * K + k) * n;
        if (ja.t_x != nullptr) {
          if (ja.f32)
            store_t_row<float>(xrow, reinterpret_cast<float*>(ja.t_x), row, r, v[d]);
          else
            store_t_row<double>(xrow, reinterpret_cast<double*>(ja.t_x), row, r, v[d]);
        }
        if (valid && ja.t_reward != nullptr) {
          if (ja.f32)
            reinterpret_cast<float*>(ja.t_reward)[row + i] = (float)tr[d];
          else
            reinterpret_cast<double*>(ja.t_reward)[row + i] = tr[d];
        }
      }
    }
  }
}

template <int TASK, int MODE, bool PARAM>
hipError_t jvp_tp(const DevConst& c, const DevState& s, const cs_rollout_io& io, const JvpArgs& ja,
                  hipStream_t stream) {
  const dim3 grid(grid_for(s.n)), block(kBlock);
  if (c.gyro)
    hipLaunchKernelGGL((rollout_jvp_kernel<TASK, MODE, true, PARAM>), grid, block, 0, stream, c, s, io, ja);
  else
    hipLaunchKernelGGL((rollout_jvp_kernel<TASK, MODE, false, PARAM>), grid, block, 0, stream, c, s, io, ja);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t jvp_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const JvpArgs& ja, bool param,
                 hipStream_t stream) {
  return param ? jvp_tp<TASK, MODE, true>(c, s, io, ja, stream) : jvp_tp<TASK, MODE, false>(c, s, io, ja, stream);
}

hipError_t launch_rollout_jvp(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const JvpArgs& ja, bool param, hipStream_t stream) {
  CS_DISPATCH(jvp_t, c, s, io, ja, param, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_jvp_rollout(cs_ctx* ctx, const cs_rollout_io* io, const cs_jvp_io* jio, void* stream) {
  using cs::report_error;
  const char* who = "cs_jvp_rollout";
  const std::string w(who);
  // (the argument blocks are checked before the context: a caller's layout error is reported as such)
  if (int rc_ = cs::check_rollout_io(io, who, true)) return rc_;
  if (jio == nullptr) return report_error(CS_ERR_ARG, (w + ": null jio").c_str());
  if (jio->struct_size != sizeof(cs_jvp_io))
    return report_error(CS_ERR_ABI, (w + ": jio->struct_size " + std::to_string(jio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_jvp_io)) + " (sizeof(cs_jvp_io))").c_str());
  if (jio->out_dtype != CS_JAC_F64 && jio->out_dtype != CS_JAC_F32)
    return report_error(CS_ERR_ARG, (w + ": unknown jio->out_dtype (CS_JAC_F64 or CS_JAC_F32)").c_str());
  if (jio->num_dirs < 1 || jio->num_dirs > CS_JVP_MAX_DIRS)
    return report_error(CS_ERR_ARG, (w + ": jio->num_dirs must be 1 .. CS_JVP_MAX_DIRS (" +
                                     std::to_string(CS_JVP_MAX_DIRS) + ")").c_str());
  const struct {
    const void* p;
    const char* name;
  } forbidden[] = {{io->reward_dev, "reward_dev"},       {io->terminated_dev, "terminated_dev"},
                   {io->truncated_dev, "truncated_dev"}, {io->gx_dev, "gx_dev"},
                   {io->gr_dev, "gr_dev"},               {io->g_actions_dev, "g_actions_dev"},
                   {io->g_x0_dev, "g_x0_dev"}};
  for (const auto& f : forbidden)
    if (f.p != nullptr) return report_error(CS_ERR_ARG, (w + ": io->" + f.name + " must be NULL").c_str());
  if (jio->t_actions_dev == nullptr && jio->t_x0_dev == nullptr && jio->t_vehicle_dev == nullptr &&
      jio->t_force_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": an input tangent is required (one of jio->t_actions_dev, t_x0_dev, "
                                         "t_vehicle_dev, t_force_dev)").c_str());
  if (jio->t_x_dev == nullptr && jio->t_reward_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": an output is required (one of jio->t_x_dev, t_reward_dev)").c_str());
  const auto aligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; };
  if (!aligned(jio->t_actions_dev, 7u) || !aligned(jio->t_x0_dev, 7u) || !aligned(jio->t_vehicle_dev, 7u) ||
      !aligned(jio->t_force_dev, 7u) || !aligned(jio->vehicle_dev, 7u))
    return report_error(CS_ERR_ARG, (w + ": a float64 array of jio is not 8-B aligned").c_str());
  if (!aligned(jio->t_x_dev, 15u) || !aligned(jio->t_reward_dev, jio->out_dtype == CS_JAC_F32 ? 3u : 7u))
    return report_error(CS_ERR_ARG, (w + ": jio->t_x_dev must be 16-B aligned, jio->t_reward_dev to its element "
                                         "size").c_str());
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, who, stream, &v)) return rc_;
  const bool param = jio->t_vehicle_dev != nullptr || jio->t_force_dev != nullptr;
  cs::DevState s = *v.s;
  cs::JvpArgs ja{};
  ja.t_actions = jio->t_actions_dev;
  ja.t_x0 = jio->t_x0_dev;
  ja.t_vehicle = jio->t_vehicle_dev;
  ja.t_force = jio->t_force_dev;
  ja.t_x = jio->t_x_dev;
  ja.t_reward = jio->t_reward_dev;
  ja.dirs = (uint32_t)jio->num_dirs;
  ja.f32 = jio->out_dtype == CS_JAC_F32 ? 1u : 0u;
  if (param || jio->vehicle_dev != nullptr) {
    cs::ParamView pv;
    if (int rc_ = cs::param_view(ctx, who, jio->vehicle_dev != nullptr, false, &pv)) return rc_;
    if (int rc_ = cs::override_vehicle(pv, jio->vehicle_dev, *v.s, (hipStream_t)stream, who, &s)) return rc_;
    ja.raw = jio->vehicle_dev != nullptr ? jio->vehicle_dev : pv.raw_dev;
    ja.lift = pv.lift;
    ja.gyro = pv.gyro;
    for (int j = 0; j < cs::kVehicleRows; ++j) ja.uni.v[j] = pv.uniform_raw[j];
  }
  const hipError_t e = cs::launch_rollout_jvp(v.task, v.mode, *v.c, s, *io, ja, param, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_jvp_rollout: kernel launch");
  return CS_OK;
}
