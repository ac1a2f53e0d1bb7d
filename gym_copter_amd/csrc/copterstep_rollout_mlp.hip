// copterstep_rollout_mlp.hip -- differentiable CLOSED-LOOP rollouts under a fused MLP policy on gfx950
// (cs_rollout_mlp_states / cs_rollout_mlp_vjp, include/copterstep.h): K steps with auto-reset disabled in which step k
// takes a_k = fl32(pi_theta(o_{k-1}) + u_k), and the reverse-mode gradient of a loss on them with respect to u, the
// explicit start and (through the action tape, host side) theta.  Nothing of the env state is written.
//
// The loop replaced: lander.py:40-65 with a policy in place of the random action -- observe, act, step -- run K times
// and differentiated (analytic policy gradients).  Upstream lines differentiated: those of copterstep_rollout_grad.hip.
//
// One lane per env on the tile layout of the step kernels, as copterstep_rollout_grad.hip.  The policy's weights are
// wave-uniform: they are read through the scalar unit (constant address space), streamed one hidden unit at a time, so a
// lane holds O(OBS + A) policy values whatever the width.  The forward is rollout_states_kernel's loop with the policy
// in front of each rollout_step; the backward is rollout_sweep.h's reverse sweep with the policy's vector-Jacobian product after each
// step_adjoint: lambda_o += J_o pi^T g_a, recomputed in float64 from the tape row already in registers.  DESIGN.md
// section 12.
#include <string>

#include "copterstep_jacobian.h"

// the primal must round as the step kernels do (copterstep_kernels.hip), and the policy's float32 arithmetic is the
// explicit fmaf chain of mlp_policy.h, whatever the compiler would contract
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
#include "mlp_policy.h"
#include "dev_launch.h"

namespace cs {
namespace {

// what the kernels take of cs_rollout_mlp_io
struct MlpArgs {
  const float* params;   // [P] float32, the layout of include/copterstep.h
  const float* offsets;  // [K,N,A] u, or nullptr
  float* actions;        // [K,N,A] the action tape
  float* obs;            // [K,N,OBS] the observation tape, or nullptr
  int hidden;            // 0 .. CS_MLP_MAX_HIDDEN
};

// One float32 row of W values per lane, [.., N, W] at row `row` (64-bit): a whole wavefront's 64 rows are contiguous
// and go out through the LDS as 16 B stores (64 W floats = 16 W float4), a partial one lane by lane.
template <int W>
__device__ __forceinline__ void store_row_f32(float* lds, float* base, size_t row, uint32_t env0, uint32_t i, int lane,
                                              bool whole, bool valid, const float (&v)[W]) {
  if (whole) {
#pragma unroll
    for (int j = 0; j < W; ++j) lds[lane * W + j] = v[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const float4* src = reinterpret_cast<const float4*>(lds);
    float4* dst = reinterpret_cast<float4*>(base + (row + env0) * W);
#pragma unroll
    for (int v4 = 0; v4 < (16 * W + kWave - 1) / kWave; ++v4) {
      const int e = v4 * kWave + lane;
      if ((16 * W) % kWave == 0 || e < 16 * W) dst[e] = src[e];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else if (valid) {
    float* dst = base + (row + i) * W;
#pragma unroll
    for (int j = 0; j < W; ++j) dst[j] = v[j];
  }
}

// The closed-loop forward keeps its own loop: rollout_forward (rollout_sweep.h) with the policy as its action source
// computed the same outputs but ran 1-3 % slower at H = 32 and 64 (profiles/rollout_sweep_refactor_ab.txt).
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void rollout_mlp_states_kernel(const DevConst c, const DevState s,
                                                                    const cs_rollout_io io, const MlpArgs m) {
  constexpr int A = task_act_dim(TASK), OBS = task_obs_dim(TASK), FIRST = task_obs_first(TASK);
  __shared__ __attribute__((aligned(16))) double xrow[kBlock * 12];  // 6 KiB: the wavefront's state rows of a step
  __shared__ __attribute__((aligned(16))) float orow[kBlock * OBS];  // its observation rows
  __shared__ __attribute__((aligned(16))) float arow[kBlock * A];    // its action rows
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const bool valid = i < n;
  const bool whole = env0 + (uint32_t)kWave <= n;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, valid ? i : 0u);
  using TILE = TileIO<MODE>;
  const TILE tile(s, tile_index, lane);
  Env<MODE> e;
  unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
  resolve_episode<MODE>(c, tile, e);
  double px, py, pz;
  rollout_start<TASK, MODE>(c, q, io, tile, i, n, valid, e, px, py, pz);

  const float* u_lane = m.offsets != nullptr ? m.offsets + (size_t)(valid ? i : 0u) * A : nullptr;
  const size_t act_step = (size_t)n * A;
#pragma clang loop unroll(disable)
  for (int k = 0; k < io.num_steps; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit: K x N x 12 doubles pass 4 GiB at 1 M envs
    // ---- the policy: o_{k-1} = what step() returned for the state before this step ----
    float o[OBS], a[A];
#pragma unroll
    for (int j = 0; j < OBS; ++j) o[j] = (float)e.x[FIRST + j];
    mlp_forward<OBS, A>(m.params, m.hidden, o, a);
    if (u_lane != nullptr) {
      const float4 u = load_action_at<TASK>(u_lane);
      u_lane += act_step;
      const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int j = 0; j < A; ++j) a[j] = a[j] + uu[j];
    }
    if (m.obs != nullptr) store_row_f32<OBS>(orow, m.obs, row, env0, i, lane, whole, valid, o);
    store_row_f32<A>(arow, m.actions, row, env0, i, lane, whole, valid, a);

    const bool resetting = e.reset_pending;
    double reward;
    bool term, trunc;
    rollout_step<TASK, MODE>(c, q, e, motors_of<A>(a), px, py, pz, reward, term, trunc);
    next_perturbation<MODE>(c, q, tile, i, resetting, e, px, py, pz);

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

// The closed-loop sweep's extension (rollout_vjp_sweep's EXT): the policy's VJP after each step's adjoint; io.actions_dev
// is the action tape.  COT (cs_rollout_mlp_vjp_ex): the caller's cotangent on the action tape, g_in [K,N,A] float64, is
// added to each step's g_a first -- a template flag, so that the kernels without it are the ones they were.
template <int TASK, bool COT = false>
struct SweepPolicy {
  static constexpr bool kParam = false, kPolicy = true;
  const MlpArgs& m;
  const double* g_in = nullptr;
  __device__ __forceinline__ void add_action_cotangent(size_t row, uint32_t env, double (&ga)[4]) const {
    if constexpr (COT) {
      constexpr int A = task_act_dim(TASK);
      const double* g = g_in + (row + env) * A;
#pragma unroll
      for (int c = 0; c < A; ++c) ga[c] += g[c];
    }
  }
  __device__ __forceinline__ void vjp(const double (&x)[12], const double (&ga)[4], double (&lam)[12]) const {
    mlp_vjp<TASK>(m.params, m.hidden, x, ga, lam);
  }
};

// The backward without the rotor-gyro term is held to 2 wavefronts per SIMD: it fits 256 VGPRs without AGPRs or scratch
// there, where the allocator left to itself takes 8-16 AGPRs and 1 wavefront.  With the term the same bound spills to
// scratch, so that form keeps the default (profiles/rollout_mlp_resources.txt).
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void rollout_mlp_vjp_kernel(
    const DevConst c, const DevState s, const cs_rollout_io io, const MlpArgs m) {
  rollout_vjp_sweep<TASK, MODE, false>(c, s, io, SweepPolicy<TASK>{m});
}
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void rollout_mlp_vjp_gyro_kernel(const DevConst c, const DevState s,
                                                                      const cs_rollout_io io, const MlpArgs m) {
  rollout_vjp_sweep<TASK, MODE, true>(c, s, io, SweepPolicy<TASK>{m});
}
// the same two with the cotangent on the action tape
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void rollout_mlp_vjp_cot_kernel(
    const DevConst c, const DevState s, const cs_rollout_io io, const MlpArgs m, const double* const g_in) {
  rollout_vjp_sweep<TASK, MODE, false>(c, s, io, SweepPolicy<TASK, true>{m, g_in});
}
template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void rollout_mlp_vjp_gyro_cot_kernel(const DevConst c, const DevState s,
                                                                          const cs_rollout_io io, const MlpArgs m,
                                                                          const double* const g_in) {
  rollout_vjp_sweep<TASK, MODE, true>(c, s, io, SweepPolicy<TASK, true>{m, g_in});
}

// the launchers of one (task, mode) instantiation (CS_DISPATCH picks it), the backward's split on the rotor-gyro term
template <int TASK, int MODE>
hipError_t mlp_states_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const MlpArgs& m,
                        hipStream_t stream) {
  hipLaunchKernelGGL((rollout_mlp_states_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, io,
                     m);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t mlp_vjp_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const MlpArgs& m,
                     const double* g_in, hipStream_t stream) {
  const dim3 grid(grid_for(s.n)), block(kBlock);
  if (g_in != nullptr && c.gyro)
    hipLaunchKernelGGL((rollout_mlp_vjp_gyro_cot_kernel<TASK, MODE>), grid, block, 0, stream, c, s, io, m, g_in);
  else if (g_in != nullptr)
    hipLaunchKernelGGL((rollout_mlp_vjp_cot_kernel<TASK, MODE>), grid, block, 0, stream, c, s, io, m, g_in);
  else if (c.gyro)
    hipLaunchKernelGGL((rollout_mlp_vjp_gyro_kernel<TASK, MODE>), grid, block, 0, stream, c, s, io, m);
  else
    hipLaunchKernelGGL((rollout_mlp_vjp_kernel<TASK, MODE>), grid, block, 0, stream, c, s, io, m);
  return hipGetLastError();
}

hipError_t launch_rollout_mlp_states(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                     const MlpArgs& m, hipStream_t stream) {
  CS_DISPATCH(mlp_states_t, c, s, io, m, stream)
}

hipError_t launch_rollout_mlp_vjp(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                  const MlpArgs& m, const double* g_in, hipStream_t stream) {
  CS_DISPATCH(mlp_vjp_t, c, s, io, m, g_in, stream)
}

// the argument blocks, checked before the context: the MLP block's own checks, then check_rollout_io on a copy of io
// whose actions_dev is the action tape (returned in `out`)
int check_rollout_io_mlp(const cs_rollout_io* io, const cs_rollout_mlp_io* mio, const char* who, bool vjp,
                         cs_rollout_io* out) {
  const std::string w(who);
  if (io == nullptr) return report_error(CS_ERR_ARG, (w + ": null io").c_str());
  if (mio == nullptr) return report_error(CS_ERR_ARG, (w + ": null mio").c_str());
  if (mio->struct_size != sizeof(cs_rollout_mlp_io))
    return report_error(CS_ERR_ABI, (w + ": mio->struct_size " + std::to_string(mio->struct_size) + " != " +
                                     std::to_string(sizeof(cs_rollout_mlp_io)) + " (sizeof(cs_rollout_mlp_io))").c_str());
  if (int rc_ = check_hidden(who, "hidden", mio->hidden)) return rc_;
  if (mio->params_dev == nullptr) return report_error(CS_ERR_ARG, (w + ": params_dev is required").c_str());
  if (mio->actions_out_dev == nullptr)
    return report_error(CS_ERR_ARG, (w + ": actions_out_dev (the action tape) is required").c_str());
  if (io->actions_dev != nullptr)
    return report_error(CS_ERR_ARG, (w + ": io->actions_dev must be NULL (the policy makes the actions; open-loop "
                                         "offsets go in mio->offsets_dev)").c_str());
  // the rest is cs_rollout_io's contract, with the action tape where the actions go
  *out = *io;
  out->actions_dev = mio->actions_out_dev;
  return check_rollout_io(out, who, vjp);
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_mlp_states(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mlp_io* mio,
                                     void* stream) {
  cs_rollout_io io2;
  if (int rc_ = cs::check_rollout_io_mlp(io, mio, "cs_rollout_mlp_states", false, &io2)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_mlp_states", stream, &v)) return rc_;
  const cs::MlpArgs m{mio->params_dev, mio->offsets_dev, mio->actions_out_dev, mio->obs_out_dev, mio->hidden};
  const hipError_t e = cs::launch_rollout_mlp_states(v.task, v.mode, *v.c, *v.s, io2, m, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mlp_states: kernel launch");
  return CS_OK;
}

extern "C" int cs_rollout_mlp_vjp(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mlp_io* mio, void* stream) {
  cs_rollout_io io2;
  if (int rc_ = cs::check_rollout_io_mlp(io, mio, "cs_rollout_mlp_vjp", true, &io2)) return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_mlp_vjp", stream, &v)) return rc_;
  const cs::MlpArgs m{mio->params_dev, nullptr, nullptr, nullptr, mio->hidden};
  const hipError_t e = cs::launch_rollout_mlp_vjp(v.task, v.mode, *v.c, *v.s, io2, m, nullptr, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mlp_vjp: kernel launch");
  return CS_OK;
}

extern "C" int cs_rollout_mlp_vjp_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mlp_io* mio,
                                     const cs_rollout_mlp_ex_io* xio, void* stream) {
  if (xio == nullptr) return cs_rollout_mlp_vjp(ctx, io, mio, stream);
  cs_rollout_io io2;
  if (int rc_ = cs::check_rollout_io_mlp(io, mio, "cs_rollout_mlp_vjp_ex", true, &io2)) return rc_;
  if (xio->struct_size != sizeof(cs_rollout_mlp_ex_io))
    return cs::report_error(CS_ERR_ABI, ("cs_rollout_mlp_vjp_ex: xio->struct_size " + std::to_string(xio->struct_size) +
                                         " != " + std::to_string(sizeof(cs_rollout_mlp_ex_io)) +
                                         " (sizeof(cs_rollout_mlp_ex_io))").c_str());
  if (xio->reserved_ != 0) return cs::report_error(CS_ERR_ARG, "cs_rollout_mlp_vjp_ex: xio->reserved_ must be 0");
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_rollout_mlp_vjp_ex", stream, &v)) return rc_;
  const cs::MlpArgs m{mio->params_dev, nullptr, nullptr, nullptr, mio->hidden};
  const hipError_t e =
      cs::launch_rollout_mlp_vjp(v.task, v.mode, *v.c, *v.s, io2, m, xio->g_actions_in_dev, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_mlp_vjp_ex: kernel launch");
  return CS_OK;
}
