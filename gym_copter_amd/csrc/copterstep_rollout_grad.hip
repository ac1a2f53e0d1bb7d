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
// the step's start (O(substeps^2) calls).  Both loops are rollout_sweep.h's, shared with the closed-loop rollouts;
// the kernels here are wrappers that pick the open-loop actions and the sweep's extension.  DESIGN.md sections 10, 11.
#include <cstring>
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
#include "rollout_sweep.h"
#include "dev_launch.h"

namespace cs {
namespace {

template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void rollout_states_kernel(const DevConst c, const DevState s,
                                                                const cs_rollout_io io) {
  __shared__ __attribute__((aligned(16))) double xrow[kBlock * 12];  // 6 KiB: the wavefront's state rows of a step
  rollout_forward<TASK, MODE>(c, s, io, xrow, OpenLoop<TASK>{io.actions_dev, 0});
}

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_vjp_kernel(const DevConst c, const DevState s,
                                                             const cs_rollout_io io) {
  rollout_vjp_sweep<TASK, MODE, GYRO>(c, s, io, SweepPlain{});
}

// The parameter-gradient backward (cs_rollout_vjp_ex): the plain sweep plus the coefficient adjoints, accumulated over
// the steps in lane-private LDS columns, read-modify-written where each term arises, not in registers: the plain sweep
// already holds 229-255 VGPRs (profiles/rollout_grad_resources.txt).  Two sets of kAccRows rows (step 0 has its
// own), 2 x 14 x 8 B x 64 lanes = 14 KiB per workgroup.  The sweep still needs 243-255 VGPRs + up to 44 AGPRs: 1
// wavefront per SIMD in 35 of 36 instantiations, where the plain kernel has 2.
template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_vjp_param_kernel(const DevConst c, const DevState s,
                                                                   const cs_rollout_io io, const ParamGradOut po) {
  __shared__ double acc[2 * kAccRows * kBlock];
  rollout_vjp_sweep<TASK, MODE, GYRO>(c, s, io, SweepParam{po, acc + threadIdx.x});
}

// the launchers of one (task, mode) instantiation (CS_DISPATCH picks it), the backward's split on the rotor-gyro term
template <int TASK, int MODE>
hipError_t states_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, hipStream_t stream) {
  hipLaunchKernelGGL((rollout_states_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, io);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t vjp_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, hipStream_t stream) {
  const dim3 grid(grid_for(s.n)), block(kBlock);
  if (c.gyro)
    hipLaunchKernelGGL((rollout_vjp_kernel<TASK, MODE, true>), grid, block, 0, stream, c, s, io);
  else
    hipLaunchKernelGGL((rollout_vjp_kernel<TASK, MODE, false>), grid, block, 0, stream, c, s, io);
  return hipGetLastError();
}

template <int TASK, int MODE>
hipError_t vjp_param_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const ParamGradOut& po,
                       hipStream_t stream) {
  const dim3 grid(grid_for(s.n)), block(kBlock);
  if (c.gyro)
    hipLaunchKernelGGL((rollout_vjp_param_kernel<TASK, MODE, true>), grid, block, 0, stream, c, s, io, po);
  else
    hipLaunchKernelGGL((rollout_vjp_param_kernel<TASK, MODE, false>), grid, block, 0, stream, c, s, io, po);
  return hipGetLastError();
}

hipError_t launch_rollout_states(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                 hipStream_t stream) {
  CS_DISPATCH(states_t, c, s, io, stream)
}

hipError_t launch_rollout_vjp(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              hipStream_t stream) {
  CS_DISPATCH(vjp_t, c, s, io, stream)
}

hipError_t launch_rollout_vjp_param(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                                    const ParamGradOut& po, hipStream_t stream) {
  CS_DISPATCH(vjp_param_t, c, s, io, po, stream)
}

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

// override_state for cs_jvp_rollout (copterstep_jvp.hip), whose block carries its own vehicle_dev
int override_vehicle(const ParamView& pv, const double* vehicle_dev, const DevState& s0, hipStream_t stream,
                     const char* who, DevState* out) {
  cs_rollout_param_io pio{};
  pio.vehicle_dev = vehicle_dev;
  return override_state(pv, &pio, s0, stream, who, out);
}

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

// the filter family's second block and what its entry points ask of io alike, in the order they always checked it
int check_filter_io(const cs_rollout_io* io, const char* who, const FilterExt& ext, const char* start_missing,
                    const char* must_be_null) {
  const std::string w(who), name(ext.name);
  if (ext.block == nullptr) return report_error(CS_ERR_ARG, (w + ": null " + name).c_str());
  uint32_t struct_size, out_dtype;  // the block's first two words (the second is read once the first says it is there)
  std::memcpy(&struct_size, ext.block, sizeof(uint32_t));
  if (struct_size != ext.size)
    return report_error(CS_ERR_ABI, (w + ": " + name + "->struct_size " + std::to_string(struct_size) + " != " +
                                     std::to_string(ext.size) + " (sizeof(" + ext.type + "))").c_str());
  if (start_missing != nullptr) return report_error(CS_ERR_ARG, (w + ": " + start_missing).c_str());
  if (io->start_force_dev != nullptr || io->start_prev_shaping_dev != nullptr)
    return report_error(CS_ERR_ARG, (w + ": start_force_dev and start_prev_shaping_dev must be NULL").c_str());
  if (must_be_null != nullptr) return report_error(CS_ERR_ARG, (w + ": " + must_be_null).c_str());
  std::memcpy(&out_dtype, static_cast<const char*>(ext.block) + sizeof(uint32_t), sizeof(uint32_t));
  if (out_dtype != CS_JAC_F64 && out_dtype != CS_JAC_F32)
    return report_error(CS_ERR_ARG, (w + ": unknown " + name + "->out_dtype (CS_JAC_F64 or CS_JAC_F32)").c_str());
  return CS_OK;
}

int check_filter_model(const char* who, int32_t num_meas, const char* own_failed,
                       std::initializer_list<const void*> required, const char* required_names) {
  const std::string w(who);
  if (num_meas < 1 || num_meas > CS_EKF_MAX_MEAS)
    return report_error(CS_ERR_ARG, (w + ": num_meas must be 1 .. CS_EKF_MAX_MEAS").c_str());
  if (own_failed != nullptr) return report_error(CS_ERR_ARG, (w + ": " + own_failed).c_str());
  for (const void* p : required)
    if (p == nullptr) return report_error(CS_ERR_ARG, (w + ": " + required_names + " are required").c_str());
  return CS_OK;
}

int enter_filter_context(cs_ctx* ctx, const char* who, void* stream, uint32_t out_dtype,
                         std::initializer_list<const void*> f64s, std::initializer_list<const void*> outs,
                         std::initializer_list<const void*> w32s, const char* w32_names, ContextView* out) {
  const std::string w(who);
  const auto aligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; };
  for (const void* p : f64s)
    if (!aligned(p, 7u)) return report_error(CS_ERR_ARG, (w + ": a float64 array is not 8-B aligned").c_str());
  for (const void* p : outs)
    if (!aligned(p, out_dtype == CS_JAC_F32 ? 3u : 7u))
      return report_error(CS_ERR_ARG, (w + ": an output array is not aligned to its element size").c_str());
  for (const void* p : w32s)
    if (!aligned(p, 3u)) return report_error(CS_ERR_ARG, (w + ": " + w32_names + " is not 4-B aligned").c_str());
  if (int rc_ = enter_context(ctx, who, stream, out)) return rc_;
  if (out->c->act_f32)
    return report_error(CS_ERR_ARG, (w + ": not available with the float32 motor model (action_arith)").c_str());
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
