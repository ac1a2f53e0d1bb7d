// copterstep_jacobian.hip -- the Jacobians of one env step on gfx950 (cs_step_jacobian, include/copterstep.h): for
// every env, d x' / d x, d x' / d action and the gradient of the reward, of the transition step() would perform from
// the stored state (or from a caller's explicit point).  Nothing of the env state is written.
//
// Upstream lines differentiated (paths relative to the upstream checkout):
//   dynamics/__init__.py:114-197 (setMotors), :249-290 (state derivative), :292-302 (_bodyZToInertial),
//   envs/task.py:77-137 (step: the clip of :91, the LANDED skip of :86-87), envs/lander.py:46-74 (reward).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t), the state decoded by the same
// unpack_env / pending_perturbation path as step_kernel: the stored-state evaluation point is the one the next step()
// starts from by construction.  The primal is the arithmetic of physics_call(); the tangents go in direction blocks
// (jacobian_tangents.h), and each block leaves through the LDS (store_slab).  DESIGN.md section 9.
#include <string>
#include <type_traits>

#include "copterstep_jacobian.h"

// the primal must round as the step kernels do (copterstep_kernels.hip)
#pragma clang fp contract(off)

#include "dev_tile.h"
#include "dev_codec.h"
#include "dev_math.h"
#include "dev_physics.h"
#include "dev_task.h"
#include "jacobian_tangents.h"
#include "dev_launch.h"

namespace cs {
namespace {

template <int TASK, int MODE>
__global__ __launch_bounds__(kBlock) void step_jacobian_kernel(const DevConst c, const DevState s,
                                                               const cs_jacobian_io io) {
  constexpr int A = task_act_dim(TASK);
  constexpr int NDIR = 12 + A;
  constexpr int NBLK = (NDIR + kJacDirs - 1) / kJacDirs;
  static_assert(12 % kJacDirs == 0, "a block is all dx or all du (the 1D tasks' last block has one zero direction)");
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  __shared__ double slab[kBlock * 12 * kJacDirs];  // 12 KiB: one block's tangents of the wavefront
  __shared__ double rslab[kBlock * kJacDirs];      // ... and the reward gradient's entries

  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const bool valid = i < n;

  // ---- evaluation point ----
  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, valid ? i : 0u);
  JacPoint pt;
  bool resetting = false, prev_none = false;
  if (io.x_dev != nullptr) {  // the caller's point: its force (if given) is pending, nothing else is
#pragma unroll
    for (int k = 0; k < 12; ++k) pt.x[k] = valid ? io.x_dev[(size_t)k * n + i] : 0.0;
    pt.fs = valid ? (int)io.status_dev[i] : CS_STATUS_AIRBORNE;
    pt.px = pt.py = pt.pz = -0.0;
    if (io.force_dev != nullptr && valid) {
      pt.px = io.force_dev[i] * q.two_inv_M;
      pt.py = io.force_dev[(size_t)n + i] * q.two_inv_M;
      pt.pz = io.force_dev[(size_t)2 * n + i] * q.two_inv_M;
    }
  } else {  // the stored state, decoded as step_kernel decodes it (tiles cover the whole grid: padding lanes read zeros)
    using TILE = TileIO<MODE>;
    const TILE tile(s, tile_index, lane);
    Env<MODE> e;
    unpack_env<MODE, TILE>(c, tile.load_group(0), tile.load_group(1), tile.load_group(2), tile.load_group(3), e);
#pragma unroll
    for (int k = 0; k < 12; ++k) pt.x[k] = e.x[k];
    pt.fs = e.fs;
    pending_perturbation<MODE>(c, q, tile, i, e.episode, e.ep_far, e.pend, e.expl, pt.px, pt.py, pt.pz);
    resetting = e.reset_pending;
    prev_none = e.prev_sh != e.prev_sh;  // upstream's None: the reward is the constant 0
  }
  pt.active = !resetting && pt.fs != CS_STATUS_LANDED;

  // ---- action: the task's motor fan-out (_get_motors), np.clip (task.py:91) and its derivative, 1 on [0, 1] ----
  const float4 act = load_action<TASK>(io.actions_dev, valid ? i : 0u);
  const float araw[4] = {act.x, act.y, act.z, act.w};
  float mf[4];
  double m[4], clipd[4];
  bool clipped = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mf[j] = clip01(araw[j]);
    m[j] = (double)mf[j];
    const bool in = araw[j] >= 0.f && araw[j] <= 1.f;
    clipd[j] = in ? 1.0 : 0.0;
    clipped |= !in;
  }
  Wrench w;
  w.bz = thrust_model(q, mf[0], mf[1], mf[2], mf[3]);  // (the float64 law also under action_arith = float32)
  torque_model(q, mf[0], mf[1], mf[2], mf[3], w);

  const bool lander = task_is_lander(TASK);
  uint32_t bits = (pt.fs == CS_STATUS_LANDED && !resetting ? (uint32_t)kJacLanded : 0u) |
                  (resetting ? (uint32_t)kJacReset : 0u) | (clipped ? (uint32_t)kJacClipped : 0u);

#pragma clang loop unroll(disable)
  for (int b = 0; b < NBLK; ++b) {
    // the block's directions: state slot g (g < 12) or action column g - 12
    double v[kJacDirs][12];
    Wrench dw[kJacDirs];
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d) {
      const int g = b * kJacDirs + d;
#pragma unroll
      for (int k = 0; k < 12; ++k) v[d][k] = (g == k) ? 1.0 : 0.0;
      double dm[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        // motor j is driven by action column j (3D), [0, 1, 1, 0][j] (2D) or 0 (1D): lander.py:95-97 and the attic
        // fan-outs; its derivative sums the motor columns into the action columns
        const int col = A == 4 ? j : A == 2 ? ((j == 1 || j == 2) ? 1 : 0) : 0;
        dm[j] = (g - 12 == col) ? clipd[j] : 0.0;
      }
      dw[d] = wrench_tangent(q, m, dm);
    }
    double x[12];
    if (c.gyro) {
      bits |= jacobian_block<FULL, true>(c, q, w, dw, pt, x, v);
    } else {
      bits |= jacobian_block<FULL, false>(c, q, w, dw, pt, x, v);
    }
    if (resetting) {  // the step replaces the state: nothing of the point survives it
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d)
#pragma unroll
        for (int k = 0; k < 12; ++k) v[d][k] = 0.0;
    }
    // reward gradient: grad shaping(x') . v for the Lander, unless the reward is a constant (Hover; upstream's None;
    // the tilt overwrite reward = -penalty, tested on the stored words as step() tests them; a pending reset)
    double rg[kJacDirs] = {};
    if constexpr (lander) {
      double xr[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) xr[k] = round_stored<MODE>(x[k]);
      const bool tilt = !test_oob(c, xr[0], xr[2]) && test_tilt(c, xr[6], xr[8]);
      if (!resetting && !prev_none && !tilt) {
        double gs[12];
        shaping_gradient(c, x, gs);
#pragma unroll
        for (int d = 0; d < kJacDirs; ++d) {
          double acc = 0.0;
#pragma unroll
          for (int k = 0; k < 12; ++k) acc = fma(gs[k], v[d][k], acc);
          rg[d] = acc;
        }
      }
    }

    // ---- stage the block in the LDS, then store it env-major ----
    __syncthreads();  // (the previous block's slab has been read)
#pragma unroll
    for (int k = 0; k < 12; ++k)
#pragma unroll
      for (int d = 0; d < kJacDirs; ++d) slab[(lane * 12 + k) * kJacDirs + d] = v[d][k];
#pragma unroll
    for (int d = 0; d < kJacDirs; ++d) rslab[lane * kJacDirs + d] = rg[d];
    __syncthreads();
    const uint32_t nst = n;  // (every store tests env0 + e < n: lanes past the end write nothing)
    if (b * kJacDirs < 12) {
      const int c0 = b * kJacDirs;
      if (io.out_dtype == CS_JAC_F32) {
        if (io.dx_dev) store_slab<float, kJacDirs, 12>((float*)io.dx_dev, slab, lane, env0, nst, 12, c0);
        if (io.reward_dx_dev) store_slab<float, kJacDirs, 1>((float*)io.reward_dx_dev, rslab, lane, env0, nst, 12, c0);
      } else {
        if (io.dx_dev) store_slab<double, kJacDirs, 12>((double*)io.dx_dev, slab, lane, env0, nst, 12, c0);
        if (io.reward_dx_dev) store_slab<double, kJacDirs, 1>((double*)io.reward_dx_dev, rslab, lane, env0, nst, 12, c0);
      }
    } else {  // action columns c0 .. c0 + WU - 1 (a 3D task's four take two blocks, a 1D task's one is half a block)
      constexpr int WU = A < kJacDirs ? A : kJacDirs;
      const int c0 = b * kJacDirs - 12;
      if (io.out_dtype == CS_JAC_F32) {
        if (io.du_dev) store_slab<float, WU, 12>((float*)io.du_dev, slab, lane, env0, nst, A, c0);
        if (io.reward_du_dev) store_slab<float, WU, 1>((float*)io.reward_du_dev, rslab, lane, env0, nst, A, c0);
      } else {
        if (io.du_dev) store_slab<double, WU, 12>((double*)io.du_dev, slab, lane, env0, nst, A, c0);
        if (io.reward_du_dev) store_slab<double, WU, 1>((double*)io.reward_du_dev, rslab, lane, env0, nst, A, c0);
      }
    }
  }
  if (valid && io.branch_dev != nullptr) io.branch_dev[i] = (uint8_t)bits;
}

template <int TASK, int MODE>
hipError_t jacobian_t(const DevConst& c, const DevState& s, const cs_jacobian_io& io, hipStream_t stream) {
  hipLaunchKernelGGL((step_jacobian_kernel<TASK, MODE>), dim3(grid_for(s.n)), dim3(kBlock), 0, stream, c, s, io);
  return hipGetLastError();
}

hipError_t launch_step_jacobian(int task, int mode, const DevConst& c, const DevState& s, const cs_jacobian_io& io,
                                hipStream_t stream) {
  CS_DISPATCH(jacobian_t, c, s, io, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_step_jacobian(cs_ctx* ctx, const cs_jacobian_io* io, void* stream) {
  using cs::report_error;
  // (the argument block is checked before the context: a caller's layout error is reported as such)
  if (io == nullptr) return report_error(CS_ERR_ARG, "cs_step_jacobian: null io");
  if (io->struct_size != sizeof(cs_jacobian_io))
    return report_error(CS_ERR_ABI, ("cs_step_jacobian: io->struct_size " + std::to_string(io->struct_size) + " != " +
                                     std::to_string(sizeof(cs_jacobian_io)) + " (sizeof(cs_jacobian_io))").c_str());
  cs::ContextView v;
  if (int rc_ = cs::enter_context(ctx, "cs_step_jacobian", stream, &v)) return rc_;
  if (io->actions_dev == nullptr) return report_error(CS_ERR_ARG, "cs_step_jacobian: actions_dev is required");
  if (io->out_dtype != CS_JAC_F64 && io->out_dtype != CS_JAC_F32)
    return report_error(CS_ERR_ARG, "cs_step_jacobian: unknown out_dtype (CS_JAC_F64 or CS_JAC_F32)");
  if (io->x_dev == nullptr && (io->status_dev != nullptr || io->force_dev != nullptr))
    return report_error(CS_ERR_ARG, "cs_step_jacobian: status_dev / force_dev describe an explicit point: x_dev is required");
  if (io->x_dev != nullptr && io->status_dev == nullptr)
    return report_error(CS_ERR_ARG, "cs_step_jacobian: an explicit point needs status_dev");
  const hipError_t e = cs::launch_step_jacobian(v.task, v.mode, *v.c, *v.s, *io, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_step_jacobian: kernel launch");
  return CS_OK;
}
