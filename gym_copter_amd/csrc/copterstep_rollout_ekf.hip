// copterstep_rollout_ekf.hip -- an extended Kalman filter over the env step on gfx950 (cs_rollout_ekf,
// include/copterstep.h): K predict / update steps per env in one launch, with a 12 x 12 symmetric covariance per env and
// the step Jacobian applied on the fly, never stored.  The filter's mean and covariance are the caller's: nothing of the
// env state is read but the constants and the vehicle table, and nothing is written.  DESIGN.md section 19.
//
// Upstream lines differentiated: those of copterstep_jacobian.hip (setMotors, the state derivative, step).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  Per step:
//   mean        the physics of rollout_step (clip, motor law, physics_substeps) from the filter's own mean and status
//   covariance  P- = A P A^T + Q by cov_predict (cov_tile.h: jacobian_block with zero wrench tangents -- the actions are
//               known -- in two passes of 6 blocks of 2 directions), the function the smoother calls for the same prior
//   update      M sequential scalar updates (ekf_update.h)
// P (78 rows, packed upper triangle), W (144 rows and one row of stage padding behind it), the mean at the start of the
// step (12 rows) and the prior / posterior mean (12 rows) live in lane-private LDS columns (element j of a lane at
// [j * 64 + lane], as section 13's): 247 rows x 512 B = 123.5 KiB, one wavefront per CU
// (profiles/rollout_ekf_resources.txt).  After the second pass W is dead: the wavefront's 12 x 12 outputs and its mean
// rows are staged there and leave as linear runs.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// the mean must round as the step kernels do: x_pred is cs_rollout_states' row from the same point bit for bit, and the
// update's float64 arithmetic is fixed (one multiply and one add per term, no fma)
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
#include "ekf_update.h"
#include "cov_tile.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the lane's LDS rows (row j at [j * kBlock]): the packed upper triangle of P, W = A P (W[i][c] at i * 12 + c) with one
// row of padding behind it (the stage of the 12 x 12 stores, cov_tile.h), the mean at the start of the step (the
// Jacobian's point) and the prior / posterior mean
constexpr int kRowW = kEkfSym;
constexpr int kRowX0 = kRowW + kStageStride;
constexpr int kRowX = kRowX0 + 12;
constexpr int kEkfRows = kRowX + 12;
static_assert(kEkfRows * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_ekf_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                             const cs_rollout_ekf_io e) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  __shared__ __attribute__((aligned(16))) double lds[kEkfRows * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes filter env 0 and store nothing)
  const int K = io.num_steps;
  const int M = e.num_meas;
  const uint32_t f32 = e.out_dtype == CS_JAC_F32 ? 1u : 0u;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const P = lds + lane;
  double* const W = P + kRowW * kBlock;
  double* const X0 = P + kRowX0 * kBlock;
  double* const X = P + kRowX * kBlock;
  double* const stage = lds + kRowW * kBlock;

  // ---- the caller's filter state: xhat_0, its status, the upper triangle of P0 ----
#pragma unroll
  for (int j = 0; j < 12; ++j) X[j * kBlock] = io.start_x_dev[(size_t)j * n + ii];
  int fs = (int)io.start_status_dev[ii];
  {
    const double* p0 = e.P0_dev + (size_t)ii * 144;
#pragma clang loop unroll(disable)
    for (int j = 0; j < 12; ++j) {
#pragma clang loop unroll(disable)
      for (int a = 0; a <= j; ++a) P[(j * (j + 1) / 2 + a) * kBlock] = p0[a * 12 + j];
    }
  }
  EkfStats st{0.0, 0.0, true};

#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit: K x N x 144 doubles pass 4 GiB at 1 M envs
    const float4 act = load_action_at<TASK>(io.actions_dev + (row + ii) * A);
    bool clipped;
    const Wrench w = step_wrench(q, act, &clipped);
    const int fs0 = fs;
    uint32_t bits = (fs0 == CS_STATUS_LANDED ? (uint32_t)kJacLanded : 0u) | (clipped ? (uint32_t)kJacClipped : 0u);

    // ---- the mean: rollout_step's physics from (xhat, status), no storage rounding; xhat is kept as the Jacobian's
    //      point ----
    {
      double x[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        x[j] = X[j * kBlock];
        X0[j * kBlock] = x[j];
      }
      if (fs0 != CS_STATUS_LANDED) {
        bool pend = false;
        physics_substeps<FULL, GYRO, false, true>(c, q, w, x, fs, pend, -0.0, -0.0, -0.0);
      }
#pragma unroll
      for (int j = 0; j < 12; ++j) X[j * kBlock] = x[j];
    }

    // ---- the covariance: P- = A P A^T + Q at the mean the step started from ----
    bits |= cov_predict<FULL, GYRO>(c, q, w, fs0, X0, kBlock, P, W, e.Q_dev);

    // ---- the prior mean out (W is dead: its rows are the stage) ----
    {
      double x[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) x[j] = X[j * kBlock];
      wave_sync();
      if (e.x_pred_dev != nullptr) store_x_row(stage, e.x_pred_dev, row, ro, x);
    }

    // ---- the update: M scalar measurements in order ----
    st.nis = 0.0;
    {
      const double* zr = e.z_dev + (row + ii) * (size_t)M;
#pragma clang loop unroll(disable)
      for (int m = 0; m < M; ++m) ekf_scalar_update(X, P, kBlock, e.H_dev + m * 12, e.r_dev[m], zr[m], st);
    }

    // ---- the tapes of row k ----
    {
      double x[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) x[j] = X[j * kBlock];
      if (io.x_dev != nullptr) store_x_row(stage, io.x_dev, row, ro, x);
    }
    const bool last = k == K - 1;
    if (e.P_tape_dev != nullptr || (last && e.P_dev != nullptr)) {
      stage_triangle(stage + lane * kStageStride, P);
      wave_sync();
      if (e.P_tape_dev != nullptr) store_matrix(e.P_tape_dev, row, stage, ro, f32);
      if (last && e.P_dev != nullptr) store_matrix(e.P_dev, 0, stage, ro, f32);
      wave_sync();  // (the next step's W is written over the stage)
    }
    if (ro.valid) {
      if (e.var_dev != nullptr) {
#pragma unroll
        for (int j = 0; j < 12; ++j) store_out(e.var_dev, (row + i) * 12 + j, P[(j * (j + 1) / 2 + j) * kBlock], f32);
      }
      if (e.nis_dev != nullptr) store_out(e.nis_dev, row + i, st.nis, f32);
      if (io.status_dev != nullptr) io.status_dev[row + i] = (uint8_t)fs;
      if (e.branch_dev != nullptr) e.branch_dev[row + i] = (uint8_t)bits;
    }
  }

  if (ro.valid) {
    if (e.loglik_dev != nullptr) store_out(e.loglik_dev, i, st.loglik, f32);
    if (e.ok_dev != nullptr) e.ok_dev[i] = st.ok ? 1 : 0;
  }
}

template <int TASK, int MODE>
hipError_t ekf_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_ekf_io& e,
                 hipStream_t stream) {
  const dim3 grid(grid_for(s.n)), block(kBlock);
  if (c.gyro)
    hipLaunchKernelGGL((rollout_ekf_kernel<TASK, MODE, true>), grid, block, 0, stream, c, s, io, e);
  else
    hipLaunchKernelGGL((rollout_ekf_kernel<TASK, MODE, false>), grid, block, 0, stream, c, s, io, e);
  return hipGetLastError();
}

hipError_t launch_rollout_ekf(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const cs_rollout_ekf_io& e, hipStream_t stream) {
  CS_DISPATCH(ekf_t, c, s, io, e, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_ekf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_ekf_io* eio, void* stream) {
  using cs::report_error;
  const char* who = "cs_rollout_ekf";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool no_start = io->start_x_dev == nullptr || io->start_status_dev == nullptr;
  const bool extra = io->reward_dev != nullptr || io->terminated_dev != nullptr || io->truncated_dev != nullptr ||
                     io->gx_dev != nullptr || io->gr_dev != nullptr || io->g_actions_dev != nullptr ||
                     io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(io, who, {"eio", "cs_rollout_ekf_io", eio, sizeof(cs_rollout_ekf_io)},
                                    no_start ? "start_x_dev (the mean) and start_status_dev are required" : nullptr,
                                    extra ? "the reward, flag, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  if (eio->num_meas < 1 || eio->num_meas > CS_EKF_MAX_MEAS)
    return report_error(CS_ERR_ARG, "cs_rollout_ekf: num_meas must be 1 .. CS_EKF_MAX_MEAS");
  if (eio->H_dev == nullptr || eio->r_dev == nullptr || eio->Q_dev == nullptr || eio->P0_dev == nullptr ||
      eio->z_dev == nullptr)
    return report_error(CS_ERR_ARG, "cs_rollout_ekf: H_dev, r_dev, Q_dev, P0_dev and z_dev are required");
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(
          ctx, who, stream, eio->out_dtype,
          {io->start_x_dev, io->x_dev, eio->H_dev, eio->r_dev, eio->Q_dev, eio->P0_dev, eio->z_dev, eio->x_pred_dev},
          {eio->P_dev, eio->P_tape_dev, eio->var_dev, eio->nis_dev, eio->loglik_dev}, {io->actions_dev}, "actions_dev",
          &v))
    return rc_;
  const hipError_t e = cs::launch_rollout_ekf(v.task, v.mode, *v.c, *v.s, *io, *eio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_ekf: kernel launch");
  return CS_OK;
}
