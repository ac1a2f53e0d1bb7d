// copterstep_rollout_ukf.hip -- an unscented Kalman filter over the env step on gfx950 (cs_rollout_ukf,
// include/copterstep.h): K predict / update steps per env in one launch, 25 sigma points per env and step, each through
// the step's own physics; no Jacobian.  The filter's mean, covariance and status are the caller's: nothing of the env
// state is read but the constants and the vehicle table, and nothing is written.  DESIGN.md section 23.
//
// Upstream lines: those of cs_rollout_states (setMotors, the state derivative, step), per point.
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t): the conventions, and every kit
// piece, of copterstep_rollout_ekf.hip.  Per step:
//   factor      U = rts_cholesky(P) on a copy (rts_solve.h)
//   points      25 trips of ONE loop body: ukf_point (ukf_points.h), the physics of rollout_step (physics_substeps) from
//               (the point, the status of the mean), ukf_moments_add -- the points are never stored
//   prior       ukf_moments_finish: x-, P- = the weighted moments + Q
//   update      M sequential scalar updates (ekf_update.h)
// The start, the prior-mean store, the update, the tapes of a row and the closing stores are filter_step.h's, the
// functions copterstep_rollout_ekf.hip calls: the update and the tapes are the EKF's by construction.  What is written
// here is the UKF's own: the factor, the points, the moments, the point tapes and the LANDED shortcut.
// P (78 rows, packed upper triangle), its factor U (78 rows), the moment sum S (78 rows, with U the stage of cov_tile.h's
// 12 x 12 stores once the prior is formed: 156 >= 145 rows), the mean (12 rows) and the propagated point 0 (12 rows)
// live in lane-private LDS columns (element j of a lane at [j * 64 + lane]): 258 rows x 512 B = 129 KiB, one wavefront
// per CU (profiles/rollout_ukf_resources.txt).
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// a propagated point must round as the step kernels do (it is cs_rollout_states' row from the same point bit for bit),
// and the float64 arithmetic of the points, the moments and the update is fixed (one multiply and one add per term)
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
#include "rts_solve.h"
#include "ukf_points.h"
#include "cov_tile.h"
#include "filter_step.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the lane's LDS rows (row j at [j * kBlock]): the packed upper triangle of P, its factor U and the moment sum S -- U and
// S together are the stage of the 12 x 12 stores and of the mean rows (cov_tile.h), dead by then -- the mean, and the
// propagated point 0
constexpr int kRowU = kEkfSym;
constexpr int kRowS = kRowU + kEkfSym;
constexpr int kRowX = kRowS + kEkfSym;
constexpr int kRowY0 = kRowX + 12;
constexpr int kUkfRows = kRowY0 + 12;
static_assert(kRowX - kRowU >= kStageStride, "the stage fits the factor and the moment sum");
static_assert(kUkfRows * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_ukf_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                             const cs_rollout_ukf_io u) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  __shared__ __attribute__((aligned(16))) double lds[kUkfRows * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes filter env 0 and store nothing)
  const int K = io.num_steps;
  const int M = u.num_meas;
  const FilterTapes t = filter_tapes(io, u);
  const UkfWeights wt{u.gamma, u.wm0, u.wc0, u.wi};

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const P = lds + lane;
  double* const U = P + kRowU * kBlock;
  double* const S = P + kRowS * kBlock;
  double* const X = P + kRowX * kBlock;
  double* const Y0 = P + kRowY0 * kBlock;
  double* const stage = lds + kRowU * kBlock;

  // ---- the caller's filter state: xhat_0, its status, the upper triangle of P0 ----
  int fs = filter_load_start(X, P, io.start_x_dev, io.start_status_dev, u.P0_dev, n, ii);
  EkfStats st{0.0, 0.0, true};
  const bool tapes = u.points_dev != nullptr || u.points_pred_dev != nullptr || u.point_status_dev != nullptr;

#pragma clang loop unroll(disable)
  for (int k = 0; k < K; ++k) {
    const size_t row = (size_t)k * n;  // 64-bit: K x N x 25 x 12 doubles pass 4 GiB at 1 M envs
    const float4 act = load_action_at<TASK>(io.actions_dev + (row + ii) * A);
    const Wrench w = step_wrench(q, act);
    const int fs0 = fs;
    const size_t prow = (row + ii) * kUkfPoints;  // the lane's first row of the point tapes
    int spread = 0;

    if (fs0 == CS_STATUS_LANDED) {
      // ---- a LANDED mean: no points; the tapes hold xhat 25 times ----
      if (tapes && ro.valid) {
#pragma clang loop unroll(disable)
        for (int p = 0; p < kUkfPoints; ++p) {
#pragma unroll
          for (int j = 0; j < 12; ++j) {
            const double v = X[j * kBlock];
            if (u.points_dev != nullptr) u.points_dev[(prow + p) * 12 + j] = v;
            if (u.points_pred_dev != nullptr) u.points_pred_dev[(prow + p) * 12 + j] = v;
          }
          if (u.point_status_dev != nullptr) u.point_status_dev[prow + p] = (uint8_t)CS_STATUS_LANDED;
        }
      }
      ukf_landed(P, u.Q_dev, kBlock);
    } else {
      // ---- the factor of P, on a copy ----
#pragma clang loop unroll(disable)
      for (int e = 0; e < kEkfSym; ++e) U[e * kBlock] = P[e * kBlock];
      st.ok = rts_cholesky(U, kBlock) && st.ok;

      // ---- the 25 points, each through the physics the filter's mean would take ----
      double sy[12];
#pragma clang loop unroll(disable)
      for (int p = 0; p < kUkfPoints; ++p) {
        double x[12];
        ukf_point(p, X, U, kBlock, wt.gamma, x);
        if (u.points_dev != nullptr && ro.valid) {
#pragma unroll
          for (int j = 0; j < 12; ++j) u.points_dev[(prow + p) * 12 + j] = x[j];
        }
        int fsp = fs0;
        bool pend = false;
        physics_substeps<FULL, GYRO, false, true>(c, q, w, x, fsp, pend, -0.0, -0.0, -0.0);
        if (ro.valid) {
          if (u.points_pred_dev != nullptr) {
#pragma unroll
            for (int j = 0; j < 12; ++j) u.points_pred_dev[(prow + p) * 12 + j] = x[j];
          }
          if (u.point_status_dev != nullptr) u.point_status_dev[prow + p] = (uint8_t)fsp;
        }
        if (p == 0) {
          fs = fsp;
          ukf_moments_begin(x, Y0, sy, S, kBlock);
        } else {
          spread += fsp != fs ? 1 : 0;
          ukf_moments_add(x, Y0, sy, S, kBlock);
        }
      }

      // ---- the prior: the weighted moments plus Q ----
      ukf_moments_finish(wt, Y0, sy, S, u.Q_dev, X, P, kBlock);
    }

    // ---- the prior mean out (U and S are dead: their rows are the stage), then copterstep_rollout_ekf.hip's update and
    //      tapes (filter_step.h) ----
    filter_store_prior(X, stage, t.x_pred, row, ro);
    const double* zr = u.z_dev + (row + ii) * (size_t)M;
    filter_update(X, P, u.H_dev, u.r_dev, M, st, [zr](int m) { return zr[m]; });
    filter_store_row<true>(t, stage, X, P, row, ro, k == K - 1, fs, (uint32_t)spread, st.nis);
  }
  filter_store_end(t, ro, st);
}

template <int TASK, int MODE>
hipError_t ukf_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_ukf_io& u,
                 hipStream_t stream) {
  CS_GYRO_LAUNCH(rollout_ukf_kernel, io, u);
}

hipError_t launch_rollout_ukf(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const cs_rollout_ukf_io& u, hipStream_t stream) {
  CS_DISPATCH(ukf_t, c, s, io, u, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_ukf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_ukf_io* uio, void* stream) {
  using cs::report_error;
  const char* who = "cs_rollout_ukf";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool no_start = io->start_x_dev == nullptr || io->start_status_dev == nullptr;
  const bool extra = io->reward_dev != nullptr || io->terminated_dev != nullptr || io->truncated_dev != nullptr ||
                     io->gx_dev != nullptr || io->gr_dev != nullptr || io->g_actions_dev != nullptr ||
                     io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(io, who, {"uio", "cs_rollout_ukf_io", uio, sizeof(cs_rollout_ukf_io)},
                                    no_start ? "start_x_dev (the mean) and start_status_dev are required" : nullptr,
                                    extra ? "the reward, flag, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  const char* weights = !(uio->gamma > 0.0) || !std::isfinite(uio->gamma) ? "gamma must be finite and > 0"
                        : !std::isfinite(uio->wm0) || !std::isfinite(uio->wc0) || !std::isfinite(uio->wi)
                            ? "the weights wm0, wc0 and wi must be finite"
                            : nullptr;
  if (int rc_ = cs::check_filter_model(who, uio->num_meas, weights,
                                       {uio->H_dev, uio->r_dev, uio->Q_dev, uio->P0_dev, uio->z_dev},
                                       "H_dev, r_dev, Q_dev, P0_dev and z_dev"))
    return rc_;
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(ctx, who, stream, uio->out_dtype,
                                         {io->start_x_dev, io->x_dev, uio->H_dev, uio->r_dev, uio->Q_dev, uio->P0_dev,
                                          uio->z_dev, uio->x_pred_dev, uio->points_dev, uio->points_pred_dev},
                                         {uio->P_dev, uio->P_tape_dev, uio->var_dev, uio->nis_dev, uio->loglik_dev},
                                         {io->actions_dev}, "actions_dev", &v))
    return rc_;
  const hipError_t e = cs::launch_rollout_ukf(v.task, v.mode, *v.c, *v.s, *io, *uio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_ukf: kernel launch");
  return CS_OK;
}
