// copterstep_urts.hip -- an unscented Rauch-Tung-Striebel fixed-interval smoother over the tapes of cs_rollout_ukf on
// gfx950 (cs_urts_smooth, include/copterstep.h): K backward steps per env in one launch, each the filter's 25 sigma
// points of that step made again from the filter's own tapes and sent through the step's physics, their moments and
// their cross-covariance with the points before the step, followed by one 12 x 12 symmetric positive definite solve.
// Every input is a tape or the caller's: nothing of the env state is read but the constants and the vehicle table, and
// nothing is written.  DESIGN.md section 25.
//
// Upstream lines: those of cs_rollout_states (setMotors, the state derivative, step), per point.
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t): the conventions, and every kit piece,
// of copterstep_rollout_rts.hip and copterstep_rollout_ukf.hip.  Per backward step j = K-2 .. -1 (row -1 is the filter's
// starting point):
//   factor      U = rts_cholesky(P_f[j]) (rts_solve.h), the filter's factor of step j+2
//   points      25 trips of ONE loop body: ukf_point (ukf_points.h), the physics of rollout_step (physics_substeps) from
//               (the point, status_f[j]) under actions[j+1], ukf_moments_add, and urts_cross_add (urts_cross.h): point
//               1 + c stores column c of dY, point 13 + c subtracts from it
//   prior       ukf_moments_finish: P- in place over the moment sum, the filter's own prior bit for bit
//   cross       W = (wi gamma) dY L^T row by row, in place (urts_cross_row)
//   LANDED row  no points: W = P_f[j], P- = P_f[j] + Q (ukf_landed)
//   solve, smoothing   copterstep_rollout_rts.hip's, with rts_solve.h's functions
// In lane-private LDS columns (element k of a lane at [k * 64 + lane]): the factor U (78 rows), the moment sum S (78),
// dY / W / G (144 rows and one row of stage padding behind them) and the propagated point 0 (12): 313 rows x 512 B =
// 156.5 KiB of the CU's 160, cs_rollout_rts' footprint, one wavefront per CU (profiles/urts_resources.txt).  The
// smoothed row above, P_s[j+1] (78 values) and x_s[j+1] (12), does not fit beside them while the points run: each lane
// parks it in its own column of the caller's workspace (tile-major, 64 lanes wide: element k of a lane at [k * 64 +
// lane] of its tile, so that a row is one coalesced line) and reads the same slots back itself once U and the point 0
// are dead -- same-thread program order, no hand-off between lanes.  The filter's mean x_f[j] is copied to that column
// too: ukf_point addresses the mean and the factor with one stride, and no tape has the LDS's.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// a propagated point and P- must round as the filter's did (the no-measurement identities of section 25 rest on it),
// and the float64 arithmetic of the points, the moments, the cross-covariance and the solve is fixed
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
#include "rts_solve.h"
#include "ukf_points.h"
#include "urts_cross.h"
#include "cov_tile.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the lane's LDS rows (row k at [k * kBlock]): the factor U of P_f[j] -- later P_s[j+1], then D --, the moment sum S --
// later P-, its factor, P_s[j] --, dY / W / G with one row of padding behind them (the stage of the 12 x 12 stores,
// cov_tile.h), and the propagated point 0 -- later x_s[j+1], then x_s[j]
constexpr int kRowS = kEkfSym;
constexpr int kRowW = kRowS + kEkfSym;
constexpr int kRowY0 = kRowW + kStageStride;
constexpr int kUrtsRows = kRowY0 + 12;
static_assert(kUrtsRows * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

// the lane's workspace rows (row k at [k * kBlock] of its tile): P_s[j+1] packed, x_s[j+1], x_f[j]
constexpr int kWsXs = kEkfSym;
constexpr int kWsXf = kWsXs + 12;
constexpr int kWsRows = kWsXf + 12;
static_assert(kWsRows == CS_URTS_WORKSPACE_ROWS, "the workspace the header promises");
static_assert(kBlock == 64, "the workspace is 64 lanes wide");

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void urts_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                      const cs_urts_io r) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  __shared__ __attribute__((aligned(16))) double lds[kUrtsRows * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes smooth env 0 and store nothing but their workspace column)
  const int K = io.num_steps;
  const uint32_t f32 = r.out_dtype == CS_JAC_F32 ? 1u : 0u;
  const UkfWeights wt{r.gamma, r.wm0, r.wc0, r.wi};
  const double scale = urts_cross_scale(wt);

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const U = lds + lane;
  double* const S = U + kRowS * kBlock;
  double* const W = U + kRowW * kBlock;
  double* const Y0 = U + kRowY0 * kBlock;
  double* const stage = lds + kRowW * kBlock;
  double* const mine = stage + lane * kStageStride;
  // the tile's workspace (a 64-bit offset); row k of the lane's column is (ws + k * kBlock)[lane] -- a row's address is
  // the wavefront's, in scalar registers, and the lane is the one offset every access shares: per-lane 64-bit pointers
  // to the rows stay live across the point loop and do not leave the physics its registers (scratch in six of the 36)
  double* const ws = r.workspace_dev + (size_t)tile_index * (kWsRows * kBlock);
  bool ok = true;

  // ---- row K-1 is given: the filter's own, or the caller's (end_x, end_P) ----
  {
    const size_t row = (size_t)(K - 1) * n;  // 64-bit: K x N x 144 doubles pass 4 GiB at 1 M envs
    double x[12];
    if (r.end_x_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) x[k] = r.end_x_dev[(size_t)k * n + ii];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) x[k] = r.x_f_dev[(row + ii) * 12 + k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) (ws + (kWsXs + k) * kBlock)[lane] = x[k];
    load_triangle(S, r.end_P_dev != nullptr ? r.end_P_dev + (size_t)ii * 144 : r.P_f_dev + (row + ii) * 144);
#pragma clang loop unroll(disable)
    for (int e = 0; e < kEkfSym; ++e) (ws + e * kBlock)[lane] = S[e * kBlock];
    if (io.x_dev != nullptr) store_x_row(stage, io.x_dev, row, ro, x);
    if (r.P_tape_dev != nullptr) {
      stage_triangle(mine, S);
      wave_sync();
      store_matrix(r.P_tape_dev, row, stage, ro, f32);
      wave_sync();  // (the first step's dY is written over the stage)
    }
    if (ro.valid && r.var_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) store_out(r.var_dev, (row + i) * 12 + k, S[(k * (k + 1) / 2 + k) * kBlock], f32);
    }
  }

#pragma clang loop unroll(disable)
  for (int j = K - 2; j >= -1; --j) {
    const bool first = j < 0;  // the filter's starting point: x0 [12,N], P0, status0
    const size_t row = first ? 0 : (size_t)j * n;
    const size_t next = (size_t)(j + 1) * n;
    const double* const xf = first ? io.start_x_dev + ii : r.x_f_dev + (row + ii) * 12;
    const size_t xf_stride = first ? (size_t)n : (size_t)1;
    const double* const pf = first ? r.P0_dev + (size_t)ii * 144 : r.P_f_dev + (row + ii) * 144;
    const int fs0 = first ? (int)io.start_status_dev[ii] : (int)r.status_f_dev[row + ii];

    load_triangle(U, pf);
    // the mean at the factor's stride (ukf_point takes one stride for both); the smoothed mean reads it back, so that
    // no pointer into the filter's tapes is live across the points
    double* const XF = ws + kWsXf * kBlock;
#pragma unroll
    for (int k = 0; k < 12; ++k) (XF + k * kBlock)[lane] = xf[k * xf_stride];

    if (fs0 == CS_STATUS_LANDED) {
      // ---- a LANDED row: the filter made no points; the step is the identity ----
      urts_cross_landed(U, W, kBlock);
#pragma clang loop unroll(disable)
      for (int e = 0; e < kEkfSym; ++e) S[e * kBlock] = U[e * kBlock];
      ukf_landed(S, r.Q_dev, kBlock);
    } else {
      // ---- the step's wrench and the factor of P_f[j], as the filter made them for step j+2 ----
      const float4 act = load_action_at<TASK>(io.actions_dev + (next + ii) * A);
      const Wrench w = step_wrench(q, act);
      ok = rts_cholesky(U, kBlock) && ok;

      // ---- the 25 points, each through the physics the filter's point took ----
      double sy[12];
#pragma clang loop unroll(disable)
      for (int p = 0; p < kUkfPoints; ++p) {
        double x[12];
        ukf_point(p, XF + lane, U, kBlock, wt.gamma, x);
        int fsp = fs0;
        bool pend = false;
        physics_substeps<FULL, GYRO, false, true>(c, q, w, x, fsp, pend, -0.0, -0.0, -0.0);
        if (p == 0) {
          ukf_moments_begin(x, Y0, sy, S, kBlock);
        } else {
          ukf_moments_add(x, Y0, sy, S, kBlock);
          urts_cross_add(p, x, W, kBlock);
        }
      }

      // ---- the prior's covariance over the moment sum (its mean goes over the point 0, dead with it: x_pred comes from
      //      the filter's tape), then W = (wi gamma) dY L^T row by row in place ----
      ukf_moments_finish(wt, Y0, sy, S, r.Q_dev, Y0, S, kBlock);
      double diag[12];
      urts_cross_diag(U, kBlock, diag);
#pragma clang loop unroll(disable)
      for (int a = 0; a < 12; ++a) urts_cross_row(W + a * 12 * kBlock, U, diag, scale, kBlock);
    }

    // ---- U and the point 0 are dead: the smoothed row above comes back from the lane's workspace column ----
#pragma unroll 13
    for (int e = 0; e < kEkfSym; ++e) U[e * kBlock] = (ws + e * kBlock)[lane];
#pragma unroll
    for (int k = 0; k < 12; ++k) Y0[k * kBlock] = (ws + (kWsXs + k) * kBlock)[lane];

    // ---- D = P_s[j+1] - P-, the factor of P-, G = P-^-1 W ----
#pragma unroll 13
    for (int e = 0; e < kEkfSym; ++e) U[e * kBlock] -= S[e * kBlock];
    ok = rts_cholesky(S, kBlock) && ok;
#pragma clang loop unroll(disable)
    for (int col = 0; col < 12; ++col) rts_solve_column(S, W, col, kBlock);

    // ---- the smoothed mean, kept for the next step ----
    double x[12];
    {
      double xp[12], dx[12];
      const double* const pred = r.x_pred_dev + (next + ii) * 12;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        xp[k] = (XF + k * kBlock)[lane];
        dx[k] = Y0[k * kBlock] - pred[k];
      }
      rts_mean(W, kBlock, xp, dx, Y0);
#pragma unroll
      for (int k = 0; k < 12; ++k) x[k] = Y0[k * kBlock];
    }

    // ---- the smoothed covariance, over the factor ----
#pragma clang loop unroll(disable)
    for (int col = 0; col < 12; ++col) rts_ps_column(U, W, col, kBlock, pf + col, S);

    // ---- the row parked for the next step ----
    if (!first) {
#pragma unroll 13
      for (int e = 0; e < kEkfSym; ++e) (ws + e * kBlock)[lane] = S[e * kBlock];
#pragma unroll
      for (int k = 0; k < 12; ++k) (ws + (kWsXs + k) * kBlock)[lane] = x[k];
    }

    // ---- row j out (G is dead: its rows are the stage) ----
    wave_sync();
    if (!first) {
      if (io.x_dev != nullptr) store_x_row(stage, io.x_dev, row, ro, x);
    } else if (ro.valid && r.x0_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) r.x0_dev[(size_t)k * n + i] = x[k];
    }
    void* const pdst = first ? r.P0_s_dev : r.P_tape_dev;
    if (pdst != nullptr) {
      stage_triangle(mine, S);
      wave_sync();
      store_matrix(pdst, row, stage, ro, f32);
    }
    wave_sync();  // (the next step's dY is written over the stage)
    if (!first && ro.valid && r.var_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) store_out(r.var_dev, (row + i) * 12 + k, S[(k * (k + 1) / 2 + k) * kBlock], f32);
    }
  }

  if (ro.valid && r.ok_dev != nullptr) r.ok_dev[i] = ok ? 1 : 0;
}

template <int TASK, int MODE>
hipError_t urts_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_urts_io& r,
                  hipStream_t stream) {
  CS_GYRO_LAUNCH(urts_kernel, io, r);
}

hipError_t launch_urts(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                       const cs_urts_io& r, hipStream_t stream) {
  CS_DISPATCH(urts_t, c, s, io, r, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_urts_smooth(cs_ctx* ctx, const cs_rollout_io* io, const cs_urts_io* sio, void* stream) {
  using cs::report_error;
  const char* who = "cs_urts_smooth";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool no_start = io->start_x_dev == nullptr || io->start_status_dev == nullptr;
  const bool extra = io->reward_dev != nullptr || io->terminated_dev != nullptr || io->truncated_dev != nullptr ||
                     io->status_dev != nullptr || io->gx_dev != nullptr || io->gr_dev != nullptr ||
                     io->g_actions_dev != nullptr || io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(
          io, who, {"sio", "cs_urts_io", sio, sizeof(cs_urts_io)},
          no_start ? "start_x_dev (the filter's x0) and start_status_dev are required" : nullptr,
          extra ? "the reward, flag, status, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  if (!(sio->gamma > 0.0) || !std::isfinite(sio->gamma))
    return report_error(CS_ERR_ARG, "cs_urts_smooth: gamma must be finite and > 0");
  if (!std::isfinite(sio->wm0) || !std::isfinite(sio->wc0) || !std::isfinite(sio->wi))
    return report_error(CS_ERR_ARG, "cs_urts_smooth: the weights wm0, wc0 and wi must be finite");
  if (sio->x_f_dev == nullptr || sio->x_pred_dev == nullptr || sio->status_f_dev == nullptr ||
      sio->P_f_dev == nullptr || sio->Q_dev == nullptr || sio->P0_dev == nullptr)
    return report_error(CS_ERR_ARG,
                        "cs_urts_smooth: x_f_dev, x_pred_dev, status_f_dev, P_f_dev, Q_dev and P0_dev are required");
  if (sio->workspace_dev == nullptr)
    return report_error(CS_ERR_ARG, "cs_urts_smooth: workspace_dev is required");
  if ((sio->end_x_dev == nullptr) != (sio->end_P_dev == nullptr))
    return report_error(CS_ERR_ARG, "cs_urts_smooth: end_x_dev and end_P_dev are given both or neither");
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(
          ctx, who, stream, sio->out_dtype,
          {io->start_x_dev, io->x_dev, sio->x_f_dev, sio->x_pred_dev, sio->P_f_dev, sio->Q_dev, sio->P0_dev,
           sio->end_x_dev, sio->end_P_dev, sio->x0_dev, sio->workspace_dev},
          {sio->P_tape_dev, sio->var_dev, sio->P0_s_dev}, {io->actions_dev}, "actions_dev", &v))
    return rc_;
  const hipError_t e = cs::launch_urts(v.task, v.mode, *v.c, *v.s, *io, *sio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_urts_smooth: kernel launch");
  return CS_OK;
}
