// copterstep_rollout_rts.hip -- a Rauch-Tung-Striebel fixed-interval smoother over the tapes of cs_rollout_ekf on gfx950
// (cs_rollout_rts, include/copterstep.h): K backward steps per env in one launch, each the filter's covariance
// prediction made again from the filter's own tapes -- the step Jacobian applied on the fly, never stored -- followed by
// one 12 x 12 symmetric positive definite solve.  Every input is a tape or the caller's: nothing of the env state is
// read but the constants and the vehicle table, and nothing is written.  DESIGN.md section 20.
//
// Upstream lines differentiated: those of copterstep_jacobian.hip (setMotors, the state derivative, step).
//
// One lane per env on the tile layout of the step kernels (tile t -> workgroup t).  Per backward step j = K-2 .. -1
// (row -1 is the filter's starting point):
//   prediction  P- = A P_f[j] A^T + Q at (x_f[j], status_f[j]) under actions[j+1] by cov_predict (cov_tile.h), the
//               function copterstep_rollout_ekf.hip calls with the same arguments: in float64 P- is the filter's own
//               prior of that step bit for bit.  W = A P_f[j] is kept.
//   solve       D = P_s[j+1] - P-, then P- = U^T U in place and G = P-^-1 W column by column in place (rts_solve.h)
//   smoothing   x_s[j] = x_f[j] + G^T (x_s[j+1] - x_pred[j+1]);  P_s[j] = P_f[j] + G^T D G, column by column into the
//               rows of the factor, which is dead once G is solved
// In lane-private LDS columns (element k of a lane at [k * 64 + lane], as section 13's): two packed triangles of 78
// rows that swap roles from step to step -- one is P_f[j], P-, U, P_s[j] in turn, the other P_s[j+1] and then D --, W / G
// (144 rows and one row of stage padding behind it) and x_s[j+1] (12 rows): 313 rows x 512 B = 156.5 KiB of the CU's
// 160, one wavefront per CU (profiles/rollout_rts_resources.txt).  What does not fit is read from the input tapes where
// it is needed: the Jacobian's point x_f[j] once per block (L2 hits beside a jacobian_block) and P_f[j] a second time
// for the smoothed covariance.  Once G is dead the wavefront's 12 x 12 outputs and its mean rows are staged in its rows
// and leave as linear runs.  No output of this launch is read back.
#include <cmath>
#include <string>

#include "copterstep_jacobian.h"

// P- must round as the filter's did (the no-measurement identities of section 20 rest on it), and the solve's float64
// arithmetic is fixed (one multiply and one add or subtract per term, no fma)
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
#include "cov_tile.h"
#include "dev_launch.h"

namespace cs {
namespace {

// the lane's LDS rows (row k at [k * kBlock]): triangle 0, W = A P_f (W[i][c] at i * 12 + c) with one row of padding
// behind it (the stage of the 12 x 12 stores, cov_tile.h), triangle 1, x_s[j+1]
constexpr int kRowW = kEkfSym;
constexpr int kRowT1 = kRowW + kStageStride;
constexpr int kRowXs = kRowT1 + kEkfSym;
constexpr int kRtsRows = kRowXs + 12;
static_assert(kRtsRows * kBlock * sizeof(double) <= 160 * 1024, "the LDS of one CU");

template <int TASK, int MODE, bool GYRO>
__global__ __launch_bounds__(kBlock) void rollout_rts_kernel(const DevConst c, const DevState s, const cs_rollout_io io,
                                                             const cs_rollout_rts_io r) {
  constexpr int A = task_act_dim(TASK);
  constexpr bool FULL = MODE == CS_STATE_F64 || kFullTrigInEveryMode;
  __shared__ __attribute__((aligned(16))) double lds[kRtsRows * kBlock];
  const int lane = threadIdx.x;
  const uint32_t tile_index = blockIdx.x;
  const uint32_t i = tile_index * kBlock + threadIdx.x;
  const uint32_t n = s.n;
  const uint32_t env0 = i - lane;
  const RowOut ro{lane, i, env0, i < n, env0 + (uint32_t)kWave <= n};
  const uint32_t ii = ro.valid ? i : 0u;  // (padding lanes smooth env 0 and store nothing)
  const int K = io.num_steps;
  const uint32_t f32 = r.out_dtype == CS_JAC_F32 ? 1u : 0u;

  Coef q = uniform_coef(c);
  if (s.veh != nullptr) q = load_coef(s.veh, s.veh_stride, ii);
  double* const W = lds + lane + kRowW * kBlock;
  double* const XS = lds + lane + kRowXs * kBlock;
  double* const stage = lds + kRowW * kBlock;
  double* const mine = stage + lane * kStageStride;
  // the two triangles by their offsets, which swap after every step: `ta` takes P_f[j] and ends as P_s[j], `tb` holds
  // P_s[j+1]
  int ta = 0, tb = kRowT1 * kBlock;
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
    for (int k = 0; k < 12; ++k) XS[k * kBlock] = x[k];
    double* const Tb = lds + lane + tb;
    load_triangle(Tb, r.end_P_dev != nullptr ? r.end_P_dev + (size_t)ii * 144 : r.P_f_dev + (row + ii) * 144);
    if (io.x_dev != nullptr) store_x_row(stage, io.x_dev, row, ro, x);
    if (r.P_tape_dev != nullptr) {
      stage_triangle(mine, Tb);
      wave_sync();
      store_matrix(r.P_tape_dev, row, stage, ro, f32);
      wave_sync();  // (the first step's W is written over the stage)
    }
    if (ro.valid && r.var_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) store_out(r.var_dev, (row + i) * 12 + k, Tb[(k * (k + 1) / 2 + k) * kBlock], f32);
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
    double* const Ta = lds + lane + ta;
    double* const Tb = lds + lane + tb;

    // ---- the step's wrench, as the filter made it for step j+2 ----
    const float4 act = load_action_at<TASK>(io.actions_dev + (next + ii) * A);
    const Wrench w = step_wrench(q, act);

    load_triangle(Ta, pf);

    // ---- the prediction: P- = A P_f[j] A^T + Q at the filter's point, by the filter's function (its branch bits are
    //      on the filter's tape already) ----
    cov_predict<FULL, GYRO>(c, q, w, fs0, xf, xf_stride, Ta, W, r.Q_dev);

    // ---- D = P_s[j+1] - P-, the factor of P-, G = P-^-1 W ----
#pragma unroll 13
    for (int k = 0; k < kEkfSym; ++k) Tb[k * kBlock] -= Ta[k * kBlock];
    ok = rts_cholesky(Ta, kBlock) && ok;
#pragma clang loop unroll(disable)
    for (int col = 0; col < 12; ++col) rts_solve_column(Ta, W, col, kBlock);

    // ---- the smoothed mean, kept for the next step ----
    double x[12];
    {
      double xp[12], dx[12];
      const double* const pred = r.x_pred_dev + (next + ii) * 12;
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        xp[k] = xf[k * xf_stride];
        dx[k] = XS[k * kBlock] - pred[k];
      }
      rts_mean(W, kBlock, xp, dx, XS);
#pragma unroll
      for (int k = 0; k < 12; ++k) x[k] = XS[k * kBlock];
    }

    // ---- the smoothed covariance, over the factor ----
#pragma clang loop unroll(disable)
    for (int col = 0; col < 12; ++col) rts_ps_column(Tb, W, col, kBlock, pf + col, Ta);

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
      stage_triangle(mine, Ta);
      wave_sync();
      store_matrix(pdst, row, stage, ro, f32);
    }
    wave_sync();  // (the next step's W is written over the stage)
    if (!first && ro.valid && r.var_dev != nullptr) {
#pragma unroll
      for (int k = 0; k < 12; ++k) store_out(r.var_dev, (row + i) * 12 + k, Ta[(k * (k + 1) / 2 + k) * kBlock], f32);
    }
    const int t = ta;
    ta = tb;
    tb = t;
  }

  if (ro.valid && r.ok_dev != nullptr) r.ok_dev[i] = ok ? 1 : 0;
}

template <int TASK, int MODE>
hipError_t rts_t(const DevConst& c, const DevState& s, const cs_rollout_io& io, const cs_rollout_rts_io& r,
                 hipStream_t stream) {
  CS_GYRO_LAUNCH(rollout_rts_kernel, io, r);
}

hipError_t launch_rollout_rts(int task, int mode, const DevConst& c, const DevState& s, const cs_rollout_io& io,
                              const cs_rollout_rts_io& r, hipStream_t stream) {
  CS_DISPATCH(rts_t, c, s, io, r, stream)
}

}  // namespace
}  // namespace cs

extern "C" int cs_rollout_rts(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_rts_io* rio, void* stream) {
  using cs::report_error;
  const char* who = "cs_rollout_rts";
  if (int rc_ = cs::check_rollout_io(io, who, false)) return rc_;
  const bool no_start = io->start_x_dev == nullptr || io->start_status_dev == nullptr;
  const bool extra = io->reward_dev != nullptr || io->terminated_dev != nullptr || io->truncated_dev != nullptr ||
                     io->status_dev != nullptr || io->gx_dev != nullptr || io->gr_dev != nullptr ||
                     io->g_actions_dev != nullptr || io->g_x0_dev != nullptr;
  if (int rc_ = cs::check_filter_io(
          io, who, {"rio", "cs_rollout_rts_io", rio, sizeof(cs_rollout_rts_io)},
          no_start ? "start_x_dev (the filter's x0) and start_status_dev are required" : nullptr,
          extra ? "the reward, flag, status, cotangent and gradient pointers must be NULL" : nullptr))
    return rc_;
  if (rio->x_f_dev == nullptr || rio->x_pred_dev == nullptr || rio->status_f_dev == nullptr ||
      rio->P_f_dev == nullptr || rio->Q_dev == nullptr || rio->P0_dev == nullptr)
    return report_error(CS_ERR_ARG,
                        "cs_rollout_rts: x_f_dev, x_pred_dev, status_f_dev, P_f_dev, Q_dev and P0_dev are required");
  if ((rio->end_x_dev == nullptr) != (rio->end_P_dev == nullptr))
    return report_error(CS_ERR_ARG, "cs_rollout_rts: end_x_dev and end_P_dev are given both or neither");
  cs::ContextView v;
  if (int rc_ = cs::enter_filter_context(ctx, who, stream, rio->out_dtype,
                                         {io->start_x_dev, io->x_dev, rio->x_f_dev, rio->x_pred_dev, rio->P_f_dev,
                                          rio->Q_dev, rio->P0_dev, rio->end_x_dev, rio->end_P_dev, rio->x0_dev},
                                         {rio->P_tape_dev, rio->var_dev, rio->P0_s_dev}, {io->actions_dev},
                                         "actions_dev", &v))
    return rc_;
  const hipError_t e = cs::launch_rollout_rts(v.task, v.mode, *v.c, *v.s, *io, *rio, (hipStream_t)stream);
  if (e != hipSuccess) return cs::report_hip(e, "cs_rollout_rts: kernel launch");
  return CS_OK;
}
